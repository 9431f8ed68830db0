"""CPU: the binding of asvrl_iqn_dist, asvrl_dist_prepare and asvrl_eval_dist_stats (new entry points, ABI 29
unchanged). Their struct sizes agree between ctypes and both compiled libraries, the symbols are exported by both, the
pinned layouts are the parent's, and every host-side refusal comes back non-zero with its exact text. The checks fail
before anything is launched: the pointers are made-up addresses that are never dereferenced."""
import ctypes as C

import pytest

import dist_cases
import rollout_abi_cases
from rollout_abi_cases import P

ACT = rollout_abi_cases.WindowAct("iqn")
NAN = float("nan")
SYMBOLS = ("asvrl_iqn_dist", "asvrl_iqn_dist_struct_size", "asvrl_dist_prepare", "asvrl_dist_prepare_struct_size",
           "asvrl_eval_dist_stats", "asvrl_eval_dist_stats_struct_size")


def _dist(**over):
    from distributional_rl_decision_and_control_amd import _abi
    d = _abi.AsvIqnDist()
    d.rows_per_step, d.cvar, d.step0, d.z_out, d.tau_out = 5, 1.0, 0, P, P
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _dist_refused(L, text, null=(), dist=None, **over):
    a = ACT.args(**over)
    a["dist"] = _dist(**(dist or {}))
    order = ("w", "hd", "io", "dist")
    rc = L.asvrl_iqn_dist(*[None if k in null else C.byref(a[k]) for k in order], None)
    assert rc != 0, text
    assert L.asvrl_last_error().decode() == text


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_struct_sizes_and_symbols(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    # rows_per_step, cvar | step0 | 5 pointers | ld_a | 2 pointers | ld_q
    assert C.sizeof(_abi.AsvIqnDist) == 2 * 4 + 8 + 5 * 8 + 8 + 2 * 8 + 8 == 88
    assert L.asvrl_iqn_dist_struct_size() == C.sizeof(_abi.AsvIqnDist)
    # rows, rows_per_step | step0 | seed | 3 pointers
    assert C.sizeof(_abi.AsvDistPrepare) == 2 * 4 + 8 + 8 + 3 * 8 == 48
    assert L.asvrl_dist_prepare_struct_size() == C.sizeof(_abi.AsvDistPrepare)
    # 4 ints | gamma | 12 pointers
    assert C.sizeof(_abi.AsvEvalDistStats) == 4 * 4 + 8 + 12 * 8 == 120
    assert L.asvrl_eval_dist_stats_struct_size() == C.sizeof(_abi.AsvEvalDistStats)
    assert _abi.DIST_SAMPLES == 32 and len(_abi.DIST_STATS_ARRAYS) == 12
    # the ABI and the pinned layouts are the parent's
    assert L.asvrl_abi_version() == 29 == _abi.ABI_VERSION
    assert L.asvrl_iqn_act_ex_struct_size() == C.sizeof(_abi.AsvIqnActEx) == 56
    assert L.asvrl_rollout_struct_size() == C.sizeof(_abi.AsvRollout) == 88
    assert L.asvrl_iqn_risk_struct_size() == C.sizeof(_abi.AsvIqnRisk)
    assert L.asvrl_eval_history_struct_size() == C.sizeof(_abi.AsvEvalHistory)
    assert L.asvrl_eval_metrics_struct_size() == C.sizeof(_abi.AsvEvalMetrics)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_refusals_of_iqn_dist(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    for k in ("w", "hd", "io", "dist"):
        _dist_refused(L, "asvrl_iqn_dist: null argument", null=(k,))
    for n in (8, 16, 7, 0):
        _dist_refused(L, "asvrl_iqn_dist: K = 32 quantile samples per state (N must be 32)", io__N=n, io__B=184)
    for img in rollout_abi_cases.IMAGES["iqn"]:   # null weights, in the IQN calls' own words
        encoder = img in ("self_w", "self_b", "obj_w", "obj_b")   # read with io->obs
        _dist_refused(L, "asvrl_iqn: needs F, or obs with the encoder weights" if encoder else "asvrl_iqn: null weight",
                      **{"w__" + img: None})
    _dist_refused(L, "asvrl_iqn: bad head", hd__wo_frag=None)
    _dist_refused(L, "asvrl_iqn: bad head", hd__n_actions=33)
    _dist_refused(L, "asvrl_iqn: needs F, or obs with the encoder weights", io__obs=None)
    for cv in (0.0, -0.5, 1.5, NAN):
        _dist_refused(L, "asvrl_iqn_dist: cvar must be in (0, 1]", dist=dict(cvar=cv))
    _dist_refused(L, "asvrl_iqn_dist: cvar must be 1 with level_rows (one level, the scalar or the rows')",
                  dist=dict(cvar=0.25, level_rows=P))
    for rps in (0, -3):
        _dist_refused(L, "asvrl_iqn_dist: rows_per_step must be >= 1", dist=dict(rows_per_step=rps))
    _dist_refused(L, "asvrl_iqn_dist: step0 must be >= 0", dist=dict(step0=-1))
    _dist_refused(L, "asvrl_iqn_dist: ld_a must cover n_actions", dist=dict(all_out=P, ld_a=8))
    _dist_refused(L, "asvrl_iqn_dist: ld_q must cover n_actions", dist=dict(qmean_out=P, ld_q=8))


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_refusals_of_dist_prepare(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)

    def prep(**over):
        p = _abi.AsvDistPrepare()
        p.rows, p.rows_per_step, p.step0, p.taus_out, p.actions, p.act_out = 15, 5, 0, P, P, P
        for k, v in over.items():
            setattr(p, k, v)
        return p
    dist_cases.refused(L, "asvrl_dist_prepare", "asvrl_dist_prepare: null struct", None)
    dist_cases.refused(L, "asvrl_dist_prepare", "asvrl_dist_prepare: rows must be >= 0", prep(rows=-1))
    dist_cases.refused(L, "asvrl_dist_prepare", "asvrl_dist_prepare: rows_per_step must be >= 1", prep(rows_per_step=0))
    dist_cases.refused(L, "asvrl_dist_prepare", "asvrl_dist_prepare: step0 must be >= 0", prep(step0=-2))
    dist_cases.refused(L, "asvrl_dist_prepare", "asvrl_dist_prepare: needs taus_out or act_out",
                       prep(taus_out=None, act_out=None))
    dist_cases.refused(L, "asvrl_dist_prepare", "asvrl_dist_prepare: act_out needs actions", prep(actions=None))


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_refusals_of_eval_dist_stats(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    who = "asvrl_eval_dist_stats"
    dist_cases.refused(L, who, who + ": null struct", None)
    for over, text in ((dict(n_steps=0), "n_steps must be >= 1"), (dict(n_envs=0), "n_envs must be >= 1"),
                       (dict(max_robots=0), "max_robots must be in 1..32"),
                       (dict(max_robots=33), "max_robots must be in 1..32"),
                       (dict(block=32), "block must be 0 or a multiple of 64 up to 1024"),
                       (dict(block=100), "block must be 0 or a multiple of 64 up to 1024"),
                       (dict(block=2048), "block must be 0 or a multiple of 64 up to 1024"),
                       (dict(gamma=NAN), "gamma must be in [0, 1]"), (dict(gamma=-0.1), "gamma must be in [0, 1]"),
                       (dict(gamma=1.5), "gamma must be in [0, 1]")):
        dist_cases.refused(L, who, f"{who}: {text}", dist_cases.stats_struct(**over))
    for name in _abi.DIST_STATS_ARRAYS:
        dist_cases.refused(L, who, f"{who}: null array {name}", dist_cases.stats_struct(**{name: None}))
