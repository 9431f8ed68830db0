"""CPU: the binding of asvrl_iqn_act_risk, asvrl_iqn_rollout_risk and asvrl_iqn_rollout_risk_ar (new entry points, ABI
29 unchanged). sizeof(AsvIqnRisk) agrees between ctypes and both compiled libraries, the three symbols are exported by
both, and every refusal comes back non-zero with its exact text. The checks fail before anything is launched: the
pointers are made-up addresses that are never dereferenced."""
import ctypes as C

import pytest

import rollout_abi_cases
from rollout_abi_cases import P

RO = rollout_abi_cases.Rollout("iqn")
ACT = rollout_abi_cases.WindowAct("iqn")
WINDOWS = ("asvrl_iqn_rollout_risk", "asvrl_iqn_rollout_risk_ar")
NAN, INF = float("nan"), float("inf")


def _risk(**over):
    from distributional_rl_decision_and_control_amd import _abi
    r = _abi.AsvIqnRisk()
    r.mode, r.near, r.margin, r.floor, r.cvar_rows = _abi.IQN_RISK_ADAPTIVE, 10.0, 2.8, 0.1, P
    for k, v in over.items():
        setattr(r, k, v)
    return r


def _act_refused(L, text, null=(), risk=None, **over):
    a = ACT.args(**over)
    a["risk"] = _risk(**(risk or {}))
    order = ("w", "hd", "io", "ex", "risk")
    rc = L.asvrl_iqn_act_risk(*[None if k in null else C.byref(a[k]) for k in order], None)
    assert rc != 0, text
    assert L.asvrl_last_error().decode() == text


def _window_refused(L, name, text, null=(), risk=None, **over):
    a = RO.args(**over)
    a["risk"] = _risk(**(risk or {}))
    order = ["params", "state", "ctl", "out", "ro", "pi", "risk"] + (["ar"] if name.endswith("_ar") else [])
    rc = getattr(L, name)(*[None if k in null else C.byref(a[k]) for k in order], None, None)
    assert rc != 0, (name, text)
    assert L.asvrl_last_error().decode() == f"{name}: {text}"


# what an AsvIqnRisk is refused for, under either call's name
RISK_REFUSALS = [
    (dict(mode=0), "risk->mode must be ASVRL_IQN_RISK_ROWS or ASVRL_IQN_RISK_ADAPTIVE"),
    (dict(mode=3), "risk->mode must be ASVRL_IQN_RISK_ROWS or ASVRL_IQN_RISK_ADAPTIVE"),
    (dict(mode=1, cvar_rows=None), "the rows mode needs risk->cvar_rows"),
    (dict(near=0.0), "risk->near must be > 0"),
    (dict(near=-1.0), "risk->near must be > 0"),
    (dict(near=NAN), "risk->near must be > 0"),
    (dict(near=INF), "risk->near must be > 0"),
    (dict(margin=NAN), "risk->margin must be finite"),
    (dict(margin=INF), "risk->margin must be finite"),
    (dict(margin=-INF), "risk->margin must be finite"),
    (dict(floor=0.0), "risk->floor must be in (0, 1]"),
    (dict(floor=-0.1), "risk->floor must be in (0, 1]"),
    (dict(floor=1.5), "risk->floor must be in (0, 1]"),
    (dict(floor=NAN), "risk->floor must be in (0, 1]")]


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_struct_size_and_symbols(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    # mode, near, margin, floor, the two pointers
    assert C.sizeof(_abi.AsvIqnRisk) == 4 * 4 + 2 * 8
    assert L.asvrl_iqn_risk_struct_size() == C.sizeof(_abi.AsvIqnRisk)
    assert (_abi.IQN_RISK_ROWS, _abi.IQN_RISK_ADAPTIVE) == (1, 2)
    for name in ("asvrl_iqn_act_risk",) + WINDOWS:
        assert hasattr(L, name), name
    for name in WINDOWS:   # the IQN calls' arguments with the risk behind the policy
        at = getattr(L, name).argtypes
        assert at[5] is C.POINTER(_abi.AsvIqnPolicy) and at[6] is C.POINTER(_abi.AsvIqnRisk)
    assert L.asvrl_iqn_rollout_risk_ar.argtypes[7] is C.POINTER(_abi.AsvAutoReset)
    # the ABI and the pinned layouts are the parent's
    assert L.asvrl_abi_version() == 29 == _abi.ABI_VERSION
    assert L.asvrl_iqn_act_ex_struct_size() == C.sizeof(_abi.AsvIqnActEx) == 56
    assert L.asvrl_iqn_policy_struct_size() == C.sizeof(_abi.AsvIqnPolicy)
    assert len(_abi.ROLLOUTS) == 5 and _abi.ROLLOUTS["iqn"] == ("asvrl_iqn_rollout", _abi.AsvIqnPolicy)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_refusals_of_the_act_call(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    for k in ("w", "hd", "io"):
        _act_refused(L, "asvrl_iqn: null argument", null=(k,))
    _act_refused(L, "asvrl_iqn_act_risk: null ex", null=("ex",))
    _act_refused(L, "asvrl_iqn_act_risk: null risk", null=("risk",))
    for over, text in RISK_REFUSALS:
        _act_refused(L, "asvrl_iqn_act_risk: " + text, risk=over)
    # the rule reads the observation row: precomputed features carry none (the rows mode takes them)
    _act_refused(L, "asvrl_iqn_act_risk: the adaptive mode needs io->obs (the rule reads the observation row)",
                 io__obs=None, io__F=P)
    _act_refused(L, "asvrl_iqn_act_risk: K = 32 quantile samples per state", risk=dict(mode=1), io__obs=None, io__F=P,
                 io__N=8, io__B=184)
    for cv in (0.25, 0.0, 1.5, NAN):
        _act_refused(L, "asvrl_iqn_act_risk: ex->cvar must be 1 (the level comes from risk)", ex__cvar=cv)
    _act_refused(L, "asvrl_iqn_act_risk: K = 32 quantile samples per state", io__N=8, io__B=184)
    need = "asvrl_iqn_act_risk: needs act_out with ld_act (or act_pair / rec_row) and the epsilon schedule"
    _act_refused(L, need, io__act_out=None)
    _act_refused(L, need, io__eps_total=0.0)
    _act_refused(L, "asvrl_iqn_act_risk: robots_per_env must be >= 1", ex__robots_per_env=0)
    _act_refused(L, "asvrl_iqn_act_risk: ld_q must cover n_actions", ex__qmean_out=P, ex__ld_q=8)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
@pytest.mark.parametrize("name", WINDOWS)
def test_refusals_of_both_window_calls(name, ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    _window_refused(L, name, "null risk", null=("risk",))
    for over, text in RISK_REFUSALS:
        _window_refused(L, name, text, risk=over)
    for cv in (0.25, 0.0, 1.5, NAN):
        _window_refused(L, name, "pi->cvar must be 1 (the level comes from risk)", pi__cvar=cv)
    # the IQN windows' own checks, under the new call's name
    for k in ("params", "state", "ctl", "out", "ro"):
        _window_refused(L, name, "null argument", null=(k,))
    _window_refused(L, name, "null policy", null=("pi",))
    _window_refused(L, name, "null obs_in", pi__obs_in=None)
    _window_refused(L, name, "is_continuous must be 0 (IQN's actions are indices)", ctl__is_continuous=1)
    _window_refused(L, name, "ro->actions must be null (the policy supplies the actions)", ro__actions=P)
    for img in RO.images:
        _window_refused(L, name, "null IQN image", **{"w__" + img: None})
    _window_refused(L, name, "null pi->head.wo_frag", hd__wo_frag=None)
    _window_refused(L, name, "pi->head.n_actions must be in 1..32", hd__n_actions=33)
    _window_refused(L, name, "n_steps must be >= 1", ro__n_steps=0)
    _window_refused(L, name, "observation rows must be 16-byte aligned", pi__obs_in=P + 4)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_auto_reset_refusals(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    name = "asvrl_iqn_rollout_risk_ar"
    _window_refused(L, name, "null ar (the auto-reset description)", null=("ar",))
    _window_refused(L, name, "ro->hold_done cannot be combined with the auto-reset", ro__hold_done=1)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_the_scalar_calls_keep_their_checks(ops):
    """asvrl_iqn_act_ex and the two IQN windows still refuse a level outside (0, 1] in their own words."""
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    ACT.refused(L, "asvrl_iqn_act_ex: cvar must be in (0, 1]", ex__cvar=1.5)
    for name in RO.names:
        RO.refused(L, name, "pi->cvar must be in (0, 1]", pi__cvar=0.0)
