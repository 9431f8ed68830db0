"""GPU: auto-reset inside the rollout windows (asvrl_env_rollout_ar / asvrl_policy_rollout_ar) against the composed
loop of the existing calls, bit for bit. For t < K the reference runs (closed loop) fused_mlp.actor_act at step
STEP0 + t, b.step(..., counter=C0 + t, trainer_deactivate=True) and b.reset_observe(cfg, b.env_done & mask,
counter=RC + t, obs_counter=OC + t) into b.obs / b.obj_cnt (the two-launch form with per-robot parameters).
Compared with rtol = atol = 0 and NaN = NaN: every record of every step (obs_prev and the actions among them),
pushed, resets, steps_run and every final array; the stats' return sum, an atomic sum, within 1e-12. E = 37 envs:
the last workgroup is partial. Episodes end inside the windows because episode_limit is 5 and ep_ts is preset to
e % 9 (and, with 12 robots, by collisions)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = 37
GAMMA = 0.99
KMAX = 13
STEP0 = 7
POLICY_SEED = 4242
C0, RC, OC = 1, 0x40000000, 0x80000000
OPEN_RECORDS = ("reward", "done", "info", "env_done", "obs", "obj_cnt", "rs", "obs_prev")
RECORDS = OPEN_RECORDS + ("actions",)
FINALS = ("rs", "rflags", "n_robots", "n_obs", "n_cores", "ep_ts", "obstacles", "cores", "obs", "obs64", "obj_cnt",
          "reward", "done", "info", "env_done")   # + stats
EPS_HALF = (1.0, 1.0, 1.0, 0.5, 0.5)
EPS_ZERO = (1.0, 1.0, 1.0, 0.0, 0.0)
SHAPES = [(1, 0, 0), (5, 4, 2), (12, 8, 0)]


def _same(got, ref, what):
    torch.testing.assert_close(got, ref, rtol=0, atol=0, equal_nan=True, msg=lambda m: f"{what}: {m}")


@functools.lru_cache(maxsize=None)
def _pack(operands="bf16"):
    from distributional_rl_decision_and_control_amd.fused_mlp import MlpPack
    from distributional_rl_decision_and_control_amd.policy.AC_IQN_model import AC_IQN_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    pol = AC_IQN_Policy(**DEFAULT_NET, value_ranges_of_action=[[-1, 1], [-1, 1]], device="cuda", seed=100)
    return MlpPack(pol.actor, "actor", operands)


def _cfg(R, O, C, width=None):
    from distributional_rl_decision_and_control_amd.device_env import reset_cfg
    W = width if width is not None else (55.0 if R <= 5 else 110.0)
    return reset_cfg(R, O, C, 20.0, width=W, height=W)


def _ending(R, O, C, fast, robot_params=False):
    """A device-reset batch with its reset observation in b.obs whose envs end at steps that differ per env:
    episode_limit 5, ep_ts preset to e % 9 (the existing rollout tests' recipe). The same call gives the same batch."""
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.device_env import DeviceEnvBatch
    b = DeviceEnvBatch(E, R, O, C, obs64=True, params=_abi.params_from(episode_limit=5))
    if robot_params:
        b.set_robot_params([b.params] * (E * R))
    b.reset(_cfg(R, O, C), seed=11)
    b.step(None, do_dynamics=False, seed=11, counter=0, fast_noise=fast)
    b.ep_ts.copy_(torch.arange(E, dtype=torch.int32, device="cuda") % 9)
    return b


def _finals(b):
    return {k: getattr(b, k).clone() for k in FINALS + ("stats",)}


def _specs(b):
    spec = b._record_specs()
    NT = b.n_envs * b.max_robots
    spec["actions"] = ((NT, 2), torch.float64, 0)
    spec["obs_prev"] = ((NT, 40), torch.float32, 0)
    return spec


def _actions(R, K=KMAX):
    g = torch.Generator(device="cuda").manual_seed(21 + R)
    return 2.0 * torch.rand((K, E * R, 2), generator=g, device="cuda", dtype=torch.float64) - 1.0


def _loop(b, cfg, K, pack=None, eps=EPS_HALF, actions=None, launch=None, env_mask=None, fast=True, two_launch=False):
    """The composed reference. Returns the records as the fused calls lay them out (rows of envs that do not step at
    the pre-fill), pushed [K], the resets after every step, and the finals after every step."""
    from distributional_rl_decision_and_control_amd.fused_mlp import actor_act
    spec = _specs(b)
    names = RECORDS if pack is not None else OPEN_RECORDS
    rec = {n: torch.full((K,) + spec[n][0], spec[n][2], dtype=spec[n][1], device="cuda") for n in names}
    R = b.max_robots
    mask = env_mask if env_mask is not None else torch.ones(E, dtype=torch.uint8, device="cuda")
    on_e = mask != 0
    on_r = on_e.repeat_interleave(R)
    slot = torch.arange(E * R, device="cuda") % R
    act64 = torch.zeros((E * R, 2), dtype=torch.float64, device="cuda")
    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")
    pushed = torch.zeros(K, dtype=torch.int32, device="cuda")
    resets = torch.zeros(E, dtype=torch.int32, device="cuda")
    finals, resets_after = [], []
    for t in range(K):
        rec["obs_prev"][t][on_r] = b.obs[on_r]
        if pack is not None:
            actor_act(pack, b.obs, act64, step, *eps, POLICY_SEED)
            step += 1
        else:
            act64 = actions[t]
        exist_r = on_r & (slot < b.n_robots.repeat_interleave(R))
        b.step(act64, seed=11, counter=C0 + t, trainer_deactivate=True, gamma=GAMMA, env_mask=env_mask, launch=launch,
               fast_noise=fast)
        for n in names:
            if n == "obs_prev":
                continue
            src = act64 if n == "actions" else getattr(b, n)
            if n == "rs":
                rec[n][t][:, exist_r] = src[:, exist_r]
            else:
                sel = on_e if n == "env_done" else on_r
                rec[n][t][sel] = src[sel]
        pushed[t] = int((b.obj_cnt[on_r] >= 0).sum())
        m = (b.env_done * mask).contiguous()
        resets += m.int()
        if two_launch:
            b.reset(cfg, m, seed=11, counter=RC + t)
            b.step(None, do_dynamics=False, seed=11, counter=OC + t, fast_noise=fast, env_mask=m)
        else:
            b.reset_observe(cfg, m, seed=11, counter=RC + t, obs_counter=OC + t, obs=b.obs, obj_cnt=b.obj_cnt,
                            fast_noise=fast)
        finals.append(_finals(b))
        resets_after.append(resets.clone())
    return rec, pushed, resets_after, finals


def _ar(b, cfg, **own):
    return dict(cfg=cfg, reset_counter=RC, obs_counter=OC, **own)


def _run(b, cfg, K, pack=None, eps=EPS_HALF, actions=None, keep=None, ar_own=None, **kw):
    """The fused call (closed loop with a pack, open loop with actions)."""
    ar = _ar(b, cfg, **(ar_own or {}))
    if pack is not None:
        step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")
        got = b.policy_rollout(pack, K, b.obs, keep=keep if keep is not None else RECORDS, step_dev=step, eps=eps,
                               policy_seed=POLICY_SEED, trainer_deactivate=True, seed=11, counter=C0, gamma=GAMMA,
                               auto_reset=ar, **kw)
        assert int(step.item()) == STEP0, "the caller's step counter is only read"
        return got
    ar["obs_in"] = b.obs
    return b.rollout(actions[:K].contiguous(), keep=keep if keep is not None else OPEN_RECORDS,
                     trainer_deactivate=True, seed=11, counter=C0, gamma=GAMMA, auto_reset=ar, **kw)


def _check(b, got, ref, K, what, closed, steps=None):
    rec, pushed, resets_after, finals = ref
    for n in (RECORDS if closed else OPEN_RECORDS):
        _same(getattr(got, n), rec[n][:K], f"{what}: record {n}")
    _same(got.pushed, pushed[:K], f"{what}: pushed")
    _same(got.resets, resets_after[K - 1], f"{what}: resets")
    _same(got.steps_run, steps if steps is not None else torch.full((E,), K, dtype=torch.int32, device="cuda"),
          f"{what}: steps_run")
    for n in FINALS:
        _same(getattr(b, n), finals[K - 1][n], f"{what}: final {n}")
    s, r = b.stats.cpu().numpy(), finals[K - 1]["stats"].cpu().numpy()
    assert np.array_equal(s[1:], r[1:]), f"{what}: stats counts {s} vs {r}"
    assert abs(s[0] - r[0]) <= 1e-12 * max(1.0, abs(r[0])), f"{what}: stats return sum {s[0]} vs {r[0]}"


@functools.lru_cache(maxsize=None)
def _reference(R, O, C, fast, closed, eps=EPS_HALF, operands="bf16"):
    """One 13-round composed loop per case: its first K rounds are the reference of a K-step window."""
    b = _ending(R, O, C, fast)
    return _loop(b, _cfg(R, O, C), KMAX, pack=_pack(operands) if closed else None, eps=eps,
                 actions=None if closed else _actions(R), fast=fast)


def _launches(R):
    from distributional_rl_decision_and_control_amd import _abi
    return (None, (_abi.ENV_LAYOUT_PAIRS, 64, max(1, 64 // R)), (0, 0, 0, 3))


def test_reference_ends_at_different_steps():
    """What the other tests rely on, asserted on the reference alone: every env ends at least twice in 13 steps, at
    steps that differ per env, some workgroups (8 envs at the automatic shape) see several ends in one step, and
    some step has no reset anywhere in some workgroup."""
    for closed in (False, True):
        rec, _, resets_after, _ = _reference(5, 4, 2, True, closed)
        ends = rec["env_done"].cpu().numpy() != 0          # [K, E]
        assert resets_after[-1].min().item() >= 2
        assert np.array_equal(ends.sum(0), resets_after[-1].cpu().numpy())
        assert len({tuple(np.nonzero(ends[:, e])[0]) for e in range(E)}) > 4, "ends at steps that differ per env"
        groups = [ends[:, g:g + 8] for g in range(0, E, 8)]
        assert any((g.sum(1) >= 2).any() for g in groups), "several ends in one step of one workgroup"
        assert any((g.sum(1) == 0).any() for g in groups), "a step with no reset anywhere in some workgroup"
        for K in (1, 2, 13):
            assert ends[K - 1].any(), f"an env ends on the last step of a {K}-step window"


@pytest.mark.parametrize("closed", [False, True], ids=["open", "closed"])
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("R,O,C", SHAPES)
def test_autoreset_matches_composed_loop(R, O, C, fast, closed):
    """K = 1, 2, 13 (an env ends on the last step of each: the final state and `last` outputs are the reset ones),
    the automatic launch shape, a forced one-wave shape and the automatic shape at max_groups = 3."""
    ref = _reference(R, O, C, fast, closed)
    n0 = _ending(R, O, C, fast).n_robots
    changed = any(not torch.equal(f["n_robots"], n0) for f in ref[3])
    print(f"R={R} O={O} C={C} fast={fast} closed={closed}: n_robots changed by a reset: {changed}; "
          f"resets per env {ref[2][-1].min().item()}..{ref[2][-1].max().item()}")
    assert ref[2][-1].min().item() >= 2
    for K in (1, 2, 13):
        for launch in _launches(R):
            b = _ending(R, O, C, fast)
            got = _run(b, _cfg(R, O, C), K, pack=_pack() if closed else None, actions=None if closed else _actions(R),
                       fast_noise=fast, launch=launch)
            _check(b, got, ref, K, f"R={R} O={O} fast={fast} closed={closed} K={K} launch={launch}", closed)


@pytest.mark.parametrize("closed", [False, True], ids=["open", "closed"])
def test_autoreset_placement_falls_short(closed):
    """12 robots reset onto a 40 m map: the rejection sampler places fewer robots than asked, so n_robots and the
    exists predicate change inside the window (asserted on the reference)."""
    R, O, C = 12, 8, 0
    cfg = _cfg(R, O, C, width=40.0)
    acts = None if closed else _actions(R)
    ref = _loop(_ending(R, O, C, True), cfg, KMAX, pack=_pack() if closed else None, actions=acts)
    n0 = _ending(R, O, C, True).n_robots
    assert (ref[3][-1]["n_robots"] < n0).any(), "the placement must fall short somewhere"
    for launch in _launches(R)[:2]:
        b = _ending(R, O, C, True)
        got = _run(b, cfg, KMAX, pack=_pack() if closed else None, actions=acts, fast_noise=True, launch=launch)
        _check(b, got, ref, KMAX, f"falls short closed={closed} launch={launch}", closed)


def test_autoreset_greedy_and_f32_build():
    """Epsilon 0, and the f32-operand build against its own loop."""
    R, O, C = 5, 4, 2
    for eps, ops in ((EPS_ZERO, "bf16"), (EPS_HALF, "f32")):
        ref = _reference(R, O, C, True, True, eps, ops)
        for launch in _launches(R)[:2]:
            b = _ending(R, O, C, True)
            got = _run(b, _cfg(R, O, C), KMAX, pack=_pack(ops), eps=eps, fast_noise=True, launch=launch)
            _check(b, got, ref, KMAX, f"eps={eps} operands={ops} launch={launch}", True)
    assert not torch.equal(_reference(R, O, C, True, True, EPS_HALF, "f32")[0]["actions"],
                           _reference(R, O, C, True, True)[0]["actions"]), "the two builds' actors differ in rounding"


@pytest.mark.parametrize("closed", [False, True], ids=["open", "closed"])
def test_autoreset_env_mask(closed):
    """A caller's mask leaves every fourth env (and one whole workgroup's envs) out: they neither step nor reset."""
    R, O, C = 5, 4, 2
    mask = torch.ones(E, dtype=torch.uint8, device="cuda")
    mask[::4] = 0
    mask[8:16] = 0
    cfg, acts = _cfg(R, O, C), None if closed else _actions(R)
    ref = _loop(_ending(R, O, C, True), cfg, KMAX, pack=_pack() if closed else None, actions=acts, env_mask=mask)
    b = _ending(R, O, C, True)
    before = _finals(b)
    got = _run(b, cfg, KMAX, pack=_pack() if closed else None, actions=acts, fast_noise=True, env_mask=mask)
    _check(b, got, ref, KMAX, f"mask closed={closed}", closed, steps=(mask != 0).int() * KMAX)
    off = mask == 0
    assert int(got.resets[off].sum().item()) == 0 and int(got.resets[~off].min().item()) >= 2
    off_r = off.repeat_interleave(R)
    for n in ("obs", "reward", "done", "info", "obj_cnt", "rflags"):
        _same(getattr(b, n)[off_r], before[n][off_r], f"masked env's {n}")
    _same(b.rs[:, off_r], before["rs"][:, off_r], "masked env's state")
    assert not got.obs_prev[:, off_r].any(), "masked envs' obs_prev rows keep their pre-fill"


@pytest.mark.parametrize("closed", [False, True], ids=["open", "closed"])
@pytest.mark.parametrize("case", ["robot_params", "layout2"])
def test_autoreset_fallback(case, closed):
    """Per-robot parameters and an explicit layout 2 run the K-launch form inside the call: the same results."""
    from distributional_rl_decision_and_control_amd import _abi
    R, O, C, K = 5, 4, 2, 8
    rp = case == "robot_params"
    launch = None if rp else (_abi.ENV_LAYOUT_SWEEP, 0, 0)
    cfg, acts = _cfg(R, O, C), None if closed else _actions(R)
    ref = _loop(_ending(R, O, C, True, robot_params=rp), cfg, K, pack=_pack() if closed else None, actions=acts,
                launch=launch, two_launch=rp)
    assert ref[2][-1].min().item() >= 1
    b = _ending(R, O, C, True, robot_params=rp)
    got = _run(b, cfg, K, pack=_pack() if closed else None, actions=acts, fast_noise=True, launch=launch)
    _check(b, got, ref, K, f"{case} closed={closed}", closed)
    # and the fused path gives what the fallback gives
    if not rp:
        b2 = _ending(R, O, C, True)
        got2 = _run(b2, cfg, K, pack=_pack() if closed else None, actions=acts, fast_noise=True)
        _check(b2, got2, ref, K, f"{case} closed={closed} fused", closed)


@pytest.mark.parametrize("closed", [False, True], ids=["open", "closed"])
def test_autoreset_graph_capture(closed):
    """One call with every buffer passed in, captured in a graph and replayed twice from a restored state."""
    R, O, C, K = 5, 4, 2, 7
    pack = _pack() if closed else None
    cfg, acts = _cfg(R, O, C), None if closed else _actions(R)
    b = _ending(R, O, C, True)
    names = ("rs", "rflags", "n_robots", "n_obs", "n_cores", "ep_ts", "obstacles", "cores", "obs", "obj_cnt", "stats",
             "env_done")
    state = {n: getattr(b, n).clone() for n in names}
    spec = _specs(b)
    recs = RECORDS if closed else OPEN_RECORDS

    def records():
        rec = {n: torch.full((K,) + spec[n][0], spec[n][2], dtype=spec[n][1], device="cuda") for n in recs}
        rec["steps_run"] = torch.zeros(E, dtype=torch.int32, device="cuda")
        own = dict(pushed=torch.zeros(K, dtype=torch.int32, device="cuda"),
                   resets=torch.zeros(E, dtype=torch.int32, device="cuda"))
        return rec, own

    def call(rec, own):
        return _run(b, cfg, K, pack=pack, actions=acts, keep=rec, ar_own=own, fast_noise=True)

    def restore():
        for n, t in state.items():
            getattr(b, n).copy_(t)

    eager, eown = records()
    call(eager, eown)
    torch.cuda.synchronize()
    finals = _finals(b)
    assert int(eown["resets"].sum().item()) > 0
    restore()
    rec, own = records()
    if closed:
        # _run reads the step counter back on the host: not inside a capture
        step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")
        ar = _ar(b, cfg, **own)
        fn = lambda: b.policy_rollout(pack, K, b.obs, keep=rec, step_dev=step, eps=EPS_HALF, policy_seed=POLICY_SEED,  # noqa: E731
                                      trainer_deactivate=True, seed=11, counter=C0, gamma=GAMMA, auto_reset=ar,
                                      fast_noise=True)
    else:
        fn = lambda: call(rec, own)  # noqa: E731
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(2):
        restore()
        g.replay()
        torch.cuda.synchronize()
        for n in recs + ("steps_run",):
            _same(rec[n], eager[n], f"replayed record {n}")
        _same(own["pushed"], eown["pushed"], "replayed pushed")
        _same(own["resets"], eown["resets"], "replayed resets")
        for n in FINALS:
            _same(getattr(b, n), finals[n], f"replayed final {n}")


def test_auto_reset_none_is_todays_call():
    """auto_reset=None: the existing calls, against the existing composed loop (no reset), one case of each."""
    from distributional_rl_decision_and_control_amd.fused_mlp import actor_act
    R, O, C, K = 5, 4, 2, 6
    old = ("reward", "done", "info", "env_done", "obs", "obj_cnt", "rs")
    for closed in (False, True):
        ref_b = _ending(R, O, C, True)
        acts = _actions(R)
        act64 = torch.zeros((E * R, 2), dtype=torch.float64, device="cuda")
        step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")
        ref = {n: [] for n in old}
        for t in range(K):
            if closed:
                actor_act(_pack(), ref_b.obs, act64, step, *EPS_HALF, POLICY_SEED)
                step += 1
            ref_b.step(act64 if closed else acts[t], seed=11, counter=C0 + t, trainer_deactivate=True, gamma=GAMMA,
                       fast_noise=True)
            for n in old:
                ref[n].append(getattr(ref_b, n).clone())
        b = _ending(R, O, C, True)
        if closed:
            step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")
            got = b.policy_rollout(_pack(), K, b.obs, keep=old, step_dev=step, eps=EPS_HALF, policy_seed=POLICY_SEED,
                                   trainer_deactivate=True, seed=11, counter=C0, gamma=GAMMA, fast_noise=True,
                                   auto_reset=None)
        else:
            got = b.rollout(acts[:K].contiguous(), keep=old, trainer_deactivate=True, seed=11, counter=C0, gamma=GAMMA,
                            fast_noise=True, auto_reset=None)
        assert not hasattr(got, "resets") and not hasattr(got, "pushed")
        for n in old:
            _same(getattr(got, n), torch.stack(ref[n]), f"closed={closed}: record {n}")
        for n in FINALS:
            _same(getattr(b, n), getattr(ref_b, n), f"closed={closed}: final {n}")
        with pytest.raises(ValueError):
            b.rollout(acts[:K].contiguous(), keep=("obs_prev",), trainer_deactivate=True)
