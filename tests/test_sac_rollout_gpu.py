"""GPU: the closed-loop rollout windows under SAC's sampled actor (asvrl_sac_rollout / asvrl_sac_rollout_ar,
env_policy_rollout_kernel's kPolSac instantiations) against the composed loop of the calls they replace, bit for bit:
for t < K, fused_sac.sac_act on the current observation at step counter STEP0 + t (the noise drawn in the kernel on
(row, step, seed); an all-zero eps_in for deterministic=True), the single env step at noise counter C0 + t on those
actions and, with the auto-reset, reset_observe on env_done & mask at (RC + t, OC + t). Every record of every step
(the actions among them; obs_prev, pushed and resets with the auto-reset), the steps every env took and every final
array are compared with atol = rtol = 0 (the stats' return sum, an atomic sum, within 1e-12 as in the Actor's tests).
E = 37 envs: the last workgroup and, at 5 and 12 robots, the last 32-row tile are partial. The weights are a seeded
SAC_Policy's actor."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = 37
GAMMA = 0.99
KMAX = 13
STEP0 = 7          # the policy's step counter at the window's start
POLICY_SEED = 4242
C0, RC, OC = 1, 0x40000000, 0x80000000
RECORDS = ("reward", "done", "info", "env_done", "obs", "obj_cnt", "rs", "actions")
AR_RECORDS = RECORDS + ("obs_prev",)
FINALS = ("rs", "rflags", "n_robots", "n_obs", "n_cores", "ep_ts", "obstacles", "cores", "obs", "obs64", "obj_cnt",
          "reward", "done", "info", "env_done")   # + stats
EPS_HALF = (1.0, 1.0, 1.0, 0.5, 0.5)    # past the exploration fraction from step 1 on: epsilon = 0.5
EPS_ZERO = (1.0, 1.0, 1.0, 0.0, 0.0)    # greedy: always the sampled action
SHAPES = [(1, 0, 0), (5, 4, 2), (12, 8, 0)]


def _same(got, ref, what):
    torch.testing.assert_close(got, ref, rtol=0, atol=0, equal_nan=True, msg=lambda m: f"{what}: {m}")


@functools.lru_cache(maxsize=None)
def _net():
    from distributional_rl_decision_and_control_amd.policy.SAC_model import SAC_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    return SAC_Policy(**DEFAULT_NET, value_ranges_of_action=[[-1.0, 1.0], [-1.0, 1.0]], device="cuda", seed=100)


@functools.lru_cache(maxsize=None)
def _pack(operands="bf16"):
    """The seeded SAC actor's packed images."""
    from distributional_rl_decision_and_control_amd.fused_sac import SacActorPack
    return SacActorPack(_net().actor, operands)


def _cfg(R, O, C):
    from distributional_rl_decision_and_control_amd.device_env import reset_cfg
    W = 55.0 if R <= 5 else 110.0
    return reset_cfg(R, O, C, 20.0, width=W, height=W)


def _batch(R, O, C, fast=True, ending=False, robot_params=False):
    """A device-reset batch with its reset observation in b.obs; the same call gives the same batch. ending: every
    env ends inside a 13-step window at a step that depends on the env (episode_limit 5, ep_ts preset to e % 9)."""
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.device_env import DeviceEnvBatch
    b = DeviceEnvBatch(E, R, O, C, obs64=True, params=_abi.params_from(episode_limit=5) if ending else None)
    if robot_params:
        b.set_robot_params([b.params] * (E * R))
    b.reset(_cfg(R, O, C), seed=11)
    b.step(None, do_dynamics=False, seed=11, counter=0, fast_noise=fast)
    if ending:
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


def _loop(b, pack, K, eps, cfg=None, hold=False, launch=None, env_mask=None, fast=True, two_launch=False,
          deterministic=False):
    """The composed reference: K rounds of sac_act on b.obs (which the step rewrites in place) at step STEP0 + t and
    b.step at counter C0 + t; hold: the mask drops an env after its env_done; cfg (the auto-reset):
    reset_observe(env_done & mask) behind every step; deterministic: eps_in = zeros. Returns a dict of the records
    as policy_rollout() lays them out (rows of steps an env did not take at the pre-fill), steps_run, pushed [K], the
    resets and finals after every step, and acted [K]: the observation every round acted on."""
    from distributional_rl_decision_and_control_amd.fused_sac import sac_act
    ar = cfg is not None
    spec = _specs(b)
    names = AR_RECORDS if ar else RECORDS
    rec = {n: torch.full((K,) + spec[n][0], spec[n][2], dtype=spec[n][1], device="cuda") for n in names}
    R = b.max_robots
    mask = env_mask.clone() if env_mask is not None else (torch.ones(E, dtype=torch.uint8, device="cuda") if hold else None)
    slot = torch.arange(E * R, device="cuda") % R
    act64 = torch.zeros((E * R, 2), dtype=torch.float64, device="cuda")
    eps_out = torch.zeros((E * R, 2), dtype=torch.float32, device="cuda")
    eps_in = torch.zeros((E * R, 2), dtype=torch.float32, device="cuda") if deterministic else None
    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")
    steps_run = torch.zeros(E, dtype=torch.int32, device="cuda")
    pushed = torch.zeros(K, dtype=torch.int32, device="cuda")
    resets = torch.zeros(E, dtype=torch.int32, device="cuda")
    finals, resets_after, acted = [], [], []
    for t in range(K):
        on_e = (mask != 0) if mask is not None else torch.ones(E, dtype=torch.bool, device="cuda")
        on_r = on_e.repeat_interleave(R)
        if ar:
            rec["obs_prev"][t][on_r] = b.obs[on_r]
        acted.append(b.obs.clone())
        sac_act(pack, b.obs, act64, eps_out, step, *eps, POLICY_SEED, eps_in=eps_in)
        step += 1
        rs_r = on_r & (slot < b.n_robots.repeat_interleave(R)) if ar else on_r
        b.step(act64, seed=11, counter=C0 + t, trainer_deactivate=True, gamma=GAMMA, env_mask=mask, launch=launch,
               fast_noise=fast)
        for n in RECORDS:
            src = act64 if n == "actions" else getattr(b, n)
            if n == "rs":
                rec[n][t][:, rs_r] = src[:, rs_r]
            else:
                sel = on_e if n == "env_done" else on_r
                rec[n][t][sel] = src[sel]
        steps_run += on_e.int()
        if hold:
            mask = mask * (b.env_done == 0).to(torch.uint8)
        if ar:
            pushed[t] = int((b.obj_cnt[on_r] >= 0).sum())
            m = (b.env_done * on_e.to(torch.uint8)).contiguous()
            resets += m.int()
            if two_launch:
                b.reset(cfg, m, seed=11, counter=RC + t)
                b.step(None, do_dynamics=False, seed=11, counter=OC + t, fast_noise=fast, env_mask=m)
            else:
                b.reset_observe(cfg, m, seed=11, counter=RC + t, obs_counter=OC + t, obs=b.obs, obj_cnt=b.obj_cnt,
                                fast_noise=fast)
        finals.append(_finals(b))
        resets_after.append(resets.clone())
    return dict(rec=rec, steps_run=steps_run, pushed=pushed, resets_after=resets_after, finals=finals, acted=acted)


def _run(b, pack, K, eps, cfg=None, t0=0, **kw):
    """The window of K steps that starts at round t0 of the composed loop."""
    step = torch.full((1,), STEP0 + t0, dtype=torch.int64, device="cuda")
    ar = dict(cfg=cfg, reset_counter=RC + t0, obs_counter=OC + t0) if cfg is not None else None
    got = b.policy_rollout(pack, K, b.obs, keep=AR_RECORDS if cfg is not None else RECORDS, step_dev=step, eps=eps,
                           policy_seed=POLICY_SEED, trainer_deactivate=True, seed=11, counter=C0 + t0, gamma=GAMMA,
                           auto_reset=ar, **kw)
    assert int(step.item()) == STEP0 + t0, "the caller's step counter is only read"
    return got


def _check(b, got, ref, K, what, steps=None, t0=0):
    ar = "obs_prev" in ref["rec"]
    for n in (AR_RECORDS if ar else RECORDS):
        _same(getattr(got, n), ref["rec"][n][t0:t0 + K], f"{what}: record {n}")
    if ar:
        _same(got.pushed, ref["pushed"][t0:t0 + K], f"{what}: pushed")
        before = ref["resets_after"][t0 - 1] if t0 > 0 else 0
        _same(got.resets, ref["resets_after"][t0 + K - 1] - before, f"{what}: resets")
    _same(got.steps_run, steps if steps is not None else torch.full((E,), K, dtype=torch.int32, device="cuda"),
          f"{what}: steps_run")
    final = ref["finals"][t0 + K - 1]
    for n in FINALS:
        _same(getattr(b, n), final[n], f"{what}: final {n}")
    s, r = b.stats.cpu().numpy(), final["stats"].cpu().numpy()
    assert np.array_equal(s[1:], r[1:]), f"{what}: stats counts {s} vs {r}"
    assert abs(s[0] - r[0]) <= 1e-12 * max(1.0, abs(r[0])), f"{what}: stats return sum {s[0]} vs {r[0]}"


def _assert_in_range(actions, what):
    """Every recorded action is finite and inside the squash's (-1, 1) (or explore()'s [-1, 1))."""
    assert bool(torch.isfinite(actions).all()) and bool((actions.abs() <= 1.0).all()), f"{what}: action range"


@functools.lru_cache(maxsize=None)
def _reference(R, O, C, fast, eps, operands="bf16", ar=False, deterministic=False):
    """One 13-round loop per case: rounds t0 .. t0 + K - 1 are the reference of a K-step window started at t0."""
    return _loop(_batch(R, O, C, fast, ending=ar), _pack(operands), KMAX, eps, cfg=_cfg(R, O, C) if ar else None,
                 fast=fast, deterministic=deterministic)


def _launches(R):
    from distributional_rl_decision_and_control_amd import _abi
    return ((_abi.ENV_LAYOUT_PAIRS, 64, max(1, 64 // R)), (0, 0, 0, 3))


def _assert_steps_and_rows_differ(actions, R, what):
    """The draws are keyed by the step and by the GLOBAL row: a row's actions at t and t + 1 differ, and row r of env e
    never agrees with row r of env e + 16 (16 envs: a multiple of every launch shape's envs per workgroup here, so
    the two rows have the same workgroup-local index)."""
    a = actions.reshape(actions.shape[0], E, R, 2)
    assert bool((a[1:] != a[:-1]).any(-1).all()), f"{what}: steps t and t + 1 must differ on every row"
    assert bool((a[:, 16:] != a[:, :E - 16]).any(-1).all()), f"{what}: env e and env e + 16 must never agree"


@pytest.mark.parametrize("eps", [EPS_HALF, EPS_ZERO], ids=["eps0.5", "greedy"])
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("R,O,C", SHAPES)
def test_sac_rollout_matches_composed_loop(R, O, C, fast, eps):
    """K = 1, 2 and 13 at the automatic launch shape and at a forced one-wave shape; K = 13 also at max_groups = 3."""
    ref = _reference(R, O, C, fast, eps)
    _assert_in_range(ref["rec"]["actions"], "reference")
    _assert_steps_and_rows_differ(ref["rec"]["actions"], R, f"reference R={R}")
    one_wave, capped = _launches(R)
    for K, launch in [(K, ln) for K in (1, 2, 13) for ln in (None, one_wave)] + [(13, capped)]:
        b = _batch(R, O, C, fast)
        got = _run(b, _pack(), K, eps, fast_noise=fast, launch=launch)
        _check(b, got, ref, K, f"R={R} O={O} K={K} launch={launch}")


def test_sac_rollout_explores_and_samples():
    """What keeps the comparison from being vacuous, at (5, 4, 2), K = 13: 37 x 5 x 13 = 2405 acting rows.
    Epsilon 0.5 against epsilon 0: the closed loop feeds on its own actions, so two windows that differ in epsilon act
    on different observations from step 1 on; the rows are therefore compared on the SAME observations -- sac_act
    under epsilon 0 on what every step of the epsilon-0.5 window acted on (same row, step and seed: the sampled
    action that row would have been given). Taking it is a 50 % event per row: between 25 % and 75 % of 2405 rows
    is more than 24 standard deviations (sqrt(2405) / 2 = 24.5 rows) wide on either side. The window's step 0,
    where both windows do act on the same rows, is also compared directly.
    Sampled against deterministic: the noise moves more than 99 % of the rows (sigma = exp(ls) of a seeded head is
    of order 1, a draw of exactly 0 has probability 2^-24)."""
    from distributional_rl_decision_and_control_amd.fused_sac import sac_act
    R, O, C = 5, 4, 2
    NT = E * R
    b = _batch(R, O, C)
    half = _run(b, _pack(), KMAX, EPS_HALF, fast_noise=True)
    ref = _reference(R, O, C, True, EPS_HALF)
    _check(b, half, ref, KMAX, "eps 0.5")
    assert half.actions.shape[0] * NT >= 2000
    sampled = torch.zeros_like(half.actions)
    eps_out = torch.zeros((NT, 2), dtype=torch.float32, device="cuda")
    for t in range(KMAX):
        step = torch.full((1,), STEP0 + t, dtype=torch.int64, device="cuda")
        sac_act(_pack(), ref["acted"][t], sampled[t], eps_out, step, *EPS_ZERO, POLICY_SEED)
    took = (half.actions == sampled).all(-1)
    frac = float(took.double().mean())
    print(f"rows that carry the sampled action at epsilon 0.5: {frac:.4f} of {took.numel()}")
    assert 0.25 <= frac <= 0.75
    b = _batch(R, O, C)
    zero = _run(b, _pack(), KMAX, EPS_ZERO, fast_noise=True)
    _same(zero.actions[0], sampled[0], "step 0 of the epsilon-0 window is the sampled action")
    f0 = float((half.actions[0] == zero.actions[0]).all(-1).double().mean())
    print(f"step 0: {f0:.4f} of {NT} rows agree between the epsilon-0.5 and the epsilon-0 window")
    assert 0.25 <= f0 <= 0.75
    _assert_steps_and_rows_differ(zero.actions, R, "sampled window")
    _assert_steps_and_rows_differ(half.actions, R, "epsilon 0.5 window")
    b = _batch(R, O, C)
    det = _run(b, _pack(), KMAX, EPS_ZERO, fast_noise=True, deterministic=True)
    moved = float((zero.actions != det.actions).any(-1).double().mean())
    print(f"rows the noise moved: {moved:.4f}")
    assert moved > 0.99
    # the Actor's route (the mean rows of the head through the Actor's output layer) is not what a SacActorPack gets:
    # the mean action of step 0 is scale * atan(mu), finite and inside the squash, and the sampled one is not it
    _assert_in_range(det.actions, "deterministic")
    assert bool((zero.actions[0] != det.actions[0]).any(-1).all()), "step 0: every row's sample differs from its mean"


@pytest.mark.parametrize("ar", [False, True], ids=["plain", "auto-reset"])
@pytest.mark.parametrize("eps", [EPS_HALF, EPS_ZERO], ids=["eps0.5", "greedy"])
def test_sac_rollout_deterministic(eps, ar):
    """deterministic=True is the composed loop with eps_in = zeros: z = mu, the epsilon schedule still applies."""
    R, O, C = 5, 4, 2
    ref = _reference(R, O, C, True, eps, ar=ar, deterministic=True)
    for K, launch in ((1, None), (KMAX, None), (KMAX, _launches(R)[0])):
        b = _batch(R, O, C, ending=ar)
        got = _run(b, _pack(), K, eps, cfg=_cfg(R, O, C) if ar else None, fast_noise=True, launch=launch,
                   deterministic=True)
        _check(b, got, ref, K, f"deterministic eps={eps} ar={ar} K={K} launch={launch}")
    if eps is EPS_ZERO and not ar:   # nothing random is left: the same observation row gives the same action
        a, x = ref["rec"]["actions"][0], ref["acted"][0]
        same_rows = (x[0] == x).all(-1)
        assert bool((a[same_rows] == a[0]).all())


def test_sac_rollout_f32_build():
    """SacActorPack(operands="f32") runs the f32-operand library (fragments from L2, no LDS weight images) against
    that library's own composed loop."""
    R, O, C = 5, 4, 2
    pack = _pack("f32")
    for eps, det in ((EPS_HALF, False), (EPS_ZERO, False), (EPS_HALF, True)):
        ref = _reference(R, O, C, True, eps, "f32", deterministic=det)
        for K, launch in ((1, None), (13, None), (13, _launches(R)[0])):
            b = _batch(R, O, C, True)
            got = _run(b, pack, K, eps, fast_noise=True, launch=launch, deterministic=det)
            _check(b, got, ref, K, f"f32 eps={eps} det={det} K={K} launch={launch}")
    ref = _reference(R, O, C, True, EPS_HALF, "f32", ar=True)
    b = _batch(R, O, C, ending=True)
    got = _run(b, pack, KMAX, EPS_HALF, cfg=_cfg(R, O, C), fast_noise=True)
    _check(b, got, ref, KMAX, "f32 auto-reset")


@pytest.mark.parametrize("masked", [False, True])
def test_sac_rollout_hold_done(masked):
    """hold_done is the chain of rounds whose env_mask drops an env after its env_done; `masked`: on top of a
    caller's mask that leaves every fourth env (and one whole workgroup's envs) out. An env that is off takes no
    action: its rows of the actions record keep their pre-fill."""
    mask = None
    if masked:
        mask = torch.ones(E, dtype=torch.uint8, device="cuda")
        mask[::4] = 0
        mask[8:16] = 0
    ref = _loop(_batch(5, 4, 0, ending=True), _pack(), KMAX, EPS_HALF, hold=True, env_mask=mask)
    b = _batch(5, 4, 0, ending=True)
    got = _run(b, _pack(), KMAX, EPS_HALF, hold_done=True, fast_noise=True, env_mask=mask)
    _check(b, got, ref, KMAX, f"hold masked={masked}", steps=ref["steps_run"])
    on = np.ones(E, bool) if mask is None else mask.cpu().numpy() != 0
    expect = got.steps_run.cpu().numpy()
    assert (expect[~on] == 0).all() and (expect[on] >= 1).all() and (expect[on] <= 6).all()   # episode_limit 5
    assert len(set(expect[on])) >= 3, "the envs must end at different steps"
    idle_r = np.repeat(np.arange(KMAX)[:, None] >= expect[None, :], 5, axis=1)
    assert not got.actions.cpu().numpy()[idle_r].any(), "idle rows of the actions record keep their pre-fill"


def test_sac_rollout_env_mask():
    """A caller's env_mask without hold_done: masked envs neither act nor step."""
    mask = torch.ones(E, dtype=torch.uint8, device="cuda")
    mask[1::3] = 0
    mask[16:24] = 0
    K = 5
    ref = _loop(_batch(5, 4, 2), _pack(), K, EPS_HALF, env_mask=mask)
    b = _batch(5, 4, 2)
    got = _run(b, _pack(), K, EPS_HALF, fast_noise=True, env_mask=mask)
    _check(b, got, ref, K, "env_mask", steps=ref["steps_run"])
    assert not got.actions[:, (mask == 0).repeat_interleave(5)].any()


@pytest.mark.parametrize("deterministic", [False, True])
def test_sac_rollout_fallback_per_robot_parameters(deterministic):
    """Per-robot parameters run K x (asvrl_sac_act, single step, record launches) inside the call: the same records
    and finals, and the caller's step counter is left alone (_run asserts it)."""
    K = 3
    ref = _loop(_batch(5, 4, 2, robot_params=True), _pack(), K, EPS_HALF, deterministic=deterministic)
    b = _batch(5, 4, 2, robot_params=True)
    got = _run(b, _pack(), K, EPS_HALF, fast_noise=True, deterministic=deterministic)
    _check(b, got, ref, K, "robot_params")
    _assert_in_range(got.actions, "robot_params")


def test_sac_rollout_fallback_layout_2():
    """layout = 2 (the sweep step) takes the K-launch form too; its composed loop steps at the same layout."""
    from distributional_rl_decision_and_control_amd import _abi
    K, launch = 4, (_abi.ENV_LAYOUT_SWEEP, 0, 0)
    ref = _loop(_batch(5, 4, 2), _pack(), K, EPS_HALF, launch=launch)
    b = _batch(5, 4, 2)
    got = _run(b, _pack(), K, EPS_HALF, fast_noise=True, launch=launch)
    _check(b, got, ref, K, "layout 2")
    _assert_steps_and_rows_differ(got.actions, 5, "layout 2")


@pytest.mark.parametrize("eps", [EPS_HALF, EPS_ZERO], ids=["eps0.5", "greedy"])
def test_sac_rollout_auto_reset(eps):
    """episode_limit 5 and ep_ts preset to e % 9: every env ends at least twice in 13 steps; obs_prev, pushed and
    resets are compared with the records."""
    R, O, C = 5, 4, 2
    ref = _reference(R, O, C, True, eps, ar=True)
    assert ref["resets_after"][-1].min().item() >= 2, "every env must end at least twice"
    assert int(ref["pushed"].min().item()) > 0
    for launch in (None,) + _launches(R):
        b = _batch(R, O, C, ending=True)
        got = _run(b, _pack(), KMAX, eps, cfg=_cfg(R, O, C), fast_noise=True, launch=launch)
        _check(b, got, ref, KMAX, f"auto-reset eps={eps} launch={launch}")
        _assert_in_range(got.actions, "auto-reset")


def test_sac_rollout_auto_reset_fallback():
    """Per-robot parameters: the K-launch form with the two reset launches behind every step."""
    R, O, C, K = 5, 4, 2, 7
    cfg = _cfg(R, O, C)
    ref = _loop(_batch(R, O, C, ending=True, robot_params=True), _pack(), K, EPS_HALF, cfg=cfg, two_launch=True)
    assert ref["resets_after"][-1].sum().item() > 0
    b = _batch(R, O, C, ending=True, robot_params=True)
    got = _run(b, _pack(), K, EPS_HALF, cfg=cfg, fast_noise=True)
    _check(b, got, ref, K, "auto-reset robot_params")


@pytest.mark.parametrize("ar", [False, True], ids=["plain", "auto-reset"])
def test_sac_rollout_split_window(ar):
    """A window of 6 and then one of 7 at STEP0 + 6 (noise, reset and observation counters moved on by 6 too) are
    the window of 13: the draws are keyed by the absolute step, not by the position in the window."""
    R, O, C = 5, 4, 2
    cfg = _cfg(R, O, C) if ar else None
    ref = _reference(R, O, C, True, EPS_HALF, ar=ar)
    b = _batch(R, O, C, ending=ar)
    first = _run(b, _pack(), 6, EPS_HALF, cfg=cfg, fast_noise=True)
    _check(b, first, ref, 6, "first 6")
    second = _run(b, _pack(), 7, EPS_HALF, cfg=cfg, t0=6, fast_noise=True)
    _check(b, second, ref, 7, "then 7", t0=6)
    b = _batch(R, O, C, ending=ar)
    whole = _run(b, _pack(), KMAX, EPS_HALF, cfg=cfg, fast_noise=True)
    _same(torch.cat([first.actions, second.actions]), whole.actions, "6 + 7 against 13")


# ------------------------------------------------------------------ the Python surface
def _vec(is_continuous):
    from distributional_rl_decision_and_control_amd.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(E, num_robots=5, num_obs=4, min_start_goal_dis=20.0, seed=5, is_continuous=is_continuous)
    env.reset()
    return env


@pytest.mark.parametrize("deterministic", [False, True])
def test_vec_env_takes_a_sac_pack_on_a_continuous_env(deterministic):
    from distributional_rl_decision_and_control_amd.fused_sac import sac_act
    K = 4
    pack = _pack()
    twin = _vec(True)
    act64 = torch.zeros((E * 5, 2), dtype=torch.float64, device="cuda")
    eps_out = torch.zeros((E * 5, 2), dtype=torch.float32, device="cuda")
    eps_in = torch.zeros_like(eps_out) if deterministic else None
    for t in range(K):
        sac_act(pack, twin.obs_cur, act64, eps_out, twin.counter, *EPS_HALF, POLICY_SEED, eps_in=eps_in)
        twin.step(act64)
        twin.advance_device()
    env = _vec(True)
    rec = env.policy_rollout(pack, K, hold_done=False, keep=("reward", "actions"), eps=EPS_HALF,
                             policy_seed=POLICY_SEED, deterministic=deterministic)
    assert rec.reward.shape == (K, E * 5) and rec.actions.shape == (K, E * 5, 2)
    _same(env.obs_next, twin.obs_next, "obs_next")
    _same(env.counter, twin.counter, "counter")
    for n in ("rs", "rflags", "ep_ts", "reward", "done", "info", "env_done"):
        _same(getattr(env.batch, n), getattr(twin.batch, n), n)
    _same(rec.actions[-1], act64, "last actions record")


def test_pack_env_and_deterministic_must_match():
    from distributional_rl_decision_and_control_amd.fused_mlp import MlpPack
    from distributional_rl_decision_and_control_amd.policy.AC_IQN_model import AC_IQN_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    with pytest.raises(ValueError, match="continuous"):
        _vec(False).policy_rollout(_pack(), 2)
    pol = AC_IQN_Policy(**DEFAULT_NET, value_ranges_of_action=[[-1, 1], [-1, 1]], device="cuda", seed=100)
    with pytest.raises(ValueError, match="deterministic"):
        _vec(True).policy_rollout(MlpPack(pol.actor, "actor"), 2, deterministic=True)
    b = _batch(5, 4, 2)
    with pytest.raises(ValueError, match="deterministic"):
        b.policy_rollout(MlpPack(pol.actor, "actor"), 2, b.obs, deterministic=True)


# ------------------------------------------------------------------ graph capture
def test_sac_rollout_graph_capture():
    """One call with caller-supplied records captured in a graph on a single stream and replayed from the restored
    state gives the eager call's records."""
    R, O, C, K = 5, 4, 2, 5
    pack = _pack()
    b = _batch(R, O, C)
    state = {n: getattr(b, n).clone() for n in ("rs", "rflags", "ep_ts", "obs", "stats")}
    spec = _specs(b)

    def records():
        rec = {n: torch.full((K,) + spec[n][0], spec[n][2], dtype=spec[n][1], device="cuda") for n in RECORDS}
        rec["steps_run"] = torch.zeros(E, dtype=torch.int32, device="cuda")
        return rec

    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")

    def call(rec):
        b.policy_rollout(pack, K, b.obs, keep=rec, step_dev=step, eps=EPS_HALF, policy_seed=POLICY_SEED,
                         trainer_deactivate=True, seed=11, counter=C0, gamma=GAMMA, fast_noise=True)

    eager = records()
    call(eager)
    torch.cuda.synchronize()
    finals = _finals(b)
    assert bool((eager["steps_run"] == K).all())

    def restore():
        for n, t in state.items():
            getattr(b, n).copy_(t)

    restore()
    rec = records()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(rec)
    restore()   # capturing ran nothing: the records are still at their pre-fill
    g.replay()
    torch.cuda.synchronize()
    for n in RECORDS + ("steps_run",):
        _same(rec[n], eager[n], f"replayed record {n}")
    for n in FINALS:
        _same(getattr(b, n), finals[n], f"replayed final {n}")
