"""GPU: the closed-loop rollout windows under Rainbow_Policy (asvrl_rainbow_rollout / asvrl_rainbow_rollout_ar: per step
the window form of the act pass, asvrl_rainbow_net_act_ex, and the env step, enqueued by one call) against the
hand-composed loop they replace, bit for bit: for t < K, fused_rainbow.rainbow_act -- the existing entry point -- on
the current observation with the step tensor at STEP0 + t, the single env step with is_continuous=False at noise
counter C0 + t on those indices and, with the auto-reset, reset_observe on env_done & mask at (RC + t, OC + t). Every
record of every step (the actions among them; obs_prev, pushed and resets with the auto-reset), the steps every env
took and every final array are compared with atol = rtol = 0, NaN = NaN (the stats' return sum, an atomic sum, within
1e-12 as in the predecessors' tests). E = 37 envs of 3 to 5 robots in one parameter group: 185 act rows, a part-filled
last 32-row tile, and robot slots no robot fills. The weights are a seeded Rainbow_Policy, in training mode (noisy)
and in eval mode (mu only)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, R, O, C = 37, 5, 4, 2
A = 25
K = 5
GAMMA = 0.99
STEP0 = 7          # the policy's step counter at the window's start
POLICY_SEED = 4242
C0, RC, OC = 1, 0x40000000, 0x80000000
RECORDS = ("reward", "done", "info", "env_done", "obs", "obj_cnt", "rs", "actions")
AR_RECORDS = RECORDS + ("obs_prev",)
FINALS = ("rs", "rflags", "n_robots", "n_obs", "n_cores", "ep_ts", "obstacles", "cores", "obs", "obs64", "obj_cnt",
          "reward", "done", "info", "env_done")   # + stats
EPS_HALF = (1.0, 1.0, 1.0, 0.5, 0.5)    # past the exploration fraction from step 1 on: epsilon = 0.5
EPS_ZERO = (1.0, 1.0, 1.0, 0.0, 0.0)    # greedy


def _same(got, ref, what):
    torch.testing.assert_close(got, ref, rtol=0, atol=0, equal_nan=True, msg=lambda m: f"{what}: {m}")


@functools.lru_cache(maxsize=None)
def _net():
    from distributional_rl_decision_and_control_amd.policy.Rainbow_model import Rainbow_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    return Rainbow_Policy(**DEFAULT_NET, action_size=A, atoms=51, device="cuda", seed=100).to("cuda")


@functools.lru_cache(maxsize=None)
def _pack(operands="bf16", noisy=True):
    from distributional_rl_decision_and_control_amd.fused_rainbow import RainbowPack
    return RainbowPack(_net(), operands, noisy=noisy)


def _cfg():
    from distributional_rl_decision_and_control_amd.device_env import reset_cfg
    return reset_cfg(R, O, C, 20.0, width=55.0, height=55.0)


def _batch(limit=None):
    """A device-reset batch whose envs hold 3, 4 or 5 robots, with its observation in b.obs; the same call gives the
    same batch. limit: the episode limit (every env then ends inside a 5-step window)."""
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.device_env import DeviceEnvBatch
    b = DeviceEnvBatch(E, R, O, C, obs64=True, params=_abi.params_from(episode_limit=limit) if limit else None)
    b.reset(_cfg(), seed=11)
    b.n_robots.copy_(3 + torch.arange(E, dtype=b.n_robots.dtype, device="cuda") % 3)
    b.step(None, do_dynamics=False, seed=11, counter=0, fast_noise=True)
    return b


def _finals(b):
    return {k: getattr(b, k).clone() for k in FINALS + ("stats",)}


def _specs(b):
    spec = b._record_specs()
    NT = b.n_envs * b.max_robots
    spec["actions"] = ((NT, 2), torch.float64, 0)
    spec["obs_prev"] = ((NT, 40), torch.float32, 0)
    return spec


def _loop(b, pack, n, eps, cfg=None, hold=False, env_mask=None):
    """The composed reference: n rounds of rainbow_act on b.obs (which the step rewrites in place) with the step
    tensor at STEP0 + t and b.step(is_continuous=False) at counter C0 + t; hold: the mask drops an env after its
    env_done; cfg (the auto-reset): reset_observe(env_done & mask) behind every step. Returns the records as
    policy_rollout() lays them out (rows of steps an env did not take at the pre-fill), steps_run, pushed [n], the
    resets and the finals after every step."""
    from distributional_rl_decision_and_control_amd.fused_rainbow import rainbow_act
    ar = cfg is not None
    spec = _specs(b)
    names = AR_RECORDS if ar else RECORDS
    rec = {k: torch.full((n,) + spec[k][0], spec[k][2], dtype=spec[k][1], device="cuda") for k in names}
    mask = env_mask.clone() if env_mask is not None else (torch.ones(E, dtype=torch.uint8, device="cuda") if hold else None)
    slot = torch.arange(E * R, device="cuda") % R
    act64 = torch.zeros((E * R, 2), dtype=torch.float64, device="cuda")
    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")
    steps_run = torch.zeros(E, dtype=torch.int32, device="cuda")
    pushed = torch.zeros(n, dtype=torch.int32, device="cuda")
    resets = torch.zeros(E, dtype=torch.int32, device="cuda")
    finals, resets_after = [], []
    for t in range(n):
        on_e = (mask != 0) if mask is not None else torch.ones(E, dtype=torch.bool, device="cuda")
        on_r = on_e.repeat_interleave(R)
        if ar:
            rec["obs_prev"][t][on_r] = b.obs[on_r]
        rainbow_act(pack, b.obs, act64, step, *eps, POLICY_SEED)
        step += 1
        rs_r = on_r & (slot < b.n_robots.repeat_interleave(R))   # the rs record holds the robot slots in use
        b.step(act64, is_continuous=False, seed=11, counter=C0 + t, trainer_deactivate=True, gamma=GAMMA,
               env_mask=mask, fast_noise=True)
        for k in RECORDS:
            src = act64 if k == "actions" else getattr(b, k)
            if k == "rs":
                rec[k][t][:, rs_r] = src[:, rs_r]
            else:
                sel = on_e if k == "env_done" else on_r
                rec[k][t][sel] = src[sel]
        steps_run += on_e.int()
        if hold:
            mask = mask * (b.env_done == 0).to(torch.uint8)
        if ar:
            pushed[t] = int((b.obj_cnt[on_r] >= 0).sum())
            m = (b.env_done * on_e.to(torch.uint8)).contiguous()
            resets += m.int()
            b.reset_observe(cfg, m, seed=11, counter=RC + t, obs_counter=OC + t, obs=b.obs, obj_cnt=b.obj_cnt,
                            fast_noise=True)
        finals.append(_finals(b))
        resets_after.append(resets.clone())
    return dict(rec=rec, steps_run=steps_run, pushed=pushed, resets_after=resets_after, finals=finals)


def _run(b, pack, n, eps, cfg=None, **kw):
    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")
    ar = dict(cfg=cfg, reset_counter=RC, obs_counter=OC) if cfg is not None else None
    got = b.policy_rollout(pack, n, b.obs, keep=AR_RECORDS if cfg is not None else RECORDS, step_dev=step, eps=eps,
                           policy_seed=POLICY_SEED, trainer_deactivate=True, seed=11, counter=C0, gamma=GAMMA,
                           fast_noise=True, auto_reset=ar, **kw)
    assert int(step.item()) == STEP0, "the caller's step counter is only read"
    return got


def _check(b, got, ref, n, what, steps=None):
    """The window's n steps against the first n rounds of the reference."""
    ar = "obs_prev" in ref["rec"]
    for k in (AR_RECORDS if ar else RECORDS):
        _same(getattr(got, k), ref["rec"][k][:n], f"{what}: record {k}")
    if ar:
        _same(got.pushed, ref["pushed"][:n], f"{what}: pushed")
        _same(got.resets, ref["resets_after"][n - 1], f"{what}: resets")
    _same(got.steps_run, steps if steps is not None else torch.full((E,), n, dtype=torch.int32, device="cuda"),
          f"{what}: steps_run")
    final = ref["finals"][n - 1]
    for k in FINALS:
        _same(getattr(b, k), final[k], f"{what}: final {k}")
    s, r = b.stats.cpu().numpy(), final["stats"].cpu().numpy()
    assert np.array_equal(s[1:], r[1:]), f"{what}: stats counts {s} vs {r}"
    assert abs(s[0] - r[0]) <= 1e-12 * max(1.0, abs(r[0])), f"{what}: stats return sum {s[0]} vs {r[0]}"


def _assert_indices(actions, what):
    """Every recorded action is an exact integer in 0..A-1 with column 1 equal to 0.0."""
    a0 = actions[..., 0]
    assert bool(((a0 >= 0) & (a0 <= A - 1) & (a0 == a0.round())).all()), f"{what}: action indices"
    assert bool((actions[..., 1] == 0.0).all()), f"{what}: column 1"


@functools.lru_cache(maxsize=None)
def _reference(operands, noisy, eps, ar=False):
    """One 5-round loop per case: its first n rounds are the reference of an n-step window."""
    return _loop(_batch(3 if ar else None), _pack(operands, noisy), K, eps, cfg=_cfg() if ar else None)


@pytest.mark.parametrize("eps", [EPS_HALF, EPS_ZERO], ids=["eps0.5", "greedy"])
@pytest.mark.parametrize("noisy", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_rainbow_rollout_matches_composed_loop(ops, noisy, eps):
    """K = 5 and 2 at the automatic step shape, K = 5 also at layout 2 (the sweep step)."""
    ref = _reference(ops, noisy, eps)
    _assert_indices(ref["rec"]["actions"], "reference")
    assert int(_batch().n_robots.min()) == 3 and int(_batch().n_robots.max()) == 5
    assert ref["rec"]["actions"][..., 0].unique().numel() >= 3, "the loop takes several actions"
    for n, launch in ((K, None), (2, None), (K, (2, 0, 0))):
        b = _batch()
        got = _run(b, _pack(ops, noisy), n, eps, launch=launch)
        _check(b, got, ref, n, f"{ops} noisy={noisy} K={n} launch={launch}")
        _assert_indices(got.actions, f"K={n}")


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_rainbow_rollout_hold_done_and_env_mask(ops):
    """hold_done on top of a caller's mask that leaves every fourth env (and eight in a row) out: the chain of rounds
    whose env_mask drops an env after its env_done. An env that is off takes no action: its rows of the actions
    record keep their pre-fill. episode_limit 3: every env that is on ends inside the window."""
    mask = torch.ones(E, dtype=torch.uint8, device="cuda")
    mask[::4] = 0
    mask[8:16] = 0
    ref = _loop(_batch(3), _pack(ops), K, EPS_HALF, hold=True, env_mask=mask)
    b = _batch(3)
    got = _run(b, _pack(ops), K, EPS_HALF, hold_done=True, env_mask=mask)
    _check(b, got, ref, K, "hold_done + env_mask", steps=ref["steps_run"])
    on = mask.cpu().numpy() != 0
    steps = got.steps_run.cpu().numpy()
    assert (steps[~on] == 0).all() and (steps[on] >= 1).all() and (steps[on] < K).all(), steps
    idle_r = np.repeat(np.arange(K)[:, None] >= steps[None, :], R, axis=1)
    assert not got.actions.cpu().numpy()[idle_r].any(), "idle rows of the actions record keep their pre-fill"


@pytest.mark.parametrize("eps", [EPS_HALF, EPS_ZERO], ids=["eps0.5", "greedy"])
@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_rainbow_rollout_auto_reset(ops, eps):
    """episode_limit 3: every env restarts inside the window of 5; obs_prev, pushed and resets are compared with the
    records."""
    ref = _reference(ops, True, eps, ar=True)
    _assert_indices(ref["rec"]["actions"], "reference")
    assert ref["resets_after"][-1].min().item() >= 1 and ref["resets_after"][-1].sum().item() >= E
    assert int(ref["pushed"].min().item()) > 0
    b = _batch(3)
    got = _run(b, _pack(ops), K, eps, cfg=_cfg())
    assert int(got.resets.sum().item()) >= E and int(got.resets.min().item()) >= 1, "every env restarts in the window"
    _check(b, got, ref, K, f"auto-reset {ops} eps={eps}")
    _assert_indices(got.actions, "auto-reset")


def test_policy_rollout_value_errors():
    b = _batch()
    with pytest.raises(ValueError, match="cvar"):
        b.policy_rollout(_pack(), 2, b.obs, cvar=0.5)
    with pytest.raises(ValueError, match="deterministic"):
        b.policy_rollout(_pack(), 2, b.obs, deterministic=True)


# ------------------------------------------------------------------ VecMarineNavEnv.policy_rollout
def _vec(is_continuous):
    from distributional_rl_decision_and_control_amd.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(E, num_robots=5, num_obs=4, min_start_goal_dis=20.0, seed=5, is_continuous=is_continuous)
    env.reset()
    return env


def test_vec_env_takes_a_rainbow_pack_on_a_discrete_env():
    from distributional_rl_decision_and_control_amd.fused_rainbow import rainbow_act
    n = 4
    pack = _pack()
    twin = _vec(False)
    act64 = torch.zeros((E * 5, 2), dtype=torch.float64, device="cuda")
    for t in range(n):
        rainbow_act(pack, twin.obs_cur, act64, twin.counter, *EPS_HALF, POLICY_SEED)
        twin.step(act64)
        twin.advance_device()
    env = _vec(False)
    rec = env.policy_rollout(pack, n, hold_done=False, keep=("reward", "actions"), eps=EPS_HALF,
                             policy_seed=POLICY_SEED)
    assert rec.reward.shape == (n, E * 5) and rec.actions.shape == (n, E * 5, 2)
    _assert_indices(rec.actions, "vec env")
    _same(env.obs_next, twin.obs_next, "obs_next")
    _same(env.counter, twin.counter, "counter")
    for k in ("rs", "rflags", "ep_ts", "reward", "done", "info", "env_done"):
        _same(getattr(env.batch, k), getattr(twin.batch, k), k)
    _same(rec.actions[-1], act64, "last actions record")
    with pytest.raises(ValueError, match="RainbowPack.*is_continuous=True"):
        _vec(True).policy_rollout(pack, 2)
    with pytest.raises(ValueError, match="cvar"):
        _vec(False).policy_rollout(pack, 2, cvar=0.5)
    with pytest.raises(ValueError, match="deterministic"):
        _vec(False).policy_rollout(pack, 2, deterministic=True)


# ------------------------------------------------------------------ graph capture
def test_rainbow_rollout_graph_capture():
    """One call of a K = 3 window with caller-supplied records captured in a graph on a single stream and replayed
    from the restored state gives the eager call's bits: the per-step launches and the call's stream-ordered scratch
    are captured as they are enqueued."""
    n = 3
    pack = _pack()
    b = _batch()
    state = {k: getattr(b, k).clone() for k in ("rs", "rflags", "ep_ts", "obs", "stats")}
    spec = _specs(b)

    def records():
        rec = {k: torch.full((n,) + spec[k][0], spec[k][2], dtype=spec[k][1], device="cuda") for k in RECORDS}
        rec["steps_run"] = torch.zeros(E, dtype=torch.int32, device="cuda")
        return rec

    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")

    def call(rec):
        b.policy_rollout(pack, n, b.obs, keep=rec, step_dev=step, eps=EPS_HALF, policy_seed=POLICY_SEED,
                         trainer_deactivate=True, seed=11, counter=C0, gamma=GAMMA, fast_noise=True)

    eager = records()
    call(eager)
    torch.cuda.synchronize()
    finals = _finals(b)
    _assert_indices(eager["actions"], "eager")
    assert bool((eager["steps_run"] == n).all())

    def restore():
        for k, t in state.items():
            getattr(b, k).copy_(t)

    restore()
    rec = records()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(rec)
    restore()   # capturing ran nothing: the records are still at their pre-fill
    g.replay()
    torch.cuda.synchronize()
    for k in RECORDS + ("steps_run",):
        _same(rec[k], eager[k], f"replayed record {k}")
    for k in FINALS:
        _same(getattr(b, k), finals[k], f"replayed final {k}")
