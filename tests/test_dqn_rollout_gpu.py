"""GPU: the closed-loop rollout windows under DQN_Policy (asvrl_dqn_rollout / asvrl_dqn_rollout_ar,
env_policy_rollout_kernel's kPolDqn instantiations) against the composed loop of the calls they replace, bit for
bit: for t < K, fused_dqn.dqn_act on the current observation at step counter STEP0 + t, the single env step with
is_continuous=False at noise counter C0 + t on those indices and, with the auto-reset, reset_observe on
env_done & mask at (RC + t, OC + t). Every record of every step (the actions among them; obs_prev, pushed and resets
with the auto-reset), the steps every env took and every final array are compared with atol = rtol = 0 (the stats'
return sum, an atomic sum, within 1e-12 as in the Actor's tests). E = 37 envs: the last workgroup and, at 5 and 12
robots, the last 32-row tile are partial. The weights are a seeded DQN_Policy."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = 37
A = 25
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
EPS_ZERO = (1.0, 1.0, 1.0, 0.0, 0.0)    # greedy
SHAPES = [(1, 0, 0), (5, 4, 2), (12, 8, 0)]


def _same(got, ref, what):
    torch.testing.assert_close(got, ref, rtol=0, atol=0, equal_nan=True, msg=lambda m: f"{what}: {m}")


@functools.lru_cache(maxsize=None)
def _net():
    from distributional_rl_decision_and_control_amd.policy.DQN_model import DQN_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    return DQN_Policy(**DEFAULT_NET, action_size=A, device="cuda", seed=100).to("cuda")


@functools.lru_cache(maxsize=None)
def _pack(operands="bf16"):
    """The seeded DQN_Policy's packed images."""
    from distributional_rl_decision_and_control_amd.fused_dqn import DqnPack
    return DqnPack(_net(), operands)


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


def _loop(b, pack, K, eps, cfg=None, hold=False, launch=None, env_mask=None, fast=True, two_launch=False):
    """The composed reference: K rounds of dqn_act on b.obs (which the step rewrites in place) at step STEP0 + t and
    b.step(is_continuous=False) at counter C0 + t; hold: the mask drops an env after its env_done; cfg (the
    auto-reset): reset_observe(env_done & mask) behind every step. Returns a dict of the records as policy_rollout()
    lays them out (rows of steps an env did not take at the pre-fill), steps_run, pushed [K], the resets and finals
    after every step."""
    from distributional_rl_decision_and_control_amd.fused_dqn import dqn_act
    ar = cfg is not None
    spec = _specs(b)
    names = AR_RECORDS if ar else RECORDS
    rec = {n: torch.full((K,) + spec[n][0], spec[n][2], dtype=spec[n][1], device="cuda") for n in names}
    R = b.max_robots
    mask = env_mask.clone() if env_mask is not None else (torch.ones(E, dtype=torch.uint8, device="cuda") if hold else None)
    slot = torch.arange(E * R, device="cuda") % R
    act64 = torch.zeros((E * R, 2), dtype=torch.float64, device="cuda")
    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")
    steps_run = torch.zeros(E, dtype=torch.int32, device="cuda")
    pushed = torch.zeros(K, dtype=torch.int32, device="cuda")
    resets = torch.zeros(E, dtype=torch.int32, device="cuda")
    finals, resets_after = [], []
    for t in range(K):
        on_e = (mask != 0) if mask is not None else torch.ones(E, dtype=torch.bool, device="cuda")
        on_r = on_e.repeat_interleave(R)
        if ar:
            rec["obs_prev"][t][on_r] = b.obs[on_r]
        dqn_act(pack, b.obs, act64, step, *eps, POLICY_SEED)
        step += 1
        rs_r = on_r & (slot < b.n_robots.repeat_interleave(R)) if ar else on_r
        b.step(act64, is_continuous=False, seed=11, counter=C0 + t, trainer_deactivate=True, gamma=GAMMA,
               env_mask=mask, launch=launch, fast_noise=fast)
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
    return dict(rec=rec, steps_run=steps_run, pushed=pushed, resets_after=resets_after, finals=finals)


def _run(b, pack, K, eps, cfg=None, **kw):
    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")
    ar = dict(cfg=cfg, reset_counter=RC, obs_counter=OC) if cfg is not None else None
    got = b.policy_rollout(pack, K, b.obs, keep=AR_RECORDS if cfg is not None else RECORDS, step_dev=step, eps=eps,
                           policy_seed=POLICY_SEED, trainer_deactivate=True, seed=11, counter=C0, gamma=GAMMA,
                           auto_reset=ar, **kw)
    assert int(step.item()) == STEP0, "the caller's step counter is only read"
    return got


def _check(b, got, ref, K, what, steps=None):
    ar = "obs_prev" in ref["rec"]
    for n in (AR_RECORDS if ar else RECORDS):
        _same(getattr(got, n), ref["rec"][n][:K], f"{what}: record {n}")
    if ar:
        _same(got.pushed, ref["pushed"][:K], f"{what}: pushed")
        _same(got.resets, ref["resets_after"][K - 1], f"{what}: resets")
    _same(got.steps_run, steps if steps is not None else torch.full((E,), K, dtype=torch.int32, device="cuda"),
          f"{what}: steps_run")
    final = ref["finals"][K - 1]
    for n in FINALS:
        _same(getattr(b, n), final[n], f"{what}: final {n}")
    s, r = b.stats.cpu().numpy(), final["stats"].cpu().numpy()
    assert np.array_equal(s[1:], r[1:]), f"{what}: stats counts {s} vs {r}"
    assert abs(s[0] - r[0]) <= 1e-12 * max(1.0, abs(r[0])), f"{what}: stats return sum {s[0]} vs {r[0]}"


def _assert_indices(actions, what):
    """Every recorded action is an exact integer in 0..A-1 with column 1 equal to 0.0."""
    a0 = actions[..., 0]
    assert bool(((a0 >= 0) & (a0 <= A - 1) & (a0 == a0.round())).all()), f"{what}: action indices"
    assert bool((actions[..., 1] == 0.0).all()), f"{what}: column 1"


@functools.lru_cache(maxsize=None)
def _reference(R, O, C, fast, eps, operands="bf16", ar=False):
    """One 13-round loop per case: its first K rounds are the reference of a K-step window."""
    return _loop(_batch(R, O, C, fast, ending=ar), _pack(operands), KMAX, eps, cfg=_cfg(R, O, C) if ar else None,
                 fast=fast)


def _launches(R):
    from distributional_rl_decision_and_control_amd import _abi
    return ((_abi.ENV_LAYOUT_PAIRS, 64, max(1, 64 // R)), (0, 0, 0, 3))


def _assert_not_vacuous(R, O, C, fast, eps, operands="bf16", ar=False):
    acts = _reference(R, O, C, fast, eps, operands, ar)["rec"]["actions"]
    _assert_indices(acts, "reference")
    greedy = _reference(R, O, C, fast, EPS_ZERO, operands, ar)["rec"]["actions"]
    if eps is EPS_HALF:
        # round 0 of both loops acts on the same observation: some rows took the arg-max, some a uniform index
        same = acts[0, :, 0] == greedy[0, :, 0]
        assert bool(same.any()) and bool((~same).any()), "epsilon 0.5 must both exploit and explore"
    assert greedy[..., 0].unique().numel() >= 3, "the greedy records must hold at least three distinct indices"


@pytest.mark.parametrize("eps", [EPS_HALF, EPS_ZERO], ids=["eps0.5", "greedy"])
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("R,O,C", SHAPES)
def test_dqn_rollout_matches_composed_loop(R, O, C, fast, eps):
    """K = 1, 2 and 13 at the automatic launch shape and at a forced one-wave shape; K = 13 also at max_groups = 3."""
    ref = _reference(R, O, C, fast, eps)
    if R > 1:   # (one robot per env: 37 rows, whose greedy indices need not spread)
        _assert_not_vacuous(R, O, C, fast, eps)
    else:
        _assert_indices(ref["rec"]["actions"], "reference")
    one_wave, capped = _launches(R)
    for K, launch in [(K, ln) for K in (1, 2, 13) for ln in (None, one_wave)] + [(13, capped)]:
        b = _batch(R, O, C, fast)
        got = _run(b, _pack(), K, eps, fast_noise=fast, launch=launch)
        _check(b, got, ref, K, f"R={R} O={O} K={K} launch={launch}")
        _assert_indices(got.actions, f"R={R} K={K}")


def test_dqn_rollout_f32_build_and_torch_argmax():
    """DqnPack(operands="f32") runs the f32-operand library (fragments from L2, no LDS weight images) against that
    library's own composed loop; there the first step's greedy actions are torch's arg-max of policy_local on the
    initial observations (rows whose two best Q values are nearly tied are left out, and they must be few)."""
    R, O, C = 5, 4, 2
    pack = _pack("f32")
    for eps in (EPS_HALF, EPS_ZERO):
        ref = _reference(R, O, C, True, eps, "f32")
        _assert_not_vacuous(R, O, C, True, eps, "f32")
        for K, launch in ((2, None), (13, None), (13, _launches(R)[0])):
            b = _batch(R, O, C, True)
            got = _run(b, pack, K, eps, fast_noise=True, launch=launch)
            _check(b, got, ref, K, f"f32 eps={eps} K={K} launch={launch}")
    b = _batch(R, O, C, True)
    x = b.obs.clone()
    got = _run(b, pack, 1, EPS_ZERO, fast_noise=True)
    with torch.no_grad():
        q_ref = _net()((x[:, 0:7], x[:, 7:32].reshape(-1, 5, 5), x[:, 32:37]))
    top2 = q_ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4 * float(q_ref.abs().max())
    assert int(clear.sum()) >= 0.9 * x.shape[0], "too many near ties in the test rows"
    first = got.actions[0, :, 0].long()
    assert torch.equal(first[clear], q_ref.argmax(1)[clear])


@pytest.mark.parametrize("masked", [False, True])
def test_dqn_rollout_hold_done(masked):
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
    expect = np.where(on, np.maximum(1, 5 - np.arange(E) % 9 + 1), 0)   # the end step is known
    assert np.array_equal(got.steps_run.cpu().numpy(), expect)
    idle_r = np.repeat(np.arange(KMAX)[:, None] >= expect[None, :], 5, axis=1)
    assert not got.actions.cpu().numpy()[idle_r].any(), "idle rows of the actions record keep their pre-fill"


def test_dqn_rollout_fallback_per_robot_parameters():
    """Per-robot parameters run K x (asvrl_dqn_act, single step, record launches) inside the call: the same records
    and finals, and the caller's step counter is left alone (_run asserts it)."""
    K = 3
    ref = _loop(_batch(5, 4, 2, robot_params=True), _pack(), K, EPS_HALF)
    b = _batch(5, 4, 2, robot_params=True)
    got = _run(b, _pack(), K, EPS_HALF, fast_noise=True)
    _check(b, got, ref, K, "robot_params")
    _assert_indices(got.actions, "robot_params")


@pytest.mark.parametrize("eps", [EPS_HALF, EPS_ZERO], ids=["eps0.5", "greedy"])
def test_dqn_rollout_auto_reset(eps):
    """episode_limit 5 and ep_ts preset to e % 9: every env ends at least twice in 13 steps; obs_prev, pushed and
    resets are compared with the records."""
    R, O, C = 5, 4, 2
    ref = _reference(R, O, C, True, eps, ar=True)
    _assert_not_vacuous(R, O, C, True, eps, ar=True)
    assert ref["resets_after"][-1].min().item() >= 2, "every env must end at least twice"
    assert int(ref["pushed"].min().item()) > 0
    for launch in (None,) + _launches(R):
        b = _batch(R, O, C, ending=True)
        got = _run(b, _pack(), KMAX, eps, cfg=_cfg(R, O, C), fast_noise=True, launch=launch)
        _check(b, got, ref, KMAX, f"auto-reset eps={eps} launch={launch}")
        _assert_indices(got.actions, "auto-reset")


def test_dqn_rollout_auto_reset_fallback():
    """Per-robot parameters: the K-launch form with the two reset launches behind every step."""
    R, O, C, K = 5, 4, 2, 7
    cfg = _cfg(R, O, C)
    ref = _loop(_batch(R, O, C, ending=True, robot_params=True), _pack(), K, EPS_HALF, cfg=cfg, two_launch=True)
    assert ref["resets_after"][-1].sum().item() > 0
    b = _batch(R, O, C, ending=True, robot_params=True)
    got = _run(b, _pack(), K, EPS_HALF, cfg=cfg, fast_noise=True)
    _check(b, got, ref, K, "auto-reset robot_params")


# ------------------------------------------------------------------ VecMarineNavEnv.policy_rollout
def _vec(is_continuous):
    from distributional_rl_decision_and_control_amd.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(E, num_robots=5, num_obs=4, min_start_goal_dis=20.0, seed=5, is_continuous=is_continuous)
    env.reset()
    return env


def test_vec_env_takes_a_dqn_pack_on_a_discrete_env():
    from distributional_rl_decision_and_control_amd.fused_dqn import dqn_act
    K = 4
    pack = _pack()
    twin = _vec(False)
    act64 = torch.zeros((E * 5, 2), dtype=torch.float64, device="cuda")
    for t in range(K):
        dqn_act(pack, twin.obs_cur, act64, twin.counter, *EPS_HALF, POLICY_SEED)
        twin.step(act64)
        twin.advance_device()
    env = _vec(False)
    rec = env.policy_rollout(pack, K, hold_done=False, keep=("reward", "actions"), eps=EPS_HALF,
                             policy_seed=POLICY_SEED)
    assert rec.reward.shape == (K, E * 5) and rec.actions.shape == (K, E * 5, 2)
    _assert_indices(rec.actions, "vec env")
    _same(env.obs_next, twin.obs_next, "obs_next")
    _same(env.counter, twin.counter, "counter")
    for n in ("rs", "rflags", "ep_ts", "reward", "done", "info", "env_done"):
        _same(getattr(env.batch, n), getattr(twin.batch, n), n)
    _same(rec.actions[-1], act64, "last actions record")


def test_vec_env_pack_and_env_must_match():
    from distributional_rl_decision_and_control_amd.fused_mlp import MlpPack
    from distributional_rl_decision_and_control_amd.policy.AC_IQN_model import AC_IQN_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    pol = AC_IQN_Policy(**DEFAULT_NET, value_ranges_of_action=[[-1, 1], [-1, 1]], device="cuda", seed=100)
    with pytest.raises(ValueError, match="continuous"):
        _vec(False).policy_rollout(MlpPack(pol.actor, "actor"), 2)
    with pytest.raises(ValueError, match="DqnPack.*is_continuous=True"):
        _vec(True).policy_rollout(_pack(), 2)


# ------------------------------------------------------------------ graph capture
def test_dqn_rollout_graph_capture():
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
    _assert_indices(eager["actions"], "eager")
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
