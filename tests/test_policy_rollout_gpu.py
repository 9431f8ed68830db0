"""GPU: the closed-loop policy rollout (asvrl_policy_rollout, env_policy_rollout_kernel<kPolActor>) against the composed
loop of the existing calls it replaces, bit for bit: for t < K, fused_mlp.actor_act on the current observation at step
counter s + t, then the single env step at noise counter c + t on those actions. Every record of every step
(the actions included), the steps every env took and the final state and outputs are compared with atol = rtol =
0 (the stats' return sum, an atomic sum, within 1e-12 as in the open-loop test), over shapes with partial groups,
both Philox precisions, three launch shapes, both operand builds, episode ends with and without hold_done and
under a caller's mask, the sweep fallback, recorded perception noise, VecMarineNavEnv.policy_rollout,
VecTrainer.greedy_episodes and a captured graph. E = 37 envs as in the open-loop tests: the last workgroup is
partial."""
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
RECORDS = ("reward", "done", "info", "env_done", "obs", "obj_cnt", "rs", "actions")
FINALS = ("rs", "rflags", "ep_ts", "obs", "obs64", "obj_cnt", "reward", "done", "info", "env_done")   # + stats
EPS_HALF = (1.0, 1.0, 1.0, 0.5, 0.5)    # past the exploration fraction from step 1 on: epsilon = 0.5
EPS_ZERO = (1.0, 1.0, 1.0, 0.0, 0.0)    # greedy
SHAPES = [(1, 0, 0), (5, 4, 2), (12, 8, 0)]


def _same(got, ref, what):
    # exact, NaN = NaN (phi is NaN in the single step too when COLREGs evaluates an object inside its radius + 1)
    torch.testing.assert_close(got, ref, rtol=0, atol=0, equal_nan=True, msg=lambda m: f"{what}: {m}")


@functools.lru_cache(maxsize=None)
def _pack(operands="bf16"):
    """A seeded random-initialised Actor's packed images."""
    from distributional_rl_decision_and_control_amd.fused_mlp import MlpPack
    from distributional_rl_decision_and_control_amd.policy.AC_IQN_model import AC_IQN_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    pol = AC_IQN_Policy(**DEFAULT_NET, value_ranges_of_action=[[-1, 1], [-1, 1]], device="cuda", seed=100)
    return MlpPack(pol.actor, "actor", operands)


def _fresh(R, O, C, fast, params=None, robot_params=False):
    """A device-reset batch with its reset observation in b.obs; the same call gives the same batch."""
    from distributional_rl_decision_and_control_amd.device_env import DeviceEnvBatch, reset_cfg
    W = 55.0 if R <= 5 else 110.0
    b = DeviceEnvBatch(E, R, O, C, obs64=True, params=params)
    if robot_params:
        b.set_robot_params([b.params] * (E * R))
    b.reset(reset_cfg(R, O, C, 20.0, width=W, height=W), seed=11)
    b.step(None, do_dynamics=False, seed=11, counter=0, fast_noise=fast)
    return b


def _ending_batch(fast=True, **kw):
    """Every env ends inside a 13-step window, at a step that depends on the env: episode_limit 5 and ep_ts
    preset to e % 9 (the open-loop test's recipe)."""
    from distributional_rl_decision_and_control_amd import _abi
    b = _fresh(5, 4, 0, fast, params=_abi.params_from(episode_limit=5), **kw)
    b.ep_ts.copy_(torch.arange(E, dtype=torch.int32, device="cuda") % 9)
    return b


def _finals(b):
    return {k: getattr(b, k).clone() for k in FINALS + ("stats",)}


def _specs(b):
    spec = b._record_specs()
    spec["actions"] = ((b.n_envs * b.max_robots, 2), torch.float64, 0)
    return spec


def _loop(b, pack, K, eps, hold=False, launch=None, env_mask=None, counter=1, noise=None, fast=True):
    """The reference: K rounds of actor_act on b.obs (which the step rewrites in place) at step STEP0 + t and
    b.step at counter + t; with hold, env_mask drops an env after its env_done. Returns the records as
    policy_rollout() lays them out (rows of steps an env did not take at the pre-fill), the steps every env took,
    the finals after each step and every round's full action tensor."""
    from distributional_rl_decision_and_control_amd.fused_mlp import actor_act
    spec = _specs(b)
    rec = {n: torch.full((K,) + spec[n][0], spec[n][2], dtype=spec[n][1], device="cuda") for n in RECORDS}
    mask = env_mask.clone() if env_mask is not None else (torch.ones(E, dtype=torch.uint8, device="cuda") if hold else None)
    steps_run = torch.zeros(E, dtype=torch.int32, device="cuda")
    R = b.max_robots
    act64 = torch.zeros((E * R, 2), dtype=torch.float64, device="cuda")
    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")
    finals, acts = [], []
    for t in range(K):
        actor_act(pack, b.obs, act64, step, *eps, POLICY_SEED)
        b.step(act64, seed=11, counter=counter + t, trainer_deactivate=True, gamma=GAMMA, env_mask=mask,
               launch=launch, noise=None if noise is None else noise[t], fast_noise=fast)
        step += 1
        on_e = (mask != 0) if mask is not None else torch.ones(E, dtype=torch.bool, device="cuda")
        on_r = on_e.repeat_interleave(R)
        for n in RECORDS:
            src = act64 if n == "actions" else getattr(b, n)
            if n == "rs":
                rec[n][t][:, on_r] = src[:, on_r]
            else:
                sel = on_e if n == "env_done" else on_r
                rec[n][t][sel] = src[sel]
        steps_run += on_e.int()
        if hold:
            mask = mask * (b.env_done == 0).to(torch.uint8)
        finals.append(_finals(b))
        acts.append(act64.clone())
    return rec, steps_run, finals, acts


def _run(b, pack, K, eps, **kw):
    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")
    got = b.policy_rollout(pack, K, b.obs, keep=RECORDS, step_dev=step, eps=eps, policy_seed=POLICY_SEED,
                           trainer_deactivate=True, seed=11, counter=1, gamma=GAMMA, **kw)
    assert int(step.item()) == STEP0, "the caller's step counter is only read"
    return got


def _check(b, got, ref_rec, ref_steps, ref_final, K, what):
    for n in RECORDS:
        _same(getattr(got, n), ref_rec[n][:K], f"{what}: record {n}")
    _same(got.steps_run, ref_steps, f"{what}: steps_run")
    for n in FINALS:
        _same(getattr(b, n), ref_final[n], f"{what}: final {n}")
    s, r = b.stats.cpu().numpy(), ref_final["stats"].cpu().numpy()
    assert np.array_equal(s[1:], r[1:]), f"{what}: stats counts {s} vs {r}"
    assert abs(s[0] - r[0]) <= 1e-12 * max(1.0, abs(r[0])), f"{what}: stats return sum {s[0]} vs {r[0]}"


@functools.lru_cache(maxsize=None)
def _reference(R, O, C, fast, eps, operands="bf16"):
    """One 13-round loop per (shape, precision, epsilon): its first K rounds are the reference of K fused steps."""
    recs, _, finals, acts = _loop(_fresh(R, O, C, fast), _pack(operands), KMAX, eps, fast=fast)
    return recs, finals, acts


def _launches(R):
    from distributional_rl_decision_and_control_amd import _abi
    return (None, (_abi.ENV_LAYOUT_PAIRS, 64, max(1, 64 // R)), (0, 0, 0, 3))


@pytest.mark.parametrize("eps", [EPS_HALF, EPS_ZERO], ids=["eps0.5", "greedy"])
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("R,O,C", SHAPES)
def test_policy_rollout_matches_composed_loop(R, O, C, fast, eps):
    """Bit-identity to the 2 K launches: every record (the actions among them), steps_run and all finals; K = 1,
    2, 13; the automatic launch shape, a forced one-wave shape and the automatic shape at max_groups = 3."""
    ref_rec, ref_finals, ref_acts = _reference(R, O, C, fast, eps)
    if eps is EPS_HALF:
        # both branches of the epsilon-greedy draw occur in the reference: some rows took the greedy action (the
        # greedy loop's first round acts on the same observation), some a uniform draw
        greedy = _reference(R, O, C, fast, EPS_ZERO)[2][0]
        same = (ref_acts[0] == greedy).all(1)
        assert bool(same.any()) and bool((~same).any()), "epsilon 0.5 must both exploit and explore"
    for K in (1, 2, 13):
        for launch in _launches(R):
            b = _fresh(R, O, C, fast)
            got = _run(b, _pack(), K, eps, fast_noise=fast, launch=launch)
            _check(b, got, ref_rec, torch.full((E,), K, dtype=torch.int32, device="cuda"), ref_finals[K - 1], K,
                   f"R={R} O={O} K={K} launch={launch}")


def test_policy_rollout_f32_build():
    """MlpPack(operands="f32") runs the f32-operand library (fragments from L2, no LDS weight images): against that
    library's own composed loop."""
    R, O, C = 5, 4, 2
    pack = _pack("f32")
    ref_rec, ref_finals, _ = _reference(R, O, C, True, EPS_HALF, "f32")
    bf_rec = _reference(R, O, C, True, EPS_HALF)[0]
    assert not torch.equal(ref_rec["actions"], bf_rec["actions"]), "the two builds' actors differ in rounding"
    for K in (2, 13):
        for launch in _launches(R):
            b = _fresh(R, O, C, True)
            got = _run(b, pack, K, EPS_HALF, fast_noise=True, launch=launch)
            _check(b, got, ref_rec, torch.full((E,), K, dtype=torch.int32, device="cuda"), ref_finals[K - 1], K,
                   f"f32 K={K} launch={launch}")


def test_policy_rollout_episode_ends_without_hold():
    ref_rec, ref_steps, ref_finals, _ = _loop(_ending_batch(), _pack(), KMAX, EPS_HALF)
    assert bool((ref_rec["env_done"].sum(0) > 0).all()), "every env must end inside the window"
    b = _ending_batch()
    got = _run(b, _pack(), KMAX, EPS_HALF, fast_noise=True)
    _check(b, got, ref_rec, ref_steps, ref_finals[-1], KMAX, "no hold")


@pytest.mark.parametrize("masked", [False, True])
def test_policy_rollout_hold_done(masked):
    """hold_done is the chain of rounds whose env_mask drops an env after its env_done; `masked`: on top of a
    caller's mask that leaves every fourth env (and one whole workgroup's envs) out. An env that is off takes no
    action: its rows of the actions record keep their pre-fill, and a masked env is untouched."""
    mask = None
    if masked:
        mask = torch.ones(E, dtype=torch.uint8, device="cuda")
        mask[::4] = 0
        mask[8:16] = 0
    ref_rec, ref_steps, ref_finals, _ = _loop(_ending_batch(), _pack(), KMAX, EPS_HALF, hold=True, env_mask=mask)
    b = _ending_batch()
    before = _finals(b)
    got = _run(b, _pack(), KMAX, EPS_HALF, hold_done=True, fast_noise=True, env_mask=mask)
    _check(b, got, ref_rec, ref_steps, ref_finals[-1], KMAX, f"hold masked={masked}")
    on = np.ones(E, bool) if mask is None else mask.cpu().numpy() != 0
    expect = np.where(on, np.maximum(1, 5 - np.arange(E) % 9 + 1), 0)   # the end step is known
    assert np.array_equal(got.steps_run.cpu().numpy(), expect)
    R = 5
    idle_r = np.repeat(np.arange(KMAX)[:, None] >= expect[None, :], R, axis=1)
    acts = got.actions.cpu().numpy()
    assert not acts[idle_r].any(), "idle rows of the actions record keep their pre-fill"
    assert (np.abs(acts[~idle_r]).sum(-1) > 0).all(), "every stepping slot's action is recorded"
    assert (got.done.cpu().numpy()[idle_r] == 1).all() and (got.info.cpu().numpy()[idle_r] == 255).all()
    off_r = torch.from_numpy(np.repeat(~on, R)).cuda()
    for n in ("obs", "reward", "done", "info", "obj_cnt"):
        _same(getattr(b, n)[off_r], before[n][off_r], f"masked env's {n}")
    _same(b.rs[:, off_r], before["rs"][:, off_r], "masked env's state")
    _same(b.rflags[off_r], before["rflags"][off_r], "masked env's flags")


@pytest.mark.parametrize("case", ["robot_params", "layout2_hold"])
def test_policy_rollout_fallback(case):
    """Per-robot parameters and an explicit layout 2 run K x (act launch, single step, record launches) inside
    the call: the same records and finals, and the caller's step counter is left alone (_run asserts it)."""
    from distributional_rl_decision_and_control_amd import _abi
    K = 3
    hold = case == "layout2_hold"
    launch = None if case == "robot_params" else (_abi.ENV_LAYOUT_SWEEP, 0, 0)
    mk = (lambda: _ending_batch()) if hold else (lambda: _fresh(5, 4, 2, True, robot_params=True))
    ref_rec, ref_steps, ref_finals, _ = _loop(mk(), _pack(), K, EPS_HALF, hold=hold, launch=launch)
    b = mk()
    got = _run(b, _pack(), K, EPS_HALF, hold_done=hold, fast_noise=True, launch=launch)
    _check(b, got, ref_rec, ref_steps, ref_finals[-1], K, case)
    if hold:
        assert int((ref_steps < K).sum()) > 0, "some env must be held inside the window"


def test_policy_rollout_recorded_noise():
    """Noise mode 0 under a live policy: row t of a recorded [K, NT, O + R, 5] tensor at step t."""
    R, O, C, K = 5, 4, 2, 6
    g = torch.Generator(device="cuda").manual_seed(9)
    noise = 0.05 * torch.randn((K, E * R, O + R, 5), generator=g, device="cuda", dtype=torch.float64)
    ref_rec, ref_steps, ref_finals, _ = _loop(_fresh(R, O, C, True), _pack(), K, EPS_HALF, noise=noise)
    for launch in _launches(R):
        b = _fresh(R, O, C, True)
        got = _run(b, _pack(), K, EPS_HALF, noise=noise, launch=launch)
        _check(b, got, ref_rec, ref_steps, ref_finals[-1], K, f"recorded noise launch={launch}")


# ------------------------------------------------------------------ VecMarineNavEnv.policy_rollout
def _vec(seed=5):
    from distributional_rl_decision_and_control_amd.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(E, num_robots=5, num_obs=4, min_start_goal_dis=20.0, seed=seed)
    env.reset()
    return env


def test_vec_env_policy_rollout_matches_rounds():
    from distributional_rl_decision_and_control_amd.fused_mlp import actor_act
    K = 4
    pack = _pack()
    twin = _vec()
    act64 = torch.zeros((E * 5, 2), dtype=torch.float64, device="cuda")
    for t in range(K):
        actor_act(pack, twin.obs_cur, act64, twin.counter, *EPS_HALF, POLICY_SEED)
        twin.step(act64)
        twin.advance_device()
    env = _vec()
    rec = env.policy_rollout(pack, K, hold_done=False, keep=("reward", "actions"), eps=EPS_HALF,
                             policy_seed=POLICY_SEED)
    assert rec.reward.shape == (K, E * 5) and rec.actions.shape == (K, E * 5, 2)
    _same(env.obs_next, twin.obs_next, "obs_next")
    _same(env.cnt_next, twin.cnt_next, "cnt_next")
    _same(env.counter, twin.counter, "counter")
    for n in ("rs", "rflags", "ep_ts", "reward", "done", "info", "env_done"):
        _same(getattr(env.batch, n), getattr(twin.batch, n), n)
    _same(rec.reward[-1], twin.batch.reward, "last reward record")
    _same(rec.actions[-1], act64, "last actions record")


# ------------------------------------------------------------------ VecTrainer.greedy_episodes
def test_greedy_episodes_matches_single_launches():
    from distributional_rl_decision_and_control_amd.fused_mlp import actor_act
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    MAX_STEPS, CHUNK = 24, 5   # the chunk does not divide max_steps: the last window is 4 steps
    tr = VecTrainer(n_envs=E, batch_size=64, buffer_size=4096, graphs=False, seed=3)
    tr.env.batch.params.episode_limit = 22   # every evaluation episode ends inside the last window
    for _ in range(2):
        tr.iteration()
    torch.cuda.synchronize()
    before = (tr.env.batch.rs.clone(), tr.env.counter.clone(), tr.replay.state.clone())
    stats = tr.greedy_episodes(max_steps=MAX_STEPS, chunk=CHUNK)
    for got, ref, what in zip((tr.env.batch.rs, tr.env.counter, tr.replay.state), before,
                              ("training state", "step counter", "replay state")):
        _same(got, ref, what)
    # the same windows as single launches on a twin batch
    env = tr._eval_env()
    mask = torch.ones(E, dtype=torch.uint8, device="cuda")
    steps = torch.zeros(E, dtype=torch.int32, device="cuda")
    act64 = torch.zeros((E * tr.R, 2), dtype=torch.float64, device="cuda")
    for t in range(MAX_STEPS):
        actor_act(tr.fused2.actor, env.obs_cur, act64, env.counter, *EPS_ZERO, 0)
        env.batch.step(act64, trainer_deactivate=True, seed=env.seed, counter=0, counter_dev=env.counter,
                       gamma=env.gamma, obs=env.obs_next, obj_cnt=env.cnt_next, fast_noise=True, env_mask=mask)
        env.advance_device()
        steps += (mask != 0).int()
        mask = mask * (env.batch.env_done == 0).to(torch.uint8)
    ref = env.episode_stats()
    assert ref["env_episodes"] == E and ref["robot_episodes"] > 0, "every twin episode must end"
    for k in ("robot_episodes", "env_episodes", "success", "collision", "timeout"):
        assert stats[k] == ref[k], (k, stats[k], ref[k])
    assert abs(stats["mean_return"] - ref["mean_return"]) <= 1e-12 * max(1.0, abs(ref["mean_return"]))
    assert np.array_equal(stats["steps_run"], steps.cpu().numpy())
    with pytest.raises(NotImplementedError):
        VecTrainer(n_envs=E, agent_type="IQN", batch_size=64, buffer_size=4096, graphs=False).greedy_episodes()


# ------------------------------------------------------------------ graph capture
def test_policy_rollout_graph_capture():
    """One call with caller-supplied records captured in a graph on a single stream and replayed from the restored
    state gives the eager call's records."""
    R, O, C, K = 5, 4, 2, 5
    pack = _pack()
    b = _fresh(R, O, C, True)
    state = {n: getattr(b, n).clone() for n in ("rs", "rflags", "ep_ts", "obs", "stats")}
    spec = _specs(b)

    def records():
        rec = {n: torch.full((K,) + spec[n][0], spec[n][2], dtype=spec[n][1], device="cuda") for n in RECORDS}
        rec["steps_run"] = torch.zeros(E, dtype=torch.int32, device="cuda")
        return rec

    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")

    def call(rec):
        b.policy_rollout(pack, K, b.obs, keep=rec, step_dev=step, eps=EPS_HALF, policy_seed=POLICY_SEED,
                         trainer_deactivate=True, seed=11, counter=1, gamma=GAMMA, fast_noise=True)

    eager = records()
    call(eager)
    torch.cuda.synchronize()
    finals = _finals(b)

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
