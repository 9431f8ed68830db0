"""GPU: the closed-loop policy rollout (asvrl_policy_rollout, env_policy_rollout_kernel<kPolActor>) against the composed
loop of the existing calls it replaces, bit for bit: for t < K, fused_mlp.actor_act on the current observation at step
counter s + t, then the single env step at noise counter c + t on those actions. Every record of every step
(the actions included), the steps every env took and the final state and outputs are compared with atol = rtol =
0 (the stats' return sum, an atomic sum, within 1e-12 as in the open-loop test), over shapes with partial groups,
both Philox precisions, three launch shapes, both operand builds, episode ends with and without hold_done and
under a caller's mask, the sweep fallback, recorded perception noise, VecMarineNavEnv.policy_rollout,
VecTrainer.greedy_episodes and a captured graph. E = 37 envs as in the open-loop tests: the last workgroup is
partial."""
import dataclasses

import numpy as np
import pytest
import torch

import window_cases as wc
from window_cases import EPS_HALF, EPS_ZERO

pytestmark = pytest.mark.gpu

E = 37
KMAX = 13
SHAPES = [(1, 0, 0), (5, 4, 2), (12, 8, 0)]
CASE = dataclasses.replace(wc.CASES["actor"], n_envs=E, kmax=KMAX, width={12: 110.0})   # 12 robots: a 110 m map


@pytest.mark.parametrize("eps", [EPS_HALF, EPS_ZERO], ids=["eps0.5", "greedy"])
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("R,O,C", SHAPES)
def test_policy_rollout_matches_composed_loop(R, O, C, fast, eps):
    """Bit-identity to the 2 K launches: every record (the actions among them), steps_run and all finals; K = 1,
    2, 13; the automatic launch shape, a forced one-wave shape and the automatic shape at max_groups = 3."""
    ref = wc.reference(CASE, R, O, C, fast, eps)
    if eps is EPS_HALF:
        # both branches of the epsilon-greedy draw occur in the reference: some rows took the greedy action (the
        # greedy loop's first round acts on the same observation), some a uniform draw
        greedy = wc.reference(CASE, R, O, C, fast, EPS_ZERO)["rec"]["actions"][0]
        same = (ref["rec"]["actions"][0] == greedy).all(1)
        assert bool(same.any()) and bool((~same).any()), "epsilon 0.5 must both exploit and explore"
    for K in (1, 2, 13):
        for launch in (None,) + wc.one_wave_and_capped(R):
            b = wc.batch(CASE, R, O, C, fast)
            got = wc.run_window(b, wc.pack(CASE), K, eps, fast_noise=fast, launch=launch)
            wc.check(b, got, ref, K, f"R={R} O={O} K={K} launch={launch}")


def test_policy_rollout_f32_build():
    """MlpPack(operands="f32") runs the f32-operand library (fragments from L2, no LDS weight images): against that
    library's own composed loop."""
    R, O, C = 5, 4, 2
    pack = wc.pack(CASE, "f32")
    ref = wc.reference(CASE, R, O, C, True, EPS_HALF, "f32")
    bf_rec = wc.reference(CASE, R, O, C, True, EPS_HALF)["rec"]
    assert not torch.equal(ref["rec"]["actions"], bf_rec["actions"]), "the two builds' actors differ in rounding"
    for K in (2, 13):
        for launch in (None,) + wc.one_wave_and_capped(R):
            b = wc.batch(CASE, R, O, C, True)
            got = wc.run_window(b, pack, K, EPS_HALF, fast_noise=True, launch=launch)
            wc.check(b, got, ref, K, f"f32 K={K} launch={launch}")


def test_policy_rollout_episode_ends_without_hold():
    ref = wc.composed_loop(CASE, wc.batch(CASE, 5, 4, 0, ending=True), wc.pack(CASE), KMAX, EPS_HALF)
    assert bool((ref["rec"]["env_done"].sum(0) > 0).all()), "every env must end inside the window"
    b = wc.batch(CASE, 5, 4, 0, ending=True)
    got = wc.run_window(b, wc.pack(CASE), KMAX, EPS_HALF, fast_noise=True)
    wc.check(b, got, ref, KMAX, "no hold", steps=ref["steps_run"])


@pytest.mark.parametrize("masked", [False, True])
def test_policy_rollout_hold_done(masked):
    """hold_done is the chain of rounds whose env_mask drops an env after its env_done; `masked`: on top of a
    caller's mask that leaves every fourth env (and one whole workgroup's envs) out. An env that is off takes no
    action: its rows of the actions record keep their pre-fill, and a masked env is untouched."""
    mask = wc.quarter_mask(E) if masked else None
    ref = wc.composed_loop(CASE, wc.batch(CASE, 5, 4, 0, ending=True), wc.pack(CASE), KMAX, EPS_HALF, hold=True,
                           env_mask=mask)
    b = wc.batch(CASE, 5, 4, 0, ending=True)
    before = wc.finals(b)
    got = wc.run_window(b, wc.pack(CASE), KMAX, EPS_HALF, hold_done=True, fast_noise=True, env_mask=mask)
    wc.check(b, got, ref, KMAX, f"hold masked={masked}", steps=ref["steps_run"])
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
        wc.same(getattr(b, n)[off_r], before[n][off_r], f"masked env's {n}")
    wc.same(b.rs[:, off_r], before["rs"][:, off_r], "masked env's state")
    wc.same(b.rflags[off_r], before["rflags"][off_r], "masked env's flags")


@pytest.mark.parametrize("case", ["robot_params", "layout2_hold"])
def test_policy_rollout_fallback(case):
    """Per-robot parameters and an explicit layout 2 run K x (act launch, single step, record launches) inside
    the call: the same records and finals, and the caller's step counter is left alone (run_window asserts it)."""
    from distributional_rl_decision_and_control_amd import _abi
    K = 3
    hold = case == "layout2_hold"
    launch = None if case == "robot_params" else (_abi.ENV_LAYOUT_SWEEP, 0, 0)
    mk = (lambda: wc.batch(CASE, 5, 4, 0, ending=True)) if hold else (
        lambda: wc.batch(CASE, 5, 4, 2, robot_params=True))
    ref = wc.composed_loop(CASE, mk(), wc.pack(CASE), K, EPS_HALF, hold=hold, launch=launch)
    b = mk()
    got = wc.run_window(b, wc.pack(CASE), K, EPS_HALF, hold_done=hold, fast_noise=True, launch=launch)
    wc.check(b, got, ref, K, case, steps=ref["steps_run"])
    if hold:
        assert int((ref["steps_run"] < K).sum()) > 0, "some env must be held inside the window"


def test_policy_rollout_recorded_noise():
    """Noise mode 0 under a live policy: row t of a recorded [K, NT, O + R, 5] tensor at step t."""
    R, O, C, K = 5, 4, 2, 6
    g = torch.Generator(device="cuda").manual_seed(9)
    noise = 0.05 * torch.randn((K, E * R, O + R, 5), generator=g, device="cuda", dtype=torch.float64)
    ref = wc.composed_loop(CASE, wc.batch(CASE, R, O, C), wc.pack(CASE), K, EPS_HALF, noise=noise)
    for launch in (None,) + wc.one_wave_and_capped(R):
        b = wc.batch(CASE, R, O, C)
        got = wc.run_window(b, wc.pack(CASE), K, EPS_HALF, noise=noise, launch=launch)
        wc.check(b, got, ref, K, f"recorded noise launch={launch}", steps=ref["steps_run"])


# ------------------------------------------------------------------ VecMarineNavEnv.policy_rollout
def test_vec_env_policy_rollout_matches_rounds():
    rec, env, twin = wc.check_vec_env(CASE, wc.pack(CASE), 4)
    wc.same(env.cnt_next, twin.cnt_next, "cnt_next")
    wc.same(rec.reward[-1], twin.batch.reward, "last reward record")


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
        wc.same(got, ref, what)
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
    wc.check_graph_capture(CASE, wc.batch(CASE, 5, 4, 2), wc.pack(CASE), 5)
