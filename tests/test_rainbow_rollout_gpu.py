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
import dataclasses

import numpy as np
import pytest

import window_cases as wc
from window_cases import EPS_HALF, EPS_ZERO

pytestmark = pytest.mark.gpu

E, R, O, C = 37, 5, 4, 2
K = 5
# envs of 3, 4 and 5 robots; episode limit 3 (no ep_ts preset): every env ends inside a 5-step window
CASE = dataclasses.replace(wc.CASES["rainbow"], n_envs=E, kmax=K, robots=(3, 4, 5), end_limit=3, end_stagger=0)

@pytest.mark.parametrize("eps", [EPS_HALF, EPS_ZERO], ids=["eps0.5", "greedy"])
@pytest.mark.parametrize("noisy", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_rainbow_rollout_matches_composed_loop(ops, noisy, eps):
    """K = 5 and 2 at the automatic step shape, K = 5 also at layout 2 (the sweep step)."""
    ref = wc.reference(CASE, R, O, C, True, eps, ops, noisy=noisy)
    wc.assert_indices(ref["rec"]["actions"], "reference")
    n_robots = wc.batch(CASE, R, O, C).n_robots
    assert int(n_robots.min()) == 3 and int(n_robots.max()) == 5
    assert ref["rec"]["actions"][..., 0].unique().numel() >= 3, "the loop takes several actions"
    for n, launch in ((K, None), (2, None), (K, (2, 0, 0))):
        b = wc.batch(CASE, R, O, C)
        got = wc.run_window(b, wc.pack(CASE, ops, noisy=noisy), n, eps, fast_noise=True, launch=launch)
        wc.check(b, got, ref, n, f"{ops} noisy={noisy} K={n} launch={launch}")
        wc.assert_indices(got.actions, f"K={n}")


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_rainbow_rollout_hold_done_and_env_mask(ops):
    """hold_done on top of a caller's mask that leaves every fourth env (and eight in a row) out: the chain of rounds
    whose env_mask drops an env after its env_done. An env that is off takes no action: its rows of the actions
    record keep their pre-fill. episode_limit 3: every env that is on ends inside the window."""
    mask = wc.quarter_mask(E)
    pack = wc.pack(CASE, ops, noisy=True)
    ref = wc.composed_loop(CASE, wc.batch(CASE, R, O, C, ending=True), pack, K, EPS_HALF, hold=True, env_mask=mask)
    b = wc.batch(CASE, R, O, C, ending=True)
    got = wc.run_window(b, pack, K, EPS_HALF, fast_noise=True, hold_done=True, env_mask=mask)
    wc.check(b, got, ref, K, "hold_done + env_mask", steps=ref["steps_run"])
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
    ref = wc.reference(CASE, R, O, C, True, eps, ops, ar=True, noisy=True)
    wc.assert_indices(ref["rec"]["actions"], "reference")
    assert ref["resets_after"][-1].min().item() >= 1 and ref["resets_after"][-1].sum().item() >= E
    assert int(ref["pushed"].min().item()) > 0
    b = wc.batch(CASE, R, O, C, ending=True)
    got = wc.run_window(b, wc.pack(CASE, ops, noisy=True), K, eps, cfg=wc.cfg(CASE, R, O, C), fast_noise=True)
    assert int(got.resets.sum().item()) >= E and int(got.resets.min().item()) >= 1, "every env restarts in the window"
    wc.check(b, got, ref, K, f"auto-reset {ops} eps={eps}")
    wc.assert_indices(got.actions, "auto-reset")


def test_policy_rollout_value_errors():
    b = wc.batch(CASE, R, O, C)
    pack = wc.pack(CASE, noisy=True)
    with pytest.raises(ValueError, match="cvar"):
        b.policy_rollout(pack, 2, b.obs, cvar=0.5)
    with pytest.raises(ValueError, match="deterministic"):
        b.policy_rollout(pack, 2, b.obs, deterministic=True)


# ------------------------------------------------------------------ VecMarineNavEnv.policy_rollout
def test_vec_env_takes_a_rainbow_pack_on_a_discrete_env():
    pack = wc.pack(CASE, noisy=True)
    wc.check_vec_env(CASE, pack, 4, assert_actions=wc.assert_indices)
    with pytest.raises(ValueError, match="RainbowPack.*is_continuous=True"):
        wc.vec_env(CASE, True).policy_rollout(pack, 2)
    with pytest.raises(ValueError, match="cvar"):
        wc.vec_env(CASE, False).policy_rollout(pack, 2, cvar=0.5)
    with pytest.raises(ValueError, match="deterministic"):
        wc.vec_env(CASE, False).policy_rollout(pack, 2, deterministic=True)


# ------------------------------------------------------------------ graph capture
def test_rainbow_rollout_graph_capture():
    """One call of a K = 3 window with caller-supplied records captured in a graph on a single stream and replayed
    from the restored state gives the eager call's bits: the per-step launches and the call's stream-ordered scratch
    are captured as they are enqueued."""
    wc.check_graph_capture(CASE, wc.batch(CASE, R, O, C), wc.pack(CASE, noisy=True), 3,
                           assert_actions=wc.assert_indices)
