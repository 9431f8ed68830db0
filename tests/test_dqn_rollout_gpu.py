"""GPU: the closed-loop rollout windows under DQN_Policy (asvrl_dqn_rollout / asvrl_dqn_rollout_ar,
env_policy_rollout_kernel's kPolDqn instantiations) against the composed loop of the calls they replace, bit for
bit: for t < K, fused_dqn.dqn_act on the current observation at step counter STEP0 + t, the single env step with
is_continuous=False at noise counter C0 + t on those indices and, with the auto-reset, reset_observe on
env_done & mask at (RC + t, OC + t). Every record of every step (the actions among them; obs_prev, pushed and resets
with the auto-reset), the steps every env took and every final array are compared with atol = rtol = 0 (the stats'
return sum, an atomic sum, within 1e-12 as in the Actor's tests). E = 37 envs: the last workgroup and, at 5 and 12
robots, the last 32-row tile are partial. The weights are a seeded DQN_Policy."""
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
CASE = dataclasses.replace(wc.CASES["dqn"], n_envs=E, kmax=KMAX, width={12: 110.0})   # 12 robots: a 110 m map


def _assert_not_vacuous(R, O, C, fast, eps, operands="bf16", ar=False):
    acts = wc.reference(CASE, R, O, C, fast, eps, operands, ar)["rec"]["actions"]
    wc.assert_indices(acts, "reference")
    greedy = wc.reference(CASE, R, O, C, fast, EPS_ZERO, operands, ar)["rec"]["actions"]
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
    ref = wc.reference(CASE, R, O, C, fast, eps)
    if R > 1:   # (one robot per env: 37 rows, whose greedy indices need not spread)
        _assert_not_vacuous(R, O, C, fast, eps)
    else:
        wc.assert_indices(ref["rec"]["actions"], "reference")
    one_wave, capped = wc.one_wave_and_capped(R)
    for K, launch in [(K, ln) for K in (1, 2, 13) for ln in (None, one_wave)] + [(13, capped)]:
        b = wc.batch(CASE, R, O, C, fast)
        got = wc.run_window(b, wc.pack(CASE), K, eps, fast_noise=fast, launch=launch)
        wc.check(b, got, ref, K, f"R={R} O={O} K={K} launch={launch}")
        wc.assert_indices(got.actions, f"R={R} K={K}")


def test_dqn_rollout_f32_build_and_torch_argmax():
    """DqnPack(operands="f32") runs the f32-operand library (fragments from L2, no LDS weight images) against that
    library's own composed loop; there the first step's greedy actions are torch's arg-max of policy_local on the
    initial observations (rows whose two best Q values are nearly tied are left out, and they must be few)."""
    R, O, C = 5, 4, 2
    pack = wc.pack(CASE, "f32")
    for eps in (EPS_HALF, EPS_ZERO):
        ref = wc.reference(CASE, R, O, C, True, eps, "f32")
        _assert_not_vacuous(R, O, C, True, eps, "f32")
        for K, launch in ((2, None), (13, None), (13, wc.one_wave_and_capped(R)[0])):
            b = wc.batch(CASE, R, O, C, True)
            got = wc.run_window(b, pack, K, eps, fast_noise=True, launch=launch)
            wc.check(b, got, ref, K, f"f32 eps={eps} K={K} launch={launch}")
    b = wc.batch(CASE, R, O, C, True)
    x = b.obs.clone()
    got = wc.run_window(b, pack, 1, EPS_ZERO, fast_noise=True)
    with torch.no_grad():
        q_ref = wc.net(CASE)((x[:, 0:7], x[:, 7:32].reshape(-1, 5, 5), x[:, 32:37]))
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
    mask = wc.quarter_mask(E) if masked else None
    ref = wc.composed_loop(CASE, wc.batch(CASE, 5, 4, 0, ending=True), wc.pack(CASE), KMAX, EPS_HALF, hold=True,
                           env_mask=mask)
    b = wc.batch(CASE, 5, 4, 0, ending=True)
    got = wc.run_window(b, wc.pack(CASE), KMAX, EPS_HALF, hold_done=True, fast_noise=True, env_mask=mask)
    wc.check(b, got, ref, KMAX, f"hold masked={masked}", steps=ref["steps_run"])
    on = np.ones(E, bool) if mask is None else mask.cpu().numpy() != 0
    expect = np.where(on, np.maximum(1, 5 - np.arange(E) % 9 + 1), 0)   # the end step is known
    assert np.array_equal(got.steps_run.cpu().numpy(), expect)
    idle_r = np.repeat(np.arange(KMAX)[:, None] >= expect[None, :], 5, axis=1)
    assert not got.actions.cpu().numpy()[idle_r].any(), "idle rows of the actions record keep their pre-fill"


def test_dqn_rollout_fallback_per_robot_parameters():
    """Per-robot parameters run K x (asvrl_dqn_act, single step, record launches) inside the call: the same records
    and finals, and the caller's step counter is left alone (run_window asserts it)."""
    K = 3
    ref = wc.composed_loop(CASE, wc.batch(CASE, 5, 4, 2, robot_params=True), wc.pack(CASE), K, EPS_HALF)
    b = wc.batch(CASE, 5, 4, 2, robot_params=True)
    got = wc.run_window(b, wc.pack(CASE), K, EPS_HALF, fast_noise=True)
    wc.check(b, got, ref, K, "robot_params")
    wc.assert_indices(got.actions, "robot_params")


@pytest.mark.parametrize("eps", [EPS_HALF, EPS_ZERO], ids=["eps0.5", "greedy"])
def test_dqn_rollout_auto_reset(eps):
    """episode_limit 5 and ep_ts preset to e % 9: every env ends at least twice in 13 steps; obs_prev, pushed and
    resets are compared with the records."""
    R, O, C = 5, 4, 2
    ref = wc.reference(CASE, R, O, C, True, eps, ar=True)
    _assert_not_vacuous(R, O, C, True, eps, ar=True)
    assert ref["resets_after"][-1].min().item() >= 2, "every env must end at least twice"
    assert int(ref["pushed"].min().item()) > 0
    for launch in (None,) + wc.one_wave_and_capped(R):
        b = wc.batch(CASE, R, O, C, ending=True)
        got = wc.run_window(b, wc.pack(CASE), KMAX, eps, cfg=wc.cfg(CASE, R, O, C), fast_noise=True, launch=launch)
        wc.check(b, got, ref, KMAX, f"auto-reset eps={eps} launch={launch}")
        wc.assert_indices(got.actions, "auto-reset")


def test_dqn_rollout_auto_reset_fallback():
    """Per-robot parameters: the K-launch form with the two reset launches behind every step."""
    R, O, C, K = 5, 4, 2, 7
    cfg = wc.cfg(CASE, R, O, C)
    ref = wc.composed_loop(CASE, wc.batch(CASE, R, O, C, ending=True, robot_params=True), wc.pack(CASE), K, EPS_HALF,
                           cfg=cfg, two_launch=True)
    assert ref["resets_after"][-1].sum().item() > 0
    b = wc.batch(CASE, R, O, C, ending=True, robot_params=True)
    got = wc.run_window(b, wc.pack(CASE), K, EPS_HALF, cfg=cfg, fast_noise=True)
    wc.check(b, got, ref, K, "auto-reset robot_params")


# ------------------------------------------------------------------ VecMarineNavEnv.policy_rollout
def test_vec_env_takes_a_dqn_pack_on_a_discrete_env():
    wc.check_vec_env(CASE, wc.pack(CASE), 4, assert_actions=wc.assert_indices)


def test_vec_env_pack_and_env_must_match():
    with pytest.raises(ValueError, match="continuous"):
        wc.vec_env(CASE, False).policy_rollout(wc.pack(wc.CASES["actor"]), 2)
    with pytest.raises(ValueError, match="DqnPack.*is_continuous=True"):
        wc.vec_env(CASE, True).policy_rollout(wc.pack(CASE), 2)


# ------------------------------------------------------------------ graph capture
def test_dqn_rollout_graph_capture():
    """One call with caller-supplied records captured in a graph on a single stream and replayed from the restored
    state gives the eager call's records."""
    wc.check_graph_capture(CASE, wc.batch(CASE, 5, 4, 2), wc.pack(CASE), 5, assert_actions=wc.assert_indices)
