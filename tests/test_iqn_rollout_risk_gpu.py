"""GPU: the IQN closed-loop windows under a risk level per robot (asvrl_iqn_rollout_risk / _risk_ar: per step
asvrl_iqn_act_risk and the env step, enqueued by one call) against the hand-composed loop, bit for bit in every
record: for t < K, iqn_act(..., cvar=<AdaptiveCvar | tensor>, actions_rec=...) on the current observation with the step
tensor at STEP0 + t, then the single env step on the indices. tests/window_cases.py's loop, window call and comparison
are used as they are; the composed loop's `actions` record is the act buffer, whose second column is 0.0, so the
wrapper below keeps every round's record row (index, level used) and writes it over the reference's rows of stepping
envs before the comparison. 5 envs x 4 robots, 2 obstacles, K = 6."""
import dataclasses

import pytest
import torch

import window_cases as wc
from window_cases import EPS_HALF, POLICY_SEED

pytestmark = pytest.mark.gpu

E, R, O, C, K = 5, 4, 2, 0, 6
NT = E * R
_LAST = {}


def _rule(**kw):
    from distributional_rl_decision_and_control_amd.fused_iqn import AdaptiveCvar
    return AdaptiveCvar(**kw)


def _risk_act(pack, obs, act64, step, eps, seed, cvar=1.0):
    """The composed round's act: the single launch with its record row, kept for _keep_rec."""
    from distributional_rl_decision_and_control_amd.fused_iqn import iqn_act
    rec = torch.full((obs.shape[0], 2), -9.0, dtype=torch.float64, device="cuda")
    iqn_act(pack, None, act64, step, *eps, seed, obs=obs, cvar=cvar, actions_rec=rec)
    _LAST["rec"] = rec


def _keep_rec(extra, case, b, pack, act64, step, on_r, eps, options):
    rec = _LAST.pop("rec")
    assert torch.equal(rec[:, 0], act64[:, 0]) and bool((act64[:, 1] == 0.0).all())
    extra.setdefault("act_rec", []).append((rec, on_r.clone()))


CASE = dataclasses.replace(wc.CASES["iqn"], n_envs=E, kmax=K, act=_risk_act, hook=_keep_rec)


def _composed(b, pack, cvar, **kw):
    ref = wc.composed_loop(CASE, b, pack, K, EPS_HALF, cvar=cvar, **kw)
    for t, (rec, on_r) in enumerate(ref["act_rec"]):   # (index, level used) on the rows of stepping envs
        wc.same(ref["rec"]["actions"][t][on_r][:, 0], rec[on_r][:, 0], "composed index")
        ref["rec"]["actions"][t][on_r] = rec[on_r]
    return ref


def _assert_records(actions, what, levels=None):
    """Every recorded action is an exact integer in 0..A-1; column 1 is a level in (0, 1] on the rows that acted and
    the 0.0 pre-fill elsewhere."""
    a0, a1 = actions[..., 0], actions[..., 1]
    assert bool(((a0 >= 0) & (a0 <= wc.A - 1) & (a0 == a0.round())).all()), f"{what}: action indices"
    assert bool(((a1 >= 0.0) & (a1 <= 1.0)).all()), f"{what}: column 1"
    assert bool((a1 > 0).any()), f"{what}: no level recorded"
    assert bool((a1 == a1.float().double()).all()), f"{what}: an f32 level, widened exactly"


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_adaptive_window_matches_composed_loop(ops):
    pack = wc.pack(CASE, ops)
    ref = _composed(wc.batch(CASE, R, O, C), pack, _rule())
    for k in (1, K):
        b = wc.batch(CASE, R, O, C)
        got = wc.run_window(b, pack, k, EPS_HALF, fast_noise=True, cvar=_rule())
        wc.check(b, got, ref, k, f"{ops} adaptive K={k}")
        _assert_records(got.actions, f"{ops} adaptive K={k}")


def test_the_level_is_the_rule_on_the_observation_and_moves():
    """The second column of `actions` at step t is AdaptiveCvar().levels of the row the robot acted on: obs_in at
    t = 0, the obs record of step t - 1 after it. It is decided per step: at least one robot's level changes between
    two steps of the window, and the robots do not all share one level."""
    pack = wc.pack(CASE)
    b = wc.batch(CASE, R, O, C)
    obs_in = b.obs.clone()
    got = wc.run_window(b, pack, K, EPS_HALF, fast_noise=True, cvar=_rule())
    acted_on = torch.cat([obs_in[None], got.obs[:-1]])
    want = _rule().levels(acted_on)
    lev = got.actions[..., 1]
    err = float((lev - want.double()).abs().max())
    print(f"max |recorded level - levels(obs)| = {err:.3e}; levels in [{float(lev.min()):.3f}, {float(lev.max()):.3f}]")
    assert err <= 1e-6
    assert bool((lev[1:] != lev[:-1]).any()), "no robot's level changed between two steps"
    assert float(lev.min()) < 1.0 and float(lev[0].min()) != float(lev[0].max())


def test_adaptive_window_hold_done():
    pack = wc.pack(CASE)
    ref = _composed(wc.batch(CASE, R, O, C, ending=True), pack, _rule(), hold=True)
    b = wc.batch(CASE, R, O, C, ending=True)
    got = wc.run_window(b, pack, K, EPS_HALF, hold_done=True, fast_noise=True, cvar=_rule())
    wc.check(b, got, ref, K, "adaptive hold_done", steps=ref["steps_run"])
    assert int(got.steps_run.min()) < K, "an env must end inside the window"
    idle = (torch.arange(K, device="cuda")[:, None] >= got.steps_run[None, :]).repeat_interleave(R, dim=1)
    assert not bool(got.actions[idle].any()), "idle rows of the actions record keep their pre-fill"


def test_adaptive_window_env_mask():
    mask = torch.ones(E, dtype=torch.uint8, device="cuda")
    mask[1::3] = 0
    pack = wc.pack(CASE)
    ref = _composed(wc.batch(CASE, R, O, C), pack, _rule(), env_mask=mask)
    b = wc.batch(CASE, R, O, C)
    got = wc.run_window(b, pack, K, EPS_HALF, fast_noise=True, env_mask=mask, cvar=_rule())
    wc.check(b, got, ref, K, "adaptive env_mask", steps=ref["steps_run"])
    off_r = (mask == 0).repeat_interleave(R)
    assert not bool(got.actions[:, off_r].any())
    assert bool((got.actions[:, ~off_r, 1] > 0).all())


def test_adaptive_window_auto_reset():
    pack = wc.pack(CASE)
    cfg = wc.cfg(CASE, R, O, C)
    ref = _composed(wc.batch(CASE, R, O, C, ending=True), pack, _rule(), cfg=cfg)
    assert ref["resets_after"][-1].sum().item() > 0
    b = wc.batch(CASE, R, O, C, ending=True)
    got = wc.run_window(b, pack, K, EPS_HALF, cfg=cfg, fast_noise=True, cvar=_rule())
    wc.check(b, got, ref, K, "adaptive auto-reset")
    # the level follows the row acted on, a reset env's reset observation included
    want = _rule().levels(got.obs_prev)
    assert float((got.actions[..., 1] - want.double()).abs().max()) <= 1e-6


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_per_slot_tensor_window_matches_composed_loop(ops):
    """One level per robot slot, constant over the window."""
    pack = wc.pack(CASE, ops)
    lev = (0.1 + 0.9 * torch.rand(NT, generator=torch.Generator().manual_seed(2))).cuda()
    ref = _composed(wc.batch(CASE, R, O, C), pack, lev)
    b = wc.batch(CASE, R, O, C)
    got = wc.run_window(b, pack, K, EPS_HALF, fast_noise=True, cvar=lev)
    wc.check(b, got, ref, K, f"{ops} per-slot levels")
    assert torch.equal(got.actions[..., 1], lev.double().expand(K, NT))


def test_a_tensor_of_one_level_is_the_scalar_window():
    pack = wc.pack(CASE)
    b = wc.batch(CASE, R, O, C)
    scalar = wc.run_window(b, pack, K, EPS_HALF, fast_noise=True, cvar=0.25)
    wc.assert_indices(scalar.actions, "scalar window")
    b2 = wc.batch(CASE, R, O, C)
    got = wc.run_window(b2, pack, K, EPS_HALF, fast_noise=True, cvar=torch.full((NT,), 0.25, device="cuda"))
    wc.same(got.actions[..., 0], scalar.actions[..., 0], "index column")
    assert bool((got.actions[..., 1] == 0.25).all())
    for n in ("reward", "done", "info", "obs", "rs"):
        wc.same(getattr(got, n), getattr(scalar, n), n)
    for n in wc.FINALS:
        wc.same(getattr(b2, n), getattr(b, n), f"final {n}")
    neutral = wc.run_window(wc.batch(CASE, R, O, C), pack, K, EPS_HALF, fast_noise=True)
    assert not torch.equal(neutral.actions[..., 0], scalar.actions[..., 0])


def test_adaptive_window_graph_capture():
    wc.check_graph_capture(CASE, wc.batch(CASE, R, O, C), wc.pack(CASE), K, assert_actions=_assert_records,
                           cvar=_rule())


def test_vec_env_matches_the_batch_level_call():
    """VecMarineNavEnv.policy_rollout(..., cvar=AdaptiveCvar()) on a discrete env is DeviceEnvBatch.policy_rollout on
    its batch with the env's own counters."""
    pack = wc.pack(CASE)
    env, twin = wc.vec_env(CASE), wc.vec_env(CASE)
    keep = ("reward", "actions", "obs")
    rec = env.policy_rollout(pack, K, hold_done=False, keep=keep, eps=EPS_HALF, policy_seed=POLICY_SEED, cvar=_rule())
    ref = twin.batch.policy_rollout(pack, K, twin.obs_cur, keep=keep, step_dev=twin.counter, eps=EPS_HALF,
                                    policy_seed=POLICY_SEED, trainer_deactivate=True, seed=twin.seed, counter=0,
                                    counter_dev=twin.counter, gamma=twin.gamma, obs=twin.obs_next,
                                    obj_cnt=twin.cnt_next, fast_noise=True, launch=twin._launch(), cvar=_rule())
    for n in keep:
        wc.same(getattr(rec, n), getattr(ref, n), f"record {n}")
    _assert_records(rec.actions, "vec env")
    wc.same(env.obs_next, twin.obs_next, "obs_next")
    for n in ("rs", "rflags", "ep_ts", "reward", "done", "info", "env_done"):
        wc.same(getattr(env.batch, n), getattr(twin.batch, n), n)
    assert int(env.counter.item()) == int(twin.counter.item()) + K


def test_policy_rollout_value_errors():
    b = wc.batch(CASE, R, O, C)
    pack = wc.pack(CASE)
    ok = torch.full((NT,), 0.5, device="cuda")
    for bad in (0.0, 1.5):
        t = ok.clone()
        t[3] = bad
        with pytest.raises(ValueError, match=r"policy_rollout: cvar must be in \(0, 1\]"):
            b.policy_rollout(pack, 2, b.obs, cvar=t)
    with pytest.raises(ValueError, match="f32"):
        b.policy_rollout(pack, 2, b.obs, cvar=ok.double())
    with pytest.raises(ValueError, match=f"{NT} values"):
        b.policy_rollout(pack, 2, b.obs, cvar=ok[:-1].contiguous())
    with pytest.raises(ValueError, match="must be on"):
        b.policy_rollout(pack, 2, b.obs, cvar=ok.cpu())
    text = ("policy_rollout: cvar is the risk distortion of IQN's quantile fractions (an IqnPack); the other policies "
            "have no quantiles to distort")
    for cvar in (ok, _rule()):
        with pytest.raises(ValueError) as e:
            b.policy_rollout(wc.pack(wc.CASES["dqn"]), 2, b.obs, cvar=cvar)
        assert str(e.value) == text
    with pytest.raises(ValueError, match="deterministic"):
        b.policy_rollout(pack, 2, b.obs, cvar=_rule(), deterministic=True)
