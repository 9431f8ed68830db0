"""GPU: return distributions in the device evaluation (DeviceEvaluator.run(..., distribution=...)).

The configs are device_eval_cases.edited_configs(): every episode ends early and certainly, robots reach their goals
(config 2) and collide (config 1, at the first step) well before the episode limit of 40; the test asserts both.

IQN (an IqnPack, distribution=True): every pre-existing result is the plain run's, bit for bit; the recomputed greedy
action is the recorded one at every acted robot-step; g0 is robot_rewards (a backward scan against the metrics'
forward sum with pow: 1e-12 of max(1, |return|), the bar of device_eval_cases); steps are the history's act counts;
the quantiles at a robot's first and last act are a direct iqn_dist on its observation history, rebuilt to 40 columns
and put into its slot so the Philox key is the window's; chunk 7, chunk 64 and sync=False give the same bits; under
cvar = 0.25 and an AdaptiveCvar no fraction exceeds the level; perception="numpy" runs.
AC-IQN (VecTrainer.evaluate(cfgs, distribution=True)): g0 as above, the quantiles of three robot-steps are
critic_forward on those rows, and the summary's PIT histogram sums to 1. Every refusal is a ValueError, and a plain run
allocates none of it."""
import functools

import numpy as np
import pytest
import torch

import device_eval_cases as dev
import window_cases as wc
from device_eval_cases import GAMMA, PSEED, SEED

pytestmark = pytest.mark.gpu

CASE = wc.CASES["iqn"]
LIMIT = 40
KW = dict(episode_limit=LIMIT, seed=SEED, policy_seed=PSEED)
ARRAYS = ("g0", "pred0", "pit", "pinball", "bias", "steps", "truncated")


@functools.lru_cache(maxsize=None)
def _evaluator(chunk=7):
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    return DeviceEvaluator(dev.edited_configs()[0], chunk=chunk, gamma=GAMMA)


def _goal_and_collision(res):
    out = np.concatenate(res["robot_outcomes"])
    assert (out == 1).any() and (out == 2).any(), "the configs must hold a goal and a collision"
    assert max(res["lengths"]) < LIMIT, "before the episode limit"


def _rows40(h, c, i, k):
    """Robot (c, i)'s first k observations as the packed 40-column rows the policy was fed."""
    s, o, cnt = h.observation(c, i)
    x = np.zeros((k, 40), np.float32)
    x[:, :7], x[:, 7:32] = s[:k], o[:k].reshape(k, 25)
    x[:, 32:37] = np.arange(5)[None, :] < cnt[:k, None]
    return torch.from_numpy(x).cuda()


def _same_distribution(a, b, ev, what):
    for name in ARRAYS:
        for c in range(len(ev.n_robots)):
            assert getattr(a, name)[c].tobytes() == getattr(b, name)[c].tobytes(), (what, name, c)
    assert a.mismatches == b.mismatches, what


def _g0_is_the_return(res):
    d = res["distribution"]
    for c, ret in enumerate(res["robot_rewards"]):
        dev.close(d.g0[c], ret, scale=np.maximum(1.0, np.abs(ret)), what=f"config {c} g0")


def test_iqn_distribution_beside_the_plain_run():
    from distributional_rl_decision_and_control_amd.fused_iqn import iqn_dist
    pack = wc.pack(CASE, "bf16")
    ev = _evaluator()
    plain = ev.run(pack, **KW)
    _goal_and_collision(plain)
    res = ev.run(pack, distribution=True, histories=True, **KW)
    steps_run = ev.steps
    assert set(res) - set(plain) == {"distribution", "history"} and set(plain) <= set(res)
    dev.same_results(res, plain, "with distribution")
    assert res["cvar"] == plain["cvar"] and res["draws_n"] is None
    alone = ev.run(pack, distribution=True, **KW)   # without histories: the records are kept, nothing is packed
    assert "history" not in alone
    dev.same_results(alone, plain, "distribution alone")
    d, h = res["distribution"], res["history"]
    _same_distribution(alone["distribution"], d, ev, "distribution alone")
    assert d.kind == "iqn" and d.mismatches == 0
    _g0_is_the_return(res)
    checked = 0
    for c, n in enumerate(ev.n_robots):
        g, row0 = ev.rows(c)
        NT = ev.groups[g].batch.n_envs * ev.groups[g].batch.max_robots
        assert d.truncated[c].tolist() == (res["robot_outcomes"][c] == 0).tolist()
        for i in range(n):
            k = int(d.steps[c][i])
            acts = h.action(c, i)
            assert k == len(acts) and k >= 1 and d.pit[c][i].sum() == k
            z, tu, G = d.quantiles(c, i), d.taus(c, i), d.returns_to_go(c, i)
            assert z.shape == tu.shape == (k, 32) and G.shape == (k,) and G[0] == d.g0[c][i]
            assert np.isfinite(z).all() and tu.min() >= 0.0 and tu.max() < 1.0
            mean0 = z[0].astype(np.float64).mean()
            assert abs(d.pred0[c][i] - mean0) <= 1e-12 * max(1.0, np.abs(z[0]).max())
            x = _rows40(h, c, i, k)
            for t in sorted({0, k - 1}):
                X = torch.zeros((NT, 40), device="cuda")
                A = torch.zeros((NT, 2), dtype=torch.float64, device="cuda")
                X[row0 + i], A[row0 + i, 0] = x[t], float(acts[t])
                one = iqn_dist(pack, X, rows_per_step=NT, step0=t, seed=PSEED + g, actions=A)
                assert one.z[row0 + i].cpu().numpy().tobytes() == z[t].tobytes(), (c, i, t)
                assert one.taus[row0 + i].cpu().numpy().tobytes() == tu[t].tobytes(), (c, i, t)
                assert int(one.greedy[row0 + i]) == int(acts[t])
                checked += 1
    assert checked > sum(ev.n_robots), "some robot acted more than once"
    assert steps_run <= LIMIT + 1
    s = d.summary(terminated_only=False)
    assert abs(s["overall"]["pit"].sum() - 1.0) < 1e-12 and s["overall"]["steps"] == sum(int(x.sum()) for x in d.steps)
    t = d.summary()
    assert t["overall"]["robots"] == int(sum((~x).sum() for x in d.truncated))


def test_iqn_chunks_and_sync_give_the_same_bits():
    pack = wc.pack(CASE, "bf16")
    a = _evaluator(7).run(pack, distribution=True, **KW)["distribution"]
    ev64 = _evaluator(64)
    b = ev64.run(pack, distribution=True, **KW)["distribution"]
    _same_distribution(a, b, ev64, "chunk 64")
    for c, i in ((0, 1), (2, 4)):
        assert a.quantiles(c, i).tobytes() == b.quantiles(c, i).tobytes()
        assert a.returns_to_go(c, i).tobytes() == b.returns_to_go(c, i).tobytes()
    nosync = ev64.run(pack, distribution=True, sync=False, **KW)["distribution"]
    assert ev64.steps == LIMIT + 1
    _same_distribution(nosync, b, ev64, "sync=False")
    assert nosync.quantiles(0, 1).tobytes() == a.quantiles(0, 1).tobytes()
    again = ev64.run(pack, distribution=True, **KW)["distribution"]   # the planes are reused
    _same_distribution(again, b, ev64, "second run")


def test_iqn_risk_levels_bound_the_fractions():
    from distributional_rl_decision_and_control_amd.fused_iqn import AdaptiveCvar
    pack = wc.pack(CASE, "bf16")
    ev = _evaluator()
    res = ev.run(pack, distribution=True, cvar=0.25, **KW)
    d = res["distribution"]
    assert d.mismatches == 0
    _g0_is_the_return(res)
    for c, n in enumerate(ev.n_robots):
        for i in range(n):
            assert d.taus(c, i).max() <= np.float32(0.25)
    res = ev.run(pack, distribution=True, histories=True, cvar=AdaptiveCvar(), **KW)
    d, h = res["distribution"], res["history"]
    assert d.mismatches == 0
    _g0_is_the_return(res)
    below = 0
    for c, n in enumerate(ev.n_robots):
        for i in range(n):
            lev = h.cvar(c, i)
            assert len(lev) == d.steps[c][i]
            assert (d.taus(c, i).max(axis=1) <= lev.astype(np.float32)).all(), (c, i)
            below += int((lev < 1.0).sum())
    assert below > 0, "no robot acted below level 1: the run does not exercise the recorded levels"


def test_iqn_numpy_perception_on_the_smallest_config():
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    pack = wc.pack(CASE, "bf16")
    ev = DeviceEvaluator(dev.edited_configs()[0][:1], chunk=7, gamma=GAMMA)
    kw = dict(episode_limit=LIMIT, policy_seed=PSEED, perception="numpy")
    plain = ev.run(pack, **kw)
    res = ev.run(pack, distribution=True, **kw)
    dev.same_results(res, plain, "numpy perception")
    assert res["distribution"].mismatches == 0 and res["draws_n"] is not None
    _g0_is_the_return(res)


def test_ac_iqn_trainer_evaluate():
    from distributional_rl_decision_and_control_amd.fused_critic import critic_forward
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    cfgs = dev.edited_configs()[0]
    tr = VecTrainer(n_envs=8, batch_size=64, agent_type="AC-IQN", buffer_size=4096, graphs=False)
    kw = dict(chunk=7, episode_limit=LIMIT, seed=SEED)
    plain = tr.evaluate(cfgs, **kw)
    res = tr.evaluate(cfgs, distribution=True, histories=True, **kw)
    dev.same_results(res, plain, "AC-IQN with distribution")
    d, h = res["distribution"], res["history"]
    assert d.kind == "critic" and d.mismatches is None
    _g0_is_the_return(res)
    cpack = tr.fused2.local_trunk
    picked = 0
    several = [(c, i) for c, n in enumerate(tr.device_evaluator(cfgs, 7).n_robots) for i in range(n)
               if d.steps[c][i] >= 2]
    assert len(several) >= 3, "three robots that acted more than once"
    for c, i in (several[0], several[len(several) // 2], several[-1]):
        k = int(d.steps[c][i])
        acts = h.action(c, i)
        assert k == len(acts)
        z, tu = d.quantiles(c, i), d.taus(c, i)
        assert tu.min() >= 0.0 and tu.max() < 1.0
        t = k - 1 if picked else k // 2
        x = _rows40(h, c, i, k)[t:t + 1].contiguous()
        a32 = torch.from_numpy(acts[t:t + 1].astype(np.float32)).cuda()
        assert (a32.double().cpu().numpy() == acts[t:t + 1]).all(), "the recorded pair is an f32 value"
        ref = critic_forward(cpack, None, None, torch.from_numpy(tu[t].copy()).cuda(), 32, obs=x, act=a32)
        assert ref.cpu().numpy().tobytes() == z[t].tobytes(), (c, i, t)
        picked += 1
    assert picked == 3
    s = d.summary(terminated_only=False)
    assert abs(s["overall"]["pit"].sum() - 1.0) < 1e-12
    assert s["configs"]["pit"].shape == (len(cfgs), 33) and np.isfinite(s["overall"]["pinball"])
    t = d.summary()
    assert t["overall"]["robots"] >= 1 and abs(t["overall"]["pit"].sum() - 1.0) < 1e-12


def test_refusals():
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    ev = _evaluator()
    iqn = wc.pack(CASE, "bf16")
    actor = wc.pack(wc.CASES["actor"])
    tr = VecTrainer(n_envs=8, batch_size=64, agent_type="AC-IQN", buffer_size=4096, graphs=False)
    critic = tr.fused2.local_trunk
    with pytest.raises(ValueError, match="critic's CriticPack"):
        ev.run(actor, distribution=True, **KW)
    with pytest.raises(ValueError, match="critic's CriticPack"):
        ev.run(actor, distribution=iqn, **KW)
    with pytest.raises(ValueError, match="distribution=True"):
        ev.run(iqn, distribution=critic, **KW)
    for other in ("dqn", "sac", "rainbow"):
        for value in (True, critic):
            with pytest.raises(ValueError, match="distribution is offered for"):
                ev.run(wc.pack(wc.CASES[other]), distribution=value, **KW)
    table = [torch.zeros((LIMIT + 1, g.batch.n_envs * g.batch.max_robots, 2), dtype=torch.float64, device="cuda")
             for g in ev.groups]
    with pytest.raises(ValueError, match="an action table has none"):
        ev.run(actions=table, distribution=True, **KW)
    ddpg = VecTrainer(n_envs=8, batch_size=64, agent_type="DDPG", buffer_size=4096, graphs=False)
    with pytest.raises(ValueError, match="DDPG's critic has none"):
        ddpg.evaluate(dev.edited_configs()[0], distribution=True, episode_limit=LIMIT)
    with pytest.raises(ValueError, match="critic's CriticPack"):
        ev.run(ddpg.learner.actor_pack, distribution=True, **KW)


def test_a_plain_run_allocates_no_distribution_plane():
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    ev = DeviceEvaluator(dev.edited_configs()[0][:2], chunk=7, gamma=GAMMA)
    res = ev.run(wc.pack(CASE, "bf16"), **KW)
    assert "distribution" not in res and "history" not in res
    assert all(grp._dist == {} and grp._hist == {} for grp in ev.groups)
    ev.run(wc.pack(CASE, "bf16"), distribution=True, **KW)
    assert all(list(grp._dist) == [LIMIT + 1] for grp in ev.groups)
