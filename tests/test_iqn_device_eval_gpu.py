"""GPU: the device-resident evaluation under IQN (DeviceEvaluator.run with an IqnPack: greedy over the mean of K = 32
quantile samples drawn per act, at a risk level cvar) on the six eval configs tests/test_device_eval_gpu.py uses
(tests/golden/eval60_ref.npz: 3, 4 and 5 robots, 0 to 4 buoys) plus two of them again under another timestep
penalty, which makes a second parameter group of two envs.

  * closed loop against the composed loop of single launches (iqn_act + step(is_continuous=False) at the same Philox
    keys: env noise seed + g, quantile fractions policy_seed + g for group g) with the bookkeeping of
    trainer.py:286-303 in numpy, both operand builds, cvar 1 and 0.25, episode_limit 22 in windows of 5; sync=False
    and a second run give the first run's bits;
  * policy_seed: the same seed gives the same bits, another seed other results; group g runs under policy_seed + g;
  * cvar and is_continuous are checked against the pack;
  * VecTrainer(agent_type="IQN"): device_evaluator(cfgs).run(fused_iqn.window_pack) leaves the training env, the
    ring, the step and learn counters and the weight images bit-identical, evaluates the current images after 12
    iterations, and policy_pack() still raises;
  * Trainer.learn with "device_eval": true and an IQN agent evaluates without evaluate_configs.

Tolerances as in tests/test_device_eval_gpu.py: integers and flags exact; f64 sums 1e-12 relative (pow and summation
order over at most 64 terms of 2.3e-16 each), the return relative to max(1, sum |term|). The weights are a seeded
IQN_Policy."""
import numpy as np
import pytest
import torch

import device_eval_cases as dev
import window_cases as wc
from device_eval_cases import CHUNK, GAMMA, LIMIT, PSEED, SEED

pytestmark = pytest.mark.gpu

CASE = wc.CASES["iqn"]


# ------------------------------------------------------------------ closed loop against the composed loop
@pytest.mark.parametrize("cvar", [1.0, 0.25])
@pytest.mark.parametrize("operands", ["bf16", "f32"])
def test_closed_loop_matches_single_launches(operands, cvar):
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    pack = wc.pack(CASE, operands)
    ev = DeviceEvaluator(dev.configs(True), chunk=CHUNK, gamma=GAMMA)
    assert [grp.members for grp in ev.groups] == [[0, 1, 2, 3, 4, 5], [6, 7]]
    kw = dict(seed=SEED, policy_seed=PSEED, cvar=cvar)
    got = dev.run_thrice(ev, pack, LIMIT, CHUNK, **kw)
    print(operands, cvar, "lengths", got["lengths"], "outcomes", [o.tolist() for o in got["robot_outcomes"]])
    assert max(got["lengths"]) > CHUNK, "some episode must run past the first window"
    if cvar != 1.0:
        other = ev.run(pack, episode_limit=LIMIT, **dict(kw, cvar=1.0))
        assert dev.differ(got, other), "cvar = 0.25 is another evaluation than cvar = 1"
    ev.observe(seed=SEED)
    for g in range(len(ev.groups)):
        st, taken = dev.composed(ev, g, CASE, pack, LIMIT, CHUNK, SEED, PSEED, cvar=cvar)
        assert (taken[..., 0] == np.round(taken[..., 0])).all() and taken[..., 0].min() >= 0
        assert taken[..., 0].max() <= wc.A - 1 and (taken[..., 1] == 0.0).all()
        dev.check_group(ev, got, g, st)


def test_policy_seed_and_groups(monkeypatch):
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    pack = wc.pack(CASE, "bf16")
    ev = DeviceEvaluator(dev.configs(True), chunk=CHUNK, gamma=GAMMA)
    seen = dev.spy_on_rollouts(monkeypatch, ev, "cvar")
    kw = dict(seed=SEED, episode_limit=LIMIT)
    a = ev.run(pack, policy_seed=PSEED, **kw)
    assert seen and {s[0] for s in seen} == {0, 1}
    assert all(s[1] == PSEED + s[0] and s[2] == 1.0 for s in seen), "group g runs under policy_seed + g"
    dev.same_results(ev.run(pack, policy_seed=PSEED, **kw), a, "the same policy_seed")
    other = ev.run(pack, policy_seed=PSEED + 50, **kw)
    assert dev.differ(other, a), "another policy_seed draws other quantile fractions"
    seen.clear()
    ev.run(pack, policy_seed=PSEED, cvar=0.25, **kw)
    assert seen and all(s[2] == 0.25 for s in seen)


def test_value_errors():
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    ev = DeviceEvaluator(dev.configs(False)[:1], chunk=5, gamma=GAMMA)
    pack = wc.pack(CASE, "bf16")
    for cvar in (0.0, -1.0, 1.25):
        with pytest.raises(ValueError, match="cvar"):
            ev.run(pack, cvar=cvar)
    with pytest.raises(ValueError, match="cvar"):
        ev.run(wc.pack(wc.CASES["actor"]), cvar=0.5)
    with pytest.raises(ValueError, match="cvar"):
        ev.run(wc.pack(wc.CASES["dqn"], "bf16"), cvar=0.5)
    with pytest.raises(ValueError, match="is_continuous"):
        ev.run(pack, is_continuous=True)
    with pytest.raises(ValueError, match="deterministic"):
        ev.run(pack, deterministic=True)
    with pytest.raises(ValueError, match="not both"):
        ev.run(pack, actions=torch.zeros((2, 5, 2), dtype=torch.float64, device="cuda"))
    # is_continuous=False agrees with the pack
    dev.same_results(ev.run(pack, episode_limit=LIMIT, is_continuous=False), ev.run(pack, episode_limit=LIMIT),
                     "discrete")


# ------------------------------------------------------------------ VecTrainer
def test_vec_trainer_window_pack_and_device_evaluator():
    from distributional_rl_decision_and_control_amd.fused_iqn import IqnPack
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    cfgs = dev.configs(True)
    tr = VecTrainer(agent_type="IQN", n_envs=37, batch_size=64, buffer_size=4096, graphs=False)
    st = tr.fused_iqn
    assert st.window_pack is st.local and st.policy_pack is None and st.actor_pack is None
    with pytest.raises(NotImplementedError):
        tr.policy_pack()
    for _ in range(2):
        tr.iteration()
    torch.cuda.synchronize()

    def watched():
        w = dict(training_state=tr.env.batch.rs, flags=tr.env.batch.rflags, ep_ts=tr.env.batch.ep_ts,
                 step_counter=tr.env.counter, learn_counter=tr.learn_counter, replay_ring=tr.replay.ring,
                 replay_state=tr.replay.state, observation=tr.env.obs_cur, stats=tr.env.batch.stats,
                 head_img=st.local.head_img)
        for k in ("wc", "w1", "w2", "w2t", "w1t"):
            w["local_" + k] = getattr(st.local, k)
        return w
    before = {k: v.clone() for k, v in watched().items()}
    host = (tr.learn_steps, tr.env.total_timesteps)
    ev = tr.device_evaluator(cfgs, chunk=CHUNK)
    got = ev.run(st.window_pack, episode_limit=LIMIT, seed=4, policy_seed=PSEED)
    torch.cuda.synchronize()
    for k, v in watched().items():
        assert torch.equal(v, before[k]), k
    assert host == (tr.learn_steps, tr.env.total_timesteps)
    assert tr.device_evaluator(cfgs, chunk=CHUNK) is ev, "the evaluator is cached"
    assert all(np.isfinite(got["rewards"])) and all(1 <= n <= LIMIT + 1 for n in got["lengths"])
    for _ in range(10):
        tr.iteration()
    torch.cuda.synchronize()
    assert tr.learn_steps >= 8, "the network must have been updated"
    now = ev.run(st.window_pack, episode_limit=LIMIT, seed=4, policy_seed=PSEED)
    fresh = IqnPack(tr.local, st.operands)
    ref = DeviceEvaluator(cfgs, chunk=CHUNK, gamma=tr.gamma).run(fresh, episode_limit=LIMIT, seed=4, policy_seed=PSEED)
    dev.same_results(now, ref, "the current images against a fresh pack of tr.local")
    dev.same_results(ev.run(st.window_pack, episode_limit=LIMIT, seed=4, cvar=0.25),
                  DeviceEvaluator(cfgs, chunk=CHUNK, gamma=tr.gamma).run(fresh, episode_limit=LIMIT, seed=4, cvar=0.25),
                  "current images, cvar = 0.25")
    for refused in (tr.policy_pack, lambda: tr.collect(2), tr.greedy_episodes, lambda: tr.evaluate(cfgs)):
        with pytest.raises(NotImplementedError):
            refused()


# ------------------------------------------------------------------ Trainer
def test_trainer_device_eval_iqn(tmp_path, monkeypatch):
    dev.check_trainer_device_eval(tmp_path, monkeypatch, "IQN", 8)
