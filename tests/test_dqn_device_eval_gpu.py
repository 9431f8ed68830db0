"""GPU: the device-resident evaluation under DQN (DeviceEvaluator.run with a DqnPack or a discrete action table,
VecTrainer.policy_pack / device_evaluator, Trainer.evaluation(batched="device") on a DQN trainer) on the six eval
configs tests/test_device_eval_gpu.py uses (tests/golden/eval60_ref.npz: 3, 4 and 5 robots, 0 to 4 buoys).

  * closed loop against the composed loop of single launches (dqn_act + step(is_continuous=False) at the same
    Philox keys) with the bookkeeping of trainer.py:286-303 in numpy, both operand builds, episode_limit 22 in
    windows of 5; sync=False and a second run give the first run's bits;
  * teacher-forced: run(actions=index table, is_continuous=False) against evaluate_configs with a DQN agent on the
    configs edited so that every episode ends early and certainly; lengths and successes exact, f64 sums 1e-12;
  * VecTrainer: policy_pack() of a DQN trainer is fused_dqn.local, and an evaluation through device_evaluator()
    leaves the training env, the replay, the step counter and the weight images bit-identical;
  * Trainer.learn with "vectorized": {..., "device_eval": true} and a DQN agent evaluates without evaluate_configs.

Tolerances as in tests/test_device_eval_gpu.py: integers and flags exact; f64 sums 1e-12 relative (pow and summation
order over at most 64 terms of 2.3e-16 each), the return relative to max(1, sum |term|). The weights are a seeded
DQN_Policy (Agent(seed=100, agent_type="DQN"))."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import device_eval_cases as dev
import window_cases as wc
from device_eval_cases import GAMMA
from window_cases import A

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _agent():
    from distributional_rl_decision_and_control_amd.agent import Agent
    return Agent(seed=100, agent_type="DQN")


CASE = dataclasses.replace(wc.CASES["dqn"], net=lambda: _agent().policy_local)


# ------------------------------------------------------------------ closed loop against the composed loop
@pytest.mark.parametrize("operands", ["bf16", "f32"])
def test_closed_loop_matches_single_launches(operands):
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    LIMIT, CHUNK, SEED = 22, 5, 17
    pack = wc.pack(CASE, operands)
    ev = DeviceEvaluator(dev.configs(False), chunk=CHUNK, gamma=GAMMA)
    got = dev.run_thrice(ev, pack, LIMIT, CHUNK, seed=SEED)
    ev.observe(seed=SEED)
    st, taken = dev.composed(ev, 0, CASE, pack, LIMIT, CHUNK, SEED, 0)
    taken = taken[..., 0]   # every action index the loop took
    print(operands, "lengths", got["lengths"], "outcomes", [o.tolist() for o in got["robot_outcomes"]])
    # the inputs cover what they were built for: the windows chain, and the greedy policy is not one constant index
    assert max(got["lengths"]) > CHUNK, "some episode must run past the first window"
    assert ((taken >= 0) & (taken < A) & (taken == np.round(taken))).all() and len(np.unique(taken)) >= 3
    dev.check_group(ev, got, 0, st)


def test_pack_and_flag_must_match():
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    ev = DeviceEvaluator(dev.configs(False)[:1], chunk=5, gamma=GAMMA)
    with pytest.raises(ValueError, match="is_continuous"):
        ev.run(wc.pack(CASE, "bf16"), is_continuous=True)
    with pytest.raises(ValueError, match="is_continuous"):
        ev.run(wc.pack(wc.CASES["actor"]), is_continuous=False)


# ------------------------------------------------------------------ teacher-forced against evaluate_configs
def test_teacher_forced_index_table_against_evaluate_configs(monkeypatch):
    """Column 0 of the table is the action index (column 1 is ignored by the discrete step): the host loop is
    given the same indices. Index 24 adds the largest thrust change to both thrusters: full thrust stays full."""
    from distributional_rl_decision_and_control_amd.policy.batched_eval import evaluate_configs
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    dev.zero_host_noise(monkeypatch)
    cfgs, full = dev.edited_configs()
    T, R = 64, 5
    ev = DeviceEvaluator(cfgs, chunk=5, gamma=GAMMA)
    assert len(ev.groups) == 1 and ev.groups[0].members == list(range(len(cfgs)))
    table = np.zeros((T, len(cfgs) * R, 2))
    table[:, :, 0] = np.random.RandomState(9).randint(0, A, (T, len(cfgs) * R))
    for c, i in full:
        table[:, c * R + i, 0] = A - 1

    def teacher(rows, states, length):
        return [int(table[length[e], e * R + i, 0]) for e, i in rows]

    agent = _agent()
    assert agent.GAMMA == GAMMA
    ref = evaluate_configs(agent, cfgs, policy=teacher)
    got = ev.run(actions=torch.from_numpy(table).cuda(), noise=ev.zero_noise(T), obs_noise=ev.zero_noise(),
                 episode_limit=1000, is_continuous=False)
    dev.check_teacher_forced(got, ref)
    # the inputs cover what they were built for (a condition on the inputs, not a tolerance)
    assert max(ref["lengths"]) < T
    out = got["robot_outcomes"]
    assert out[0].tolist() == [1, 2, 2] and ref["lengths"][0] > 1, "config 0: a goal, then a collision at a later step"
    assert ref["successes"][2] and ref["successes"][4] and not ref["successes"][0]
    assert ref["lengths"][1] == 1 and 2 in out[1].tolist(), "config 1: a collision at the first step"
    # the same table read as thrust commands is another evaluation: the flag reaches the step
    cont = ev.run(actions=torch.from_numpy(table).cuda(), noise=ev.zero_noise(T), obs_noise=ev.zero_noise(),
                  episode_limit=1000)
    assert cont["energies"] != got["energies"]


# ------------------------------------------------------------------ VecTrainer
def test_vec_trainer_policy_pack_and_device_evaluator():
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    cfgs = dev.configs(False)
    tr = VecTrainer(n_envs=37, agent_type="DQN", batch_size=64, buffer_size=4096, graphs=False, seed=3, gamma=GAMMA)
    for _ in range(2):
        tr.iteration()
    torch.cuda.synchronize()
    assert tr.policy_pack() is tr.fused_dqn.local
    watched = dict(training_state=tr.env.batch.rs, flags=tr.env.batch.rflags, step_counter=tr.env.counter,
                   replay_ring=tr.replay.ring, replay_state=tr.replay.state, observation=tr.env.obs_cur,
                   stats=tr.env.batch.stats, params=tr.opt.flat, head_image=tr.fused_dqn.local.head,
                   enc_image=tr.fused_dqn.local.enc, w1_image=tr.fused_dqn.local.w1, w2_image=tr.fused_dqn.local.w2,
                   target_head_image=tr.fused_dqn.target.head)
    before = {k: v.clone() for k, v in watched.items()}
    ev = tr.device_evaluator(cfgs, chunk=5)
    got = ev.run(tr.policy_pack(), episode_limit=22, seed=4)
    torch.cuda.synchronize()
    for k, v in watched.items():
        assert torch.equal(v, before[k]), k
    assert tr.device_evaluator(cfgs, chunk=5) is ev, "the evaluator is cached"
    assert ev.run(tr.policy_pack(), episode_limit=22, seed=4)["rewards"] == got["rewards"]
    ref = DeviceEvaluator(cfgs, chunk=5, gamma=GAMMA).run(tr.fused_dqn.local, episode_limit=22, seed=4)
    assert got["lengths"] == ref["lengths"] and got["successes"] == ref["successes"]
    for name in ("rewards", "times", "energies"):
        assert np.array(got[name]).tobytes() == np.array(ref[name]).tobytes(), name
    assert all(np.isfinite(got["rewards"])) and all(1 <= n <= 23 for n in got["lengths"])
    with pytest.raises(NotImplementedError):
        VecTrainer(n_envs=37, agent_type="IQN", batch_size=64, buffer_size=4096, graphs=False).policy_pack()


# ------------------------------------------------------------------ Trainer
def test_trainer_device_eval_dqn(tmp_path, monkeypatch):
    dev.check_trainer_device_eval(tmp_path, monkeypatch, "DQN", 8)
