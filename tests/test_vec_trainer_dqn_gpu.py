"""GPU: DQN on the batched loop (VecTrainer(agent_type="DQN")) and through the drop-in Trainer.learn with a
"vectorized" schedule block. Shape: 37 envs x 5 robots (185 rows: a partial last tile), B = 64, buffer 4096.

  * iteration() is the composition act, env.step, _push, auto_reset, advance_device, learn (and the hard update every
    target_update_interval learn steps) bit for bit;
  * the captured graph (one and two iterations per replay) equals the eager two-stream schedule bit for bit;
  * load_policies starts from a drop-in agent's networks: the act kernel's greedy actions are that network's arg-max;
  * the closed-loop windows stay AC-IQN only;
  * Trainer.learn runs the batched loop for a DQN agent, evaluates, checkpoints, and hands the trained networks back."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPE = dict(n_envs=37, agent_type="DQN", batch_size=64, buffer_size=4096)


def _trainer(**kw):
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    return VecTrainer(**dict(SHAPE, **kw))


def _state(tr):
    return dict(ring=tr.replay.ring, ring_state=tr.replay.state, step_counter=tr.env.counter,
                learn_counter=tr.learn_counter, params=tr.opt.flat, target=torch.cat(
                    [p.detach().reshape(-1) for p in tr.target.parameters()]),
                exp_avg=tr.opt.exp_avg, exp_avg_sq=tr.opt.exp_avg_sq, env=tr.env.batch.rs, obs=tr.env.obs_cur,
                head_image=tr.fused_dqn.local.head, w1_image=tr.fused_dqn.local.w1,
                target_head_image=tr.fused_dqn.target.head)


def _assert_same(a, b):
    torch.cuda.synchronize()
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_iteration_equals_hand_composed_steps():
    a = _trainer(graphs=False, overlap=False, seed=3, target_update_interval=2)
    b = _trainer(graphs=False, overlap=False, seed=3, target_update_interval=2)
    assert a.action_dim == 1 and not a.continuous and a.replay is not None and a.per is None and not a._chained()
    init_target = torch.cat([p.detach().reshape(-1).clone() for p in a.target.parameters()])
    learned = 0
    for it in range(6):
        out_a = a.iteration()
        do_learn = b.replay_size_host() >= b.learning_starts
        b.act()
        b.env.step(b.actions)
        counted = b._push()
        b.env.auto_reset(counted)
        b.env.advance_device(counted)
        out_b = b.learn() if do_learn else None
        b.env.advance_host()
        if do_learn:
            learned += 1
            if learned % 2 == 0:
                b.hard_update()
        assert (out_a is None) == (out_b is None), it
        if out_a is not None:
            assert torch.equal(out_a[0], out_b[0]) and torch.equal(out_a[1], out_b[1]), it
            assert bool(torch.isfinite(out_a[0])) and out_a[1].item() > 0
        _assert_same(a, b)
    assert a.learn_steps == learned >= 4 and int(a.learn_counter.item()) == learned
    # a hard update fired: the target left its initial weights and the loop's actions are discrete indices
    assert not torch.equal(torch.cat([p.detach().reshape(-1) for p in a.target.parameters()]), init_target)
    acts = a.actions[:, 0]
    assert bool(((acts >= 0) & (acts < 25) & (acts == acts.round())).all()) and bool((a.actions[:, 1] == 0).all())


def _run(graphs, unroll, learn_iters):
    tr = _trainer(graphs=graphs, unroll=unroll, overlap=True, seed=21, learning_starts=256)
    assert tr.chain is False   # chain=None resolves as for IQN: the joined schedule
    while tr.replay_size_host() < tr.learning_starts:
        tr.iteration()
    for _ in range(learn_iters):
        out = tr.iteration()
    torch.cuda.synchronize()
    return tr, out


@pytest.mark.parametrize("unroll", [1, 2])
def test_graph_equals_eager_overlapped_schedule(unroll):
    """Six learning iterations from the captured graph. The capture warms up with three eager iterations of the
    same body, so the eager twin runs nine: the same operations on the same data."""
    g, out_g = _run(True, unroll, 6)
    assert g.graphs and g._graph is not None, "the graph was captured"
    e, out_e = _run(False, unroll, 9)
    assert int(g.env.counter.item()) == int(e.env.counter.item())
    assert int(g.learn_counter.item()) == int(e.learn_counter.item()) == 9
    assert bool(torch.isfinite(out_g[0])) and torch.equal(out_g[0], out_e[0]) and torch.equal(out_g[1], out_e[1])
    _assert_same(g, e)


def test_load_policies_then_act_is_the_agents_argmax():
    from distributional_rl_decision_and_control_amd.agent import Agent
    ag = Agent(seed=5, agent_type="DQN")
    tr = _trainer(graphs=False, operands="f32", seed=4, initial_eps=0.0, final_eps=0.0)
    before = tr.opt.flat.clone()
    tr.load_policies(ag.policy_local, ag.policy_target)
    assert not torch.equal(before, tr.opt.flat)
    for (n1, p), (n2, q) in zip(ag.policy_local.state_dict().items(), tr.local.state_dict().items()):
        assert n1 == n2 and torch.equal(p, q), n1
    tr.act()
    x = tr.env.obs_cur
    with torch.no_grad():
        q_ref = ag.policy_local((x[:, 0:7], x[:, 7:32].reshape(-1, 5, 5), x[:, 32:37]))
    top2 = q_ref.topk(2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-4 * float(q_ref.abs().max()), "a near tie in the test rows"
    assert torch.equal(tr.actions[:, 0].long(), q_ref.argmax(1))


def test_closed_loop_windows_stay_ac_iqn_only():
    tr = _trainer(graphs=False)
    with pytest.raises(NotImplementedError):
        tr.collect(4)
    with pytest.raises(NotImplementedError):
        tr.greedy_episodes(max_steps=4)
    with pytest.raises(NotImplementedError):
        tr.evaluate([])


def test_trainer_learn_vectorized_dqn(tmp_path):
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.envs.marinenav.env import MarineNavEnv3
    from distributional_rl_decision_and_control_amd.policy.trainer import Trainer
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    E = 64
    sched = {"timesteps": [0], "num_robots": [3], "num_cores": [0], "num_obstacles": [2], "min_start_goal_dis": [30.0],
             "vectorized": {"n_envs": E, "batch_size": 64, "buffer_size": 8192, "graphs": False}}
    eval_sched = {"num_episodes": [1], "num_robots": [3], "num_cores": [0], "num_obstacles": [2],
                  "min_start_goal_dis": [30.0]}
    torch.manual_seed(0)
    agent = Agent(seed=100, agent_type="DQN")
    init = [p.detach().clone() for p in agent.policy_local.parameters()]
    trainer = Trainer(MarineNavEnv3(seed=1, schedule=sched), MarineNavEnv3(seed=253, is_eval_env=True), eval_sched,
                      agent, learning_starts=100)
    vt = trainer.learn(total_timesteps=E * 8, eval_freq=E * 4, eval_log_path=str(tmp_path), verbose=False)
    assert isinstance(vt, VecTrainer) and vt is trainer.vec_trainer
    assert vt.agent_type == "DQN" and vt.fused_dqn is not None and vt.learn_steps >= 4
    assert len(trainer.eval_timesteps) >= 2 and trainer.eval_timesteps[-1] == E * 8
    assert all(np.isfinite(trainer.eval_rewards[-1]))
    for f in ("evaluations.npz", "network_params.pth", "constructor_params.json"):
        assert os.path.exists(os.path.join(str(tmp_path), f)), f
    ev = np.load(os.path.join(str(tmp_path), "evaluations.npz"), allow_pickle=True)   # our own file
    assert list(ev["timesteps"]) == trainer.eval_timesteps
    # rl_agent holds the batched loop's trained networks, and so does the checkpoint
    for (n1, p), (n2, q) in zip(agent.policy_local.state_dict().items(), vt.local.state_dict().items()):
        assert n1 == n2 and torch.equal(p, q), n1
    assert any(not torch.equal(p, q) for p, q in zip(init, agent.policy_local.parameters()))
    loaded = Agent(agent_type="DQN")
    loaded.load_model(str(tmp_path))
    for (n1, p), (n2, q) in zip(loaded.policy_local.state_dict().items(), vt.local.state_dict().items()):
        assert n1 == n2 and torch.equal(p.cpu(), q.cpu()), n1
