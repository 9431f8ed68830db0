"""GPU: the learner surface VecTrainer calls through (learners.LEARNERS and the five Fused*State classes), for every
batched agent type at the smallest shape the loop takes: 37 envs x 5 robots (185 rows: a partial last tile), B = 64,
N = 8, buffer 4096, eager.

  * the trainer holds one learner: the one fused field that is not None; policy_pack() is the learner's, or raises for
    the types that act inside their own kernels; continuous / action_dim are the table's;
  * load_policies for every type: a trainer that loads another trainer's networks over its own initialisation trains
    bit for bit like it, through refresh_local() and, at every hard update, target_changed()."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPE = dict(n_envs=37, batch_size=64, num_tau=8, buffer_size=4096, graphs=False)
TYPES = ("AC-IQN", "IQN", "Rainbow", "DQN", "DDPG")
FIELDS = ("fused2", "fused_iqn", "fused_rb", "fused_dqn", "fused_ddpg")


def _trainer(agent_type, **kw):
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    return VecTrainer(**dict(SHAPE, agent_type=agent_type, **kw))


def _params(policy):
    mods = [policy.actor, policy.critic] if hasattr(policy, "actor") else [policy]
    return [p.detach() for m in mods for p in m.parameters()]


@pytest.mark.parametrize("agent_type", TYPES)
def test_surface(agent_type):
    from distributional_rl_decision_and_control_amd.learners import LEARNERS
    spec = LEARNERS[agent_type]
    tr = _trainer(agent_type)
    held = [f for f in FIELDS if getattr(tr, f) is not None]
    assert held == [spec.field] and tr.learner is getattr(tr, spec.field)
    assert tr.continuous == spec.continuous == (agent_type in ("AC-IQN", "DDPG"))
    assert tr.action_dim == spec.action_dim == (2 if tr.continuous else 1)
    assert (tr.per is not None) == spec.per == (agent_type == "Rainbow") and (tr.replay is None) == spec.per
    assert isinstance(tr.local, spec.policy) and isinstance(tr.target, spec.policy)
    if agent_type in ("IQN", "Rainbow"):
        assert tr.learner.policy_pack is None and tr.learner.actor_pack is None
        with pytest.raises(NotImplementedError):
            tr.policy_pack()
    else:
        assert tr.learner.policy_pack is not None and tr.policy_pack() is tr.learner.policy_pack
        if agent_type == "DQN":
            assert tr.learner.actor_pack is None and tr.policy_pack() is tr.fused_dqn.local
        else:
            assert tr.learner.actor_pack is tr.policy_pack() is tr.learner.actor
    # one name per purpose: what _collect_window takes and what DeviceEvaluator.run takes
    if agent_type == "Rainbow":
        assert tr.learner.window_pack.noisy and tr.learner.window_pack.image is tr.fused_rb.img
        assert not tr.learner.eval_pack.noisy and tr.learner.eval_pack is not tr.learner.window_pack
    else:
        want = {"AC-IQN": lambda: tr.fused2.actor, "DDPG": lambda: tr.fused_ddpg.actor,
                "DQN": lambda: tr.fused_dqn.local, "IQN": lambda: tr.fused_iqn.local}[agent_type]()
        assert tr.learner.window_pack is want and tr.learner.eval_pack is want


def test_sac_window_and_eval_packs():
    """The sixth batched agent type: both names are the local actor's pack, and the refusals stay."""
    tr = _trainer("SAC")
    assert tr.learner is tr.fused_sac and tr.learner.window_pack is tr.learner.eval_pack is tr.fused_sac.actor
    assert tr.learner.policy_pack is None and tr.learner.actor_pack is None
    with pytest.raises(NotImplementedError):
        tr.policy_pack()


@pytest.mark.parametrize("agent_type", TYPES)
def test_load_policies_then_trains_like_the_source(agent_type):
    kw = dict(seed=3, target_update_interval=2)
    a = _trainer(agent_type, net_seed=100, **kw)
    b = _trainer(agent_type, net_seed=7, **kw)
    assert not all(torch.equal(p, q) for p, q in zip(_params(a.local), _params(b.local)))
    b.load_policies(a.local, a.target)
    for _ in range(12):   # learning starts within 6 iterations (Rainbow: four pushes of 185 rows + a batch)
        a.iteration()
        b.iteration()
    torch.cuda.synchronize()
    assert a.learn_steps == b.learn_steps >= 5, "at least two hard updates (every 2 learn steps)"
    assert int(a.learn_counter.item()) == int(b.learn_counter.item()) == a.learn_steps
    for name in ("local", "target"):
        pa, pb = _params(getattr(a, name)), _params(getattr(b, name))
        assert len(pa) == len(pb) > 0
        for k, (p, q) in enumerate(zip(pa, pb)):
            assert torch.equal(p, q) and bool(torch.isfinite(p).all()), (name, k)
    assert len(a.last_losses) == len(b.last_losses) >= 2
    for k, (x, y) in enumerate(zip(a.last_losses, b.last_losses)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all()), k
