"""GPU: SAC on the batched loop (VecTrainer(agent_type="SAC")). Shape: 37 envs x 5 robots (185 rows: a partial last
tile), B = 64, buffer 4096.

  * the learner table's facts: fused_sac is the only fused field set, a continuous 2-d action, three optimisers;
  * the closed-loop windows and the device evaluation are refused (a sampled head inside the env kernel is not
    built), and so is the dependency-chained schedule;
  * iteration() is the composition act, env.step, _push, auto_reset, advance_device, learn (and the hard update every
    target_update_interval learn steps) bit for bit;
  * the captured graph (one and two iterations per replay) equals the eager two-stream schedule bit for bit;
  * load_policies from a twin with another net_seed then trains like the source bit for bit, through hard updates;
  * after 12 iterations all losses and weights are finite, and tr.local.save() / SAC_Policy.load() round-trips."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPE = dict(n_envs=37, agent_type="SAC", batch_size=64, buffer_size=4096)
FUSED = ("fused2", "fused_iqn", "fused_rb", "fused_dqn", "fused_ddpg", "fused_sac")
NETS = ("actor", "critic_1", "critic_2")


def _trainer(**kw):
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    return VecTrainer(**dict(SHAPE, **kw))


def _flat(policy):
    return torch.cat([p.detach().reshape(-1) for kind in NETS for p in getattr(policy, kind).parameters()])


def _state(tr):
    st = tr.fused_sac
    d = dict(ring=tr.replay.ring, ring_state=tr.replay.state, step_counter=tr.env.counter,
             learn_counter=tr.learn_counter, target=_flat(tr.target), env=tr.env.batch.rs, obs=tr.env.obs_cur,
             target_actor_w1_image=st.target_actor.w1, target_actor_head=st.target_actor.head)
    for name, o in (("actor", tr.actor_opt), ("critic_1", tr.critic_opts[0]), ("critic_2", tr.critic_opts[1])):
        d[name + "_params"], d[name + "_exp_avg"], d[name + "_exp_avg_sq"] = o.flat, o.exp_avg, o.exp_avg_sq
        d[name + "_step"] = o.step_t
    for k in range(2):
        for img in ("enc", "w1", "w2", "wo", "bo"):
            d[f"critic_{k + 1}_{img}_image"] = getattr(st.local[k], img)
        d[f"target_{k + 1}_w2_image"] = st.target[k].w2
    for k in ("enc", "b_enc", "w1", "w2", "w1t", "w2t", "b1", "b2", "head", "bhead"):   # the current actor image set
        d["actor_" + k] = getattr(st.actor, k)
    return d


def _assert_same(a, b):
    torch.cuda.synchronize()
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_learner_facts_and_refusals():
    from distributional_rl_decision_and_control_amd.fused_sac import FusedSACState
    from distributional_rl_decision_and_control_amd.learner import FusedAdam
    from distributional_rl_decision_and_control_amd.policy.SAC_model import SAC_Policy
    tr = _trainer(graphs=False)
    assert [f for f in FUSED if getattr(tr, f) is not None] == ["fused_sac"]
    assert isinstance(tr.fused_sac, FusedSACState) and tr.learner is tr.fused_sac
    assert isinstance(tr.local, SAC_Policy) and isinstance(tr.target, SAC_Policy)
    assert tr.continuous and tr.action_dim == 2 and tr.replay is not None and tr.per is None and not tr.chain
    assert isinstance(tr.actor_opt, FusedAdam) and len(tr.critic_opts) == 2
    assert all(isinstance(o, FusedAdam) for o in tr.critic_opts) and tr.critic_opts[0] is not tr.critic_opts[1]
    assert not hasattr(tr, "critic_opt")
    assert tr.fused_sac.policy_pack is None and tr.fused_sac.actor_pack is None
    with pytest.raises(NotImplementedError):
        tr.policy_pack()
    with pytest.raises(NotImplementedError):
        tr.collect(4)
    with pytest.raises(NotImplementedError):
        tr.greedy_episodes(max_steps=4)
    with pytest.raises(NotImplementedError):
        tr.evaluate([])
    with pytest.raises(ValueError, match="chained"):
        _trainer(graphs=True, unroll=2, chain=True)
    with pytest.raises(ValueError, match="SAC learner kernels"):
        _trainer(graphs=False, batch_size=48)


def test_iteration_equals_hand_composed_steps():
    a = _trainer(graphs=False, overlap=False, seed=3, target_update_interval=2)
    b = _trainer(graphs=False, overlap=False, seed=3, target_update_interval=2)
    assert a.fused_sac.actor.double and not a._chained()
    init_target = _flat(a.target).clone()
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
            assert len(out_a) == 6
            for x, y in zip(out_a, out_b):
                assert torch.equal(x, y) and bool(torch.isfinite(x)), it
            assert all(out_a[k].item() > 0 for k in (0, 1, 3, 4, 5))   # two MSE losses, three gradient norms
        _assert_same(a, b)
        assert a.fused_sac.actor.parity == b.fused_sac.actor.parity == learned % 2
    assert a.learn_steps == learned >= 4 and int(a.learn_counter.item()) == learned
    # a hard update fired: the target left its initial weights; the loop's actions are continuous pairs in [-1, 1]
    assert not torch.equal(_flat(a.target), init_target)
    assert torch.equal(_flat(a.target), _flat(a.local)) == (learned % 2 == 0)
    assert bool((a.actions.abs() <= 1).all()) and bool((a.actions[:, 1] != 0).any())


def _run(graphs, unroll, learn_iters):
    tr = _trainer(graphs=graphs, unroll=unroll, overlap=True, seed=21, learning_starts=256)
    assert tr.chain is False   # chain=None resolves to the joined schedule
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
    # two actor image sets only where a replay ends on the set it started from
    assert g.fused_sac.actor.double == (unroll % 2 == 0)
    e, out_e = _run(False, unroll, 9)
    assert e.fused_sac.actor.double
    assert int(g.env.counter.item()) == int(e.env.counter.item())
    assert int(g.learn_counter.item()) == int(e.learn_counter.item()) == 9
    for x, y in zip(out_g, out_e):
        assert bool(torch.isfinite(x)) and torch.equal(x, y)
    _assert_same(g, e)


def test_load_policies_then_trains_like_the_source():
    """A twin built with another net_seed takes the source's networks, then both train alike through two hard
    updates: all three networks, on both sides, were copied and re-packed."""
    kw = dict(graphs=False, overlap=False, seed=5, target_update_interval=2, learning_starts=185)
    src, twin = _trainer(net_seed=100, **kw), _trainer(net_seed=7, **kw)
    assert not torch.equal(_flat(src.local), _flat(twin.local))
    with torch.no_grad():   # a target that differs from the local nets must arrive as it is
        for p in src.target.critic_2.parameters():
            p.mul_(1.25)
        src.fused_sac.target_changed()
    twin.load_policies(src.local, src.target)
    assert torch.equal(_flat(src.local), _flat(twin.local)) and torch.equal(_flat(src.target), _flat(twin.target))
    for _ in range(6):
        oa, ob = src.iteration(), twin.iteration()
        assert (oa is None) == (ob is None)
        if oa is not None:
            for x, y in zip(oa, ob):
                assert torch.equal(x, y)
        _assert_same(src, twin)
    assert src.learn_steps >= 4


def test_twelve_iterations_stay_finite_and_checkpoint_round_trips(tmp_path):
    import os

    from distributional_rl_decision_and_control_amd.policy.SAC_model import SAC_Policy
    tr = _trainer(graphs=False, seed=9, learning_starts=185)
    losses = []
    for _ in range(12):
        out = tr.iteration()
        if out is not None:
            losses.append([v.item() for v in out])
    torch.cuda.synchronize()
    assert len(losses) >= 10
    assert all(all(x == x and abs(x) < 1e30 for x in row) for row in losses), losses
    assert bool(torch.isfinite(_flat(tr.local)).all()) and bool(torch.isfinite(_flat(tr.target)).all())
    tr.local.save(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["actor_constructor_params.json", "actor_network_params.pth",
                                            "critic_1_constructor_params.json", "critic_1_params.pth",
                                            "critic_2_constructor_params.json", "critic_2_params.pth"]
    back = SAC_Policy.load(str(tmp_path), device="cuda")
    for kind in NETS:
        a, b = getattr(tr.local, kind).state_dict(), getattr(back, kind).state_dict()
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (kind, k)
