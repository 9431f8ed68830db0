"""GPU: the device-resident evaluation under SAC (DeviceEvaluator.run with a SacActorPack, sampled as act_sac samples
in evaluation too, or deterministic=True: the mean action) on the six eval configs tests/test_device_eval_gpu.py uses
(tests/golden/eval60_ref.npz: 3, 4 and 5 robots, 0 to 4 buoys) plus two of them again under another timestep
penalty, which makes a second parameter group of two envs.

  * closed loop against the composed loop of single launches (sac_act + step at the same Philox keys: env noise
    seed + g, action noise policy_seed + g for group g) with the bookkeeping of trainer.py:286-303 in numpy, both
    operand builds, sampled and deterministic, episode_limit 22 in windows of 5; sync=False and a second run give
    the first run's bits;
  * policy_seed: the same seed gives the same bits, another seed other sampled results and the same deterministic
    ones; group g is run under policy_seed + g;
  * deterministic=True is refused for the Actor's and DQN's packs;
  * VecTrainer(agent_type="SAC"): device_evaluator(cfgs).run(fused_sac.window_pack) leaves the training env, the
    ring, the step and learn counters and the weight images bit-identical, evaluates the current image set after 12
    iterations, and policy_pack() still raises.

Tolerances as in tests/test_device_eval_gpu.py: integers and flags exact; f64 sums 1e-12 relative (pow and summation
order over at most 64 terms of 2.3e-16 each), the return relative to max(1, sum |term|). The weights are a seeded
SAC_Policy's actor."""
import numpy as np
import pytest
import torch

import device_eval_cases as dev
import window_cases as wc
from device_eval_cases import CHUNK, GAMMA, LIMIT, PSEED, SEED

pytestmark = pytest.mark.gpu

CASE = wc.CASES["sac"]


# ------------------------------------------------------------------ closed loop against the composed loop
@pytest.mark.parametrize("deterministic", [False, True], ids=["sampled", "deterministic"])
@pytest.mark.parametrize("operands", ["bf16", "f32"])
def test_closed_loop_matches_single_launches(operands, deterministic):
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    pack = wc.pack(CASE, operands)
    ev = DeviceEvaluator(dev.configs(True), chunk=CHUNK, gamma=GAMMA)
    assert [grp.members for grp in ev.groups] == [[0, 1, 2, 3, 4, 5], [6, 7]]
    got = dev.run_thrice(ev, pack, LIMIT, CHUNK, seed=SEED, policy_seed=PSEED, deterministic=deterministic)
    print(operands, "lengths", got["lengths"], "outcomes", [o.tolist() for o in got["robot_outcomes"]])
    assert max(got["lengths"]) > CHUNK, "some episode must run past the first window"
    ev.observe(seed=SEED)
    first = []
    for g in range(len(ev.groups)):
        st, taken = dev.composed(ev, g, CASE, pack, LIMIT, CHUNK, SEED, PSEED, deterministic=deterministic)
        first.append(taken[0])
        assert np.isfinite(taken).all() and (np.abs(taken) <= 1.0).all()
        assert len(np.unique(taken[0])) > taken[0].size // 4
        dev.check_group(ev, got, g, st)
    # configs 6 and 7 start where 2 and 3 start, at batch-local rows 0..9 of their group: under one seed their first
    # actions would repeat rows 0..9 of group 0's draws. They are drawn under policy_seed + 1 (and act on another
    # observation noise, seed + 1), so no row agrees; without noise in the action, rows may.
    R = ev.groups[0].batch.max_robots
    if not deterministic:
        assert (first[1] != first[0][:first[1].shape[0]]).any(-1).all()
        assert (first[1] != first[0][2 * R:2 * R + first[1].shape[0]]).any(-1).all()


def test_policy_seed_and_groups(monkeypatch):
    from distributional_rl_decision_and_control_amd.fused_sac import sac_act
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    pack = wc.pack(CASE, "bf16")
    ev = DeviceEvaluator(dev.configs(True), chunk=CHUNK, gamma=GAMMA)
    seen = dev.spy_on_rollouts(monkeypatch, ev, "deterministic")
    kw = dict(seed=SEED, episode_limit=LIMIT)
    a = ev.run(pack, policy_seed=PSEED, **kw)
    assert seen and {s[0] for s in seen} == {0, 1}
    assert all(s[1] == PSEED + s[0] and s[2] is False for s in seen), "group g runs under policy_seed + g"
    dev.same_results(ev.run(pack, policy_seed=PSEED, **kw), a, "the same policy_seed")
    other = ev.run(pack, policy_seed=PSEED + 50, **kw)
    assert other["rewards"] != a["rewards"], "another policy_seed is another sampled evaluation"
    seen.clear()
    d0 = ev.run(pack, policy_seed=PSEED, deterministic=True, **kw)
    assert seen and all(s[2] is True for s in seen)
    dev.same_results(ev.run(pack, policy_seed=PSEED + 50, deterministic=True, **kw), d0,
                     "deterministic: no draw is used")
    assert d0["rewards"] != a["rewards"], "the mean action is another evaluation than the sampled one"
    dev.same_results(ev.run(pack, deterministic=True, **kw), d0, "policy_seed defaults to 0; unused when deterministic")
    # two seeds that differ by one (two groups) share no draw: the eps of every row differs
    x = ev.groups[0].batch.obs
    n = x.shape[0]
    act, step = torch.zeros((n, 2), dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    e0, e1 = (torch.zeros((n, 2), dtype=torch.float32, device="cuda") for _ in range(2))
    sac_act(pack, x, act, e0, step, 1.0, 1.0, 1.0, 0.0, 0.0, PSEED)
    sac_act(pack, x, act, e1, step, 1.0, 1.0, 1.0, 0.0, 0.0, PSEED + 1)
    assert bool((e0 != e1).all())


def test_deterministic_is_the_sampled_actors_own():
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    ev = DeviceEvaluator(dev.configs(False)[:1], chunk=5, gamma=GAMMA)
    actor = wc.pack(wc.CASES["actor"])
    with pytest.raises(ValueError, match="deterministic"):
        ev.run(actor, deterministic=True)
    with pytest.raises(ValueError, match="deterministic"):
        ev.run(wc.pack(wc.CASES["dqn"], "bf16"), deterministic=True)
    # for the Actor's pack nothing changes: the greedy schedule uses no draw, whatever the seed
    dev.same_results(ev.run(actor, episode_limit=LIMIT, policy_seed=5), ev.run(actor, episode_limit=LIMIT), "Actor")


# ------------------------------------------------------------------ VecTrainer
def test_vec_trainer_window_pack_and_device_evaluator():
    from distributional_rl_decision_and_control_amd.fused_sac import SacActorPack
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    cfgs = dev.configs(True)
    tr = VecTrainer(agent_type="SAC", n_envs=37, batch_size=64, buffer_size=4096, graphs=False)
    st = tr.fused_sac
    assert st.window_pack is st.actor and st.policy_pack is None and st.actor_pack is None
    with pytest.raises(NotImplementedError):
        tr.policy_pack()
    for _ in range(2):
        tr.iteration()
    torch.cuda.synchronize()

    def watched():
        w = dict(training_state=tr.env.batch.rs, flags=tr.env.batch.rflags, ep_ts=tr.env.batch.ep_ts,
                 step_counter=tr.env.counter, learn_counter=tr.learn_counter, replay_ring=tr.replay.ring,
                 replay_state=tr.replay.state, observation=tr.env.obs_cur, stats=tr.env.batch.stats)
        for s, t in enumerate(st.actor.sets):
            for k in ("enc", "w1", "w2", "head", "bhead"):
                w[f"actor_set{s}_{k}"] = t[k]
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
    # after more updates the window pack is the current image set (the update writes the other set and flips)
    for _ in range(10):
        tr.iteration()
    torch.cuda.synchronize()
    assert tr.learn_steps >= 8, "the actor must have been updated"
    now = ev.run(st.window_pack, episode_limit=LIMIT, seed=4, policy_seed=PSEED)
    assert now["rewards"] != got["rewards"], "the updated actor is another policy"
    fresh = SacActorPack(tr.local.actor, st.operands)
    ref = DeviceEvaluator(cfgs, chunk=CHUNK, gamma=tr.gamma).run(fresh, episode_limit=LIMIT, seed=4, policy_seed=PSEED)
    dev.same_results(now, ref, "the current image set against a fresh pack of tr.local.actor")
    for kw in (dict(), dict(deterministic=True)):
        dev.same_results(ev.run(st.window_pack, episode_limit=LIMIT, seed=4, **kw),
                      DeviceEvaluator(cfgs, chunk=CHUNK, gamma=tr.gamma).run(fresh, episode_limit=LIMIT, seed=4, **kw),
                      f"current image set {kw}")
    with pytest.raises(NotImplementedError):
        tr.policy_pack()
