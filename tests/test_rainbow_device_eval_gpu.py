"""GPU: the device-resident evaluation under Rainbow (DeviceEvaluator.run with a RainbowPack: greedy on the mu-only
images, as the reference's policy_local.eval()) on the eight configs of tests/test_iqn_device_eval_gpu.py: six picked
from tests/golden/eval60_ref.npz (3, 4 and 5 robots, 0 to 4 buoys) plus two of them again under another timestep
penalty, which makes a second parameter group of two envs.

  * closed loop against the composed loop of single launches (rainbow_act + step(is_continuous=False) at the same
    Philox keys: env noise seed + g, policy_seed + g for group g) with the bookkeeping of trainer.py:286-303 in numpy,
    both operand builds, episode_limit 22 in windows of 5; sync=False and a second run give the first run's bits;
  * cvar, deterministic and is_continuous are checked against the pack; group g runs under policy_seed + g;
  * VecTrainer(agent_type="Rainbow"): after 12 iterations fused_rb.eval_pack evaluates to the bits of a fresh
    RainbowPack(tr.local, ops, noisy=False), and the evaluation leaves the training env, the replay, both counters and
    the learner's noisy images bit-identical;
  * Trainer.learn with "device_eval": true and a Rainbow agent evaluates without evaluate_configs.

Tolerances as in tests/test_device_eval_gpu.py: integers and flags exact; f64 sums 1e-12 relative (pow and summation
order over at most 64 terms of 2.3e-16 each), the return relative to max(1, sum |term|). The weights are a seeded
Rainbow_Policy."""
import numpy as np
import pytest
import torch

import device_eval_cases as dev
import window_cases as wc
from device_eval_cases import CHUNK, GAMMA, LIMIT, PSEED, SEED

pytestmark = pytest.mark.gpu

CASE = wc.CASES["rainbow"]   # evaluated on the eval-mode (mu only) pack of the seeded network: noisy=False


# ------------------------------------------------------------------ closed loop against the composed loop
@pytest.mark.parametrize("operands", ["bf16", "f32"])
def test_closed_loop_matches_single_launches(operands):
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    pack = wc.pack(CASE, operands, noisy=False)
    ev = DeviceEvaluator(dev.configs(True), chunk=CHUNK, gamma=GAMMA)
    assert [grp.members for grp in ev.groups] == [[0, 1, 2, 3, 4, 5], [6, 7]]
    got = dev.run_thrice(ev, pack, LIMIT, CHUNK, seed=SEED, policy_seed=PSEED)
    print(operands, "lengths", got["lengths"], "outcomes", [o.tolist() for o in got["robot_outcomes"]])
    assert max(got["lengths"]) > CHUNK, "some episode must run past the first window"
    ev.observe(seed=SEED)
    for g in range(len(ev.groups)):
        st, taken = dev.composed(ev, g, CASE, pack, LIMIT, CHUNK, SEED, PSEED)
        assert (taken[..., 0] == np.round(taken[..., 0])).all() and taken[..., 0].min() >= 0
        assert taken[..., 0].max() <= wc.A - 1 and (taken[..., 1] == 0.0).all()
        dev.check_group(ev, got, g, st)


def test_groups_seeds_and_value_errors(monkeypatch):
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    pack = wc.pack(CASE, "bf16", noisy=False)
    ev = DeviceEvaluator(dev.configs(True), chunk=CHUNK, gamma=GAMMA)
    seen = dev.spy_on_rollouts(monkeypatch, ev)
    kw = dict(seed=SEED, episode_limit=LIMIT)
    a = ev.run(pack, policy_seed=PSEED, **kw)
    assert seen and {s[0] for s in seen} == {0, 1}
    assert all(s[1] == PSEED + s[0] for s in seen), "group g runs under policy_seed + g"
    # at epsilon 0 nothing depends on the key: another policy_seed is the same evaluation
    dev.same_results(ev.run(pack, policy_seed=PSEED + 50, **kw), a, "greedy: the key changes nothing")
    dev.same_results(ev.run(pack, is_continuous=False, **kw), a, "is_continuous=False agrees with the pack")
    with pytest.raises(ValueError, match="cvar"):
        ev.run(pack, cvar=0.5)
    with pytest.raises(ValueError, match="deterministic"):
        ev.run(pack, deterministic=True)
    with pytest.raises(ValueError, match="is_continuous"):
        ev.run(pack, is_continuous=True)
    with pytest.raises(ValueError, match="not both"):
        ev.run(pack, actions=torch.zeros((2, 5, 2), dtype=torch.float64, device="cuda"))


# ------------------------------------------------------------------ VecTrainer
def test_vec_trainer_eval_pack_and_device_evaluator():
    from distributional_rl_decision_and_control_amd.fused_rainbow import RainbowPack
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    cfgs = dev.configs(True)
    tr = VecTrainer(agent_type="Rainbow", n_envs=37, batch_size=64, buffer_size=37 * 5 * 40, graphs=False)
    fr = tr.fused_rb
    assert fr.policy_pack is None and fr.actor_pack is None
    assert fr.window_pack.noisy and not fr.eval_pack.noisy and fr.eval_pack.image is not fr.img
    for _ in range(12):
        tr.iteration()
    torch.cuda.synchronize()
    assert tr.learn_steps >= 4, "the network must have been updated"

    def watched():
        w = dict(training_state=tr.env.batch.rs, flags=tr.env.batch.rflags, ep_ts=tr.env.batch.ep_ts,
                 step_counter=tr.env.counter, learn_counter=tr.learn_counter, observation=tr.env.obs_cur,
                 stats=tr.env.batch.stats, noisy_img=fr.img.img, noisy_bias=fr.img.bias, composed=fr.pack.flat,
                 target_img=fr.timg.img)
        for n in ("rows", "tree", "state", "t", "maxp", "dirty"):
            w["per_" + n] = getattr(tr.per, n)
        return w
    before = {k: v.clone() for k, v in watched().items()}
    host = (tr.learn_steps, tr.env.total_timesteps, tr.per.pushed)
    ev = tr.device_evaluator(cfgs, chunk=CHUNK)
    now = ev.run(fr.eval_pack, episode_limit=LIMIT, seed=4, policy_seed=PSEED)
    torch.cuda.synchronize()
    for k, v in watched().items():
        assert torch.equal(v, before[k]), k
    assert host == (tr.learn_steps, tr.env.total_timesteps, tr.per.pushed)
    assert tr.device_evaluator(cfgs, chunk=CHUNK) is ev, "the evaluator is cached"
    assert all(np.isfinite(now["rewards"])) and all(1 <= n <= LIMIT + 1 for n in now["lengths"])
    fresh = RainbowPack(tr.local, fr.window_pack.operands, noisy=False)
    ref = DeviceEvaluator(cfgs, chunk=CHUNK, gamma=tr.gamma).run(fresh, episode_limit=LIMIT, seed=4, policy_seed=PSEED)
    dev.same_results(now, ref, "the current mu images against a fresh eval pack of tr.local")
    assert torch.equal(fr.eval_pack.image.img, fresh.image.img) and torch.equal(fr.eval_pack.image.bias, fresh.image.bias)
    assert not torch.equal(fr.eval_pack.image.img, fr.img.img[:fresh.image.img.numel()]), "mu only is not the noisy image"
    for refused in (tr.policy_pack, lambda: tr.collect(2), tr.greedy_episodes, lambda: tr.evaluate(cfgs)):
        with pytest.raises(NotImplementedError):
            refused()


# ------------------------------------------------------------------ Trainer
def test_trainer_device_eval_rainbow(tmp_path, monkeypatch):
    """The prioritised replay learns once it holds n + 1 = 4 pushes and a batch: the sixth iteration; evaluations at
    that iteration and at the next multiple of eval_freq."""
    dev.check_trainer_device_eval(tmp_path, monkeypatch, "Rainbow", 12)
