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
import copy
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval60_ref.npz")
PICK = (0, 10, 20, 30, 40, 55)   # 3, 4, 5 robots without buoys; 5 robots with 2, 3 and 4 buoys
GAMMA = 0.99
A = 25
LIMIT, CHUNK, SEED, PSEED = 22, 5, 17, 900


@functools.lru_cache(maxsize=None)
def _all_configs():
    return json.loads(str(np.load(GOLDEN)["trained/configs"]))


def _configs(second_group=True):
    out = [copy.deepcopy(_all_configs()[i]) for i in PICK]
    assert [c["env"]["num_robots"] for c in out] == [3, 4, 5, 5, 5, 5]
    assert [len(c["env"]["obstacles"]["r"]) for c in out] == [0, 0, 0, 2, 3, 4]
    if second_group:   # another env-level parameter: a DeviceEnvBatch of their own
        for i in (2, 3):
            c = copy.deepcopy(out[i])
            c["env"]["timestep_penalty"] = 2.0 * c["env"]["timestep_penalty"] - 0.25
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def _net():
    from distributional_rl_decision_and_control_amd.policy.Rainbow_model import Rainbow_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    return Rainbow_Policy(**DEFAULT_NET, action_size=A, atoms=51, device="cuda", seed=100).to("cuda")


@functools.lru_cache(maxsize=None)
def _pack(operands):
    """The eval-mode (mu only) pack of the seeded network."""
    from distributional_rl_decision_and_control_amd.fused_rainbow import RainbowPack
    return RainbowPack(_net(), operands, noisy=False)


def _close(got, ref, scale=None, what=""):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref) if scale is None else np.asarray(scale, dtype=np.float64)
    err = np.abs(got - ref) / np.maximum(scale, 1e-300)
    print(f"{what}: max relative error {err.max():.2e}")
    assert (np.abs(got - ref) <= 1e-12 * scale).all(), (what, got, ref)


def _same_results(a, b, what):
    assert a["lengths"] == b["lengths"] and a["successes"] == b["successes"], what
    for name in ("rewards", "times", "energies"):
        assert np.array(a[name]).tobytes() == np.array(b[name]).tobytes(), (what, name)
    for name in ("robot_rewards", "robot_times", "robot_energies", "robot_outcomes"):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[name], b[name])), (what, name)


# ------------------------------------------------------------------ closed loop against the composed loop
def _bookkeep(st, n_robots, R, reward, info, tl, tr, dt, N, pc, stepping, limit):
    """trainer.py:286-303 for one step of every env in `stepping` (numpy, in place)."""
    from distributional_rl_decision_and_control_amd import _abi
    for e in np.nonzero(stepping)[0]:
        if st["ended"][e]:
            continue
        collided = False
        for i in range(n_robots[e]):
            r = e * R + i
            if st["deact"][r]:
                continue
            term = GAMMA ** int(st["length"][e]) * reward[r]
            st["ret"][r] += term
            st["abs"][r] += abs(term)
            st["time"][r] += dt[r] * N[r]
            st["energy"][r] += pc[r] * np.abs(tl[r]) * dt[r] * N[r] + pc[r] * np.abs(tr[r]) * dt[r] * N[r]
            if info[r] in (_abi.INFO_COLLISION, _abi.INFO_REACH_GOAL):
                st["deact"][r] = 1
                st["outcome"][r] = 2 if info[r] == _abi.INFO_COLLISION else 1
                collided |= info[r] == _abi.INFO_COLLISION
        end = st["length"][e] >= limit or collided or bool(st["deact"][e * R:e * R + n_robots[e]].all())
        st["length"][e] += 1
        st["ended"][e] = end


def _composed(ev, g, pack, limit, chunk, seed, policy_seed):
    """Group g's evaluation as single launches on the evaluator's own batch (after ev.observe): greedy-schedule
    rainbow_act + the discrete step at the Philox keys run() uses for the group, an env leaving at a window's start
    once the bookkeeping ended it and inside a window once the step's env_done held it. Also returns every action."""
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.fused_rainbow import rainbow_act
    grp = ev.groups[g]
    b = grp.batch
    E, R = b.n_envs, b.max_robots
    NT = E * R
    n_robots = b.n_robots.cpu().numpy()
    dt, N, pc = (t.cpu().numpy() for t in (grp.dt, grp.N, grp.pc))
    st = dict(length=np.zeros(E, np.int64), ended=np.zeros(E, bool), deact=np.zeros(NT, np.uint8),
              outcome=np.zeros(NT, np.uint8), ret=np.zeros(NT), time=np.zeros(NT), energy=np.zeros(NT),
              abs=np.zeros(NT))
    act64 = torch.zeros((NT, 2), dtype=torch.float64, device="cuda")
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    mask = None
    taken = []
    for t in range(limit + 1):
        if t % chunk == 0:
            mask = torch.from_numpy((~st["ended"]).astype(np.uint8)).cuda()
        step.fill_(t)
        rainbow_act(pack, b.obs, act64, step, 1.0, 1.0, 1.0, 0.0, 0.0, policy_seed + g)
        taken.append(act64.cpu().numpy().copy())
        b.step(act64, is_continuous=False, trainer_deactivate=True, seed=seed + g, counter=t, fast_noise=True,
               env_mask=mask)
        rs = b.rs.cpu().numpy()
        _bookkeep(st, n_robots, R, b.reward.cpu().numpy(), b.info.cpu().numpy(), rs[_abi.F_TL], rs[_abi.F_TR], dt, N,
                  pc, mask.cpu().numpy() != 0, limit)
        mask = mask * (b.env_done == 0).to(torch.uint8)
    return st, np.stack(taken)


@pytest.mark.parametrize("operands", ["bf16", "f32"])
def test_closed_loop_matches_single_launches(operands):
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    pack = _pack(operands)
    ev = DeviceEvaluator(_configs(), chunk=CHUNK, gamma=GAMMA)
    assert [grp.members for grp in ev.groups] == [[0, 1, 2, 3, 4, 5], [6, 7]]
    kw = dict(seed=SEED, episode_limit=LIMIT, policy_seed=PSEED)
    got = ev.run(pack, **kw)
    assert ev.windows <= math.ceil((LIMIT + 1) / CHUNK) and ev.steps <= LIMIT + 1
    again = ev.run(pack, **kw)          # restored by copy: the same bits
    nosync = ev.run(pack, sync=False, **kw)
    assert ev.windows == math.ceil((LIMIT + 1) / CHUNK) and ev.steps == LIMIT + 1
    _same_results(again, got, "second run")
    _same_results(nosync, got, "sync=False")
    print(operands, "lengths", got["lengths"], "outcomes", [o.tolist() for o in got["robot_outcomes"]])
    assert max(got["lengths"]) > CHUNK, "some episode must run past the first window"
    ev.observe(seed=SEED)
    for g, grp in enumerate(ev.groups):
        st, taken = _composed(ev, g, pack, LIMIT, CHUNK, SEED, PSEED)
        R = grp.batch.max_robots
        assert st["ended"].all()
        assert (taken[..., 0] == np.round(taken[..., 0])).all() and taken[..., 0].min() >= 0
        assert taken[..., 0].max() <= A - 1 and (taken[..., 1] == 0.0).all()
        for le, c in enumerate(grp.members):
            sl = slice(le * R, le * R + ev.n_robots[c])
            assert got["lengths"][c] == int(st["length"][le])
            assert got["robot_outcomes"][c].tolist() == st["outcome"][sl].tolist()
            assert got["successes"][c] == bool((st["outcome"][sl] == 1).all())
            _close(got["robot_times"][c], st["time"][sl], what=f"config {c} times")
            _close(got["robot_energies"][c], st["energy"][sl], what=f"config {c} energies")
            _close(got["robot_rewards"][c], st["ret"][sl], scale=np.maximum(1.0, st["abs"][sl]),
                   what=f"config {c} returns")
            assert got["rewards"][c] == np.mean(got["robot_rewards"][c])
            assert got["times"][c] == np.mean(got["robot_times"][c])
            assert got["energies"][c] == np.mean(got["robot_energies"][c])


def test_groups_seeds_and_value_errors(monkeypatch):
    from distributional_rl_decision_and_control_amd.device_env import DeviceEnvBatch
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    pack = _pack("bf16")
    ev = DeviceEvaluator(_configs(), chunk=CHUNK, gamma=GAMMA)
    seen = []
    inner = DeviceEnvBatch.policy_rollout

    def spy(self, *a, **kw):
        seen.append((next(g for g, grp in enumerate(ev.groups) if grp.batch is self), kw["policy_seed"]))
        return inner(self, *a, **kw)
    monkeypatch.setattr(DeviceEnvBatch, "policy_rollout", spy)
    kw = dict(seed=SEED, episode_limit=LIMIT)
    a = ev.run(pack, policy_seed=PSEED, **kw)
    assert seen and {s[0] for s in seen} == {0, 1}
    assert all(s[1] == PSEED + s[0] for s in seen), "group g runs under policy_seed + g"
    # at epsilon 0 nothing depends on the key: another policy_seed is the same evaluation
    _same_results(ev.run(pack, policy_seed=PSEED + 50, **kw), a, "greedy: the key changes nothing")
    _same_results(ev.run(pack, is_continuous=False, **kw), a, "is_continuous=False agrees with the pack")
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
    cfgs = _configs()
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
    _same_results(now, ref, "the current mu images against a fresh eval pack of tr.local")
    assert torch.equal(fr.eval_pack.image.img, fresh.image.img) and torch.equal(fr.eval_pack.image.bias, fresh.image.bias)
    assert not torch.equal(fr.eval_pack.image.img, fr.img.img[:fresh.image.img.numel()]), "mu only is not the noisy image"
    for refused in (tr.policy_pack, lambda: tr.collect(2), tr.greedy_episodes, lambda: tr.evaluate(cfgs)):
        with pytest.raises(NotImplementedError):
            refused()


# ------------------------------------------------------------------ Trainer
def test_trainer_device_eval_rainbow(tmp_path, monkeypatch):
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.envs.marinenav.env import MarineNavEnv3
    from distributional_rl_decision_and_control_amd.policy import batched_eval
    from distributional_rl_decision_and_control_amd.policy.trainer import Trainer

    def refuse(*a, **k):
        raise AssertionError("evaluate_configs was called: the evaluation left the device")
    monkeypatch.setattr(batched_eval, "evaluate_configs", refuse)
    E = 64
    sched = {"timesteps": [0], "num_robots": [3], "num_cores": [0], "num_obstacles": [2], "min_start_goal_dis": [30.0],
             "vectorized": {"n_envs": E, "batch_size": 64, "buffer_size": 8192, "graphs": False, "device_eval": True}}
    eval_sched = {"num_episodes": [1], "num_robots": [3], "num_cores": [0], "num_obstacles": [2],
                  "min_start_goal_dis": [30.0]}
    torch.manual_seed(0)
    trainer = Trainer(MarineNavEnv3(seed=1, schedule=sched), MarineNavEnv3(seed=253, is_eval_env=True), eval_sched,
                      Agent(seed=100, agent_type="Rainbow"), learning_starts=100)
    # the prioritised replay learns once it holds n + 1 = 4 pushes and a batch: the sixth iteration; evaluations at
    # that iteration and at the next multiple of eval_freq
    vt = trainer.learn(total_timesteps=E * 12, eval_freq=E * 4, eval_log_path=str(tmp_path), verbose=False)
    assert vt is trainer.vec_trainer and vt.agent_type == "Rainbow"
    n = len(trainer.eval_timesteps)
    assert n >= 2 and trainer.eval_timesteps[-1] == E * 12
    assert len(trainer.eval_rewards) == n and all(np.isfinite(r).all() for r in trainer.eval_rewards)
    assert all(isinstance(s, bool) for s in trainer.eval_successes[-1])
    assert all(t > 0 for t in trainer.eval_times[-1])
    ev = np.load(os.path.join(str(tmp_path), "evaluations.npz"), allow_pickle=True)   # our own file
    assert list(ev["timesteps"]) == trainer.eval_timesteps and ev["rewards"].shape == (n, 1)
