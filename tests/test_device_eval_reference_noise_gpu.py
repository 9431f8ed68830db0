"""GPU: DeviceEvaluator.run(perception="numpy") in the closed loop and through its front ends, on the six eval configs
tests/test_device_eval_gpu.py uses (tests/golden/eval60_ref.npz, 'trained': 3, 4 and 5 robots, 0 to 4 buoys).
tests/test_eval60_reference_noise_gpu.py pins the mode's values to the reference; here:

  * the streams behind observe() stand where each robot's own Perception stands after reset_with_eval_config
    (get_state(): key, pos, has_gauss), and the counters are zero there;
  * closed loop with the Actor's pack and a DQN pack, episode_limit 22: two runs give the same bits, sync=False equals
    sync=True, and a Philox run afterwards equals a Philox run before (the mode leaves nothing behind); run() without
    `perception` is perception="philox" to the bit;
  * VecTrainer.evaluate(cfgs, perception="numpy") equals DeviceEvaluator.run with the trainer's pack and leaves the
    training state alone;
  * Trainer.learn_vectorized with "device_eval": {"perception": "numpy"} fills eval_* and evaluations.npz through that
    mode;
  * every ValueError of the mode on the device path.
"""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval60_ref.npz")
PICK = (0, 10, 20, 30, 40, 55)   # 3, 4, 5 robots without buoys; 5 robots with 2, 3 and 4 buoys
GAMMA = 0.99
LIMIT = 22
KEYS = ("rewards", "times", "energies")
ROBOT_KEYS = ("robot_rewards", "robot_times", "robot_energies", "robot_outcomes")
DRAW_KEYS = ("draws_n", "draws_sum", "draws_sq")


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(GOLDEN)
    configs = json.loads(str(z["trained/configs"]))
    sd = {k[len("trained/net/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("trained/net/")}
    return configs, sd


def _configs():
    out = [copy.deepcopy(_golden()[0][i]) for i in PICK]
    assert [c["env"]["num_robots"] for c in out] == [3, 4, 5, 5, 5, 5]
    assert [len(c["env"]["obstacles"]["r"]) for c in out] == [0, 0, 0, 2, 3, 4]
    return out


@functools.lru_cache(maxsize=None)
def _pack(kind):
    if kind == "dqn":
        from distributional_rl_decision_and_control_amd.agent import Agent
        from distributional_rl_decision_and_control_amd.fused_dqn import DqnPack
        return DqnPack(Agent(seed=100, agent_type="DQN").policy_local, "bf16")
    from distributional_rl_decision_and_control_amd.fused_mlp import MlpPack
    from distributional_rl_decision_and_control_amd.policy.AC_IQN_model import AC_IQN_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    pol = AC_IQN_Policy(**DEFAULT_NET, value_ranges_of_action=[[-1, 1], [-1, 1]], device="cuda", seed=100)
    pol.actor.load_state_dict(_golden()[1])
    return MlpPack(pol.actor, "actor", "bf16")


def _same(a, b, what, draws):
    assert a["lengths"] == b["lengths"] and a["successes"] == b["successes"], what
    for name in KEYS:
        assert np.array(a[name]).tobytes() == np.array(b[name]).tobytes(), (what, name)
    for name in ROBOT_KEYS + (DRAW_KEYS if draws else ()):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[name], b[name])), (what, name)
    if not draws:
        assert all(a[name] is None and b[name] is None for name in DRAW_KEYS), what


def test_streams_behind_observe_are_the_robots_own():
    from distributional_rl_decision_and_control_amd.envs.marinenav.env import MarineNavEnv3
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    cfgs = _configs()
    ev = DeviceEvaluator(cfgs, chunk=5, gamma=GAMMA)
    ev.observe(perception="numpy")
    checked = 0
    for grp in ev.groups:
        ns, R = grp.streams(), grp.batch.max_robots
        n, s, q = ns.counters()
        assert not n.any() and not s.any() and not q.any(), "zeroed behind the observation pass"
        for le, c in enumerate(grp.members):
            # the host objects right behind reset_with_eval_config (the evaluator's own envs have drawn once more
            # since: the loader's _pack call draws, and discards, another pass)
            host = MarineNavEnv3(seed=0, is_eval_env=True)
            host.reset_with_eval_config(cfgs[c])
            assert [r.perception.seed for r in host.robots] == [r.perception.seed for r in ev.envs[c].robots]
            for i, rob in enumerate(host.robots):
                _, key, pos, has_gauss, _ = rob.perception.rd.get_state()
                mine = ns.state(le * R + i)
                np.testing.assert_array_equal(mine[1], key)
                assert mine[2:4] == (pos, has_gauss)
                fresh = np.random.RandomState(rob.perception.seed).get_state()
                assert pos != fresh[2] or (key != fresh[1]).any(), "the pass drew"
                checked += 1
    assert checked == sum(ev.n_robots) == 27


@pytest.mark.parametrize("kind", ["actor", "dqn"])
def test_closed_loop_repeats_and_leaves_nothing_behind(kind):
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    pack = _pack(kind)
    ev = DeviceEvaluator(_configs(), chunk=5, gamma=GAMMA)
    before = ev.run(pack, seed=17, episode_limit=LIMIT, perception="philox")
    default = ev.run(pack, seed=17, episode_limit=LIMIT)
    _same(default, before, "run() without perception is the Philox mode", draws=False)
    got = ev.run(pack, seed=17, episode_limit=LIMIT, perception="numpy")
    assert ev.steps <= LIMIT + 1 and ev.windows == ev.steps, "windows of one step"
    again = ev.run(pack, seed=17, episode_limit=LIMIT, perception="numpy")
    other_seed = ev.run(pack, seed=99, episode_limit=LIMIT, perception="numpy")
    nosync = ev.run(pack, seed=17, episode_limit=LIMIT, perception="numpy", sync=False)
    assert ev.steps == ev.windows == LIMIT + 1
    _same(again, got, "second run", draws=True)
    _same(other_seed, got, "seed does not enter the perception noise", draws=True)
    _same(nosync, got, "sync=False", draws=True)
    after = ev.run(pack, seed=17, episode_limit=LIMIT, perception="philox")
    _same(after, before, "a Philox run after the numpy runs", draws=False)
    print(kind, "lengths", got["lengths"], "draws", [int(d.sum()) for d in got["draws_n"]])
    for c, k in enumerate(ev.n_robots):
        assert got["draws_n"][c].shape == (k,) and (got["draws_n"][c] % 5 == 0).all()
        if k > 1:   # every robot of a crowd has a candidate at the first step at the least
            assert (got["draws_n"][c] >= 5 * (k - 1)).all() and (got["draws_sq"][c] > 0).all()
    assert max(got["lengths"]) == LIMIT + 1, "at least one env runs to the step limit"
    if kind == "actor":   # continuous actions follow the observation's last bits: other noise, other episodes
        assert any(np.array(got[name]).tobytes() != np.array(before[name]).tobytes() for name in KEYS)


def test_vec_trainer_evaluate_takes_the_mode():
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    cfgs = _configs()
    tr = VecTrainer(n_envs=37, batch_size=64, buffer_size=4096, graphs=False, seed=3, gamma=GAMMA)
    for _ in range(2):
        tr.iteration()
    torch.cuda.synchronize()
    watched = dict(training_state=tr.env.batch.rs, flags=tr.env.batch.rflags, step_counter=tr.env.counter,
                   replay_state=tr.replay.state, observation=tr.env.obs_cur, stats=tr.env.batch.stats)
    before = {k: v.clone() for k, v in watched.items()}
    got = tr.evaluate(cfgs, chunk=5, episode_limit=LIMIT, seed=4, perception="numpy")
    for k, v in watched.items():
        assert torch.equal(v, before[k]), k
    ref = DeviceEvaluator(cfgs, chunk=5, gamma=GAMMA).run(tr.fused2.actor, episode_limit=LIMIT, seed=4,
                                                          perception="numpy")
    _same(got, ref, "VecTrainer.evaluate against DeviceEvaluator.run", draws=True)
    assert sum(int(d.sum()) for d in got["draws_n"]) > 0
    with pytest.raises(ValueError, match="perception must be one of"):
        tr.evaluate(cfgs, chunk=5, episode_limit=LIMIT, perception="mt19937")


def test_learn_vectorized_device_eval_with_the_mode(tmp_path, monkeypatch):
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.envs.marinenav.env import MarineNavEnv3
    from distributional_rl_decision_and_control_amd.policy import batched_eval, device_eval
    from distributional_rl_decision_and_control_amd.policy.trainer import Trainer
    host_calls, modes = [], []
    monkeypatch.setattr(batched_eval, "evaluate_configs", lambda *a, **k: host_calls.append(1))
    orig = device_eval.DeviceEvaluator.run

    def spy(self, *a, **k):
        res = orig(self, *a, **k)
        modes.append((k.get("perception"), res["draws_n"]))
        return res
    monkeypatch.setattr(device_eval.DeviceEvaluator, "run", spy)
    E = 64
    vec = {"n_envs": E, "batch_size": 64, "num_tau": 32, "graphs": False, "buffer_size": 8192,
           "device_eval": {"perception": "numpy"}}
    sched = {"timesteps": [0], "num_robots": [3], "num_cores": [0], "num_obstacles": [2], "min_start_goal_dis": [30.0],
             "vectorized": vec}
    eval_sched = {"num_episodes": [2, 1], "num_robots": [3, 5], "num_cores": [0, 0], "num_obstacles": [2, 4],
                  "min_start_goal_dis": [30.0, 40.0]}
    torch.manual_seed(0)
    trainer = Trainer(MarineNavEnv3(seed=1, schedule=sched), MarineNavEnv3(seed=253, is_eval_env=True), eval_sched,
                      Agent(seed=100, agent_type="AC-IQN"), learning_starts=100)
    trainer.learn(total_timesteps=E * 8, eval_freq=E * 4, eval_log_path=str(tmp_path), verbose=False)
    n = len(trainer.eval_timesteps)
    assert n >= 2 and not host_calls and len(modes) == n
    for mode, draws_n in modes:
        assert mode == "numpy" and [len(d) for d in draws_n] == [3, 3, 5] and all((d > 0).all() for d in draws_n)
    for name in ("observations", "actions", "trajectories", "rewards", "successes", "times", "energies", "relations"):
        lst = getattr(trainer, "eval_" + name)
        assert len(lst) == n and all(len(entry) == 3 for entry in lst), name
    assert all(np.isfinite(trainer.eval_rewards[-1])) and all(t > 0 for t in trainer.eval_times[-1])
    ev = np.load(os.path.join(str(tmp_path), "evaluations.npz"), allow_pickle=True)   # our own file
    assert list(ev["timesteps"]) == trainer.eval_timesteps and ev["rewards"].shape == (n, 3)
    # an option the block does not know is refused before anything is built
    bad = dict(sched, vectorized=dict(vec, device_eval={"noise": "numpy"}))
    with pytest.raises(ValueError, match="device_eval: unknown option"):
        Trainer(MarineNavEnv3(seed=1, schedule=bad), MarineNavEnv3(seed=253, is_eval_env=True), eval_sched,
                Agent(seed=100, agent_type="AC-IQN"), learning_starts=100).learn(
                    total_timesteps=E, eval_freq=E, eval_log_path=str(tmp_path), verbose=False)


def test_refusals_on_the_device_path():
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    pack = _pack("actor")
    ev = DeviceEvaluator(_configs(), chunk=5, gamma=GAMMA)
    b = ev.groups[0].batch
    table = torch.zeros((4, b.n_envs * b.max_robots, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="explicit noise"):
        ev.run(pack, perception="numpy", obs_noise=ev.zero_noise())
    with pytest.raises(ValueError, match="explicit noise"):
        ev.run(actions=table, perception="numpy", noise=ev.zero_noise(4))
    with pytest.raises(ValueError, match="explicit noise"):
        ev.run(actions=table, perception="numpy", noise=ev.zero_noise(4), obs_noise=ev.zero_noise())
    with pytest.raises(ValueError, match="explicit noise"):
        ev.observe(noise=ev.zero_noise(), perception="numpy")
    for bad in ("mt19937", "Numpy", None, 1):
        with pytest.raises(ValueError, match="perception must be one of"):
            ev.run(pack, perception=bad)
        with pytest.raises(ValueError, match="perception must be one of"):
            ev.observe(perception=bad)
    with pytest.raises(ValueError, match="not both"):   # the existing refusals come first, unchanged
        ev.run(pack, actions=table, perception="numpy")
    # and the mode still runs behind them
    res = ev.run(pack, episode_limit=3, perception="numpy")
    assert res["lengths"] and all(d is not None for d in res["draws_n"])
