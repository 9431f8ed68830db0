"""GPU: Trainer.learn with "device_eval": {"histories": true} (the setup of device_eval_cases.check_trainer_device_eval)
writes an evaluations.npz whose observation, action and trajectory histories the reference's episode player can walk:
utils/env_visualizer.py:415-483 takes max_steps from len(trajectory), indexes trajectories[j][i][0..12] as floats
and unpacks observations[id][i] into (self_obs, objects_obs), either of them None for a deactivated robot. The walk is
restated here without matplotlib. An unknown option beside "histories" is still refused."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = 64


def _trainer(device_eval, agent_type="AC-IQN"):
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.envs.marinenav.env import MarineNavEnv3
    from distributional_rl_decision_and_control_amd.policy.trainer import Trainer
    sched = {"timesteps": [0], "num_robots": [3], "num_cores": [0], "num_obstacles": [2], "min_start_goal_dis": [30.0],
             "vectorized": {"n_envs": E, "batch_size": 64, "buffer_size": 8192, "graphs": False,
                            "device_eval": device_eval}}
    eval_sched = {"num_episodes": [1, 1], "num_robots": [3, 4], "num_cores": [0, 0], "num_obstacles": [2, 3],
                  "min_start_goal_dis": [30.0, 30.0]}
    torch.manual_seed(0)
    return Trainer(MarineNavEnv3(seed=1, schedule=sched), MarineNavEnv3(seed=253, is_eval_env=True), eval_sched,
                   Agent(seed=100, agent_type=agent_type), learning_starts=100)


def _play_episode(trajectories, observations, actions, n_robots, continuous):
    """env_visualizer.play_episode's walk over one episode's histories. Returns the steps it would draw."""
    assert len(trajectories) == len(observations) == len(actions) == n_robots
    max_steps = max(len(traj) for traj in trajectories) - 1   # the player draws up to the longest trajectory
    assert max_steps >= 1, "the player would show nothing"
    for j, traj in enumerate(trajectories):
        assert len(traj) == len(actions[j]) + 1
        for i in range(len(traj)):
            row = [traj[i][k] for k in range(13)]
            assert len(traj[i]) == 13 and all(type(v) is float and np.isfinite(v) for v in row)
        for a in actions[j]:
            if continuous:
                assert len(a) == 2 and all(type(v) is float for v in a)
            else:
                assert type(a) is int
    length = len(observations[0]) - 1
    for idx, obs in enumerate(observations):
        assert len(obs) == length + 1, "every robot has the episode's observations, active or not"
        assert len(trajectories[idx]) <= length + 1
        for i in range(len(obs)):
            self_obs, objects_obs = obs[i]
            if self_obs is None:
                assert objects_obs is None and i > 0, "the reset observation of a placed robot is never None"
                continue
            assert len(self_obs) == 7 and all(type(v) is float for v in self_obs)
            assert len(objects_obs) <= 5 and all(len(o) == 5 and all(type(v) is float for v in o) for o in objects_obs)
    return max_steps, length


@pytest.mark.parametrize("agent_type", ["AC-IQN", "DQN"])
def test_trainer_histories_replay(tmp_path, monkeypatch, agent_type):
    from distributional_rl_decision_and_control_amd.policy import batched_eval

    def refuse(*a, **k):
        raise AssertionError("evaluate_configs was called: the evaluation left the device")
    monkeypatch.setattr(batched_eval, "evaluate_configs", refuse)
    trainer = _trainer({"histories": True}, agent_type)
    trainer.learn(total_timesteps=E * 8, eval_freq=E * 4, eval_log_path=str(tmp_path), verbose=False)
    n = len(trainer.eval_timesteps)
    assert n >= 2 and trainer.eval_timesteps[-1] == E * 8
    ev = np.load(os.path.join(str(tmp_path), "evaluations.npz"), allow_pickle=True)   # our own file
    assert list(ev["timesteps"]) == trainer.eval_timesteps and ev["rewards"].shape == (n, 2)
    for k in range(n):   # every evaluation, every episode: visualize_eval_episode's indexing
        for ep, robots in enumerate((3, 4)):
            steps, length = _play_episode(ev["trajectories"][k][ep], ev["observations"][k][ep], ev["actions"][k][ep],
                                          robots, continuous=agent_type == "AC-IQN")
            assert 1 <= steps <= length <= 1001
            assert [len(r) for r in ev["relations"][k][ep]] == [0] * robots


def test_unknown_option_beside_histories_is_refused(tmp_path):
    with pytest.raises(ValueError, match="device_eval: unknown option"):
        _trainer({"histories": True, "noise": 1}).learn(total_timesteps=E, eval_freq=E, eval_log_path=str(tmp_path),
                                                        verbose=False)
