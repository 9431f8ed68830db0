"""GPU: "device_eval": {"distribution": true} in the `vectorized` dict. Trainer.learn with an IQN and an AC-IQN agent
evaluates on the device with the return distributions read out (IQN's own quantiles; the AC-IQN local critic's),
keeps every evaluation's summary in Trainer.eval_distributions and writes eval_distributions.npz beside an
evaluations.npz that keeps the reference's keys exactly. Any other agent type is refused when the option is read."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = 64
REFERENCE_KEYS = {"timesteps", "observations", "actions", "trajectories", "rewards", "successes", "times", "energies",
                  "relations"}
SUMMARY = ("pit", "pinball", "bias", "pred0_minus_g0", "robots", "steps")


def _trainer(device_eval, agent_type):
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.envs.marinenav.env import MarineNavEnv3
    from distributional_rl_decision_and_control_amd.policy.trainer import Trainer
    sched = {"timesteps": [0], "num_robots": [3], "num_cores": [0], "num_obstacles": [2], "min_start_goal_dis": [30.0],
             "vectorized": {"n_envs": E, "batch_size": 64, "buffer_size": 8192, "graphs": False,
                            "device_eval": device_eval}}
    eval_sched = {"num_episodes": [2], "num_robots": [3], "num_cores": [0], "num_obstacles": [2],
                  "min_start_goal_dis": [30.0]}
    torch.manual_seed(0)
    return Trainer(MarineNavEnv3(seed=1, schedule=sched), MarineNavEnv3(seed=253, is_eval_env=True), eval_sched,
                   Agent(seed=100, agent_type=agent_type), learning_starts=100)


@pytest.mark.parametrize("agent_type", ["IQN", "AC-IQN"])
def test_trainer_keeps_and_saves_the_summaries(tmp_path, monkeypatch, agent_type):
    from distributional_rl_decision_and_control_amd.policy import batched_eval

    def refuse(*a, **k):
        raise AssertionError("evaluate_configs was called: the evaluation left the device")
    monkeypatch.setattr(batched_eval, "evaluate_configs", refuse)
    trainer = _trainer({"distribution": True}, agent_type)
    trainer.learn(total_timesteps=E * 4, eval_freq=E * 4, eval_log_path=str(tmp_path), verbose=False)
    assert trainer._device_eval_dist is True and "distribution" not in trainer._device_eval_kw
    n = len(trainer.eval_timesteps)
    assert n >= 1 and len(trainer.eval_distributions) == n
    for d, ts in zip(trainer.eval_distributions, trainer.eval_timesteps):
        assert d["timestep"] == ts and d["terminated_only"] is True
        assert d["configs"]["pit"].shape == (2, 33) and d["overall"]["pit"].shape == (33,)
        if d["overall"]["steps"]:
            assert abs(d["overall"]["pit"].sum() - 1.0) < 1e-12 and np.isfinite(d["overall"]["pinball"])
    ev = np.load(os.path.join(str(tmp_path), "evaluations.npz"), allow_pickle=True)   # our own file
    assert set(ev.files) == REFERENCE_KEYS
    assert list(ev["timesteps"]) == trainer.eval_timesteps and ev["rewards"].shape == (n, 2)
    dz = np.load(os.path.join(str(tmp_path), "eval_distributions.npz"))
    assert set(dz.files) == {"timesteps"} | set(SUMMARY) | {"overall_" + k for k in SUMMARY}
    assert list(dz["timesteps"]) == trainer.eval_timesteps
    assert dz["pit"].shape == (n, 2, 33) and dz["overall_pit"].shape == (n, 33) and dz["pinball"].shape == (n, 2)
    # the same evaluation again through the public call: one more summary
    trainer.evaluation(batched="device")
    assert len(trainer.eval_distributions) == n + 1


def test_without_the_option_nothing_is_kept_or_written(tmp_path):
    trainer = _trainer(True, "IQN")
    trainer.learn(total_timesteps=E * 4, eval_freq=E * 4, eval_log_path=str(tmp_path), verbose=False)
    assert not getattr(trainer, "eval_distributions", None)
    assert not os.path.exists(os.path.join(str(tmp_path), "eval_distributions.npz"))
    assert all(grp._dist == {} for grp in trainer.vec_trainer._dev_eval[2].groups)


@pytest.mark.parametrize("agent_type", ["DQN", "DDPG", "Rainbow"])
def test_other_agent_types_are_refused(tmp_path, agent_type):
    with pytest.raises(ValueError, match="device_eval: \"distribution\" reads IQN's or the AC-IQN critic's quantiles"):
        _trainer({"distribution": True}, agent_type).learn(total_timesteps=E, eval_freq=E, eval_log_path=str(tmp_path),
                                                           verbose=False)
