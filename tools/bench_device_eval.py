#!/usr/bin/env python
"""Wall time of one evaluation of the shipped schedule's 60 'trained' eval configs with the network of
tests/golden/eval60_ref.npz: policy/batched_eval.evaluate_configs (the Python eval envs, one policy call and one
env-step launch per step) against policy/device_eval.DeviceEvaluator.run (device-resident configs, closed-loop
windows, asvrl_eval_metrics behind each), in one process.

After one warm-up of each, --reps alternating repetitions: a host clock around each evaluation, ending in a device
synchronise. The device path is timed with its per-window host wait (sync=True, stops when every episode has ended)
and without (sync=False, every window enqueued). The metrics kernel is also timed alone (device events around
--kernel-launches launches on one window's records of the whole batch), beside one closed-loop window. The device
run's success rate and mean reward are printed next to the golden's for the record only: the perception noise is
another stream, so nothing is asserted on them. One process, no retries; run it under a timeout:

    timeout 600 python tools/bench_device_eval.py [--out profiles/device_eval.json]

--agent DQN: the same procedure with a seeded Agent(agent_type="DQN") (no trained DQN network is shipped) and its
DqnPack in the closed-loop windows; the default output is profiles/device_eval_dqn.json (its golden_* fields stay
the trained AC-IQN network's, for the record only).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCHEDULE = {"num_episodes": [10] * 6, "num_robots": [3, 4, 5, 5, 5, 5], "num_cores": [0] * 6,
            "num_obstacles": [0, 0, 0, 2, 3, 4], "min_start_goal_dis": [30.0, 35.0, 40.0, 40.0, 40.0, 40.0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--kernel-launches", type=int, default=200)
    ap.add_argument("--agent", default="AC-IQN", choices=("AC-IQN", "DQN"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "device_eval_dqn.json" if a.agent == "DQN" else "device_eval.json")
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.envs.marinenav.env import MarineNavEnv3
    from distributional_rl_decision_and_control_amd.fused_dqn import DqnPack
    from distributional_rl_decision_and_control_amd.fused_mlp import MlpPack
    from distributional_rl_decision_and_control_amd.policy.batched_eval import evaluate_configs
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator, eval_metrics
    from distributional_rl_decision_and_control_amd.policy.trainer import Trainer

    z = np.load(os.path.join(ROOT, "tests", "golden", "eval60_ref.npz"))
    configs = json.loads(str(z["trained/configs"]))
    torch.manual_seed(0)
    agent = Agent(seed=100, agent_type=a.agent)
    if a.agent == "AC-IQN":
        agent.policy_local.actor.load_state_dict({k[len("trained/net/"):]: torch.from_numpy(z[k]) for k in z.files
                                                  if k.startswith("trained/net/")})
    tr = Trainer(MarineNavEnv3(seed=1), MarineNavEnv3(seed=253, is_eval_env=True), SCHEDULE, agent)
    pack = DqnPack(agent.policy_local) if a.agent == "DQN" else MlpPack(agent.policy_local.actor, "actor")

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    load_s, ev = clock(lambda: DeviceEvaluator(configs, template_env=tr.eval_env, chunk=a.chunk, gamma=agent.GAMMA))
    runs = {"host": lambda: evaluate_configs(agent, configs, template_env=tr.eval_env),
            "device_sync": lambda: ev.run(pack, seed=1),
            "device_nosync": lambda: ev.run(pack, seed=1, sync=False)}
    times = {k: [] for k in runs}
    last, windows = {}, {}
    for rep in range(a.reps + 1):   # the first round is the warm-up
        for name, fn in runs.items():
            s, last[name] = clock(fn)
            windows[name] = ev.windows
            if rep > 0:
                times[name].append(s)

    # the metrics kernel alone, and one closed-loop window, on the whole batch from the initial state
    grp = ev.groups[0]
    b, K = grp.batch, a.chunk
    rec = grp.records(K)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window():
        b.policy_rollout(pack, K, b.obs, keep=rec, hold_done=True, trainer_deactivate=True, step_dev=grp.step,
                         env_mask=grp.state["alive"], seed=1, counter=0, fast_noise=True)
    win_us = []
    for i in range(6):
        ev.observe(seed=1)
        e0.record()
        window()
        e1.record()
        torch.cuda.synchronize()
        if i > 0:
            win_us.append(1e3 * e0.elapsed_time(e1))
    args = (pack.L, K, b.n_envs, b.max_robots, rec, b.n_robots, grp.dt, grp.N, grp.pc)

    def rewind():   # every env and robot running again: each launch walks the window as the first one did
        grp.state["ended"].zero_()
        grp.state["deact"].zero_()
        grp.state["length"].zero_()
    rewind()
    eval_metrics(*args, grp.state, agent.GAMMA, 1000)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.kernel_launches):
        rewind()
        eval_metrics(*args, grp.state, agent.GAMMA, 1000)
    e1.record()
    torch.cuda.synchronize()
    with_zero = 1e3 * e0.elapsed_time(e1) / a.kernel_launches
    e0.record()
    for _ in range(a.kernel_launches):
        rewind()
    e1.record()
    torch.cuda.synchronize()
    zero_us = 1e3 * e0.elapsed_time(e1) / a.kernel_launches

    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    dev = last["device_sync"]
    res = {
        "agent": a.agent, "configs": len(configs), "chunk": K, "reps": a.reps, "groups": len(ev.groups),
        "per_robot_params": b.robot_params is not None, "load_s": load_s,
        "host_s": times["host"], "device_sync_s": times["device_sync"], "device_nosync_s": times["device_nosync"],
        "host_s_median": med(times["host"]), "device_sync_s_median": med(times["device_sync"]),
        "device_nosync_s_median": med(times["device_nosync"]),
        "host_spread_s": max(times["host"]) - min(times["host"]),
        "device_sync_spread_s": max(times["device_sync"]) - min(times["device_sync"]),
        "device_nosync_spread_s": max(times["device_nosync"]) - min(times["device_nosync"]),
        "speedup_sync": med(times["host"]) / med(times["device_sync"]),
        "host_env_steps": int(sum(last["host"]["lengths"])), "device_env_steps": int(sum(dev["lengths"])),
        "device_windows_sync": windows["device_sync"], "device_windows_nosync": windows["device_nosync"],
        "window_us": win_us, "window_us_median": med(win_us),
        "metrics_kernel_us": with_zero - zero_us, "metrics_kernel_with_fill_us": with_zero, "fill_us": zero_us,
        "device_success_rate": float(np.mean(dev["successes"])), "device_mean_reward": float(np.mean(dev["rewards"])),
        "host_success_rate": float(np.mean(last["host"]["successes"])),
        "host_mean_reward": float(np.mean(last["host"]["rewards"])),
        "golden_success_rate": float(np.mean(z["trained/successes"])),
        "golden_mean_reward": float(np.mean(z["trained/rewards"])),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
