#!/usr/bin/env python
"""Wall time of one evaluation of the shipped schedule's 60 'trained' eval configs with the network of
tests/golden/eval60_ref.npz, three ways in one process:

  philox   DeviceEvaluator.run(pack) at chunk 64: the default device evaluation (Philox perception noise);
  numpy    DeviceEvaluator.run(pack, perception="numpy"): every robot's RandomState stream continued on the device,
           one asvrl_noise_streams launch, a one-step window and asvrl_eval_metrics per step;
  host     policy/batched_eval.evaluate_configs: the Python eval envs.

After one warm-up of each, --reps alternating repetitions: a host clock around each evaluation, ending in a device
synchronise; median and spread (max - min) are reported. The noise kernel is also timed alone: device events around
--kernel-launches launches on the whole batch at its initial state (every robot of every config drawing: the most a
step of this schedule costs), in microseconds per step. One process, no retries; run it under a timeout:

    timeout 900 python tools/eval_noise_bench.py [--out profiles/eval_reference_noise.json]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--kernel-launches", type=int, default=500)
    ap.add_argument("--no-host", action="store_true", help="skip evaluate_configs (the slow one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_reference_noise.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.envs.marinenav.env import MarineNavEnv3
    from distributional_rl_decision_and_control_amd.fused_mlp import MlpPack
    from distributional_rl_decision_and_control_amd.policy.batched_eval import evaluate_configs
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    from distributional_rl_decision_and_control_amd.policy.trainer import Trainer

    z = np.load(os.path.join(ROOT, "tests", "golden", "eval60_ref.npz"))
    configs = json.loads(str(z["trained/configs"]))
    torch.manual_seed(0)
    agent = Agent(seed=100, agent_type="AC-IQN")
    agent.policy_local.actor.load_state_dict({k[len("trained/net/"):]: torch.from_numpy(z[k]) for k in z.files
                                              if k.startswith("trained/net/")})
    tr = Trainer(MarineNavEnv3(seed=1), MarineNavEnv3(seed=253, is_eval_env=True), SCHEDULE, agent)
    pack = MlpPack(agent.policy_local.actor, "actor")
    ev = DeviceEvaluator(configs, template_env=tr.eval_env, chunk=a.chunk, gamma=agent.GAMMA)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    runs = {"philox": lambda: ev.run(pack, seed=1),
            "numpy": lambda: ev.run(pack, perception="numpy"),
            "numpy_nosync": lambda: ev.run(pack, perception="numpy", sync=False)}
    if not a.no_host:
        runs["host"] = lambda: evaluate_configs(agent, configs, template_env=tr.eval_env)
    times = {k: [] for k in runs}
    last, steps = {}, {}
    for rep in range(a.reps + 1):   # the first round is the warm-up
        for name, fn in runs.items():
            s, last[name] = clock(fn)
            steps[name] = ev.steps
            if rep > 0:
                times[name].append(s)

    # the noise kernel alone: the whole batch at its initial state, every robot drawing
    per_launch = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for grp in ev.groups:
        grp.restore()
        ns = grp.streams()
        ns.restore()
        ns.fill(grp.batch)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.kernel_launches):
            ns.fill(grp.batch)
        e1.record()
        torch.cuda.synchronize()
        per_launch.append(1e3 * e0.elapsed_time(e1) / a.kernel_launches)

    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res = {"configs": len(configs), "robots": int(sum(ev.n_robots)), "chunk": a.chunk, "reps": a.reps,
           "groups": len(ev.groups), "noise_kernel_us_per_step": sum(per_launch),
           "noise_kernel_launches": a.kernel_launches}
    for name, v in times.items():
        res[name + "_s"] = v
        res[name + "_s_median"] = med(v)
        res[name + "_spread_s"] = max(v) - min(v)
        res[name + "_steps"] = steps[name]
        res[name + "_env_steps"] = int(sum(last[name]["lengths"]))
        res[name + "_success_rate"] = float(np.mean(last[name]["successes"]))
        res[name + "_mean_reward"] = float(np.mean(last[name]["rewards"]))
    res["numpy_us_per_step"] = 1e6 * res["numpy_s_median"] / max(steps["numpy"], 1)
    res["numpy_draws"] = int(sum(int(d.sum()) for d in last["numpy"]["draws_n"]))
    if "host" in times:
        # the same streams and the same env arithmetic: the two differ only by the policy's rounding (a batched f32
        # GEMM against the pack's bf16 operands), so the outcomes are close, not equal
        res["numpy_vs_host_lengths_equal"] = int(sum(x == y for x, y in zip(last["numpy"]["lengths"],
                                                                             last["host"]["lengths"])))
    res["golden_success_rate"] = float(np.mean(z["trained/successes"]))
    res["golden_mean_reward"] = float(np.mean(z["trained/rewards"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
