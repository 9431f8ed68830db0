#!/usr/bin/env python
"""Time the DDPG learner: (a) the drop-in Agent's learn step at the reference shape (B = 64) on the fused-f32 and
fused-bf16 learners against the torch learner, and (b) the batched loop (VecTrainer, graphs on) for DDPG beside
AC-IQN at the same shape -- AC-IQN on its default (dependency-chained) schedule and on the joined schedule DDPG
runs.

One process. Each variant is built once; a measurement is --steps timed steps after --warmup steps (wall clock
around a device synchronise), the variants alternate, and --reps measurements give the median and the spread
(max - min) per variant. (a) times Agent.train() as the drop-in loop calls it: the host-side batch assembly and the
loss read-back are part of the step for every learner. One process, no retries; run it under a timeout:

    timeout 900 python tools/ddpg_bench.py [--out-dir profiles]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _med(v):
    return sorted(v)[len(v) // 2]


def _summary(samples):
    return {k: dict(samples=v, median=_med(v), spread=max(v) - min(v)) for k, v in samples.items()}


def agent_bench(a):
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.learn_ops import split_rows
    B = a.agent_batch
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.zeros(B, 88, device="cuda")
    rows[:, 0:32] = torch.randn(B, 32, generator=g, device="cuda")
    rows[:, 32:37] = (torch.rand(B, 5, generator=g, device="cuda") > 0.4).float()
    rows[:, 40:80] = rows[:, 0:40].roll(1, 0)
    rows[:, 80:82] = torch.rand(B, 2, generator=g, device="cuda") * 2 - 1
    rows[:, 82] = torch.randn(B, generator=g, device="cuda")
    rows[:, 83] = (torch.rand(B, generator=g, device="cuda") > 0.9).float()
    batch = split_rows(rows)
    agents = {}
    for learner in ("torch", "fused-f32", "fused-bf16"):
        ag = Agent(seed=100, agent_type="DDPG", BATCH_SIZE=B)
        ag.set_learner(learner)
        ag.memory.sample = (lambda b=batch: b)
        agents[learner] = ag

    def measure(ag):
        for _ in range(a.warmup):
            ag.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            ag.train()
        torch.cuda.synchronize()
        return a.steps / (time.perf_counter() - t0)

    samples = {k: [] for k in agents}
    for _ in range(a.reps):
        for k, ag in agents.items():
            samples[k].append(measure(ag))
    res = dict(bench="agent_ddpg_learn_steps_per_s", batch=B, steps=a.steps, warmup=a.warmup, reps=a.reps,
               launches_per_fused_update=11, **_summary(samples))
    t = res["torch"]
    for k in ("fused-f32", "fused-bf16"):
        res[k]["speedup_vs_torch"] = res[k]["median"] / t["median"]
        res[k]["faster_than_spread"] = bool(res[k]["median"] - t["median"] > max(res[k]["spread"], t["spread"]))
    return res


def vec_bench(a):
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    E, R, B = a.envs, a.robots, a.batch
    trainers = {}
    for name, agent_type, chain in (("DDPG", "DDPG", None), ("AC-IQN", "AC-IQN", None),
                                    ("AC-IQN-joined", "AC-IQN", False)):
        tr = VecTrainer(n_envs=E, agent_type=agent_type, num_robots=R, batch_size=B, num_tau=32, graphs=True,
                        unroll=a.unroll, seed=1, buffer_size=1 << 20, chain=chain)
        while tr.replay_size_host() < tr.learning_starts:
            tr.iteration()
        for _ in range(max(a.warmup, 2 * a.unroll)):   # captures the graph
            tr.iteration()
        torch.cuda.synchronize()
        assert tr.graphs and tr._graph is not None, f"{name}: the graph was not captured"
        trainers[name] = tr

    def measure(tr):
        n = (a.steps // a.unroll) * a.unroll
        for _ in range(a.unroll * 2):
            tr.iteration()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            tr.iteration()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    samples = {k: [] for k in trainers}
    for _ in range(a.reps):
        for k, tr in trainers.items():
            samples[k].append(measure(tr))
    res = dict(bench="vec_trainer_ms_per_step", envs=E, robots=R, batch=B, unroll=a.unroll, steps=a.steps, reps=a.reps,
               **_summary(samples))
    for k in trainers:
        res[k]["env_steps_per_s"] = E / (res[k]["median"] * 1e-3)
    d = res["DDPG"]
    for k in ("AC-IQN", "AC-IQN-joined"):
        i = res[k]
        d["ratio_to_" + k] = d["median"] / i["median"]
        d["below_" + k + "_by_more_than_spread"] = bool(i["median"] - d["median"] > max(d["spread"], i["spread"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agent-batch", type=int, default=64)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--robots", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--unroll", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["agent", "vec"], default=None)
    ap.add_argument("--out-dir", default=None, help="also write ddpg_bench_<part>.json files to this directory")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    for name, fn in (("agent", agent_bench), ("vec", vec_bench)):
        if a.only not in (None, name):
            continue
        line = json.dumps(fn(a))
        print(line, flush=True)
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"ddpg_bench_{name}.json"), "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
