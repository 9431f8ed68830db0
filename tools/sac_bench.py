#!/usr/bin/env python
"""Time the SAC learner beside DDPG's, in one process: (a) the update alone (sac_update_fused / ddpg_update_fused,
bf16 build) replayed from a HIP graph at B = --batch on fixed replay rows, the noise drawn in the kernels, and (b) the
batched loop (VecTrainer, graphs on, the joined schedule both run) at --envs x --robots.

Each variant is built once; a measurement is --steps timed steps after --warmup steps (wall clock around a device
synchronise), the variants alternate, and --reps measurements give the median and the spread (max - min) per variant.
DDPG is the yardstick: SAC does the critic work twice plus one extra critic pass. One process, no retries; run it
under a timeout:

    timeout 900 python tools/sac_bench.py [--out-dir profiles]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAUNCHES = {"SAC": 15, "DDPG": 11}   # per update from given rows (fused_sac.py, fused_ddpg.py)


def _med(v):
    return sorted(v)[len(v) // 2]


def _summary(samples):
    return {k: dict(samples=v, median=_med(v), spread=max(v) - min(v)) for k, v in samples.items()}


def _compare(res):
    s, d = res["SAC"], res["DDPG"]
    s["ratio_to_DDPG"] = s["median"] / d["median"]
    s["above_DDPG_by_more_than_spread"] = bool(s["median"] - d["median"] > max(s["spread"], d["spread"]))
    return res


def _rows(B):
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.zeros(B, 88, device="cuda")
    rows[:, 0:32] = torch.randn(B, 32, generator=g, device="cuda")
    rows[:, 32:37] = (torch.rand(B, 5, generator=g, device="cuda") > 0.4).float()
    rows[:, 40:80] = rows[:, 0:40].roll(1, 0)
    rows[:, 80:82] = torch.rand(B, 2, generator=g, device="cuda") * 2 - 1
    rows[:, 82] = torch.randn(B, generator=g, device="cuda")
    rows[:, 83] = (torch.rand(B, generator=g, device="cuda") > 0.9).float()
    return rows


def update_bench(a):
    from distributional_rl_decision_and_control_amd import fused_ddpg, fused_sac
    from distributional_rl_decision_and_control_amd.learner import FusedAdam
    from distributional_rl_decision_and_control_amd.learners import LEARNERS
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    B, rows = a.batch, _rows(a.batch)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    steps = {}

    def build(name):
        spec = LEARNERS[name]
        local = spec.make_policy(DEFAULT_NET.values(), "cuda", 100)
        target = spec.make_policy(DEFAULT_NET.values(), "cuda", 100)
        ao = FusedAdam(local.actor.parameters(), lr=1e-4)
        if name == "SAC":
            co = [FusedAdam(c.parameters(), lr=1e-4) for c in (local.critic_1, local.critic_2)]
            st = fused_sac.FusedSACState(local, target, B)
            return lambda: fused_sac.sac_update_fused(st, local, ao, co, rows, seed=3, counter=counter,
                                                      counter_dev=counter)
        co = FusedAdam(local.critic.parameters(), lr=1e-4)
        st = fused_ddpg.FusedDDPGState(local, target, B)
        return lambda: fused_ddpg.ddpg_update_fused(st, local, ao, co, co.grads, ao.grads, rows, counter=counter)

    for name in ("SAC", "DDPG"):
        step = build(name)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        steps[name] = g

    def measure(g):
        for _ in range(a.warmup):
            g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            g.replay()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.steps

    samples = {k: [] for k in steps}
    for _ in range(a.reps):
        for k, g in steps.items():
            samples[k].append(measure(g))
    res = dict(bench="update_ms_graph_replay", batch=B, steps=a.steps, warmup=a.warmup, reps=a.reps,
               launches_per_update=LAUNCHES, **_summary(samples))
    return _compare(res)


def vec_bench(a):
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    E, R, B = a.envs, a.robots, a.batch
    trainers = {}
    for name in ("SAC", "DDPG"):
        tr = VecTrainer(n_envs=E, agent_type=name, num_robots=R, batch_size=B, graphs=True, unroll=a.unroll, seed=1,
                        buffer_size=1 << 20)
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
    return _compare(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--robots", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--unroll", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["update", "vec"], default=None)
    ap.add_argument("--out-dir", default=None, help="also write sac_bench_<part>.json files to this directory")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    for name, fn in (("update", update_bench), ("vec", vec_bench)):
        if a.only not in (None, name):
            continue
        line = json.dumps(fn(a))
        print(line, flush=True)
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"sac_bench_{name}.json"), "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
