#!/usr/bin/env python
"""Cost of the device-side target update (VecTrainer target_update="device") on the AC-IQN loop at the bench shape:
4096 envs x 5 robots, B = 4096, N = 32, graphs on, 20 iterations per captured graph. Three trainers in one process:

    default     target_update="host", tau = 1 (what bench.py runs: no target launch in the graph)
    device-off  target_update="device", interval 2500, tau = 1: the two predicated-off launches every step
    device-on   target_update="device", interval 1, tau = 0.005: Polyak averaging every step

A measurement is --steps timed steps after two warm-up replays (wall clock around a device synchronise); the
trainers alternate, and --reps measurements give the median and the spread (max - min) of each. With --trace the
trainers run one after the other instead, device-off first, each for --steps steps once: the workload for

    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/target_update_bench.py --trace

and `--summarise DIR/.../run_kernel_trace.csv` then splits target_update_kernel's dispatches into the ones that
wrote nothing (the first trainer's) and the ones that fired, per grid size (actor, critic). One process, no retries;
run it under a timeout:

    timeout 600 python tools/target_update_bench.py [--out profiles/NAME.json]
"""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = (("default", {}),
           ("device-off", dict(target_update="device", target_update_interval=2500, tau=1.0)),
           ("device-on", dict(target_update="device", target_update_interval=1, tau=0.005)))


def _med(v):
    return sorted(v)[len(v) // 2]


def _trainer(a, kw):
    import torch
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    tr = VecTrainer(n_envs=a.envs, agent_type="AC-IQN", num_robots=5, batch_size=a.batch, num_tau=32, graphs=True,
                    unroll=a.unroll, seed=1, buffer_size=1 << 20, **kw)
    while tr.replay_size_host() < tr.learning_starts:
        tr.iteration()
    for _ in range(2 * a.unroll):   # captures the graph
        tr.iteration()
    torch.cuda.synchronize()
    assert tr.graphs and tr._graph is not None, "the graph was not captured"
    return tr


def _measure(tr, a):
    import torch
    n = (a.steps // a.unroll) * a.unroll
    for _ in range(2 * a.unroll):
        tr.iteration()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tr.iteration()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def bench(a):
    trainers = {name: _trainer(a, kw) for name, kw in CONFIGS}
    samples = {k: [] for k in trainers}
    for _ in range(a.reps):
        for k, tr in trainers.items():
            samples[k].append(_measure(tr, a))
    res = dict(bench="target_update_ms_per_step", envs=a.envs, batch=a.batch, unroll=a.unroll, steps=a.steps,
               reps=a.reps)
    for k, v in samples.items():
        res[k] = dict(samples=v, median=_med(v), spread=max(v) - min(v), config=dict(CONFIGS)[k])
    for k in ("device-off", "device-on"):
        res[k]["minus_default_ms"] = res[k]["median"] - res["default"]["median"]
    return res


def trace(a):
    """device-off, then device-on, each captured and run for --steps steps: the kernel trace's first
    target_update_kernel dispatches are the predicated-off ones."""
    counts = {}
    for name, kw in CONFIGS[1:]:
        tr = _trainer(a, kw)
        _measure(tr, a)
        counts[name] = int(tr.learn_counter.item())
        del tr
    return dict(bench="target_update_trace", learn_steps=counts, launches_per_step=2)


def summarise(path):
    """Per grid size: the dispatches of target_update_kernel in time order, split where device-off ends (its
    launches write nothing and return at once; the trace holds them first)."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "target_update_kernel" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]),
                             int(r["Grid_Size_X"] if "Grid_Size_X" in r else r["Grid_Size"])))
    rows.sort()
    out = {"dispatches": len(rows)}
    half = len(rows) // 2   # both trainers enqueue the same number of steps (trace())
    for name, part in (("off", rows[:half]), ("fired", rows[half:])):
        for grid in sorted({g for _, _, g in part}):
            d = sorted(t for _, t, g in part if g == grid)
            out[f"{name}_grid{grid}"] = dict(n=len(d), median_ns=d[len(d) // 2], min_ns=d[0], max_ns=d[-1],
                                             mean_ns=sum(d) / len(d))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--unroll", type=int, default=20)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="CSV", default=None)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.summarise:
        res = summarise(a.summarise)
    else:
        import torch
        assert torch.cuda.is_available(), "this benchmark needs the GPU"
        res = trace(a) if a.trace else bench(a)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
