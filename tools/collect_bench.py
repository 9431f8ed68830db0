#!/usr/bin/env python
"""Time VecTrainer.collect(K) (one closed-loop window with auto-reset + one window push) against the K calls of
VecTrainer.rollout() it replaces (act, env step, replay push, reset + observation, per step), at the training shape.

Both variants are captured as HIP graphs in the same process and timed with device events around each replay, from
the same restored state (the restore is outside the timed window): --replays timed replays after --warmup replays
make one measurement, the variants alternate, and --reps measurements give the median and the spread (max - min),
per K. The envs' step counts are preset evenly over the episode limit, so every window has the steady state's share
of episode ends (about K / 1000 of the envs). The composed variant flips the observation double buffer (no copies;
K is even), the fused one copies the window's last observation once. After each K the two variants' env state, ring
state and step counter are compared bit for bit. One process, no retries; run it under a timeout:

    timeout 600 python tools/collect_bench.py [--out-dir profiles]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--robots", type=int, default=5)
    ap.add_argument("--obstacles", type=int, default=4)
    ap.add_argument("--steps", default="4,16,64", help="the window lengths K (even)")
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=None, help="also write collect_k<K>.json files to this directory")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer

    Ks = [int(k) for k in a.steps.split(",")]
    assert all(k % 2 == 0 for k in Ks), "the composed variant flips the observation buffers: K must be even"
    E, R = a.envs, a.robots
    tr = VecTrainer(n_envs=E, num_robots=R, num_obs=a.obstacles, batch_size=64, buffer_size=max(Ks) * E * R,
                    graphs=False, seed=1)
    env, b = tr.env, tr.env.batch
    limit = int(b.params.episode_limit)
    b.ep_ts.copy_((torch.arange(E, dtype=torch.int64, device="cuda") * 7919 % limit).to(torch.int32))
    torch.cuda.synchronize()
    tensors = (b.rs, b.rflags, b.n_robots, b.n_obs, b.n_cores, b.ep_ts, b.obstacles, b.cores, b.env_done, b.stats,
               env.obs[0], env.obs[1], env.cnt[0], env.cnt[1], env.counter, tr.replay.state)
    start = [t.clone() for t in tensors]

    def restore():
        for t, s0 in zip(tensors, start):
            t.copy_(s0)

    def capture(call, swap):
        env.swap, env._p = swap, 0
        restore()
        call()   # eager once: code objects loaded and buffers allocated before the capture
        torch.cuda.synchronize()
        env._p = 0
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        env._p = 0
        return g

    def measure(g, K):
        """us per step over --replays timed replays (each from the restored state) after --warmup replays."""
        total = 0.0
        for i in range(a.warmup + a.replays):
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                total += e0.elapsed_time(e1)
        return 1e3 * total / (a.replays * K)

    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    compared = (b.rs, b.rflags, b.n_robots, b.ep_ts, b.obstacles, env.obs[0], env.cnt[0], env.counter, tr.replay.state)
    for K in Ks:
        gf = capture(lambda: tr.collect(K), False)

        def composed():
            for _ in range(K):
                tr.rollout()
        gl = capture(composed, True)
        us_f, us_l = [], []
        for _ in range(a.reps):
            us_f.append(measure(gf, K))
            us_l.append(measure(gl, K))
        final_l = [t.clone() for t in compared]   # the last replay was the composed loop's
        measure(gf, K)
        same = all(bool(torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))) for x, y in zip(compared, final_l))
        resets = int(tr._collect_bufs[K]["resets"].sum().item())
        spread_f, spread_l = max(us_f) - min(us_f), max(us_l) - min(us_l)
        res = {
            "envs": E, "robots": R, "obstacles": a.obstacles, "steps": K, "replays": a.replays, "warmup": a.warmup,
            "reps": a.reps, "resets_per_window": resets,
            "fused_us_per_step": us_f, "composed_us_per_step": us_l,
            "fused_us_per_step_median": med(us_f), "composed_us_per_step_median": med(us_l),
            "fused_spread_us": spread_f, "composed_spread_us": spread_l,
            "speedup": med(us_l) / med(us_f),
            "faster_than_spread": bool(med(us_l) - med(us_f) > max(spread_f, spread_l)),
            "same_final_state": same,
        }
        line = json.dumps(res)
        print(line, flush=True)
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"collect_k{K}.json"), "w") as f:
                f.write(line + "\n")
        del gf, gl


if __name__ == "__main__":
    main()
