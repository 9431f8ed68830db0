#!/usr/bin/env python
"""Time the closed-loop rollout under DQN_Policy (asvrl_dqn_rollout: asvrl_dqn_act and the env step fused for K
steps in one launch) against the path it replaces: K x (fused_dqn.dqn_act + DeviceEnvBatch.step(is_continuous=False)),
2 K launches.

For every K of --steps both variants are captured as HIP graphs in the same process (a: one fused call; b: the 2 K
launches) and timed with device events around each replay, from the same restored state (the restore is outside the
timed window): --replays timed replays after --warmup replays make one measurement, the variants alternate, and
--reps measurements give the median and the spread (max - min). The final state of the two variants is compared bit
for bit. One JSON file per K. One process, no retries; run it under a timeout:

    timeout 300 python tools/dqn_rollout_bench.py [--out-dir profiles]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEP0, POLICY_SEED = 7, 4242
EPS = (4096.0, 6e6, 0.25, 0.6, 0.05)   # the training schedule (VecTrainer defaults at 4096 envs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--robots", type=int, default=5)
    ap.add_argument("--obstacles", type=int, default=4)
    ap.add_argument("--steps", default="1,8,64", help="the window lengths K, comma-separated")
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launch", default=None, help="layout,block,envs_per_block of the fused call (default: automatic)")
    ap.add_argument("--out-dir", default=None, help="also write dqn_rollout_k<K>.json for every K into this directory")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from distributional_rl_decision_and_control_amd.device_env import DeviceEnvBatch, reset_cfg
    from distributional_rl_decision_and_control_amd.fused_dqn import DqnPack, dqn_act
    from distributional_rl_decision_and_control_amd.policy.DQN_model import DQN_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET

    E, R, O = a.envs, a.robots, a.obstacles
    ln = tuple(int(v) for v in a.launch.split(",")) if a.launch else None
    Ks = [int(v) for v in a.steps.split(",")]
    pack = DqnPack(DQN_Policy(**DEFAULT_NET, action_size=25, device="cuda", seed=100).to("cuda"))
    b = DeviceEnvBatch(E, R, O, 0)
    b.reset(reset_cfg(R, O, 0, 40.0), seed=1)
    b.step(None, do_dynamics=False, seed=1, counter=0, fast_noise=True)   # noise mode 2
    torch.cuda.synchronize()
    tensors = (b.rs, b.rflags, b.ep_ts, b.obs)
    start = [t.clone() for t in tensors]

    def restore():
        for t, s0 in zip(tensors, start):
            t.copy_(s0)

    act64 = torch.zeros((E * R, 2), dtype=torch.float64, device="cuda")
    steps = STEP0 + torch.arange(max(Ks), dtype=torch.int64, device="cuda")   # round t's step counter

    def fused_graph(K):
        spec = b._record_specs()
        spec["actions"] = ((E * R, 2), torch.float64, 0)
        rec = {n: torch.full((K,) + spec[n][0], spec[n][2], dtype=spec[n][1], device="cuda")
               for n in ("reward", "done", "info", "actions")}
        rec["steps_run"] = torch.zeros(E, dtype=torch.int32, device="cuda")

        def call():
            b.policy_rollout(pack, K, b.obs, keep=rec, step_dev=steps[:1], eps=EPS, policy_seed=POLICY_SEED, seed=1,
                             counter=10, fast_noise=True, launch=ln)
        g = capture(call)
        # the graph writes the records at every replay and holds no reference to them: they live as long as it does
        # (a later capture empties the allocator's cache, which would unmap them once freed)
        g.records = rec
        return g

    def loop_graph(K):
        def call():
            for t in range(K):
                dqn_act(pack, b.obs, act64, steps[t:t + 1], *EPS, POLICY_SEED)
                b.step(act64, is_continuous=False, seed=1, counter=10 + t, fast_noise=True)
        return capture(call)

    def capture(call):
        restore()
        call()   # eager once: code objects loaded before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
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
    for K in Ks:
        gf, gl = fused_graph(K), loop_graph(K)
        us_f, us_l = [], []
        for _ in range(a.reps):
            us_f.append(measure(gf, K))
            us_l.append(measure(gl, K))
        final_l = b.rs.clone()   # the last replay was the loop's
        measure(gf, K)
        same = bool(torch.equal(torch.nan_to_num(b.rs), torch.nan_to_num(final_l)))
        spread_f, spread_l = max(us_f) - min(us_f), max(us_l) - min(us_l)
        res = {
            "agent": "DQN", "envs": E, "robots": R, "obstacles": O, "noise": "f32", "launch": list(ln) if ln else "auto",
            "steps": K, "replays": a.replays, "warmup": a.warmup, "reps": a.reps,
            "records": ["reward", "done", "info", "actions"],
            "fused_us_per_step": us_f, "loop_us_per_step": us_l,
            "fused_us_per_step_median": med(us_f), "loop_us_per_step_median": med(us_l),
            "fused_spread_us": spread_f, "loop_spread_us": spread_l,
            "speedup": med(us_l) / med(us_f),
            "faster_than_spread": bool(med(us_l) - med(us_f) > max(spread_f, spread_l)),
            "same_final_state": same,
        }
        line = json.dumps(res)
        print(line)
        if a.out_dir:
            os.makedirs(os.path.abspath(a.out_dir), exist_ok=True)
            with open(os.path.join(a.out_dir, f"dqn_rollout_k{K}.json"), "w") as f:
                f.write(line + "\n")
        del gf, gl


if __name__ == "__main__":
    main()
