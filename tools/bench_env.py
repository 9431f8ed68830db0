#!/usr/bin/env python3
"""Env-step kernel alone (asvrl_env_step, Philox perception noise, random continuous actions) at
E = 4096 ... 2^18 envs (R=5, O=4, 55 m map): average launch time with HIP
events, env-steps/s and the algorithmic-byte rate (1,904 B per env-step) against the 8 TB/s
HBM peak. One JSON line per E.

    python tools/bench_env.py [--envs 4096,16384,65536,262144] [--iters 20]

--rollout [K] (K = 64 when not given) times the fused K-step rollout (asvrl_env_rollout, one launch) against K
back-to-back single launches on the same stream in the same process, from the same state, --reps times each
in alternation; default 4096 envs, f32 draws. Per-step time of both, the algorithmic bytes per step (one step's
state and outputs once per launch, plus every step's actions and kept records) and the HBM fraction
(roofline_env_k<K>); --no-records keeps no per-step record (default: reward, done, info).

    python tools/bench_env.py --rollout 64 [--no-records] [--reps 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default=None, help="default 4096,16384,65536,262144 (--rollout: 4096)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--robots", type=int, default=5)
    ap.add_argument("--obstacles", type=int, default=4)
    ap.add_argument("--width", type=float, default=55.0, help="map width = height (config 5: 110)")
    ap.add_argument("--noise", default=None,
                    help="Philox draw precision(s): f32 (noise_mode 2), f64 (1); default f32,f64 (--rollout: f32)")
    ap.add_argument("--rollout", type=int, nargs="?", const=64, default=None, metavar="K",
                    help="time the fused K-step rollout against K single launches (K = 64 when not given)")
    ap.add_argument("--no-records", action="store_true", help="--rollout: keep no per-step record")
    ap.add_argument("--reps", type=int, default=5, help="--rollout: timed repetitions of each path")
    ap.add_argument("--obs-only", action="store_true", help="time the observation pass alone (do_dynamics=0)")
    ap.add_argument("--launch", default="auto",
                    help="';'-separated launch shapes layout,block,envs_per_block (asvrl_env_step_ex), or auto")
    a = ap.parse_args()
    a.envs = a.envs or ("4096" if a.rollout else "4096,16384,65536,262144")
    a.noise = a.noise or ("f32" if a.rollout else "f32,f64")
    from distributional_rl_decision_and_control_amd.device_env import DeviceEnvBatch, reset_cfg
    R, O = a.robots, a.obstacles
    bpe = R * 360 + 24 * O + 8
    shapes = [None if x == "auto" else tuple(int(v) for v in x.split(",")) for x in a.launch.split(";")]
    for E, mode, ln in [(int(x), m, s) for x in a.envs.split(",") for m in a.noise.split(",") for s in shapes]:
        fast = mode == "f32"
        if a.rollout:
            bench_rollout(a, E, R, O, fast, ln, bpe)
            continue
        b = DeviceEnvBatch(E, R, O, 0)
        b.reset(reset_cfg(R, O, 0, 40.0, a.width, a.width), seed=1)
        b.step(None, do_dynamics=False, seed=1, counter=0, fast_noise=fast)
        g = torch.Generator(device="cuda").manual_seed(0)
        acts = [(torch.rand((E * R, 2), generator=g, device="cuda", dtype=torch.float64) * 2 - 1) for _ in range(4)]
        for t in range(3):
            b.step(acts[t % 4], seed=1, counter=t + 1, trainer_deactivate=False, fast_noise=fast)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(a.iters):
            if a.obs_only:
                b.step(None, do_dynamics=False, seed=1, counter=t + 10, fast_noise=fast, launch=ln)
            else:
                b.step(acts[t % 4], seed=1, counter=t + 10, trainer_deactivate=False, fast_noise=fast, launch=ln)
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / a.iters
        gbs = bpe * E / (us * 1e-6) / 1e9
        print(json.dumps({"envs": E, "noise": mode, "obs_only": a.obs_only, "robots": R, "obstacles": O, "width": a.width,
                          "launch": list(ln) if ln else "auto", "us_per_step": us, "env_steps_per_s": E / (us * 1e-6),
                          "alg_bytes_per_env_step": bpe, "achieved_GBps": gbs, "hbm_frac": gbs / 8000.0}))
        del b


def bench_rollout(a, E, R, O, fast, ln, bpe):
    """One JSON line: the K-step rollout and the K-launch loop, per step, from the same state."""
    from distributional_rl_decision_and_control_amd.device_env import DeviceEnvBatch, reset_cfg
    K = a.rollout
    keep = () if a.no_records else ("reward", "done", "info")
    b = DeviceEnvBatch(E, R, O, 0)
    b.reset(reset_cfg(R, O, 0, 40.0, a.width, a.width), seed=1)
    b.step(None, do_dynamics=False, seed=1, counter=0, fast_noise=fast)
    g = torch.Generator(device="cuda").manual_seed(0)
    acts = torch.rand((K, E * R, 2), generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    start = [t.clone() for t in (b.rs, b.rflags, b.ep_ts)]
    spec = b._record_specs()
    rec = {n: torch.full((K,) + spec[n][0], spec[n][2], dtype=spec[n][1], device="cuda") for n in keep}
    rec["steps_run"] = torch.zeros(E, dtype=torch.int32, device="cuda")

    def restore():
        for t, s0 in zip((b.rs, b.rflags, b.ep_ts), start):
            t.copy_(s0)

    def fused():
        b.rollout(acts, keep=rec, seed=1, counter=10, fast_noise=fast, launch=ln)

    def loop():
        for t in range(K):
            b.step(acts[t], seed=1, counter=10 + t, trainer_deactivate=False, fast_noise=fast, launch=ln)

    def timed(fn):
        restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / K

    for fn in (fused, loop, fused, loop):   # warm-up
        timed(fn)
    us_f, us_l = [], []
    for _ in range(a.reps):
        us_f.append(timed(fused))
        us_l.append(timed(loop))
    final_f = b.rs.clone()   # the last timed run was the loop: its state against the rollout's
    timed(fused)
    final_l, final_f = final_f, b.rs.clone()
    per_robot = {"reward": 8, "done": 1, "info": 1, "obs": 160, "obj_cnt": 1, "rs": 136}
    rec_bytes = sum(R * per_robot[n] for n in keep)   # per env, per step
    bytes_launch = E * (bpe + (K - 1) * 16 * R + K * rec_bytes)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    us = med(us_f)
    gbs = bytes_launch / K / (us * 1e-6) / 1e9
    print(json.dumps({
        "envs": E, "noise": "f32" if fast else "f64", "robots": R, "obstacles": O, "width": a.width,
        "launch": list(ln) if ln else "auto", "rollout_steps": K, "records": list(keep), "reps": a.reps,
        "rollout_us_per_step": us_f, "loop_us_per_step": us_l, "rollout_us_per_step_median": us,
        "loop_us_per_step_median": med(us_l), "loop_spread_us": max(us_l) - min(us_l),
        "rollout_spread_us": max(us_f) - min(us_f), "speedup": med(us_l) / us,
        "same_final_state": bool(torch.equal(torch.nan_to_num(final_f), torch.nan_to_num(final_l))),
        "alg_bytes_per_env_step_single": bpe, "alg_bytes_per_env_step": bytes_launch / K / E,
        f"roofline_env_k{K}": {"kernel": "asvrl_env_rollout (env_rollout_kernel)", "bound": "hbm",
                               "us_per_step": us, "alg_bytes_per_step": bytes_launch / K, "achieved_GBps": gbs,
                               "peak_GBps": 8000.0, "hbm_frac": gbs / 8000.0}}))


if __name__ == "__main__":
    main()
