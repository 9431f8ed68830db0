#!/usr/bin/env python
"""Time the closed-loop rollout under SAC's sampled actor (asvrl_sac_rollout: asvrl_sac_act and the env step fused for
K steps in one launch) against the path it replaces, K x (fused_sac.sac_act + DeviceEnvBatch.step), 2 K launches; and
one device evaluation of the 60 eval configs (DeviceEvaluator.run with a SacActorPack) against the same evaluation
composed of single launches.

window: for every K of --steps both variants are captured as HIP graphs in the same process (a: one fused call; b: the
2 K launches) and timed with device events around each replay, from the same restored state (the restore is outside
the timed window): --replays timed replays after --warmup replays make one measurement, the variants alternate, and
--reps measurements give the median and the spread (max - min). The final state of the two variants is compared bit
for bit.
eval: wall clock around one whole evaluation of a seeded SAC actor (sampled, as act_sac samples in evaluation), the
windows of DeviceEvaluator.run against per-step sac_act + step + asvrl_eval_metrics launches on the same batches, one
host wait per window / per step; alternated, --reps each. One process, no retries; run it under a timeout:

    timeout 600 python tools/sac_window_bench.py [--out-dir profiles]
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

STEP0, POLICY_SEED = 7, 4242
EPS = (4096.0, 6e6, 0.25, 0.6, 0.05)   # the training schedule (VecTrainer defaults at 4096 envs)
GREEDY = (1.0, 1.0, 1.0, 0.0, 0.0)


def _med(v):
    return sorted(v)[len(v) // 2]


def _actor_pack():
    from distributional_rl_decision_and_control_amd.fused_sac import SacActorPack
    from distributional_rl_decision_and_control_amd.policy.SAC_model import SAC_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    pol = SAC_Policy(**DEFAULT_NET, value_ranges_of_action=[[-1.0, 1.0], [-1.0, 1.0]], device="cuda", seed=100)
    return SacActorPack(pol.actor)


def window_bench(a, pack):
    from distributional_rl_decision_and_control_amd.device_env import DeviceEnvBatch, reset_cfg
    from distributional_rl_decision_and_control_amd.fused_sac import sac_act
    E, R, O = a.envs, a.robots, a.obstacles
    Ks = [int(v) for v in a.steps.split(",")]
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
    eps_out = torch.zeros((E * R, 2), dtype=torch.float32, device="cuda")
    steps = STEP0 + torch.arange(max(Ks), dtype=torch.int64, device="cuda")   # round t's step counter

    def capture(call):
        restore()
        call()   # eager once: code objects loaded before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        return g

    def fused_graph(K):
        spec = b._record_specs()
        spec["actions"] = ((E * R, 2), torch.float64, 0)
        rec = {n: torch.full((K,) + spec[n][0], spec[n][2], dtype=spec[n][1], device="cuda")
               for n in ("reward", "done", "info", "actions")}
        rec["steps_run"] = torch.zeros(E, dtype=torch.int32, device="cuda")
        g = capture(lambda: b.policy_rollout(pack, K, b.obs, keep=rec, step_dev=steps[:1], eps=EPS,
                                             policy_seed=POLICY_SEED, seed=1, counter=10, fast_noise=True))
        g.records = rec   # the graph writes them at every replay and holds no reference: they live as long as it does
        return g

    def loop_graph(K):
        def call():
            for t in range(K):
                sac_act(pack, b.obs, act64, eps_out, steps[t:t + 1], *EPS, POLICY_SEED)
                b.step(act64, seed=1, counter=10 + t, fast_noise=True)
        return capture(call)

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

    out = []
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
        out.append({
            "bench": "sac_window_us_per_step", "agent": "SAC", "envs": E, "robots": R, "obstacles": O, "noise": "f32",
            "steps": K, "replays": a.replays, "warmup": a.warmup, "reps": a.reps,
            "records": ["reward", "done", "info", "actions"],
            "fused_us_per_step": us_f, "loop_us_per_step": us_l,
            "fused_us_per_step_median": _med(us_f), "loop_us_per_step_median": _med(us_l),
            "fused_spread_us": spread_f, "loop_spread_us": spread_l,
            "speedup": _med(us_l) / _med(us_f),
            "faster_than_spread": bool(_med(us_l) - _med(us_f) > max(spread_f, spread_l)),
            "same_final_state": same,
        })
        print(json.dumps(out[-1]), flush=True)
        del gf, gl
    return out


def eval_bench(a, pack):
    from distributional_rl_decision_and_control_amd.fused_sac import sac_act
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator, eval_metrics
    z = np.load(os.path.join(ROOT, "tests", "golden", "eval60_ref.npz"))
    configs = json.loads(str(z["trained/configs"]))
    ev = DeviceEvaluator(configs, chunk=a.chunk)
    limit, seed = a.episode_limit, 0

    def windows():
        return ev.run(pack, seed=seed, episode_limit=limit, policy_seed=POLICY_SEED)

    scratch = []
    for grp in ev.groups:
        b = grp.batch
        NT = b.n_envs * b.max_robots
        scratch.append((torch.zeros((NT, 2), dtype=torch.float64, device="cuda"),
                        torch.zeros((NT, 2), dtype=torch.float32, device="cuda")))

    def composed():
        """run()'s evaluation in single launches: per step and group sac_act, the step under the metrics' alive mask,
        and asvrl_eval_metrics on that one step."""
        ev.observe(None, seed)
        for t in range(limit + 1):
            for g, grp in enumerate(ev.groups):
                b, st = grp.batch, grp.state
                act64, eps_out = scratch[g]
                rec = grp.records(1)
                grp.step.fill_(t)
                sac_act(pack, b.obs, act64, eps_out, grp.step, *GREEDY, POLICY_SEED + g)
                b.step(act64, trainer_deactivate=True, seed=seed + g, counter=t, fast_noise=True, env_mask=st["alive"])
                rec["reward"][0].copy_(b.reward)
                rec["info"][0].copy_(b.info)
                rec["rs"][0].copy_(b.rs)
                rec["steps_run"].copy_(st["alive"])
                eval_metrics(pack.L, 1, b.n_envs, b.max_robots, rec, b.n_robots, grp.dt, grp.N, grp.pc, st, ev.gamma,
                             limit)
            if not any(bool(grp.state["alive"].any().item()) for grp in ev.groups):
                break
        return ev._result()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    timed(windows), timed(composed)   # code objects loaded, records allocated
    s_w, s_c = [], []
    for _ in range(a.reps):
        tw, rw = timed(windows)
        tc, rc = timed(composed)
        s_w.append(tw)
        s_c.append(tc)
    res = {
        "bench": "sac_device_eval_s", "configs": len(configs), "groups": len(ev.groups), "chunk": a.chunk,
        "episode_limit": limit, "reps": a.reps, "sampled": True,
        "windows_s": s_w, "composed_s": s_c, "windows_s_median": _med(s_w), "composed_s_median": _med(s_c),
        "windows_spread_s": max(s_w) - min(s_w), "composed_spread_s": max(s_c) - min(s_c),
        "speedup": _med(s_c) / _med(s_w), "windows_run": ev.windows,
        "same_lengths_and_successes": rw["lengths"] == rc["lengths"] and rw["successes"] == rc["successes"],
        "max_episode_length": max(rw["lengths"]), "success_rate": float(np.mean(rw["successes"])),
    }
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--robots", type=int, default=5)
    ap.add_argument("--obstacles", type=int, default=4)
    ap.add_argument("--steps", default="1,64", help="the window lengths K, comma-separated")
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=64, help="steps per window of the evaluation")
    ap.add_argument("--episode-limit", type=int, default=1000)
    ap.add_argument("--only", choices=["window", "eval"], default=None)
    ap.add_argument("--out-dir", default=None, help="also write sac_window_bench.json into this directory")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    pack = _actor_pack()
    res = {}
    if a.only in (None, "window"):
        res["window"] = window_bench(a, pack)
    if a.only in (None, "eval"):
        res["eval"] = eval_bench(a, pack)
    if a.out_dir:
        os.makedirs(os.path.abspath(a.out_dir), exist_ok=True)
        with open(os.path.join(a.out_dir, "sac_window_bench.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
