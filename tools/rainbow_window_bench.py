#!/usr/bin/env python
"""Time the closed-loop window under Rainbow_Policy (asvrl_rainbow_rollout: per step the window form of the act pass
and the env step, all enqueued by one C call) against the way the same steps were taken before it, K Python rounds of
fused_rainbow.rainbow_act + DeviceEnvBatch.step (which keep no per-step record; also timed with the four copies a step
that give the window's outputs, and the window with no record kept); one evaluation of the 60 eval configs with a
seeded Rainbow network through policy/batched_eval.evaluate_configs against DeviceEvaluator.run(RainbowPack(noisy=False)),
both the eval-mode (mu only) network; and whether the window can be captured in a HIP graph.

window: both variants run eagerly in the same process from the same restored state (the restore is outside the timed
span), device events around each; --calls timed calls after --warmup make one measurement, the variants alternate,
--reps measurements give the median and the spread (max - min). The final state of the two variants is compared bit
for bit. Shapes: --shapes "E:R:O,..." (default 4096 x 5 and the 60-env evaluation shape).
eval: tools/bench_device_eval.py's protocol (one warm-up, --reps alternating repetitions, a host clock ending in a
device synchronise).
graph: one capture attempt of a K-step window with caller-supplied records, replayed once against the eager call; a
refusal by the runtime is recorded as its message, nothing is worked around. Runs last.
One process, no retries; run it under a timeout:

    timeout 600 python tools/rainbow_window_bench.py [--out-dir profiles]
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
SCHEDULE = {"num_episodes": [10] * 6, "num_robots": [3, 4, 5, 5, 5, 5], "num_cores": [0] * 6,
            "num_obstacles": [0, 0, 0, 2, 3, 4], "min_start_goal_dis": [30.0, 35.0, 40.0, 40.0, 40.0, 40.0]}


def _med(v):
    return sorted(v)[len(v) // 2]


def _batch(E, R, O):
    from distributional_rl_decision_and_control_amd.device_env import DeviceEnvBatch, reset_cfg
    b = DeviceEnvBatch(E, R, O, 0)
    b.reset(reset_cfg(R, O, 0, 40.0), seed=1)
    b.step(None, do_dynamics=False, seed=1, counter=0, fast_noise=True)   # noise mode 2
    torch.cuda.synchronize()
    return b


def _records(b, K):
    E, R = b.n_envs, b.max_robots
    spec = b._record_specs()
    spec["actions"] = ((E * R, 2), torch.float64, 0)
    rec = {n: torch.full((K,) + spec[n][0], spec[n][2], dtype=spec[n][1], device="cuda")
           for n in ("reward", "done", "info", "actions")}
    rec["steps_run"] = torch.zeros(E, dtype=torch.int32, device="cuda")
    return rec


def window_bench(a, pack):
    from distributional_rl_decision_and_control_amd.fused_rainbow import rainbow_act
    K = a.steps
    out = []
    for shape in a.shapes.split(","):
        E, R, O = (int(v) for v in shape.split(":"))
        b = _batch(E, R, O)
        tensors = (b.rs, b.rflags, b.ep_ts, b.obs)
        start = [t.clone() for t in tensors]

        def restore():
            for t, s0 in zip(tensors, start):
                t.copy_(s0)

        act64 = torch.zeros((E * R, 2), dtype=torch.float64, device="cuda")
        steps = STEP0 + torch.arange(K, dtype=torch.int64, device="cuda")   # round t's step counter
        rec = _records(b, K)

        def window():
            b.policy_rollout(pack, K, b.obs, keep=rec, step_dev=steps[:1], eps=EPS, policy_seed=POLICY_SEED, seed=1,
                             counter=10, fast_noise=True)

        def rounds():
            for t in range(K):
                rainbow_act(pack, b.obs, act64, steps[t:t + 1], *EPS, POLICY_SEED)
                b.step(act64, is_continuous=False, seed=1, counter=10 + t, fast_noise=True)

        def rounds_recording():
            """the rounds with the window's outputs: four copies a step into the same records"""
            for t in range(K):
                rainbow_act(pack, b.obs, act64, steps[t:t + 1], *EPS, POLICY_SEED)
                b.step(act64, is_continuous=False, seed=1, counter=10 + t, fast_noise=True)
                rec["reward"][t].copy_(b.reward)
                rec["done"][t].copy_(b.done)
                rec["info"][t].copy_(b.info)
                rec["actions"][t].copy_(act64)

        bare = {"steps_run": rec["steps_run"]}

        def window_bare():
            """the window with no per-step record (the record launch still counts the steps)"""
            b.policy_rollout(pack, K, b.obs, keep=bare, step_dev=steps[:1], eps=EPS, policy_seed=POLICY_SEED, seed=1,
                             counter=10, fast_noise=True)

        def measure(fn):
            """us per step over --calls timed calls (each from the restored state) after --warmup calls."""
            total = 0.0
            for i in range(a.warmup + a.calls):
                restore()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    total += e0.elapsed_time(e1)
            return 1e3 * total / (a.calls * K)

        us_w, us_r, us_rr, us_wb = [], [], [], []
        for _ in range(a.reps):
            us_w.append(measure(window))
            us_rr.append(measure(rounds_recording))
            us_wb.append(measure(window_bare))
            us_r.append(measure(rounds))
        final_r = b.rs.clone()   # the last call was the rounds'
        measure(window)
        same = bool(torch.equal(torch.nan_to_num(b.rs), torch.nan_to_num(final_r)))
        spread_w, spread_r = max(us_w) - min(us_w), max(us_r) - min(us_r)
        out.append({
            "bench": "rainbow_window_us_per_step", "agent": "Rainbow", "envs": E, "robots": R, "obstacles": O, "noise": "f32",
            "steps": K, "calls": a.calls, "warmup": a.warmup, "reps": a.reps,
            "records": ["reward", "done", "info", "actions"],
            "window_us_per_step": us_w, "rounds_us_per_step": us_r,
            "window_us_per_step_median": _med(us_w), "rounds_us_per_step_median": _med(us_r),
            "rounds_recording_us_per_step": us_rr, "rounds_recording_us_per_step_median": _med(us_rr),
            "window_bare_us_per_step": us_wb, "window_bare_us_per_step_median": _med(us_wb),
            "speedup_same_outputs": _med(us_rr) / _med(us_w),
            "window_spread_us": spread_w, "rounds_spread_us": spread_r,
            "speedup": _med(us_r) / _med(us_w),
            "differs_by_more_than_spread": bool(abs(_med(us_r) - _med(us_w)) > max(spread_w, spread_r)),
            "same_final_state": same,
        })
        print(json.dumps(out[-1]), flush=True)
    return out


def eval_bench(a, agent, pack):
    from distributional_rl_decision_and_control_amd.envs.marinenav.env import MarineNavEnv3
    from distributional_rl_decision_and_control_amd.policy.batched_eval import evaluate_configs
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    from distributional_rl_decision_and_control_amd.policy.trainer import Trainer
    z = np.load(os.path.join(ROOT, "tests", "golden", "eval60_ref.npz"))
    configs = json.loads(str(z["trained/configs"]))
    tr = Trainer(MarineNavEnv3(seed=1), MarineNavEnv3(seed=253, is_eval_env=True), SCHEDULE, agent)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

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
    res = {"bench": "rainbow_device_eval_s", "agent": "Rainbow", "configs": len(configs), "groups": len(ev.groups),
           "chunk": a.chunk, "reps": a.reps, "load_s": load_s}
    for name, v in times.items():
        res[name + "_s"], res[name + "_s_median"], res[name + "_spread_s"] = v, _med(v), max(v) - min(v)
    res["speedup_sync"] = _med(times["host"]) / _med(times["device_sync"])
    res["host_env_steps"] = int(sum(last["host"]["lengths"]))
    res["device_env_steps"] = int(sum(last["device_sync"]["lengths"]))
    res["device_windows_sync"], res["device_windows_nosync"] = windows["device_sync"], windows["device_nosync"]
    for name in ("host", "device_sync"):
        res[name + "_success_rate"] = float(np.mean(last[name]["successes"]))
        res[name + "_mean_reward"] = float(np.mean(last[name]["rewards"]))
    print(json.dumps(res), flush=True)
    return res


def graph_probe(a, pack):
    """Capture one K-step window in a graph and replay it against the eager call."""
    E, R, O = 60, 5, 4
    K = 5
    b = _batch(E, R, O)
    state = [(t, t.clone()) for t in (b.rs, b.rflags, b.ep_ts, b.obs)]
    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")

    def restore():
        for t, s0 in state:
            t.copy_(s0)

    def call(rec):
        b.policy_rollout(pack, K, b.obs, keep=rec, step_dev=step, eps=EPS, policy_seed=POLICY_SEED, seed=1, counter=10,
                         fast_noise=True)
    eager = _records(b, K)
    call(eager)
    torch.cuda.synchronize()
    final = b.rs.clone()
    restore()
    rec = _records(b, K)
    res = {"bench": "rainbow_window_graph_capture", "envs": E, "robots": R, "steps": K}
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            call(rec)
    except Exception as e:   # the runtime's refusal, for the record
        res.update(captured=False, error=f"{type(e).__name__}: {e}"[:400])
        print(json.dumps(res), flush=True)
        return res
    restore()
    g.replay()
    torch.cuda.synchronize()
    res.update(captured=True,
               same_records=all(bool(torch.equal(rec[n], eager[n])) for n in eager),
               same_final_state=bool(torch.equal(torch.nan_to_num(b.rs), torch.nan_to_num(final))))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096:5:4,60:5:4", help="E:R:O of the timed windows, comma-separated")
    ap.add_argument("--steps", type=int, default=64, help="the window length K")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=64, help="steps per window of the evaluation")
    ap.add_argument("--only", choices=["window", "eval", "graph"], default=None)
    ap.add_argument("--out-dir", default=None, help="also write rainbow_window_bench.json into this directory")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.fused_rainbow import RainbowPack
    torch.manual_seed(0)
    agent = Agent(seed=100, agent_type="Rainbow")
    pack = RainbowPack(agent.policy_local, noisy=True)        # the windows: training mode, as the collect runs them
    eval_pack = RainbowPack(agent.policy_local, noisy=False)  # the evaluation: mu only, as act_rainbow(use_eval=True)
    res = {}

    def save():
        if a.out_dir:
            os.makedirs(os.path.abspath(a.out_dir), exist_ok=True)
            with open(os.path.join(a.out_dir, "rainbow_window_bench.json"), "w") as f:
                f.write(json.dumps(res) + "\n")
    if a.only in (None, "window"):
        res["window"] = window_bench(a, pack)
        save()
    if a.only in (None, "eval"):
        res["eval"] = eval_bench(a, agent, eval_pack)
        save()
    if a.only in (None, "graph"):
        res["graph"] = graph_probe(a, pack)
        save()


if __name__ == "__main__":
    main()
