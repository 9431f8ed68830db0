#!/usr/bin/env python
"""Time the closed-loop window of one policy (DeviceEnvBatch.policy_rollout with that policy's pack) against the path it
replaces, K x (the policy's act call + DeviceEnvBatch.step); for SAC, IQN and Rainbow also one device evaluation of the
60 eval configs, and for IQN and Rainbow whether the window can be captured in a HIP graph.

    timeout 600 python tools/window_bench.py --policy {actor,dqn,sac,iqn,rainbow} [--out-dir profiles]

window: the protocol follows from the pack. Where the act runs inside the env kernel (an MlpPack: actor, dqn, sac; one
launch for K steps) both variants are captured as HIP graphs (a: one fused call; b: the 2 K launches) and timed with
device events around each replay: --calls timed replays after --warmup make one measurement. Where the window is K
launches enqueued by one C call (iqn, rainbow) both variants run eagerly, device events around each call; the rounds
are also timed with the four copies a step that give the window's outputs, and the window with no record kept; for IQN also the window
at cvar = 0.25 and under fused_iqn.AdaptiveCvar (window_cvar025, window_adaptive). Either
way every call starts from the same restored state (the restore is outside the timed span), the variants alternate,
--reps measurements give the median and the spread (max - min), and the final state of the two variants is compared
bit for bit. Shapes: --shapes "E:R:O,..."; window lengths: --steps "K,...". The Actor's fused per-step time is also
taken at K = 1 and K = 8.
eval (sac): wall clock around one whole evaluation of a seeded SAC actor (sampled, as act_sac samples in evaluation),
the windows of DeviceEvaluator.run against per-step sac_act + step + asvrl_eval_metrics launches on the same batches,
one host wait per window / per step; alternated, --reps each.
eval (iqn, rainbow): tools/bench_device_eval.py's protocol (one warm-up, --reps alternating repetitions, a host clock
ending in a device synchronise) of policy/batched_eval.evaluate_configs against DeviceEvaluator.run (Rainbow: both the
eval-mode, mu only, network; IQN: also at cvar = 0.25 and under AdaptiveCvar, device_cvar025 and device_adaptive).
graph (iqn, rainbow): one capture attempt of a K-step window with caller-supplied records, replayed once against the
eager call; a refusal by the runtime is recorded as its message, nothing is worked around. Runs last.

Output: every result is printed as one JSON line. actor: --out FILE (profiles/policy_rollout_k64.json); dqn: --out-dir
gets dqn_rollout_k<K>.json for every K; sac, iqn, rainbow: --out-dir gets <policy>_window_bench.json. The library is
chosen by ASVRL_LIB as everywhere (_abi.py). One process, no retries; run it under a timeout."""
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
RECORDS = ("reward", "done", "info", "actions")
SCHEDULE = {"num_episodes": [10] * 6, "num_robots": [3, 4, 5, 5, 5, 5], "num_cores": [0] * 6,
            "num_obstacles": [0, 0, 0, 2, 3, 4], "min_start_goal_dis": [30.0, 35.0, 40.0, 40.0, 40.0, 40.0]}
# per policy: the agent's name, the sections, and the defaults of --shapes, --steps, --calls, --warmup, --reps
POLICIES = {
    "actor": ("AC-IQN", ("window",), "4096:5:4", "64", 20, 5, 5),
    "dqn": ("DQN", ("window",), "4096:5:4", "1,8,64", 20, 5, 5),
    "sac": ("SAC", ("window", "eval"), "4096:5:4", "1,64", 20, 5, 5),
    "iqn": ("IQN", ("window", "eval", "graph"), "4096:5:4,60:5:4", "64", 10, 3, 3),
    "rainbow": ("Rainbow", ("window", "eval", "graph"), "4096:5:4,60:5:4", "64", 10, 3, 3),
}


def _med(v):
    return sorted(v)[len(v) // 2]


def make_policy(policy):
    """(agent or None, the window's pack, the evaluation's pack, act(pack, obs, act64, step, eps, seed)) on a seeded
    network; the packs and the act calls are the package's own."""
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    if policy == "actor":
        from distributional_rl_decision_and_control_amd.fused_mlp import MlpPack, actor_act
        from distributional_rl_decision_and_control_amd.policy.AC_IQN_model import AC_IQN_Policy
        pol = AC_IQN_Policy(**DEFAULT_NET, value_ranges_of_action=[[-1, 1], [-1, 1]], device="cuda", seed=100)
        pack = MlpPack(pol.actor, "actor")
        return None, pack, pack, lambda p, obs, a64, step, eps, seed: actor_act(p, obs, a64, step, *eps, seed)
    if policy == "dqn":
        from distributional_rl_decision_and_control_amd.fused_dqn import DqnPack, dqn_act
        from distributional_rl_decision_and_control_amd.policy.DQN_model import DQN_Policy
        pack = DqnPack(DQN_Policy(**DEFAULT_NET, action_size=25, device="cuda", seed=100).to("cuda"))
        return None, pack, pack, lambda p, obs, a64, step, eps, seed: dqn_act(p, obs, a64, step, *eps, seed)
    if policy == "sac":
        from distributional_rl_decision_and_control_amd.fused_sac import SacActorPack, sac_act
        from distributional_rl_decision_and_control_amd.policy.SAC_model import SAC_Policy
        pol = SAC_Policy(**DEFAULT_NET, value_ranges_of_action=[[-1.0, 1.0], [-1.0, 1.0]], device="cuda", seed=100)
        pack = SacActorPack(pol.actor)
        eps_out = {}   # rows -> the eps of the sample, which nothing here reads

        def act(p, obs, a64, step, eps, seed):
            n = obs.shape[0]
            if n not in eps_out:
                eps_out[n] = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
            sac_act(p, obs, a64, eps_out[n], step, *eps, seed)
        return None, pack, pack, act
    from distributional_rl_decision_and_control_amd.agent import Agent
    torch.manual_seed(0)
    agent = Agent(seed=100, agent_type=POLICIES[policy][0])
    if policy == "iqn":
        from distributional_rl_decision_and_control_amd.fused_iqn import IqnPack, iqn_act
        pack = IqnPack(agent.policy_local)
        return agent, pack, pack, lambda p, obs, a64, step, eps, seed: iqn_act(p, None, a64, step, *eps, seed, obs=obs)
    from distributional_rl_decision_and_control_amd.fused_rainbow import RainbowPack, rainbow_act
    pack = RainbowPack(agent.policy_local, noisy=True)        # the windows: training mode, as the collect runs them
    eval_pack = RainbowPack(agent.policy_local, noisy=False)  # the evaluation: mu only, as act_rainbow(use_eval=True)
    return agent, pack, eval_pack, lambda p, obs, a64, step, eps, seed: rainbow_act(p, obs, a64, step, *eps, seed)


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
    rec = {n: torch.full((K,) + spec[n][0], spec[n][2], dtype=spec[n][1], device="cuda") for n in RECORDS}
    rec["steps_run"] = torch.zeros(E, dtype=torch.int32, device="cuda")
    return rec


def _restorer(b):
    state = [(t, t.clone()) for t in (b.rs, b.rflags, b.ep_ts, b.obs)]

    def restore():
        for t, s0 in state:
            t.copy_(s0)
    return restore


# ------------------------------------------------------------------ window
def window_bench(a, pack, act):
    from distributional_rl_decision_and_control_amd.fused_mlp import MlpPack
    one_launch = isinstance(pack, MlpPack)   # the act runs inside the env kernel: graphs; else K launches: eager
    Ks = [int(v) for v in a.steps.split(",")]
    out = []
    for shape in a.shapes.split(","):
        E, R, O = (int(v) for v in shape.split(":"))
        b = _batch(E, R, O)
        restore = _restorer(b)
        act64 = torch.zeros((E * R, 2), dtype=torch.float64, device="cuda")
        steps = STEP0 + torch.arange(max(Ks + [8]), dtype=torch.int64, device="cuda")   # round t's step counter

        def window(K, rec, **options):
            b.policy_rollout(pack, K, b.obs, keep=rec, step_dev=steps[:1], eps=EPS, policy_seed=POLICY_SEED, seed=1,
                             counter=10, fast_noise=True, launch=a.launch, **options)

        def rounds(K, rec=None):
            """rec: the rounds with the window's outputs, four copies a step into the same records"""
            for t in range(K):
                act(pack, b.obs, act64, steps[t:t + 1], EPS, POLICY_SEED)
                b.step(act64, is_continuous=pack.continuous, seed=1, counter=10 + t, fast_noise=True)
                if rec is not None:
                    for n, src in zip(RECORDS, (b.reward, b.done, b.info, act64)):
                        rec[n][t].copy_(src)

        def graph(call):
            restore()
            call()   # eager once: code objects loaded before the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                call()
            return g

        def measure(fn, K):
            """us per step over --calls timed calls (each from the restored state) after --warmup calls."""
            total = 0.0
            for i in range(a.warmup + a.calls):
                restore()
                if not one_launch:
                    torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    total += e0.elapsed_time(e1)
            return 1e3 * total / (a.calls * K)

        def fused(K):
            rec = _records(b, K)
            g = graph(lambda: window(K, rec))
            # the graph writes the records at every replay and holds no reference to them: they live as long as it does
            # (a later capture empties the allocator's cache, which would unmap them once freed)
            g.records = rec
            return g

        for K in Ks:
            res = {"envs": E, "robots": R, "obstacles": O, "noise": "f32", "steps": K, "warmup": a.warmup,
                   "reps": a.reps, "records": list(RECORDS)}
            if one_launch:
                gf, gl = fused(K), graph(lambda: rounds(K))
                w, r = gf.replay, gl.replay
                names = ("fused", "loop")
                variants = {"fused": w, "loop": r}
            else:
                rec, bare = _records(b, K), {"steps_run": torch.zeros(E, dtype=torch.int32, device="cuda")}
                w, r = (lambda: window(K, rec)), (lambda: rounds(K))
                names = ("window", "rounds")
                # (the bare window keeps no per-step record: the record launch still counts the steps)
                variants = {"window": w, "rounds_recording": lambda: rounds(K, rec),
                            "window_bare": lambda: window(K, bare), "rounds": r}
                if pack.takes_cvar:   # IQN: the scalar risk level and the per-robot adaptive one, in the same session
                    from distributional_rl_decision_and_control_amd.fused_iqn import AdaptiveCvar
                    variants["window_cvar025"] = lambda: window(K, rec, cvar=0.25)
                    variants["window_adaptive"] = lambda: window(K, rec, cvar=AdaptiveCvar())
                    variants["rounds"] = variants.pop("rounds")   # the rounds stay the last call of a repetition
            us = {n: [] for n in variants}
            for _ in range(a.reps):
                for n, fn in variants.items():
                    us[n].append(measure(fn, K))
            final_r = b.rs.clone()   # the last call was the rounds'
            measure(w, K)
            same = bool(torch.equal(torch.nan_to_num(b.rs), torch.nan_to_num(final_r)))
            for n, v in us.items():
                res[n + "_us_per_step"], res[n + "_us_per_step_median"] = v, _med(v)
            mw, mr = _med(us[names[0]]), _med(us[names[1]])
            spread = [max(us[n]) - min(us[n]) for n in names]
            res[names[0] + "_spread_us"], res[names[1] + "_spread_us"] = spread
            res["speedup"] = mr / mw
            if one_launch:
                res["replays"] = a.calls
                res["faster_than_spread"] = bool(mr - mw > max(spread))
            else:
                res["calls"] = a.calls
                res["speedup_same_outputs"] = _med(us["rounds_recording"]) / mw
                res["differs_by_more_than_spread"] = bool(abs(mr - mw) > max(spread))
            res["same_final_state"] = same
            if a.policy == "actor":
                for k in (1, 8):
                    g = fused(k)
                    small = [measure(g.replay, k) for _ in range(a.reps)]
                    res[f"fused_us_per_step_k{k}"], res[f"fused_us_per_step_k{k}_median"] = small, _med(small)
            else:
                res["agent"] = POLICIES[a.policy][0]
            if a.policy in ("actor", "dqn"):   # the two oldest files name the launch shape, the later ones the bench
                res["launch"] = list(a.launch) if a.launch else "auto"
            else:
                res["bench"] = a.policy + "_window_us_per_step"
            out.append(res)
            print(json.dumps(res), flush=True)
            del variants, w, r   # and the graphs with them, before the next capture
            gf = gl = None
    return out


# ------------------------------------------------------------------ eval
def _eval_configs():
    z = np.load(os.path.join(ROOT, "tests", "golden", "eval60_ref.npz"))
    return json.loads(str(z["trained/configs"]))


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def eval_against_single_launches(a, pack, act):
    """sac: the windows of DeviceEvaluator.run against the same evaluation composed of single launches."""
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator, eval_metrics
    configs = _eval_configs()
    ev = DeviceEvaluator(configs, chunk=a.chunk)
    limit, seed = a.episode_limit, 0

    def windows():
        return ev.run(pack, seed=seed, episode_limit=limit, policy_seed=POLICY_SEED)

    scratch = [torch.zeros((grp.batch.n_envs * grp.batch.max_robots, 2), dtype=torch.float64, device="cuda")
               for grp in ev.groups]

    def composed():
        """run()'s evaluation in single launches: per step and group the act, the step under the metrics' alive mask,
        and asvrl_eval_metrics on that one step."""
        ev.observe(None, seed)
        for t in range(limit + 1):
            for g, grp in enumerate(ev.groups):
                b, st = grp.batch, grp.state
                rec = grp.records(1)
                grp.step.fill_(t)
                act(pack, b.obs, scratch[g], grp.step, GREEDY, POLICY_SEED + g)
                b.step(scratch[g], trainer_deactivate=True, seed=seed + g, counter=t, fast_noise=True,
                       env_mask=st["alive"])
                rec["reward"][0].copy_(b.reward)
                rec["info"][0].copy_(b.info)
                rec["rs"][0].copy_(b.rs)
                rec["steps_run"].copy_(st["alive"])
                eval_metrics(pack.L, 1, b.n_envs, b.max_robots, rec, b.n_robots, grp.dt, grp.N, grp.pc, st, ev.gamma,
                             limit)
            if not any(bool(grp.state["alive"].any().item()) for grp in ev.groups):
                break
        return ev._result()

    _clock(windows), _clock(composed)   # code objects loaded, records allocated
    s_w, s_c = [], []
    for _ in range(a.reps):
        tw, rw = _clock(windows)
        tc, rc = _clock(composed)
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


def eval_against_host(a, agent, pack):
    """iqn, rainbow: evaluate_configs on the host against DeviceEvaluator.run."""
    from distributional_rl_decision_and_control_amd.envs.marinenav.env import MarineNavEnv3
    from distributional_rl_decision_and_control_amd.policy.batched_eval import evaluate_configs
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    from distributional_rl_decision_and_control_amd.policy.trainer import Trainer
    configs = _eval_configs()
    tr = Trainer(MarineNavEnv3(seed=1), MarineNavEnv3(seed=253, is_eval_env=True), SCHEDULE, agent)
    load_s, ev = _clock(lambda: DeviceEvaluator(configs, template_env=tr.eval_env, chunk=a.chunk, gamma=agent.GAMMA))
    runs = {"host": lambda: evaluate_configs(agent, configs, template_env=tr.eval_env),
            "device_sync": lambda: ev.run(pack, seed=1),
            "device_nosync": lambda: ev.run(pack, seed=1, sync=False)}
    if pack.takes_cvar:
        from distributional_rl_decision_and_control_amd.fused_iqn import AdaptiveCvar
        runs["device_cvar025"] = lambda: ev.run(pack, seed=1, cvar=0.25)
        runs["device_adaptive"] = lambda: ev.run(pack, seed=1, cvar=AdaptiveCvar())
    times = {k: [] for k in runs}
    last, windows = {}, {}
    for rep in range(a.reps + 1):   # the first round is the warm-up
        for name, fn in runs.items():
            s, last[name] = _clock(fn)
            windows[name] = ev.windows
            if rep > 0:
                times[name].append(s)
    res = {"bench": a.policy + "_device_eval_s", "agent": POLICIES[a.policy][0], "configs": len(configs),
           "groups": len(ev.groups), "chunk": a.chunk, "reps": a.reps, "load_s": load_s}
    for name, v in times.items():
        res[name + "_s"], res[name + "_s_median"], res[name + "_spread_s"] = v, _med(v), max(v) - min(v)
    res["speedup_sync"] = _med(times["host"]) / _med(times["device_sync"])
    res["host_env_steps"] = int(sum(last["host"]["lengths"]))
    res["device_env_steps"] = int(sum(last["device_sync"]["lengths"]))
    res["device_windows_sync"], res["device_windows_nosync"] = windows["device_sync"], windows["device_nosync"]
    for name in runs:
        if name != "device_nosync":
            res[name + "_success_rate"] = float(np.mean(last[name]["successes"]))
            res[name + "_mean_reward"] = float(np.mean(last[name]["rewards"]))
    print(json.dumps(res), flush=True)
    return res


# ------------------------------------------------------------------ graph
def graph_probe(a, pack):
    """Capture one K-step window in a graph and replay it against the eager call."""
    E, R, O = 60, 5, 4
    K = 5
    b = _batch(E, R, O)
    restore = _restorer(b)
    step = torch.full((1,), STEP0, dtype=torch.int64, device="cuda")

    def call(rec):
        b.policy_rollout(pack, K, b.obs, keep=rec, step_dev=step, eps=EPS, policy_seed=POLICY_SEED, seed=1, counter=10,
                         fast_noise=True)
    eager = _records(b, K)
    call(eager)
    torch.cuda.synchronize()
    final = b.rs.clone()
    restore()
    rec = _records(b, K)
    res = {"bench": a.policy + "_window_graph_capture", "envs": E, "robots": R, "steps": K}
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
    ap.add_argument("--policy", choices=list(POLICIES), required=True)
    ap.add_argument("--shapes", default=None, help="E:R:O of the timed windows, comma-separated")
    ap.add_argument("--steps", default=None, help="the window lengths K, comma-separated")
    ap.add_argument("--calls", "--replays", type=int, default=None, help="timed calls (graph replays) a measurement")
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--launch", default=None, help="layout,block,envs_per_block of the window (default: automatic)")
    ap.add_argument("--chunk", type=int, default=64, help="steps per window of the evaluation")
    ap.add_argument("--episode-limit", type=int, default=1000, help="of the sac evaluation")
    ap.add_argument("--only", choices=["window", "eval", "graph"], default=None)
    ap.add_argument("--out", default=None, help="actor: also write the JSON result to this file")
    ap.add_argument("--out-dir", default=None, help="also write the policy's JSON file(s) into this directory")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    _, sections, *defaults = POLICIES[a.policy]
    for name, dflt in zip(("shapes", "steps", "calls", "warmup", "reps"), defaults):
        if getattr(a, name) is None:
            setattr(a, name, dflt)
    a.launch = tuple(int(v) for v in a.launch.split(",")) if a.launch else None
    if a.only is not None and a.only not in sections:
        ap.error(f"--policy {a.policy} has no {a.only} section")
    agent, pack, eval_pack, act = make_policy(a.policy)
    res = {}

    def write(path, obj):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(obj) + "\n")

    def save():   # after every section: what a timeout leaves behind is complete up to there
        if a.out_dir and a.policy not in ("actor", "dqn"):
            write(os.path.join(a.out_dir, a.policy + "_window_bench.json"), res)
    if a.only in (None, "window"):
        res["window"] = window_bench(a, pack, act)
        save()
        if a.policy == "actor" and a.out:   # the two oldest files hold one result each
            write(a.out, res["window"][-1])
        if a.policy == "dqn" and a.out_dir:
            for r in res["window"]:
                write(os.path.join(a.out_dir, f"dqn_rollout_k{r['steps']}.json"), r)
    if a.only in (None, "eval") and "eval" in sections:
        res["eval"] = (eval_against_host(a, agent, eval_pack) if agent is not None
                       else eval_against_single_launches(a, pack, act))
        save()
    if a.only in (None, "graph") and "graph" in sections:
        res["graph"] = graph_probe(a, pack)
        save()


if __name__ == "__main__":
    main()
