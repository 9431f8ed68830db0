#!/usr/bin/env python
"""Wall time of one evaluation of the shipped schedule's 60 'trained' eval configs with the network of
tests/golden/eval60_ref.npz: policy/batched_eval.evaluate_configs (the Python eval envs, one policy call and one
env-step launch per step) against policy/device_eval.DeviceEvaluator.run (device-resident configs, closed-loop
windows, asvrl_eval_metrics behind each), in one process.

After one warm-up of each, --reps alternating repetitions: a host clock around each evaluation, ending in a device
synchronise. The device path is timed with its per-window host wait (sync=True, stops when every episode has ended)
and without (sync=False, every window enqueued). The metrics kernel is also timed alone (device events around
--kernel-launches launches on one window's records of the whole batch), beside one closed-loop window. The device
run's success rate and mean reward are printed next to the golden's for the record only: the perception noise is
another stream, so nothing is asserted on them. One process, no retries; run it under a timeout:

    timeout 600 python tools/bench_device_eval.py [--out profiles/device_eval.json]

--agent DQN: the same procedure with a seeded Agent(agent_type="DQN") (no trained DQN network is shipped) and its
DqnPack in the closed-loop windows; the default output is profiles/device_eval_dqn.json (its golden_* fields stay
the trained AC-IQN network's, for the record only).

--histories: no host evaluation; the device evaluation without histories, with them as packed arrays
(run(histories=True)) and with device_eval.history_lists on top, alternating; then the asvrl_eval_history_pack launch
alone with its achieved bytes per second, against the same packing by torch (permute and boolean mask), whose outputs
are first compared with the kernel's byte for byte. The default output is profiles/eval_histories.json.

--distribution (--agent AC-IQN or IQN; IQN is a seeded network, none is shipped): no host evaluation; the device
evaluation without it, with histories=True and with distribution= (the AC-IQN critic's CriticPack, or True for the
IqnPack), alternating; then the post-pass alone on the last run's records -- the readout launches and
asvrl_eval_dist_stats -- between device events, with the bytes they move. The result is added to
profiles/eval_distribution.json under the agent's name (--label), one entry per process. The parent commit's seconds
belong in the same file from the same session: --plain times the evaluation with no option only, and with
--package-root <a built checkout of the parent> it runs the parent's package (--label "AC-IQN parent"); --plain
without it gives this commit's repeated plain runs as a separate process, for the run-to-run spread.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCHEDULE = {"num_episodes": [10] * 6, "num_robots": [3, 4, 5, 5, 5, 5], "num_cores": [0] * 6,
            "num_obstacles": [0, 0, 0, 2, 3, 4], "min_start_goal_dis": [30.0, 35.0, 40.0, 40.0, 40.0, 40.0]}


HBM_BYTES_PER_S = 8.0e12   # MI355X HBM3E peak, for the pack launch's share


def torch_pack(grp, H, actions, counts, steps):
    """The packing of asvrl_eval_history_pack by the obvious torch route: put the row in front of step 0 on top of
    the records' first `steps` rows, permute to robot-major and select with a boolean mask of the counts."""
    from distributional_rl_decision_and_control_amd import _abi
    k = torch.arange(steps + 1, device=counts.device)[None, :]
    n_traj, n_act, n_obs = (counts[q].long()[:, None] for q in range(3))
    fields = torch.tensor(_abi.TRAJ_FIELDS, device=counts.device)
    rs = torch.cat([grp.initial["rs"][None], H["rs"][:steps]])[:, fields]             # [steps + 1, 13, NT]
    obs = torch.cat([H["obs0"][None], H["obs"][:steps]])[:, :, :_abi.HISTORY_OBS_DIM]   # [steps + 1, NT, 32]
    cnt = torch.cat([H["cnt0"][None], H["obj_cnt"][:steps]])
    return dict(traj=rs.permute(2, 0, 1)[k < n_traj], act=actions[:steps].permute(1, 0, 2)[k[:, :steps] < n_act],
                obs=obs.permute(1, 0, 2)[k < n_obs], cnt=cnt.permute(1, 0)[k < n_obs])


def histories(a, ev, pack, clock, z):
    """--histories: the per-evaluation time without histories, with them as packed arrays and with history_lists on
    top (alternating, after a warm-up round of each); then the pack launch alone on the last run's records (device
    events around --kernel-launches launches, and a host clock around one launch and a synchronise) against
    torch_pack on the same records (a host clock: its mask selection waits for the device itself), compared byte
    for byte first."""
    from distributional_rl_decision_and_control_amd.policy import device_eval as de
    runs = {"off": lambda: ev.run(pack, seed=1),
            "arrays": lambda: ev.run(pack, seed=1, histories=True),
            "lists": lambda: de.history_lists(ev.run(pack, seed=1, histories=True))}
    times = {k: [] for k in runs}
    last = {}
    for rep in range(a.reps + 1):   # the first round is the warm-up (it also allocates the episode-long records)
        for name, fn in runs.items():
            s, last[name] = clock(fn)
            if rep > 0:
                times[name].append(s)
    assert len(ev.groups) == 1 and not any(last["off"][n][0][0] for n in ("observations", "actions", "trajectories"))
    assert all(last["off"][n] == last["arrays"][n] for n in ("lengths", "successes", "rewards", "times", "energies")), \
        "histories changed the metrics"
    h = last["arrays"]["history"]
    grp = ev.groups[0]
    b = grp.batch
    T = 1001
    H = grp.history(T)
    counts, offsets = H["counts"], H["offsets"]
    totals = [int(v) for v in counts.sum(dim=1).cpu()]
    assert totals == [len(h.traj), len(h.act), len(h.obs)]
    out = dict(traj=torch.empty((totals[0], 13), dtype=torch.float64, device="cuda"),
               act=torch.empty((totals[1], 2), dtype=torch.float64, device="cuda"),
               obs=torch.empty((totals[2], 32), dtype=torch.float32, device="cuda"),
               cnt=torch.empty(totals[2], dtype=torch.int8, device="cuda"))
    src = dict(rs0=grp.initial["rs"], rs=H["rs"], actions=H["actions"], obs0=H["obs0"], obs=H["obs"], cnt0=H["cnt0"],
               obj_cnt=H["obj_cnt"])

    def launch():
        de.history_pack(pack.L, T, b.n_envs, b.max_robots, counts, offsets, src, out)
    steps = max(last["arrays"]["lengths"])
    ref = torch_pack(grp, H, H["actions"], counts, steps)
    launch()
    torch.cuda.synchronize()
    for n in out:
        assert torch.equal(out[n], ref[n]), f"torch route and kernel differ in {n}"
        assert out[n].cpu().numpy().tobytes() == getattr(h, n).tobytes(), n
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.kernel_launches):
        launch()
    e1.record()
    torch.cuda.synchronize()
    pack_us = 1e3 * e0.elapsed_time(e1) / a.kernel_launches
    pack_host, torch_host = [], []
    for _ in range(max(a.reps, 5)):
        pack_host.append(1e6 * clock(launch)[0])
        torch_host.append(1e6 * clock(lambda: torch_pack(grp, H, H["actions"], counts, steps))[0])
    payload = totals[0] * 13 * 8 + totals[1] * 16 + totals[2] * (32 * 4 + 1)   # bytes read = bytes written
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res = {"agent": a.agent, "configs": len(ev.envs), "chunk": a.chunk, "reps": a.reps, "robot_rows": b.n_envs * b.max_robots,
           "record_steps": T, "record_bytes": de.HISTORY_BYTES * T * b.n_envs * b.max_robots,
           "env_steps": int(sum(last["arrays"]["lengths"])), "longest_episode": steps,
           "history_rows": dict(zip(("traj", "act", "obs"), totals)),
           "off_s": times["off"], "arrays_s": times["arrays"], "lists_s": times["lists"],
           "off_s_median": med(times["off"]), "arrays_s_median": med(times["arrays"]),
           "lists_s_median": med(times["lists"]),
           "off_spread_s": max(times["off"]) - min(times["off"]),
           "arrays_spread_s": max(times["arrays"]) - min(times["arrays"]),
           "lists_spread_s": max(times["lists"]) - min(times["lists"]),
           "pack_launches": a.kernel_launches, "pack_us": pack_us, "pack_payload_bytes": 2 * payload,
           "pack_bytes_per_s": 2 * payload / (pack_us * 1e-6),
           "pack_share_of_hbm_peak": 2 * payload / (pack_us * 1e-6) / HBM_BYTES_PER_S,
           "pack_host_us": pack_host, "pack_host_us_median": med(pack_host),
           "torch_route_host_us": torch_host, "torch_route_host_us_median": med(torch_host),
           "golden_success_rate": float(np.mean(z["trained/successes"])),
           "device_success_rate": float(np.mean(last["arrays"]["successes"]))}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def distribution(a, ev, pack, source, clock):
    """--distribution: the per-evaluation time without it, with histories=True and with distribution=source
    (alternating, after a warm-up round of each); then, on the last run's records, the readout launches
    (asvrl_iqn_dist, or asvrl_dist_prepare + asvrl_critic_forward) and the two launches of asvrl_eval_dist_stats, each
    between device events over --kernel-launches repetitions, with the bytes they move."""
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.policy import device_eval as de
    runs = {"off": lambda: ev.run(pack, seed=1),
            "histories": lambda: ev.run(pack, seed=1, histories=True),
            "distribution": lambda: ev.run(pack, seed=1, distribution=source)}
    times = {k: [] for k in runs}
    last = {}
    for rep in range(a.reps + 1):   # the first round is the warm-up (it also allocates the records and the planes)
        for name, fn in runs.items():
            sec, last[name] = clock(fn)
            if rep > 0:
                times[name].append(sec)
    assert len(ev.groups) == 1
    assert all(last["off"][n] == last["distribution"][n] for n in ("lengths", "successes", "rewards", "times",
                                                                   "energies")), "distribution changed the metrics"
    d = last["distribution"]["distribution"]
    grp = ev.groups[0]
    b, T = grp.batch, 1001
    NT = b.n_envs * b.max_robots
    H, D = grp.history(T), grp.distribution(T, d.kind)
    hist = dict(L=pack.L, T=T, records=[H])
    dist = dict(kind=d.kind, pack=pack if d.kind == "iqn" else source, seed=0, cvar=1.0)
    steps = ev.steps
    acted = int(sum(int(x.sum()) for x in d.steps))

    def stats():
        de.eval_dist_stats(pack.L, T, b.n_envs, b.max_robots, D["z"], D["tau"], H["reward"], H["counts"][1],
                           b.n_robots, ev.gamma, D["out"], D["G"])

    def whole():   # the readout launches and the stats launches, as run() enqueues them
        ev._distribution_pass(0, hist, dist)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = {}
    for name, fn in (("stats", stats), ("pass", whole)):
        fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.kernel_launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us[name] = 1e3 * e0.elapsed_time(e1) / a.kernel_launches
    rows = steps * NT   # the readout covers every slot of the steps that ran
    readout_bytes = rows * (4 * _abi.OBS_DIM + 16 + 2 * 4 * _abi.DIST_SAMPLES + (4 if d.kind == "iqn" else 8 + 4 * 32))
    stats_bytes = acted * (2 * 4 * _abi.DIST_SAMPLES + 8 + 2 * 8) + NT * (4 * 8 + 4 * 34)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    summ = d.summary()["overall"]
    res = {"agent": a.agent, "kind": d.kind, "configs": len(ev.envs), "chunk": a.chunk, "reps": a.reps,
           "robot_rows": NT, "steps_run": steps, "acted_robot_steps": acted,
           "plane_bytes": T * NT * (2 * 4 * _abi.DIST_SAMPLES + 8),
           "off_s": times["off"], "histories_s": times["histories"], "distribution_s": times["distribution"],
           "off_s_median": med(times["off"]), "histories_s_median": med(times["histories"]),
           "distribution_s_median": med(times["distribution"]),
           "off_spread_s": max(times["off"]) - min(times["off"]),
           "launches": a.kernel_launches, "stats_us": us["stats"], "readout_us": us["pass"] - us["stats"],
           "pass_us": us["pass"], "readout_bytes": readout_bytes, "stats_bytes": stats_bytes,
           "mismatches": d.mismatches, "pinball_per_sample": summ["pinball"], "mean_bias": summ["bias"],
           "pred0_minus_g0": summ["pred0_minus_g0"], "terminated_robots": summ["robots"]}
    print(json.dumps(res))
    merge_out(a.out, a.label or a.agent, res)


def merge_out(path, label, res):
    """profiles/eval_distribution.json is one object of results by label ("AC-IQN", "IQN", "AC-IQN parent", ...):
    the runs of one session are separate processes, and each adds its own entry."""
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc[label] = {k: (None if isinstance(v, float) and not math.isfinite(v) else v) for k, v in res.items()}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def plain(a, ev, pack, clock):
    """--plain: the evaluation with no option, a warm-up and --reps repetitions; with --package-root it runs the
    package of another checkout (the parent commit's, built), which is how the parent's seconds get into the same
    file in the same session (--label "AC-IQN parent")."""
    times = []
    for rep in range(a.reps + 1):
        sec, last = clock(lambda: ev.run(pack, seed=1))
        if rep > 0:
            times.append(sec)
    res = {"agent": a.agent, "package": "another checkout (--package-root)" if a.package_root else "this checkout", "reps": a.reps, "chunk": a.chunk,
           "off_s": times, "off_s_median": sorted(times)[len(times) // 2], "off_spread_s": max(times) - min(times),
           "env_steps": int(sum(last["lengths"]))}
    print(json.dumps(res))
    merge_out(a.out, a.label or a.agent + " plain", res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--kernel-launches", type=int, default=200)
    ap.add_argument("--agent", default="AC-IQN", choices=("AC-IQN", "DQN", "IQN"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--histories", action="store_true",
                    help="time the device evaluation without histories, with them as arrays and with history_lists, "
                         "the pack launch alone and the same packing by torch (no host evaluation)")
    ap.add_argument("--distribution", action="store_true",
                    help="time the device evaluation without, with histories and with the return distributions "
                         "(AC-IQN: the critic's; IQN: its own), and the readout and stats launches alone")
    ap.add_argument("--plain", action="store_true",
                    help="time the evaluation with no option only and add it to profiles/eval_distribution.json")
    ap.add_argument("--package-root", default=None,
                    help="with --plain: import the package from this checkout (the parent commit's, built) instead")
    ap.add_argument("--label", default=None, help="the entry's key in profiles/eval_distribution.json")
    a = ap.parse_args()
    if a.agent == "IQN" and not (a.distribution or a.plain):
        ap.error("--agent IQN goes with --distribution or --plain")
    if a.package_root:
        if not a.plain:
            ap.error("--package-root goes with --plain")
        sys.path.insert(0, os.path.abspath(a.package_root))
    if a.out is None and (a.distribution or a.plain):
        a.out = os.path.join(ROOT, "profiles", "eval_distribution.json")
    if a.out is None:
        name = "eval_histories.json" if a.histories else ("device_eval_dqn.json" if a.agent == "DQN"
                                                          else "device_eval.json")
        a.out = os.path.join(ROOT, "profiles", name)
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.envs.marinenav.env import MarineNavEnv3
    from distributional_rl_decision_and_control_amd.fused_dqn import DqnPack
    from distributional_rl_decision_and_control_amd.fused_mlp import MlpPack
    from distributional_rl_decision_and_control_amd.policy.batched_eval import evaluate_configs
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator, eval_metrics
    from distributional_rl_decision_and_control_amd.policy.trainer import Trainer

    z = np.load(os.path.join(ROOT, "tests", "golden", "eval60_ref.npz"))
    configs = json.loads(str(z["trained/configs"]))
    torch.manual_seed(0)
    agent = Agent(seed=100, agent_type=a.agent)
    if a.agent == "AC-IQN":
        agent.policy_local.actor.load_state_dict({k[len("trained/net/"):]: torch.from_numpy(z[k]) for k in z.files
                                                  if k.startswith("trained/net/")})
    tr = Trainer(MarineNavEnv3(seed=1), MarineNavEnv3(seed=253, is_eval_env=True), SCHEDULE, agent)
    if a.agent == "IQN":
        from distributional_rl_decision_and_control_amd.fused_iqn import IqnPack
        pack = IqnPack(agent.policy_local)
    else:
        pack = DqnPack(agent.policy_local) if a.agent == "DQN" else MlpPack(agent.policy_local.actor, "actor")

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    load_s, ev = clock(lambda: DeviceEvaluator(configs, template_env=tr.eval_env, chunk=a.chunk, gamma=agent.GAMMA))
    if a.histories:
        return histories(a, ev, pack, clock, z)
    if a.plain:
        return plain(a, ev, pack, clock)
    if a.distribution:
        if a.agent == "DQN":
            ap.error("--distribution reads IQN's or the AC-IQN critic's quantiles")
        from distributional_rl_decision_and_control_amd.fused_critic import CriticPack
        return distribution(a, ev, pack, True if a.agent == "IQN" else CriticPack(agent.policy_local.critic), clock)
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

    # the metrics kernel alone, and one closed-loop window, on the whole batch from the initial state
    grp = ev.groups[0]
    b, K = grp.batch, a.chunk
    rec = grp.records(K)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window():
        b.policy_rollout(pack, K, b.obs, keep=rec, hold_done=True, trainer_deactivate=True, step_dev=grp.step,
                         env_mask=grp.state["alive"], seed=1, counter=0, fast_noise=True)
    win_us = []
    for i in range(6):
        ev.observe(seed=1)
        e0.record()
        window()
        e1.record()
        torch.cuda.synchronize()
        if i > 0:
            win_us.append(1e3 * e0.elapsed_time(e1))
    args = (pack.L, K, b.n_envs, b.max_robots, rec, b.n_robots, grp.dt, grp.N, grp.pc)

    def rewind():   # every env and robot running again: each launch walks the window as the first one did
        grp.state["ended"].zero_()
        grp.state["deact"].zero_()
        grp.state["length"].zero_()
    rewind()
    eval_metrics(*args, grp.state, agent.GAMMA, 1000)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.kernel_launches):
        rewind()
        eval_metrics(*args, grp.state, agent.GAMMA, 1000)
    e1.record()
    torch.cuda.synchronize()
    with_zero = 1e3 * e0.elapsed_time(e1) / a.kernel_launches
    e0.record()
    for _ in range(a.kernel_launches):
        rewind()
    e1.record()
    torch.cuda.synchronize()
    zero_us = 1e3 * e0.elapsed_time(e1) / a.kernel_launches

    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    dev = last["device_sync"]
    res = {
        "agent": a.agent, "configs": len(configs), "chunk": K, "reps": a.reps, "groups": len(ev.groups),
        "per_robot_params": b.robot_params is not None, "load_s": load_s,
        "host_s": times["host"], "device_sync_s": times["device_sync"], "device_nosync_s": times["device_nosync"],
        "host_s_median": med(times["host"]), "device_sync_s_median": med(times["device_sync"]),
        "device_nosync_s_median": med(times["device_nosync"]),
        "host_spread_s": max(times["host"]) - min(times["host"]),
        "device_sync_spread_s": max(times["device_sync"]) - min(times["device_sync"]),
        "device_nosync_spread_s": max(times["device_nosync"]) - min(times["device_nosync"]),
        "speedup_sync": med(times["host"]) / med(times["device_sync"]),
        "host_env_steps": int(sum(last["host"]["lengths"])), "device_env_steps": int(sum(dev["lengths"])),
        "device_windows_sync": windows["device_sync"], "device_windows_nosync": windows["device_nosync"],
        "window_us": win_us, "window_us_median": med(win_us),
        "metrics_kernel_us": with_zero - zero_us, "metrics_kernel_with_fill_us": with_zero, "fill_us": zero_us,
        "device_success_rate": float(np.mean(dev["successes"])), "device_mean_reward": float(np.mean(dev["rewards"])),
        "host_success_rate": float(np.mean(last["host"]["successes"])),
        "host_mean_reward": float(np.mean(last["host"]["rewards"])),
        "golden_success_rate": float(np.mean(z["trained/successes"])),
        "golden_mean_reward": float(np.mean(z["trained/rewards"])),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
