"""Shared by the return-distribution tests (tests/test_*dist*): the numpy restatement of asvrl_eval_dist_stats, which
is the oracle of that kernel, and the launch of the kernel on numpy inputs.

Per robot row n that exists (n % R < n_robots[n // R]) with A = n_act[n], everything in f64:
    G_A = 0, G_t = reward[t][n] + gamma * G_{t+1} for t = A-1 .. 0
    u_t = #{ j : (double) z[t][n][j] <= G_t },  pit[n][u_t] += 1
    pinball[n] += sum_j rho(tau[t][n][j], G_t - z[t][n][j]),  rho(tau, d) = d * (tau - (d < 0 ? 1 : 0))
    mean_t = (1/32) sum_j z[t][n][j],  bias[n] += mean_t - G_t,  pred0[n] = mean_0
    g0[n] = G_0 (0 when A = 0), steps[n] = A
Rows that do not exist keep the pre-fill of every output; rows of G at or behind A keep theirs.

Tolerance of the f64 outputs against this restatement: 1e-12 of the magnitude of what is summed (the project's f64
bar): the kernel sums the 32 samples by a butterfly and numpy pairwise, each sum of at most T * 32 terms of 1.1e-16
relative error."""
import ctypes as C

import numpy as np

S = 32
PREFILL = dict(g0=-7.0, pred0=-7.0, pinball=-7.0, bias=-7.0, steps=-7, pit=-7, G=-7.0)
F64_OUTPUTS = ("G", "g0", "pred0", "pinball", "bias")


def dist_stats_numpy(z, tau, reward, n_act, n_robots, R, gamma, prefill=PREFILL):
    """z, tau [T, NT, 32] f32; reward [T, NT] f64; n_act [NT]; n_robots [E]. Returns the outputs as a dict, with
    "G" [T, NT] and "scale" (per output, the sum of the magnitudes of what it sums: the tolerance's reference)."""
    T, NT, _ = z.shape
    out = dict(G=np.full((T, NT), prefill["G"]), g0=np.full(NT, prefill["g0"]), pred0=np.full(NT, prefill["pred0"]),
               pinball=np.full(NT, prefill["pinball"]), bias=np.full(NT, prefill["bias"]),
               steps=np.full(NT, prefill["steps"], np.int32), pit=np.full((NT, S + 1), prefill["pit"], np.int32))
    scale = {k: np.ones_like(out[k]) for k in F64_OUTPUTS}
    for n in range(NT):
        if n % R >= n_robots[n // R]:
            continue
        A = int(min(max(n_act[n], 0), T))
        G, Gabs = 0.0, 0.0
        for t in range(A - 1, -1, -1):
            G = float(reward[t, n]) + gamma * G
            Gabs = abs(float(reward[t, n])) + gamma * Gabs
            out["G"][t, n] = G
            scale["G"][t, n] = max(Gabs, 1.0)
        out["g0"][n], scale["g0"][n] = G, max(Gabs, 1.0)
        out["steps"][n] = A
        pit = np.zeros(S + 1, np.int32)
        pin = bias = pred0 = 0.0
        pin_abs = bias_abs = pred_abs = 0.0
        for t in range(A):
            zt, tt, Gt = z[t, n].astype(np.float64), tau[t, n].astype(np.float64), out["G"][t, n]
            pit[int((zt <= Gt).sum())] += 1
            d = Gt - zt
            terms = d * (tt - (d < 0))
            pin += float(terms.sum())
            pin_abs += float(np.abs(terms).sum())
            mean = float(zt.sum()) / S
            bias += mean - Gt
            bias_abs += float(np.abs(zt).sum()) / S + abs(Gt)
            if t == 0:
                pred0, pred_abs = mean, float(np.abs(zt).sum()) / S
        out["pit"][n] = pit
        out["pinball"][n], out["bias"][n], out["pred0"][n] = pin, bias, pred0
        scale["pinball"][n], scale["bias"][n], scale["pred0"][n] = max(pin_abs, 1.0), max(bias_abs, 1.0), max(pred_abs, 1.0)
    out["scale"] = scale
    return out


def dist_stats_device(z, tau, reward, n_act, n_robots, R, gamma, block=0, prefill=PREFILL, operands="bf16"):
    """asvrl_eval_dist_stats on the same numpy inputs, the outputs pre-filled as the restatement's. Returns numpy."""
    import torch
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.policy import device_eval
    T, NT, _ = z.shape
    E = NT // R
    dev = "cuda"
    out = device_eval.new_dist_outputs(NT, dev)
    for k, t in out.items():
        t.fill_(prefill[k])
    G = torch.full((T, NT), prefill["G"], dtype=torch.float64, device=dev)
    cu = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt).contiguous()
    device_eval.eval_dist_stats(_abi.lib(operands), T, E, R, cu(z, torch.float32), cu(tau, torch.float32),
                                cu(reward, torch.float64), cu(n_act, torch.int32), cu(n_robots, torch.int32), gamma,
                                out, G, block=block)
    got = {k: t.cpu().numpy() for k, t in out.items()}
    got["G"] = G.cpu().numpy()
    return got


def stats_struct(**over):
    """An AsvEvalDistStats that passes every host check (made-up addresses, never dereferenced: the tests override
    one member into a refusal, so nothing is launched)."""
    from distributional_rl_decision_and_control_amd import _abi
    s = _abi.AsvEvalDistStats()
    s.n_steps, s.n_envs, s.max_robots, s.block, s.gamma = 5, 3, 3, 0, 0.99
    for name in _abi.DIST_STATS_ARRAYS:
        setattr(s, name, 0x1000)
    for k, v in over.items():
        setattr(s, k, v)
    return s


def refused(L, entry, text, *structs):
    rc = getattr(L, entry)(*[None if s is None else C.byref(s) for s in structs], None)
    assert rc != 0, text
    assert L.asvrl_last_error().decode() == text
