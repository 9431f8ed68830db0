"""The batch cases tests/test_noise_streams_cpu.py and tests/test_noise_streams_gpu.py share, and their numpy
reference: a loop in MarineNavEnv3._pack's order over one Perception(seed) object per robot row.

Case "mixed": 7 envs x 5 robot slots x 4 obstacle slots, 12 steps; n_robots 1, 3 and 5, n_obs 0, 2 and 4; every robot
its own pos_std / vel_std / r_kappa (the per-robot table; kappa 0.3 to 4, and one each of 0, 3e-7 and 50: numpy's three
branches); env 4 masked
out in every step; robot 1 of env 2 deactivated from step 3 on; env 5 with all but robot 2 deactivated from step 6 on.
Case "crowd": one env of 17 robots with no obstacle slot in use (max_obs 0), 3 steps, one robot deactivated from
step 1 on, one shared parameter set.
"""
import numpy as np

FLAG_DEACTIVATED = 1


class Case:
    def __init__(self, name, E, R, O, steps, n_robots, n_obs, seeds, sigma, deact, mask):
        self.name, self.E, self.R, self.O, self.steps = name, E, R, O, steps
        self.n_robots = np.asarray(n_robots, np.int32)
        self.n_obs = np.asarray(n_obs, np.int32)
        self.seeds = list(seeds)     # [E * R]
        self.sigma = sigma           # [E * R][3] (pos_std, vel_std, r_kappa), or one triple for every robot
        self.deact = deact           # step -> u8 [E * R] flags
        self.mask = mask             # u8 [E] or None

    def per_robot(self):
        return np.ndim(self.sigma) == 2

    def triple(self, row):
        return self.sigma[row] if self.per_robot() else self.sigma


def mixed():
    E, R, O, steps = 7, 5, 4, 12
    n_robots = [1, 3, 5, 5, 4, 5, 3]
    n_obs = [0, 2, 4, 4, 3, 2, 0]
    rd = np.random.RandomState(5)
    seeds = [int(s) for s in rd.randint(0, 25, E * R)]
    sigma = np.stack([rd.uniform(0.01, 0.1, E * R), rd.uniform(0.01, 0.1, E * R), rd.uniform(0.3, 4.0, E * R)], 1)
    sigma[2 * R + 0, 2] = 0.0    # kappa < 1e-8: the uniform branch
    sigma[3 * R + 1, 2] = 3e-7   # kappa < 1e-5: numpy's second-order envelope
    sigma[3 * R + 2, 2] = 50.0   # a narrow one
    mask = np.ones(E, np.uint8)
    mask[4] = 0

    def deact(t):
        fl = np.zeros(E * R, np.uint8)
        fl[3 * R + 4] = 2   # a flag that is not the deactivation bit: draws go on
        if t >= 3:
            fl[2 * R + 1] = FLAG_DEACTIVATED | 4
        if t >= 6:
            for i in (0, 1, 3, 4):
                fl[5 * R + i] = FLAG_DEACTIVATED | 2
        return fl
    return Case("mixed", E, R, O, steps, n_robots, n_obs, seeds, sigma, deact, mask)


def crowd():
    R = 17

    def deact(t):
        fl = np.zeros(R, np.uint8)
        if t >= 1:
            fl[9] = FLAG_DEACTIVATED
        return fl
    return Case("crowd", 1, R, 0, 3, [R], [0], range(100, 100 + R), (0.05, 0.05, 1.0), deact, None)


CASES = {"mixed": mixed, "crowd": crowd}


def reference(case):
    """Per step the rows [E * R, O + R, 5]; then the counters (n, sum, sq) and the final Perception objects."""
    from distributional_rl_decision_and_control_amd.envs.marinenav.vehicles.wamv import Perception
    E, R, O = case.E, case.R, case.O
    per = []
    for row, seed in enumerate(case.seeds):
        p = Perception(seed)
        p.pos_std, p.vel_std, p.r_kappa = (float(v) for v in case.triple(row))
        per.append(p)
    n = np.zeros(E * R, np.int64)
    s = np.zeros(E * R)
    q = np.zeros(E * R)
    rows = []

    def draw(row):
        v = per[row].draw_candidate_noise()
        for x in v:
            n[row] += 1
            s[row] += x
            q[row] += x * x
        return v

    for t in range(case.steps):
        fl = case.deact(t)
        out = np.zeros((E * R, O + R, 5))
        for e in range(E):
            if case.mask is not None and not case.mask[e]:
                continue
            for i in range(case.n_robots[e]):
                row = e * R + i
                if fl[row] & FLAG_DEACTIVATED:
                    continue
                for k in range(case.n_obs[e]):
                    out[row, k] = draw(row)
                for j in range(case.n_robots[e]):
                    if j == i or fl[e * R + j] & FLAG_DEACTIVATED:
                        continue
                    out[row, O + j] = draw(row)
        rows.append(out)
    return rows, (n, s, q), per


def never_draws(case):
    """Rows whose stream must stay at its initial state through every step: masked envs, padding rows."""
    rows = []
    for e in range(case.E):
        for i in range(case.R):
            if i >= case.n_robots[e] or (case.mask is not None and not case.mask[e]):
                rows.append(e * case.R + i)
    return rows


def run(case, device):
    """The case through NoiseStreams.fill_raw on `device` ("cpu": the host twin). Returns (rows per step, the
    NoiseStreams)."""
    import torch

    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.noise_streams import NoiseStreams
    E, R, O = case.E, case.R, case.O
    ns = NoiseStreams(case.seeds, device=device)
    params = _abi.params_from()
    table = None
    if case.per_robot():
        arr = (_abi.AsvParams * (E * R))()
        for row in range(E * R):
            arr[row] = _abi.params_from()
            arr[row].pos_std, arr[row].vel_std, arr[row].r_kappa = (float(v) for v in case.sigma[row])
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
        params.pos_std = params.vel_std = params.r_kappa = 123.0   # must not be read
    else:
        params.pos_std, params.vel_std, params.r_kappa = (float(v) for v in case.sigma)
    n_robots = torch.from_numpy(case.n_robots).to(device)
    n_obs = torch.from_numpy(case.n_obs).to(device)
    mask = torch.from_numpy(case.mask).to(device) if case.mask is not None else None
    rows = []
    for t in range(case.steps):
        fl = torch.from_numpy(case.deact(t)).to(device)
        out = torch.full((E * R, O + R, 5), 7.0, dtype=torch.float64, device=device)   # the padding must be written
        ns.fill_raw(params, E, R, O, n_robots, n_obs, fl, env_mask=mask, robot_params=table, out=out)
        rows.append(out.cpu().numpy())
    return rows, ns
