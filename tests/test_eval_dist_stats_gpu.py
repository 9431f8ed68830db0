"""GPU: asvrl_eval_dist_stats against its numpy restatement (tests/dist_cases.py).

T = 5 steps, E = 3 envs of R = 3 slots (NT = 9) with n_robots = [3, 1, 2], so slots 4, 5 and 8 are absent; the act
counts of the robots that exist are 5 (= T), 0, 1, 3, 2, 4. The rewards are random multiples of 1/8 in [-4, 4] and
gamma is 0.5, so every return-to-go is a multiple of 2^-7 below 8 in magnitude: exact in f64 and representable in
f32. Samples are then planted ON the return (z == G exactly, which must count as <=), one ulp above and one below.
pit and steps are exact; the f64 outputs are within 1e-12 of the magnitude of what they sum. Absent slots keep their
pre-fill. Two runs, and every block size, give the same bits; so does an E = 70 case over several blocks."""
import numpy as np
import pytest

import dist_cases

pytestmark = pytest.mark.gpu

T, E, R, S = 5, 3, 3, dist_cases.S
N_ROBOTS = np.array([3, 1, 2], np.int32)
N_ACT = np.array([5, 0, 1, 3, 9, 9, 2, 4, 9], np.int32)   # 9: an absent slot's stale count, never read
GAMMA = 0.5


def _case(E=E, n_robots=N_ROBOTS, n_act=N_ACT, seed=3):
    rng = np.random.RandomState(seed)
    NT = E * R
    reward = rng.randint(-32, 33, size=(T, NT)) / 8.0
    tau = rng.rand(T, NT, S).astype(np.float32)
    G = np.zeros((T + 1, NT))
    for t in range(T - 1, -1, -1):
        G[t] = reward[t] + GAMMA * G[t + 1] * (t + 1 < n_act)
    assert (G.astype(np.float32).astype(np.float64) == G).all(), "the returns are f32 values"
    z = (G[:T, :, None] + rng.randn(T, NT, S) * 2.0).astype(np.float32)
    g32 = G[:T].astype(np.float32)
    z[:, :, 3] = g32                                   # ties: equal to the return, counted as <=
    z[:, :, 17] = g32
    z[:, :, 5] = np.nextafter(g32, np.float32(np.inf))    # one ulp above: not counted
    z[:, :, 6] = np.nextafter(g32, np.float32(-np.inf))   # one ulp below: counted
    z[1, :, :] = g32[1][:, None]                       # a step whose 32 samples all tie: bin 32
    return z, tau, reward, n_act, n_robots


def _check(got, ref, n_robots, n_act):
    NT = len(n_act)
    exists = np.array([n % R < n_robots[n // R] for n in range(NT)])
    assert np.array_equal(got["pit"], ref["pit"]) and np.array_equal(got["steps"], ref["steps"])
    assert (got["pit"][exists].sum(axis=1) == got["steps"][exists]).all()
    for name in dist_cases.F64_OUTPUTS:
        err = np.abs(got[name] - ref[name]) / ref["scale"][name]
        print(f"{name}: max error / magnitude {err.max():.2e}")
        assert (err <= 1e-12).all(), name
    for name in ("g0", "pred0", "pinball", "bias", "steps", "pit"):   # absent slots: the pre-fill, untouched
        assert (got[name][~exists] == dist_cases.PREFILL[name]).all(), name
    assert (got["G"][:, ~exists] == dist_cases.PREFILL["G"]).all()
    for n in np.nonzero(exists)[0]:   # rows of G at or behind the act count are not written
        assert (got["G"][min(n_act[n], T):, n] == dist_cases.PREFILL["G"]).all()


def _same_bits(a, b, what):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def test_against_the_numpy_restatement():
    z, tau, reward, n_act, n_robots = _case()
    ref = dist_cases.dist_stats_numpy(z, tau, reward, n_act, n_robots, R, GAMMA)
    got = dist_cases.dist_stats_device(z, tau, reward, n_act, n_robots, R, GAMMA)
    _check(got, ref, n_robots, n_act)
    # the planted ties were counted: robot 0's step 1 has all 32 samples on the return
    assert got["pit"][0][32] >= 1
    assert got["steps"].tolist()[:4] == [5, 0, 1, 3] and got["g0"][1] == 0.0 and got["pit"][1].sum() == 0
    _same_bits(got, dist_cases.dist_stats_device(z, tau, reward, n_act, n_robots, R, GAMMA), "second run")
    for block in (64, 128, 512, 1024):
        _same_bits(got, dist_cases.dist_stats_device(z, tau, reward, n_act, n_robots, R, GAMMA, block=block),
                   f"block {block}")
    _same_bits(got, dist_cases.dist_stats_device(z, tau, reward, n_act, n_robots, R, GAMMA, operands="f32"),
               "the f32-operand build")


def test_many_envs_over_several_blocks():
    rng = np.random.RandomState(11)
    E2 = 70
    n_robots = rng.randint(0, R + 1, size=E2).astype(np.int32)
    n_act = rng.randint(0, T + 1, size=E2 * R).astype(np.int32)
    z, tau, reward, n_act, n_robots = _case(E2, n_robots, n_act, seed=12)
    ref = dist_cases.dist_stats_numpy(z, tau, reward, n_act, n_robots, R, GAMMA)
    got = dist_cases.dist_stats_device(z, tau, reward, n_act, n_robots, R, GAMMA, block=64)
    _check(got, ref, n_robots, n_act)
    _same_bits(got, dist_cases.dist_stats_device(z, tau, reward, n_act, n_robots, R, GAMMA, block=256), "block 256")


def test_counts_outside_the_records_are_clamped():
    """n_act above T or below 0 (device data) reads nothing outside the planes: clamped to 0..T."""
    z, tau, reward, n_act, n_robots = _case()
    wild = n_act.copy()
    wild[0], wild[2] = 1000, -5
    clamped = n_act.copy()
    clamped[0], clamped[2] = T, 0
    _same_bits(dist_cases.dist_stats_device(z, tau, reward, wild, n_robots, R, GAMMA),
               dist_cases.dist_stats_device(z, tau, reward, clamped, n_robots, R, GAMMA), "clamped")
