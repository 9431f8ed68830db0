"""CPU: the reference's perception-noise streams (csrc/asvrl_rs_stream.h) through asvrl_noise_streams_host, the
host twin of the device kernel, against numpy itself.

  * draw for draw: seeds 0-24 and 2**31 - 1, 2,000 candidates each (about 34,000 MT19937 words: 54 regenerations),
    every value assert_array_equal to Perception.draw_candidate_noise on a RandomState of the same seed, and the
    final key / pos / has_gauss / gauss equal to get_state();
  * batch form (tests/noise_stream_cases.py): rows, zero padding and counters against a numpy loop in _pack's order,
    bit for bit; masked, deactivated and padding robots keep their streams;
  * the ABI: struct size and exports in both libraries, null-pointer and shape refusals;
  * the Python-level ValueErrors that can be reached without a GPU.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import noise_stream_cases as cases

SEEDS = list(range(25)) + [2 ** 31 - 1]
CANDIDATES = 2000


def _same_state(ns, row, rd):
    _, key, pos, has_gauss, gauss = rd.get_state()
    mine = ns.state(row)
    np.testing.assert_array_equal(mine[1], key)
    assert mine[2:] == (pos, has_gauss, gauss)


def test_host_twin_equals_numpy_draw_for_draw():
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.envs.marinenav.vehicles.wamv import Perception
    from distributional_rl_decision_and_control_amd.noise_streams import NoiseStreams
    E, O, calls = len(SEEDS), 50, CANDIDATES // 50   # one robot per env, 50 obstacles: 50 candidates per call
    ns = NoiseStreams(SEEDS, device="cpu")
    p = _abi.params_from()
    n_robots = torch.ones(E, dtype=torch.int32)
    n_obs = torch.full((E,), O, dtype=torch.int32)
    flags = torch.zeros(E, dtype=torch.uint8)
    got = np.concatenate([ns.fill_raw(p, E, 1, O, n_robots, n_obs, flags).numpy()[:, :O].copy() for _ in range(calls)], 1)
    n, s, q = ns.counters()
    for row, seed in enumerate(SEEDS):
        per = Perception(seed)
        ref = np.array([per.draw_candidate_noise() for _ in range(CANDIDATES)])
        np.testing.assert_array_equal(got[row], ref, err_msg=f"seed {seed}")
        _same_state(ns, row, per.rd)
        assert n[row] == 5 * CANDIDATES
        flat = ref.reshape(-1)
        acc = acc2 = 0.0
        for x in flat:
            acc += x
            acc2 += x * x
        assert s[row] == acc and q[row] == acc2
    # at least 50 regenerations per stream: a candidate takes 8 doubles at the least, 16 words
    assert CANDIDATES * 16 >= 50 * 624


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_batch_form_on_the_host(name):
    from distributional_rl_decision_and_control_amd.noise_streams import initial_state
    case = cases.CASES[name]()
    ref_rows, (n, s, q), per = cases.reference(case)
    rows, ns = cases.run(case, "cpu")
    for t in range(case.steps):
        np.testing.assert_array_equal(rows[t], ref_rows[t], err_msg=f"{name} step {t}")
    gn, gs, gq = ns.counters()
    np.testing.assert_array_equal(gn, n)
    np.testing.assert_array_equal(gs, s)
    np.testing.assert_array_equal(gq, q)
    for row in range(case.E * case.R):
        _same_state(ns, row, per[row].rd)
    quiet = cases.never_draws(case)
    assert quiet if name == "mixed" else not quiet
    for row in quiet:   # untouched bit for bit: still the state the seed gives
        key, pos, has_gauss, gauss = initial_state(case.seeds[row])
        mine = ns.state(row)
        np.testing.assert_array_equal(mine[1], key)
        assert mine[2:] == (pos, has_gauss, gauss) and gn[row] == 0
    # the cases cover what they were built for
    assert (n > 0).any() and any((r != 0).any() for r in ref_rows)
    if name == "mixed":
        R = case.R
        assert n[2 * R + 1] == 5 * 3 * (4 + 4) and n[2 * R + 0] == 5 * (3 * 8 + 9 * 7), "a robot leaves at step 3"
        assert n[5 * R + 2] == 5 * (6 * (2 + 4) + 6 * 2), "alone with its obstacles from step 6 on"
        assert (ref_rows[0][4 * R:5 * R] == 0).all(), "the masked env's rows are zero"


def test_abi_struct_exports_and_refusals():
    from distributional_rl_decision_and_control_amd import _abi
    assert C.sizeof(_abi.AsvNoiseStreams) == 16 + 13 * 8
    names = {e[0] for e in _abi.EXPORTS}
    assert {"asvrl_noise_streams", "asvrl_noise_streams_host", "asvrl_noise_streams_struct_size"} <= names
    p = _abi.params_from()
    for ops in ("bf16", "f32"):
        L = _abi.lib(ops)
        assert L.asvrl_noise_streams_struct_size() == C.sizeof(_abi.AsvNoiseStreams)
        assert L.asvrl_abi_version() == _abi.ABI_VERSION
        key = np.zeros((2, 624), np.uint32)
        i32 = np.zeros(2, np.int32)
        f64 = np.zeros(2)
        out = np.zeros((2, 3, 5))
        i64 = np.zeros(2, np.int64)
        fl = np.zeros(2, np.uint8)

        def good():
            s = _abi.AsvNoiseStreams()
            s.n_envs, s.max_robots, s.max_obs = 1, 2, 1
            s.n_robots, s.n_obs, s.rflags = i32.ctypes.data, i32.ctypes.data, fl.ctypes.data
            s.key, s.pos, s.has_gauss, s.gauss = key.ctypes.data, i32.ctypes.data, i32.ctypes.data, f64.ctypes.data
            s.noise_out = out.ctypes.data
            return s

        for fn in (L.asvrl_noise_streams_host, L.asvrl_noise_streams):   # the refusals come before any launch
            who = b"asvrl_noise_streams_host" if fn is L.asvrl_noise_streams_host else b"asvrl_noise_streams:"
            assert fn(C.byref(p), None, None) != 0 and b"null struct" in L.asvrl_last_error()
            assert fn(None, C.byref(good()), None) != 0 and b"null params" in L.asvrl_last_error()
            for member in ("n_robots", "n_obs", "rflags", "key", "pos", "has_gauss", "gauss", "noise_out"):
                s = good()
                setattr(s, member, None)
                assert fn(C.byref(p), C.byref(s), None) != 0
                msg = L.asvrl_last_error()
                assert who in msg and b"null array " + member.encode() in msg, msg
            for member, bad, word in (("n_envs", 0, b"n_envs"), ("max_robots", 0, b"max_robots"),
                                      ("max_robots", 257, b"max_robots"), ("max_obs", -1, b"max_obs"),
                                      ("max_obs", 1023, b"max_obs + max_robots")):
                s = good()
                setattr(s, member, bad)
                assert fn(C.byref(p), C.byref(s), None) != 0 and word in L.asvrl_last_error(), (member, bad)
            s = good()
            s.draws_n = i64.ctypes.data   # the counters go together
            assert fn(C.byref(p), C.byref(s), None) != 0 and b"all or none" in L.asvrl_last_error()
        # and the good struct runs on the host: nobody exists, so nothing is drawn and the row is zeroed
        out[:] = 1.0
        assert L.asvrl_noise_streams_host(C.byref(p), C.byref(good()), None) == 0
        assert not out.any() and not key.any()


def test_python_refusals_without_a_gpu():
    from distributional_rl_decision_and_control_amd.noise_streams import NoiseStreams
    from distributional_rl_decision_and_control_amd.policy import device_eval
    from distributional_rl_decision_and_control_amd import _abi
    for who in ("run", "observe"):
        with pytest.raises(ValueError, match="perception must be one of"):
            device_eval._check_perception(who, "mt19937")
        with pytest.raises(ValueError, match="perception must be one of"):
            device_eval._check_perception(who, None)
        with pytest.raises(ValueError, match="explicit noise"):
            device_eval._check_perception(who, "numpy", None, torch.zeros(1))
        device_eval._check_perception(who, "numpy", None, None)
        device_eval._check_perception(who, "philox", torch.zeros(1))
    ns = NoiseStreams([1, 2, 3], device="cpu")
    z = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="3 streams for 4 robot rows"):
        ns.fill_raw(_abi.params_from(), 2, 2, 0, z, z, torch.zeros(4, dtype=torch.uint8))
