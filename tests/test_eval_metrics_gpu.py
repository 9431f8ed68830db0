"""GPU: asvrl_eval_metrics on synthetic rollout records against a numpy restatement of the evaluation's bookkeeping
(trainer.py:286-303), written here.

11 envs of at most 5 robots (1, 3 and 5 present), 13 steps, episode_limit 9. The records are built by hand so that
the batch holds: a goal at step 3 while the env's other robots go on; a later collision that ends the env, with the
rows behind it present and non-zero (the rollout steps an env on until all its robots are deactivated); a timeout;
an env that ends on the last step of a 5-step window and one that ends on the first step of the next; an env masked
from the start (steps_run 0); envs held inside a window (steps_run < K, the pre-fill behind it); absent robot slots;
dt, N and the power coefficient different from row to row. The same 13 steps fed as one window, as 5 + 5 + 3 and as
thirteen windows of one step must leave bit-identical state, with alive == !ended after every launch.

Tolerances: integers and flags exact; the f64 sums within 1e-12 relative (pow and the summation order are the only
freedom, over at most 10 terms here), the return relative to max(1, sum |term|) since its terms change sign."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, R, T, LIMIT, GAMMA = 11, 5, 13, 9, 0.99
NT = E * R
NROB = [5, 3, 1, 3, 5, 3, 5, 1, 3, 5, 3]
DSTEPS = [13, 13, 13, 13, 0, 3, 13, 13, 13, 13, 7]   # steps the rollout itself ran every env
# (env, robot, step, what): what 3 = reaches its goal, 2 = collides (the ASVRL_INFO_* codes)
EVENTS = [(0, 1, 3, 3), (0, 0, 7, 2),          # goal at 3, the others go on; collision at 7 ends the env
          (2, 0, 4, 3),                        # ends on the last step of the first 5-step window
          (3, 1, 5, 2),                        # ends on the first step of the second
          (6, 0, 1, 3), (6, 1, 2, 3), (6, 2, 3, 3), (6, 3, 4, 3), (6, 4, 6, 3),   # all deactivated at 6
          (7, 0, 0, 2),                        # collision at the first step
          (8, 0, 3, 3), (8, 2, 8, 2),          # goal, then a collision right before the limit
          (9, 2, 9, 3),                        # a goal on the timeout step
          (10, 1, 2, 3)]                       # held at 7 steps, not ended
STATE = ("length", "ended", "alive", "deact", "outcome", "ret", "time", "energy")


@functools.lru_cache(maxsize=None)
def _table():
    """The 13-step records of the whole batch (numpy) and the per-row constants."""
    from distributional_rl_decision_and_control_amd import _abi
    rng = np.random.RandomState(5)
    reward = rng.uniform(-3.0, 3.0, (T, NT))
    rs = rng.uniform(-900.0, 900.0, (T, _abi.NUM_FIELDS, NT))
    info = np.full((T, NT), _abi.INFO_NORMAL, np.uint8)
    for e in range(E):
        info[:, e * R + NROB[e]:(e + 1) * R] = _abi.INFO_ABSENT
    for e, i, t, code in EVENTS:
        info[t, e * R + i] = code
        info[t + 1:, e * R + i] = _abi.INFO_DEACT_COLLISION if code == 2 else _abi.INFO_DEACT_GOAL
    rows = np.arange(NT)
    dt = 0.05 + 0.01 * (rows % 3)
    N = 10.0 + (rows % 4)
    pc = 1.0 + 0.1 * (rows % 5)
    assert np.abs(reward).min() > 0 and np.abs(rs[:, _abi.F_TL]).min() > 0   # rows behind an end are non-zero
    return reward, info, rs, dt, N, pc


@functools.lru_cache(maxsize=None)
def _reference():
    """trainer.py:286-303 per env over the table; abs_ret: sum |term| of every robot's return."""
    from distributional_rl_decision_and_control_amd import _abi
    reward, info, rs, dt, N, pc = _table()
    st = dict(length=np.zeros(E, np.int32), ended=np.zeros(E, np.uint8), deact=np.zeros(NT, np.uint8),
              outcome=np.zeros(NT, np.uint8), ret=np.zeros(NT), time=np.zeros(NT), energy=np.zeros(NT))
    abs_ret = np.zeros(NT)
    for e in range(E):
        length, end_episode = 0, False
        t = 0
        while not end_episode and t < DSTEPS[e]:
            collided = False
            for i in range(NROB[e]):
                r = e * R + i
                if st["deact"][r]:
                    continue
                term = GAMMA ** length * reward[t, r]
                st["ret"][r] += term
                abs_ret[r] += abs(term)
                st["time"][r] += dt[r] * N[r]
                left = pc[r] * np.abs(rs[t, _abi.F_TL, r]) * dt[r] * N[r]
                right = pc[r] * np.abs(rs[t, _abi.F_TR, r]) * dt[r] * N[r]
                st["energy"][r] += left + right
                if info[t, r] in (_abi.INFO_COLLISION, _abi.INFO_REACH_GOAL):
                    st["deact"][r] = 1
                    st["outcome"][r] = 2 if info[t, r] == _abi.INFO_COLLISION else 1
                    collided |= info[t, r] == _abi.INFO_COLLISION
            end_episode = (length >= LIMIT) or collided or bool(st["deact"][e * R:e * R + NROB[e]].all())
            length += 1
            t += 1
        st["length"][e], st["ended"][e] = length, end_episode
    st["alive"] = (1 - st["ended"]).astype(np.uint8)
    return st, abs_ret


def _feed(ops, windows):
    """The table through asvrl_eval_metrics window by window, as the evaluator feeds it: steps_run from the steps
    the rollout ran (0 for an env the previous alive mask dropped), the rows behind steps_run at the records'
    pre-fill. Returns the state after the last window."""
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.policy.device_eval import eval_metrics, new_metrics_state
    reward, info, rs, dt, N, pc = _table()
    L = _abi.lib(ops)
    dev = torch.device("cuda")
    st = new_metrics_state(E, R, dev)
    n_robots = torch.tensor(NROB, dtype=torch.int32, device=dev)
    consts = [torch.from_numpy(a.copy()).to(dev) for a in (dt, N, pc)]
    t0 = 0
    for k in windows:
        alive = st["alive"].cpu().numpy()
        steps_run = np.clip(np.array(DSTEPS) - t0, 0, k) * (alive != 0)
        w = dict(reward=reward[t0:t0 + k].copy(), info=info[t0:t0 + k].copy(), rs=rs[t0:t0 + k].copy())
        for e in range(E):
            sl = slice(e * R, (e + 1) * R)
            w["reward"][steps_run[e]:, sl] = 0.0
            w["info"][steps_run[e]:, sl] = _abi.INFO_ABSENT
            w["rs"][steps_run[e]:, :, sl] = 0.0
        rec = {n: torch.from_numpy(a).to(dev) for n, a in w.items()}
        rec["steps_run"] = torch.from_numpy(steps_run.astype(np.int32)).to(dev)
        eval_metrics(L, k, E, R, rec, n_robots, *consts, st, GAMMA, LIMIT)
        assert torch.equal(st["alive"], 1 - st["ended"]), f"alive != !ended after the window at step {t0}"
        t0 += k
    assert t0 == T
    return {n: st[n].cpu().numpy() for n in STATE}


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_eval_metrics_against_numpy_and_across_windowings(ops):
    ref, abs_ret = _reference()
    # the cases the records were built for are really in the reference
    assert ref["length"].tolist() == [8, 10, 5, 6, 0, 3, 7, 1, 9, 10, 7]
    assert ref["ended"].tolist() == [1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0]
    assert ref["outcome"][0 * R + 1] == 1 and ref["outcome"][0 * R] == 2 and ref["outcome"][9 * R + 2] == 1
    got = _feed(ops, (T,))
    for n in ("length", "ended", "alive", "deact", "outcome"):
        np.testing.assert_array_equal(got[n], ref[n], err_msg=n)
    for n in ("time", "energy"):
        err = np.abs(got[n] - ref[n]) / np.maximum(np.abs(ref[n]), 1e-300)
        print(f"{ops} {n}: max rel err {err[ref[n] != 0].max():.2e}")
        np.testing.assert_allclose(got[n], ref[n], rtol=1e-12, atol=0, err_msg=n)
    err = np.abs(got["ret"] - ref["ret"]) / np.maximum(1.0, abs_ret)
    print(f"{ops} ret: max err relative to max(1, sum |term|) {err.max():.2e}")
    assert err.max() <= 1e-12, err
    # absent slots and the masked env stay untouched
    for e in range(E):
        for n in ("deact", "outcome", "ret", "time", "energy"):
            assert not got[n][e * R + NROB[e]:(e + 1) * R].any(), (e, n)
    assert not any(got[n][4 * R:5 * R].any() for n in ("ret", "time", "energy", "deact")) and got["alive"][4] == 1
    # the same steps in other windows: the same bits
    for windows in ((5, 5, 3), (1,) * T):
        other = _feed(ops, windows)
        for n in STATE:
            assert got[n].tobytes() == other[n].tobytes(), (windows, n)
