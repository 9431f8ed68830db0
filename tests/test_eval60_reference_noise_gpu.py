"""GPU: the device evaluation with perception="numpy" pinned to the reference's own evaluation.

tests/golden/eval60_ref.npz + eval60_tf.npz hold the reference's 60 evaluation episodes of two agents (270 robots):
every robot's recorded actions and the count, sum and sum of squares of its perception-noise draws. With every robot
applying the reference's actions (an open-loop action table) and the perception noise drawn on the device from each
robot's own RandomState stream (asvrl_noise_streams), DeviceEvaluator.run must reproduce those episodes -- the bars of
tests/test_eval60_teacher_forced_gpu.py, which pins the host path the same way:

  * successes and times exact;
  * returns and energies within 1e-5 relative on all 60 configs (the measured maximum is printed; the host path
    measures 7.9e-15);
  * the final rs rows' 13 trajectory fields within 1e-9 of traj_last;
  * every robot's draws_n equal to the fixture's, |draws_sum - fixture| <= draws_n * 1e-12 and
    |draws_sq - fixture| <= draws_n * 2 pi * 1e-12 (the per-draw bar of 1e-12 on values of at most pi: d(x^2) = 2 |x| dx).

The same call with perception="philox" does not meet the draws_n check (it has no such streams): asserted, so the test
shows what it tests.
"""
import functools
import json

import numpy as np
import pytest
import torch

from oracle import env_oracle as eo

pytestmark = pytest.mark.gpu

SCHEDULE = {"num_episodes": [10, 10, 10, 10, 10, 10], "num_robots": [3, 4, 5, 5, 5, 5],
            "num_cores": [0, 0, 0, 0, 0, 0], "num_obstacles": [0, 0, 0, 2, 3, 4],
            "min_start_goal_dis": [30.0, 35.0, 40.0, 40.0, 40.0, 40.0]}   # config/ac_iqn.json eval_schedule
# trajectory_row's order in rs fields: ..., left_pos, right_pos, left_thrust, right_thrust = F_LP, F_RP, F_TL, F_TR
TRAJ_FIELDS = list(range(9)) + [11, 12, 9, 10]


@functools.lru_cache(maxsize=None)
def _template_env():
    """The eval env of the Trainer tests/test_eval60_teacher_forced_gpu.py builds."""
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.envs.marinenav.env import MarineNavEnv3
    from distributional_rl_decision_and_control_amd.policy.trainer import Trainer
    torch.manual_seed(0)
    agent = Agent(seed=100, agent_type="AC-IQN")
    tr = Trainer(MarineNavEnv3(seed=1), MarineNavEnv3(seed=253, is_eval_env=True), SCHEDULE, agent)
    return tr.eval_env


def _draws_n_match(res, want):
    return res["draws_n"] is not None and np.array_equal(np.concatenate(res["draws_n"]), want)


@pytest.mark.parametrize("tag", ["init", "trained"])
def test_device_evaluation_reproduces_the_reference_episodes(tag):
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.policy.device_eval import DeviceEvaluator
    assert (_abi.F_TL, _abi.F_TR, _abi.F_LP, _abi.F_RP) == (9, 10, 11, 12)
    z = np.load(eo.GOLDEN + "/eval60_ref.npz")
    t = np.load(eo.GOLDEN + "/eval60_tf.npz")
    p = tag + "/"
    robots = [int(n) for n in z[p + "robots"]]
    configs = json.loads(str(z[p + "configs"]))
    ev = DeviceEvaluator(configs, template_env=_template_env())
    # the action table: the reference's recorded actions, zero past a robot's own length
    lens = t[p + "act_len"]
    offs = np.concatenate([[0], np.cumsum(lens)])
    T = max(int(lens.max()), 1001)   # the whole episode limit, so that the Philox run below cannot run out of rows
    tables = [np.zeros((T, g.batch.n_envs * g.batch.max_robots, 2)) for g in ev.groups]
    k = 0
    for c, n in enumerate(robots):
        g, row0 = ev.rows(c)
        for i in range(n):
            a = t[p + "act"][offs[k]:offs[k + 1]]
            tables[g][:len(a), row0 + i] = a
            k += 1
    assert k == len(lens) == 270
    tables = [torch.from_numpy(a).cuda() for a in tables]
    table = tables[0] if len(tables) == 1 else tables

    res = ev.run(actions=table, perception="numpy")

    assert ev.steps <= int(lens.max()) + ev.chunk, "sync=True stops at the first host wait behind the last episode"
    np.testing.assert_array_equal(np.array(res["successes"]), z[p + "successes"])
    np.testing.assert_array_equal(np.array(res["times"]), z[p + "times"])
    rr = np.abs(np.array(res["rewards"]) / z[p + "rewards"] - 1)
    re = np.abs(np.array(res["energies"]) / z[p + "energies"] - 1)
    last = []
    for c, n in enumerate(robots):
        g, row0 = ev.rows(c)
        rs = ev.groups[g].batch.rs.cpu().numpy()
        last += [rs[TRAJ_FIELDS, row0 + i] for i in range(n)]
    d = np.abs(np.array(last) - z[p + "traj_last"]).max()
    dn, ds, dq = (np.concatenate(res[name]) for name in ("draws_n", "draws_sum", "draws_sq"))
    es = np.abs(ds - t[p + "draws_sum"])
    eq = np.abs(dq - t[p + "draws_sq"])
    n_ref = t[p + "draws_n"]
    print(f"{tag} device evaluation on the reference's streams: {ev.steps} steps, {int(dn.sum())} draws (reference "
          f"{int(n_ref.sum())}); return rel diff max {rr.max():.2e}, energy {re.max():.2e}, final rows {d:.2e}; "
          f"draws_sum diff max {es.max():.2e} (largest share of its bar {np.max(es / (n_ref * 1e-12)):.2e}), "
          f"draws_sq {eq.max():.2e} ({np.max(eq / (n_ref * 2 * np.pi * 1e-12)):.2e})")
    assert rr.max() <= 1e-5, rr
    assert re.max() <= 1e-5, re
    assert d <= 1e-9, d
    np.testing.assert_array_equal(dn, n_ref)
    assert _draws_n_match(res, n_ref)
    assert (es <= n_ref * 1e-12).all(), es.max()
    assert (eq <= n_ref * 2 * np.pi * 1e-12).all(), eq.max()

    # the default mode has no such streams: the same call does not meet the draws_n check
    philox = ev.run(actions=table, perception="philox")
    assert not _draws_n_match(philox, n_ref)
    assert philox["draws_n"] is None and philox["draws_sum"] is None and philox["draws_sq"] is None
