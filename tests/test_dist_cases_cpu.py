"""CPU: the numpy restatement of asvrl_eval_dist_stats (tests/dist_cases.py) on a case computed by hand.

2 robots of one env, 3 steps, gamma 0.5, every step's 32 samples one constant.
Robot 0 acts 3 times, rewards 1, 2, 4:   G_2 = 4, G_1 = 2 + 0.5 * 4 = 4, G_0 = 1 + 0.5 * 4 = 3.
  samples z = 3 (step 0), 5 (step 1), 1 (step 2), fractions 0.25 everywhere:
  step 0: z = G: all 32 count as <=, bin 32; d = 0, pinball 0;             mean - G = 0
  step 1: z > G: none, bin 0; d = -1, rho = -1 * (0.25 - 1) = 0.75, x 32 = 24;  mean - G = 1
  step 2: z < G: all, bin 32; d = 3, rho = 3 * 0.25 = 0.75, x 32 = 24;          mean - G = -3
  pit[0] = 1, pit[32] = 2; pinball = 48; bias = -2; pred0 = 3; g0 = 3; steps = 3.
Robot 1 acts once, reward -2: G_0 = -2; samples -2.5 with fraction 0.5: bin 32, d = 0.5, rho = 0.25, x 32 = 8;
  bias = -0.5; pred0 = -2.5; g0 = -2; steps = 1; its G rows 1, 2 keep the pre-fill."""
import numpy as np

import dist_cases


def test_hand_computed_case():
    T, NT, S = 3, 2, dist_cases.S
    z = np.zeros((T, NT, S), np.float32)
    tau = np.full((T, NT, S), 0.25, np.float32)
    z[:, 0] = np.array([3.0, 5.0, 1.0], np.float32)[:, None]
    z[:, 1] = -2.5
    tau[:, 1] = 0.5
    reward = np.array([[1.0, -2.0], [2.0, 9.0], [4.0, 9.0]])
    out = dist_cases.dist_stats_numpy(z, tau, reward, np.array([3, 1]), np.array([2]), 2, 0.5)
    assert out["g0"].tolist() == [3.0, -2.0]
    assert out["G"][:, 0].tolist() == [3.0, 4.0, 4.0]
    assert out["G"][:, 1].tolist() == [-2.0, dist_cases.PREFILL["G"], dist_cases.PREFILL["G"]]
    assert out["steps"].tolist() == [3, 1]
    pit0 = np.zeros(S + 1, np.int32)
    pit0[0], pit0[32] = 1, 2
    pit1 = np.zeros(S + 1, np.int32)
    pit1[32] = 1
    assert out["pit"][0].tolist() == pit0.tolist() and out["pit"][1].tolist() == pit1.tolist()
    assert out["pinball"].tolist() == [48.0, 8.0]
    assert out["bias"].tolist() == [-2.0, -0.5]
    assert out["pred0"].tolist() == [3.0, -2.5]


def test_absent_rows_and_zero_acts_keep_or_zero():
    """A slot behind n_robots keeps every pre-fill; a robot that never acted has zeros and an empty histogram."""
    T, R, S = 2, 3, dist_cases.S
    z = np.ones((T, R, S), np.float32)
    tau = np.full((T, R, S), 0.5, np.float32)
    out = dist_cases.dist_stats_numpy(z, tau, np.ones((T, R)), np.array([0, 2, 2]), np.array([2]), R, 0.9)
    assert out["steps"].tolist() == [0, 2, dist_cases.PREFILL["steps"]]
    assert out["g0"].tolist() == [0.0, 1.9, dist_cases.PREFILL["g0"]]
    assert out["pit"][0].sum() == 0 and (out["pit"][2] == dist_cases.PREFILL["pit"]).all()
    assert out["pred0"][0] == 0.0 and out["pinball"][0] == 0.0 and out["bias"][0] == 0.0
