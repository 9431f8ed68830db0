"""GPU: VecTrainer._collect_window(fused_sac.window_pack, K) on a SAC trainer against K calls of VecTrainer.rollout(),
bit for bit (rtol = atol = 0, NaN = NaN; the stats' return sum, an atomic sum, within 1e-12): one closed-loop window
under the sampled actor with the auto-reset and one push of the window into the uniform ring (SAC's ring rows are
DDPG's) in place of K x (sac_act, step, push, reset, advance). episode_limit 3: every env restarts inside each window
of 5."""
import pytest
import torch

import window_cases as wc

pytestmark = pytest.mark.gpu

E, K = 37, 5
LIMIT = 3   # the episode limit, set before the first step: every env ends inside a window of 5


def test_collect_window_matches_rollouts():
    """Two windows of 5 against 10 rollout() calls: compared after each window, so the second window starts from
    reset envs and a part-filled ring."""
    ref, tr = wc.trainer("SAC", LIMIT, E), wc.trainer("SAC", LIMIT, E)
    pack = tr.fused_sac.window_pack
    assert pack is tr.fused_sac.actor and tr.learner.actor_pack is None
    resets = 0
    for w in range(2):
        for _ in range(K):
            ref.rollout()
            ref.env.advance_host()
        rec = tr._collect_window(pack, K)
        for _ in range(K):
            tr.env.advance_host()
        torch.cuda.synchronize()
        resets += int(rec.resets.sum().item())
        if w == 0:
            assert resets >= E, "every env must reset inside the first window"
        pushed = int(rec.pushed.sum().item())
        assert 0 < pushed <= K * E * tr.R
        wc.same(rec.pushed.sum().to(torch.int64), tr.replay.state[1] - (0 if w == 0 else first_size),
                f"window {w}: pushed")
        first_size = tr.replay.state[1].clone()
        wc.compare_trainers(tr, ref, f"window {w}")
        # the actions of the window are the sampled actor's: the last step's are what rollout() left in ref.actions
        wc.same(rec.actions[-1], ref.actions, f"window {w}: last actions")
    assert resets >= 2 * E, "every env restarts inside both windows"
    assert ref.env.episode_stats()["env_episodes"] == resets
    wc.same_learn(tr, ref, "loss after the windows")   # the update draws from identical rings


def test_collect_itself_still_refuses_sac():
    tr = wc.trainer("SAC", LIMIT, E)
    with pytest.raises(NotImplementedError):
        tr.collect(K)
