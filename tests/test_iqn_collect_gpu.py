"""GPU: VecTrainer._collect_window(fused_iqn.window_pack, K) on an IQN trainer against K calls of VecTrainer.rollout(),
bit for bit (rtol = atol = 0, NaN = NaN; the stats' return sum, an atomic sum, within 1e-12): one closed-loop window
under IQN_Policy with the auto-reset and one push of the window into the uniform ring in place of K x (iqn_act, step,
push, reset, advance). rollout() pushes the one action column and the window its (index, 0.0) pair: the ring row is
the same (index, 0). episode_limit 3: every env restarts inside each window of 5."""
import pytest
import torch

import window_cases as wc

pytestmark = pytest.mark.gpu

E, K = 37, 5
LIMIT = 3   # the episode limit, set before the first step: every env ends inside a window of 5


def test_collect_window_matches_rollouts():
    """Two windows of 5 against 10 rollout() calls: compared after each window, so the second window starts from
    reset envs and a part-filled ring."""
    ref, tr = wc.trainer("IQN", LIMIT, E), wc.trainer("IQN", LIMIT, E)
    pack = tr.fused_iqn.window_pack
    assert pack is tr.fused_iqn.local and tr.learner.actor_pack is None and not tr.env.is_continuous
    resets = 0
    first_size = 0
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
        wc.same(rec.pushed.sum().to(torch.int64), tr.replay.state[1] - first_size, f"window {w}: pushed")
        first_size = tr.replay.state[1].clone()
        wc.compare_trainers(tr, ref, f"window {w}")
        # the last step's actions are what rollout() left in ref.actions: (index, 0.0)
        wc.same(rec.actions[-1], ref.actions, f"window {w}: last actions")
        a0 = rec.actions[..., 0]
        assert bool(((a0 >= 0) & (a0 < tr.fused_iqn.A) & (a0 == a0.round())).all())
        assert bool((rec.actions[..., 1] == 0.0).all())
        assert a0.unique().numel() >= 3, "the exploring window takes several actions"
    assert resets >= 2 * E, "every env restarts inside both windows"
    assert ref.env.episode_stats()["env_episodes"] == resets
    wc.same_learn(tr, ref, "loss after the windows")   # the update draws from identical rings


def test_collect_itself_still_refuses_iqn():
    tr = wc.trainer("IQN", LIMIT, E)
    with pytest.raises(NotImplementedError):
        tr.collect(K)
