"""GPU: VecTrainer._collect_window(fused_iqn.window_pack, K) on an IQN trainer against K calls of VecTrainer.rollout(),
bit for bit (rtol = atol = 0, NaN = NaN; the stats' return sum, an atomic sum, within 1e-12): one closed-loop window
under IQN_Policy with the auto-reset and one push of the window into the uniform ring in place of K x (iqn_act, step,
push, reset, advance). rollout() pushes the one action column and the window its (index, 0.0) pair: the ring row is
the same (index, 0). episode_limit 3: every env restarts inside each window of 5."""
import pytest
import torch

pytestmark = pytest.mark.gpu

E, K = 37, 5
ENV_ARRAYS = ("rs", "rflags", "n_robots", "n_obs", "n_cores", "ep_ts", "obstacles", "cores", "obs", "obj_cnt", "reward",
              "done", "info", "env_done")


def _same(got, ref, what):
    torch.testing.assert_close(got, ref, rtol=0, atol=0, equal_nan=True, msg=lambda m: f"{what}: {m}")


def _trainer():
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    tr = VecTrainer(agent_type="IQN", n_envs=E, batch_size=64, buffer_size=4096, graphs=False, seed=3)
    tr.env.batch.params.episode_limit = 3   # before the first step: every env ends inside a window of 5
    return tr


def _compare(a, b, what):
    _same(a.replay.ring, b.replay.ring, f"{what}: ring")
    _same(a.replay.state, b.replay.state, f"{what}: ring state")
    _same(a.env.counter, b.env.counter, f"{what}: env.counter")
    _same(a.learn_counter, b.learn_counter, f"{what}: learn counter")
    _same(a.env.obs_cur, b.env.obs_cur, f"{what}: obs_cur")
    _same(a.env.cnt_cur, b.env.cnt_cur, f"{what}: cnt_cur")
    for n in ENV_ARRAYS:
        _same(getattr(a.env.batch, n), getattr(b.env.batch, n), f"{what}: {n}")
    assert a.env.total_timesteps == b.env.total_timesteps
    sa, sb = a.env.episode_stats(), b.env.episode_stats()
    for k in ("robot_episodes", "env_episodes", "success", "collision", "timeout"):
        assert sa[k] == sb[k], (what, k, sa[k], sb[k])
    assert abs(sa["mean_return"] - sb["mean_return"]) <= 1e-12 * max(1.0, abs(sb["mean_return"]))


def test_collect_window_matches_rollouts():
    """Two windows of 5 against 10 rollout() calls: compared after each window, so the second window starts from
    reset envs and a part-filled ring."""
    ref, tr = _trainer(), _trainer()
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
        _same(rec.pushed.sum().to(torch.int64), tr.replay.state[1] - first_size, f"window {w}: pushed")
        first_size = tr.replay.state[1].clone()
        _compare(tr, ref, f"window {w}")
        # the last step's actions are what rollout() left in ref.actions: (index, 0.0)
        _same(rec.actions[-1], ref.actions, f"window {w}: last actions")
        a0 = rec.actions[..., 0]
        assert bool(((a0 >= 0) & (a0 < tr.fused_iqn.A) & (a0 == a0.round())).all())
        assert bool((rec.actions[..., 1] == 0.0).all())
        assert a0.unique().numel() >= 3, "the exploring window takes several actions"
    assert resets >= 2 * E, "every env restarts inside both windows"
    assert ref.env.episode_stats()["env_episodes"] == resets
    la, lb = tr.learn(), ref.learn()   # the update draws from identical rings
    torch.cuda.synchronize()
    for x, y in zip(la, lb):
        if torch.is_tensor(x):
            _same(x, y, "loss after the windows")
        else:
            assert x == y


def test_collect_itself_still_refuses_iqn():
    tr = _trainer()
    with pytest.raises(NotImplementedError):
        tr.collect(K)
