"""GPU: the window push (asvrl_replay_push_window) against K single pushes, and VecTrainer.collect(K) against K
calls of VecTrainer.rollout(), bit for bit (rtol = atol = 0, NaN = NaN; the stats' return sum, an atomic sum,
within 1e-12)."""
import numpy as np
import pytest
import torch

import window_cases as wc
from window_cases import ENV_ARRAYS

pytestmark = pytest.mark.gpu

E = 37
LIMIT = 5   # the episode limit, set before the first step: every env ends several times


def _synthetic(K, n, seed=3):
    """K steps of n rows; rows with obj_cnt = -1 scattered, a whole step of them among them."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rec = dict(obs_prev=torch.randn((K, n, 40), generator=g, device="cuda"),
               obs=torch.randn((K, n, 40), generator=g, device="cuda"),
               obj_cnt=(torch.randint(0, 8, (K, n), generator=g, device="cuda") - 2).clamp(max=5).to(torch.int8),
               actions=torch.rand((K, n, 2), generator=g, device="cuda", dtype=torch.float64),
               reward=torch.randn((K, n), generator=g, device="cuda", dtype=torch.float64),
               done=torch.randint(0, 2, (K, n), generator=g, device="cuda").to(torch.uint8))
    rec["obj_cnt"][2] = -1
    rec["obj_cnt"].clamp_(min=-1)
    return rec


@pytest.mark.parametrize("given", [True, False], ids=["pushed", "pushed_null"])
def test_push_window_matches_single_pushes(given):
    from distributional_rl_decision_and_control_amd.learn_ops import DeviceReplay
    K, n, CAP = 7, 185, 4096
    rec = _synthetic(K, n)
    counts = (rec["obj_cnt"] >= 0).sum(1).to(torch.int32)
    assert counts[2].item() == 0 and 0 < counts[0].item() < n
    head0 = CAP - 300   # the window (about 900 rows) wraps
    rings = []
    for window in (False, True):
        rp = DeviceReplay(CAP)
        g = torch.Generator(device="cuda").manual_seed(1)
        rp.ring.copy_(torch.randn(rp.ring.shape, generator=g, device="cuda"))
        rp.state.copy_(torch.tensor([head0, 2000], device="cuda"))
        snap = torch.zeros(2, dtype=torch.int64, device="cuda")
        counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
        if window:
            rp.push_window(rec, K, pushed=counts if given else None, snap=snap, counter_inc=counter)
        else:
            for t in range(K):
                rp.push(rec["obs_prev"][t], rec["obs"][t], rec["obj_cnt"][t], rec["actions"][t], rec["reward"][t],
                        rec["done"][t], snap=snap, counter_inc=counter)
        rings.append((rp.ring.clone(), rp.state.clone(), snap, counter))
    total = int(counts.sum().item())
    assert rings[0][1].tolist() == [(head0 + total) % CAP, min(2000 + total, CAP)] and head0 + total > CAP
    for got, ref, what in zip(rings[1], rings[0], ("ring", "{head, size}", "snap", "counter")):
        wc.same(got, ref, what)
    # a second window on the same replay: the scratch is left ready
    rp = DeviceReplay(CAP)
    rp.push_window(rec, K)
    rp.push_window(rec, K)
    assert rp.state.tolist() == [(2 * total) % CAP, min(2 * total, CAP)]
    with pytest.raises(ValueError):
        DeviceReplay(K * n - 1).push_window(rec, K)


def test_collect_matches_rollouts():
    """collect(13) twice against rollout() 26 times: the ring (which wraps), its state, the counter, the current
    observation, every env array, the episode statistics, and a learn() afterwards."""
    K = 13
    ref, tr = wc.trainer("AC-IQN", LIMIT, E), wc.trainer("AC-IQN", LIMIT, E)
    for _ in range(2 * K):
        ref.rollout()
    resets = 0
    for _ in range(2):
        rec = tr.collect(K)
        resets += int(rec.resets.sum().item())
    torch.cuda.synchronize()
    assert resets >= 2 * E, "every env restarts inside the windows"
    assert ref.env.episode_stats()["env_episodes"] == resets
    pushed = 2 * K * E * tr.R   # an upper bound; the ring of 4096 rows must have wrapped
    assert ref.replay.size() == 4096 and pushed > 4096
    wc.compare_trainers(tr, ref, "collect(13) x 2", host_counters=False)
    wc.same_learn(tr, ref, "loss after the windows")


def test_collect_other_agents():
    from distributional_rl_decision_and_control_amd.vec_trainer import VecTrainer
    with pytest.raises(NotImplementedError):
        VecTrainer(n_envs=E, agent_type="IQN", batch_size=64, buffer_size=4096, graphs=False).collect(4)


def test_collect_graph_capture():
    """collect(4) captured in a graph and replayed equals the eager call."""
    ref, tr = wc.trainer("AC-IQN", LIMIT, E), wc.trainer("AC-IQN", LIMIT, E)
    for t in (ref, tr):
        t.env.swap = False   # a captured window finds the same observation buffers at every replay
    for _ in range(2):
        ref.collect(4)
    tr.collect(4)          # eager: allocates the persistent buffers
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    keep = {n: getattr(tr.env.batch, n).clone() for n in ENV_ARRAYS + ("stats",)}
    side = (tr.replay.ring.clone(), tr.replay.state.clone(), tr.env.counter.clone(), tr.env.obs[0].clone(),
            tr.env.cnt[0].clone(), tr.env.obs[1].clone(), tr.env.cnt[1].clone())
    with torch.cuda.graph(g):
        tr.collect(4)
    # capturing ran nothing; restore what a capture may have touched, then replay once
    for n, t in keep.items():
        getattr(tr.env.batch, n).copy_(t)
    for dst, src in zip((tr.replay.ring, tr.replay.state, tr.env.counter, tr.env.obs[0], tr.env.cnt[0], tr.env.obs[1],
                         tr.env.cnt[1]), side):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    wc.compare_trainers(tr, ref, "captured collect(4)", host_counters=False)
    assert np.isfinite(tr.env.episode_stats()["mean_return"])
