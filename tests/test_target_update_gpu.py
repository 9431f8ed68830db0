"""GPU: asvrl_target_update_pack at the kernel level, in both builds.

  * the flat blend equals torch's own tau * l + (1.0 - tau) * t bit for bit, at one element, around one block, and one
    element past 1024 blocks x 256 threads (the grid-stride loop); tau = 1 is a copy, whatever the target held;
  * the predicate: with counter % interval != 0 the launch leaves the target and every image untouched, with a null
    counter it always fires, and it never writes the counter;
  * the images: for every pack class the batched learners use as a target pack, one device step at tau = 0.25 through
    the pack's own segment table leaves every tensor the pack's refresh() writes equal to a second pack of the same
    class built over a torch-blended copy of the target network and refreshed."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GRID = 1024 * 256   # the launch's largest grid: past it a thread takes a second element


def _launch(L, target, local, tau, counter=None, interval=0, segs=()):
    from distributional_rl_decision_and_control_amd import _abi
    arr = (_abi.AsvPackSeg * max(1, len(segs)))(*segs)
    rc = L.asvrl_target_update_pack(_abi.ptr(target), _abi.ptr(local), target.numel(), float(tau), 1.0 - float(tau),
                                    _abi.ptr(counter), interval, arr, len(segs), _abi.stream_ptr(None))
    _abi.check(rc, "asvrl_target_update_pack", L)


def _pair(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    # magnitudes over many binades, both signs: the rounding of the two products and of the sum all matter
    mk = lambda: torch.randn(n, generator=g, device=DEV) * torch.exp2(torch.randint(-12, 6, (n,), generator=g,
                                                                                   device=DEV).float())
    return mk(), mk()


@pytest.mark.parametrize("ops", ["bf16", "f32"])
@pytest.mark.parametrize("tau", [1.0, 0.25, 0.005])
@pytest.mark.parametrize("n", [1, 255, 256, 257, GRID + 257])
def test_flat_blend_is_torchs_expression(n, tau, ops):
    from distributional_rl_decision_and_control_amd import _abi
    local, target = _pair(n, 1000 + n % 977)
    want = tau * local + (1.0 - tau) * target   # Agent.soft_update's expression, evaluated by torch on the device
    local0 = local.clone()
    _launch(_abi.lib(ops), target, local, tau)
    torch.cuda.synchronize()
    assert torch.equal(target, want), float((target - want).abs().max())
    assert torch.equal(local, local0)


def test_tau_one_is_a_copy_whatever_the_target_held():
    from distributional_rl_decision_and_control_amd import _abi
    local, target = _pair(257, 5)
    target[3], target[200], target[256] = float("inf"), float("nan"), float("-inf")
    _launch(_abi.lib(), target, local, 1.0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(target).all()) and torch.equal(target, local)


def _hand_table(flat_t, img, bias_img):
    """A 32 x 16 weight at the buffer's start into a K = 16 fragment image, a 32-vector behind it into an f32 image."""
    from distributional_rl_decision_and_control_amd import _abi
    w, b = _abi.AsvPackSeg(), _abi.AsvPackSeg()
    w.flat_off, w.image, w.rows, w.cols, w.K, w.nrep = 0, img.data_ptr(), 32, 16, 16, 1
    b.flat_off, b.image, b.rows, b.cols, b.f32, b.nrep = 512, bias_img.data_ptr(), 32, 1, 1, 1
    return [w, b]


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_predicate_on_the_device_counter(ops):
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.fused_critic import frag_index
    L, interval, tau = _abi.lib(ops), 3, 0.25
    n = 512 + 32 + 300   # the two packed parameters and a tail no image takes, over several blocks
    local, t0 = _pair(n, 11)
    idx = frag_index(32, 16, False, DEV)
    for count in (0, 1, interval - 1, interval, 2 * interval + 1, None):
        target = t0.clone()
        img = torch.full((512,), 7.0, dtype=_abi.operand_dtype(ops), device=DEV)   # the sentinel
        bias_img = torch.full((32,), 7.0, dtype=torch.float32, device=DEV)
        counter = torch.tensor([count], dtype=torch.int64, device=DEV) if count is not None else None
        _launch(L, target, local, tau, counter, interval, _hand_table(target, img, bias_img))
        torch.cuda.synchronize()
        if counter is not None:
            assert int(counter.item()) == count, "the counter is read only"
        if count is None or count % interval == 0:
            want = tau * local + (1.0 - tau) * t0
            assert torch.equal(target, want), count
            assert torch.equal(img, torch.index_select(want[:512], 0, idx).to(img.dtype)), count
            assert torch.equal(bias_img, want[512:544]), count
        else:
            assert torch.equal(target, t0), count
            assert bool((img == 7.0).all()) and bool((bias_img == 7.0).all()), count


# ---------------------------------------------------------------------------------------------------- the pack classes

def _images(pack):
    """Every tensor the pack's refresh() writes."""
    if hasattr(pack, "sets"):   # MlpPack and its subclasses: one image set here (the targets are never double)
        assert len(pack.sets) == 1
        return {k: v for k, v in pack.sets[0].items() if isinstance(v, torch.Tensor)}
    out = {k: getattr(pack, k) for k in ("wc", "w1", "w2", "w2t", "w1t")}   # CriticPack
    if hasattr(pack, "head_img"):
        out["head_img"] = pack.head_img
    return out


def _mlp(net, ops):
    from distributional_rl_decision_and_control_amd.fused_mlp import MlpPack
    return MlpPack(net, "actor", ops)


def _critic(net, ops):
    from distributional_rl_decision_and_control_amd.fused_critic import CriticPack
    return CriticPack(net, ops)


def _iqn(net, ops):
    from distributional_rl_decision_and_control_amd.fused_iqn import IqnPack
    return IqnPack(net, ops)


def _dqn(net, ops):
    from distributional_rl_decision_and_control_amd.fused_dqn import DqnPack
    return DqnPack(net, ops)


def _ddpg(net, ops):
    from distributional_rl_decision_and_control_amd.fused_ddpg import DdpgCriticPack
    return DdpgCriticPack(net, ops)


def _sac(net, ops):
    from distributional_rl_decision_and_control_amd.fused_sac import SacActorPack
    return SacActorPack(net, ops)


# pack class -> (agent whose policy holds the network, the module inside it, the pack's constructor, images expected)
PACKS = {
    "MlpPack": ("AC-IQN", "actor", _mlp, {"enc", "b_enc", "w1", "w2", "w2t", "w1t"}),
    "CriticPack": ("AC-IQN", "critic", _critic, {"wc", "w1", "w2", "w2t", "w1t"}),
    "IqnPack": ("IQN", None, _iqn, {"wc", "w1", "w2", "w2t", "w1t", "head_img"}),
    "DqnPack": ("DQN", None, _dqn, {"enc", "b_enc", "w1", "w2", "w2t", "w1t", "head"}),
    "DdpgCriticPack": ("DDPG", "critic", _ddpg, {"enc", "b_enc", "w1", "w2", "w2t", "w1t", "wo", "bo"}),
    "SacActorPack": ("SAC", "actor", _sac, {"enc", "b_enc", "w1", "w2", "w2t", "w1t", "b1", "b2", "head", "bhead"}),
}


def _net(agent, module, seed):
    from distributional_rl_decision_and_control_amd.learners import LEARNERS
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    policy = LEARNERS[agent].make_policy(DEFAULT_NET.values(), torch.device(DEV), seed)
    return getattr(policy, module) if module else policy


@pytest.mark.parametrize("ops", ["bf16", "f32"])
@pytest.mark.parametrize("name", sorted(PACKS))
def test_images_equal_a_refreshed_pack_over_the_blended_network(name, ops):
    from distributional_rl_decision_and_control_amd.learner import FlatParams, FusedAdam
    agent, module, make, expected = PACKS[name]
    tau = 0.25
    local, target, blended = _net(agent, module, 100), _net(agent, module, 7), _net(agent, module, 7)
    with torch.no_grad():
        assert not all(torch.equal(l, t) for l, t in zip(local.parameters(), target.parameters()))
        for b, l, t in zip(blended.parameters(), local.parameters(), target.parameters()):
            b.copy_(tau * l + (1.0 - tau) * t)   # Agent.soft_update's expression
    opt = FusedAdam(local.parameters(), operands=ops)
    for p in target.parameters():
        p.requires_grad_(False)
    flat = FlatParams(target.parameters(), ops)   # before the pack, which caches parameter pointers
    assert flat.n == opt.n and all(p.data_ptr() >= flat.flat.data_ptr() for p in target.parameters())
    pack, want = make(target, ops), make(blended, ops)
    got_imgs, want_imgs = _images(pack), _images(want)
    assert set(got_imgs) == set(want_imgs) == expected
    before = {k: v.clone() for k, v in got_imgs.items()}
    flat.update_from(opt, tau, pack)
    torch.cuda.synchronize()
    for t, b in zip(target.parameters(), blended.parameters()):
        assert torch.equal(t, b)
    for k in sorted(expected):
        assert torch.equal(got_imgs[k], want_imgs[k]), k
        assert not torch.equal(got_imgs[k], before[k]), k   # the step did write this image
    # ... and the same table again is the next blend: nothing about the first call was one-shot
    with torch.no_grad():
        for b, l in zip(blended.parameters(), local.parameters()):
            b.copy_(tau * l + (1.0 - tau) * b)
    want.refresh()
    flat.update_from(opt, tau, pack)
    torch.cuda.synchronize()
    for k in sorted(expected):
        assert torch.equal(got_imgs[k], want_imgs[k]), k
