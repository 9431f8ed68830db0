"""GPU: the readout of the quantile samples behind IQN's decisions (asvrl_iqn_dist, critic kernel mode IQN_DIST).

f32 build against torch: IQN_Policy.forward(x, 32, cvar, taus) with the fractions given, at the project's f32 parity
bar of 1e-5 (the output scale is ~0.2), for M = 1, 15, 16, 17 and 33 rows: one state, one below / at / above the
16-wave workgroup, three workgroups. Arg-maxes are not compared with torch (an untrained net has near ties); z is
compared with the kernel's own all-actions block at the kernel's own selection, exactly.

bf16 build: the Philox keys (one launch over a [3][5] plane = three launches with step0 = t = three act launches with
step_add = t, bit for bit), the per-row levels, the range check of device-side action indices and the wrapper's
refusals."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

A = 25
SEED = 4242
EPS_ZERO = (1.0, 1.0, 1.0, 0.0, 0.0)
T, NT = 3, 5


@functools.lru_cache(maxsize=None)
def _net():
    from distributional_rl_decision_and_control_amd.policy.IQN_model import IQN_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    return IQN_Policy(**DEFAULT_NET, action_size=A, device="cuda", seed=100).cuda()


@functools.lru_cache(maxsize=None)
def _pack(operands="bf16"):
    from distributional_rl_decision_and_control_amd.fused_iqn import IqnPack
    return IqnPack(_net(), operands)


@functools.lru_cache(maxsize=None)
def _inputs(n=33):
    g = torch.Generator().manual_seed(5)
    x = torch.zeros(n, 40)
    x[:, 0:7] = torch.randn(n, 7, generator=g) * 3
    x[:, 7:32] = torch.randn(n, 25, generator=g) * 3
    x[:, 32:37] = (torch.rand(n, 5, generator=g) > 0.4).float()
    taus = torch.rand(n, 32, generator=g)
    return x.cuda(), taus.cuda()


def _split(x):
    n = x.shape[0]
    return x[:, 0:7], x[:, 7:32].reshape(n, 5, 5), x[:, 32:37]


def _dist(*a, **kw):
    from distributional_rl_decision_and_control_amd.fused_iqn import iqn_dist
    return iqn_dist(*a, **kw)


def _same(a, b, what):
    for name, x, y in zip(a._fields, a, b):
        assert torch.equal(x, y), (what, name)
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (what, name)


@pytest.mark.parametrize("cvar", [1.0, 0.25])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 33])
def test_f32_build_against_torch(M, cvar):
    x, taus = (t[:M].contiguous() for t in _inputs())
    with torch.no_grad():
        ref, ref_taus = _net()(_split(x), 32, cvar, taus=taus)
    d = _dist(_pack("f32"), x, cvar=cvar, taus=taus)
    assert d.all.shape == (M, 32, A) and d.z.shape == (M, 32) and d.q.shape == (M, A)
    err = float((d.all - ref).abs().max())
    print(f"M = {M}, cvar = {cvar}: max |all - torch| = {err:.2e} (scale {float(ref.abs().max()):.3f})")
    assert err <= 1e-5
    assert torch.equal(d.taus, taus * cvar) and torch.equal(d.taus, ref_taus.view(M, 32))
    sel = d.greedy.long()
    assert bool(((sel >= 0) & (sel < A)).all())
    assert torch.equal(d.z, d.all.gather(2, sel.view(M, 1, 1).expand(M, 32, 1)).squeeze(2))
    # the selection is the first arg-max of the kernel's own 32-sample sums; its action values are their means
    assert float((d.q - ref.mean(1)).abs().max()) <= 1e-5
    assert torch.equal(d.q.max(1).values, d.q.gather(1, sel.view(M, 1)).squeeze(1))


def test_given_actions_select_the_column():
    x, taus = _inputs()
    M = x.shape[0]
    acts = torch.zeros((M, 2), dtype=torch.float64, device="cuda")
    acts[:, 0] = torch.arange(M, device="cuda") % A
    acts[:, 1] = 0.5   # the second slot is not the kernel's business
    for ops in ("f32", "bf16"):
        d = _dist(_pack(ops), x, taus=taus, actions=acts)
        free = _dist(_pack(ops), x, taus=taus)
        assert torch.equal(d.all, free.all) and torch.equal(d.greedy, free.greedy) and torch.equal(d.q, free.q)
        idx = acts[:, 0].long().view(M, 1, 1).expand(M, 32, 1)
        assert torch.equal(d.z, d.all.gather(2, idx).squeeze(2))


def test_one_launch_over_the_plane_is_the_launches_per_step():
    """bf16: the drawn fractions are keyed (slot * 32 + sample, step, seed): a [T][NT] plane in one launch, T launches
    of NT rows with step0 = t, and the act launches of the windows (iqn_act at epsilon 0 with step_add = t and its
    q_out) agree bit for bit."""
    from distributional_rl_decision_and_control_amd.fused_iqn import iqn_act
    x, _ = _inputs()
    x = x[:T * NT].contiguous()
    pack = _pack()
    whole = _dist(pack, x, rows_per_step=NT, step0=0, seed=SEED, cvar=0.5)
    assert float(whole.taus.max()) <= 0.5 and float(whole.taus.min()) >= 0.0
    assert len(torch.unique(whole.taus)) > T * NT * 16, "the draws repeat"
    for t in range(T):
        rows = x[t * NT:(t + 1) * NT]
        part = _dist(pack, rows, rows_per_step=NT, step0=t, seed=SEED, cvar=0.5)
        _same(part, type(part)(*[v[t * NT:(t + 1) * NT] for v in whole]), f"step {t}")
        act = torch.full((NT, 2), -1.0, dtype=torch.float64, device="cuda")
        q = torch.zeros((NT, A), device="cuda")
        for step_dev in (None, torch.zeros(1, dtype=torch.int64, device="cuda")):
            iqn_act(pack, None, act, step_dev, *EPS_ZERO, SEED, obs=rows, cvar=0.5, step_add=t, q_out=q)
            assert torch.equal(act[:, 0], part.greedy.double()), t
            assert q.cpu().numpy().tobytes() == part.q.cpu().numpy().tobytes(), t
    other = _dist(pack, x, rows_per_step=NT, step0=0, seed=SEED + 1, cvar=0.5)
    assert not torch.equal(other.taus, whole.taus)


def test_levels_per_row():
    x, _ = _inputs()
    M = 6
    x = x[:M].contiguous()
    pack = _pack()
    lev = torch.tensor([1.0, 0.5, 0.1, 0.1, 0.5, 1.0], device="cuda")
    one = _dist(pack, x, rows_per_step=3, step0=2, seed=SEED)
    got = _dist(pack, x, rows_per_step=3, step0=2, seed=SEED, levels=lev)
    assert torch.equal(got.taus, one.taus * lev.view(M, 1))
    for i in (0, 5):   # level 1: the scalar run's bits
        assert torch.equal(got.all[i], one.all[i]) and torch.equal(got.z[i], one.z[i])
    # a row under level l is the scalar run at cvar = l
    for l, rows in ((0.5, (1, 4)), (0.1, (2, 3))):
        sc = _dist(pack, x, rows_per_step=3, step0=2, seed=SEED, cvar=l)
        for i in rows:
            assert torch.equal(got.all[i], sc.all[i]) and torch.equal(got.z[i], sc.z[i]) and got.greedy[i] == sc.greedy[i]


@pytest.mark.parametrize("bad", [25.0, -1.0, float("nan"), 1e30])
def test_an_action_index_out_of_range_gives_a_nan_row(bad):
    x, taus = _inputs()
    M = 17
    x, taus = x[:M].contiguous(), taus[:M].contiguous()
    acts = torch.zeros((M, 2), dtype=torch.float64, device="cuda")
    acts[:, 0] = 3.0
    acts[7, 0] = bad
    acts[16, 0] = bad
    d = _dist(_pack(), x, taus=taus, actions=acts)
    torch.cuda.synchronize()
    nan = torch.isnan(d.z).all(dim=1)
    assert nan.nonzero().view(-1).tolist() == [7, 16]
    assert bool(torch.isfinite(d.z[~nan]).all()) and bool(torch.isfinite(d.all).all())
    assert torch.equal(d.z[~nan], d.all[~nan][:, :, 3])


def test_given_outputs_are_filled_in_place():
    x, taus = _inputs()
    M = x.shape[0]
    z = torch.zeros((M, 32), device="cuda")
    al = torch.full((M, 32, 32), -3.0, device="cuda")   # padded to 32 columns
    q = torch.full((M, 28), -3.0, device="cuda")
    d = _dist(_pack(), x, taus=taus, z_out=z, all_out=al, q_out=q)
    ref = _dist(_pack(), x, taus=taus)
    assert d.z is z and d.all is al and d.q is q
    assert torch.equal(z, ref.z) and torch.equal(al[:, :, :A], ref.all) and torch.equal(q[:, :A], ref.q)
    assert bool((al[:, :, A:] == -3.0).all()) and bool((q[:, A:] == -3.0).all())


def test_refusals_of_the_wrapper():
    x, taus = _inputs()
    pack = _pack()
    M = x.shape[0]
    lev = torch.ones(M, device="cuda")
    for kw in (dict(cvar=0.0), dict(cvar=1.5), dict(cvar=-1.0), dict(cvar=0.5, levels=lev), dict(rows_per_step=0),
               dict(step0=-1), dict(levels=lev[:5]), dict(levels=lev.double()), dict(taus=taus[:, :16]),
               dict(actions=torch.zeros((M, 2), device="cuda")), dict(z_out=torch.zeros((M, 16), device="cuda")),
               dict(all_out=torch.zeros((M, 32, 8), device="cuda")), dict(q_out=torch.zeros((M, 8), device="cuda")),
               dict(greedy_out=torch.zeros(M, dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            _dist(pack, x, **kw)
    with pytest.raises(ValueError):
        _dist(pack, x.double())
    with pytest.raises(ValueError):
        _dist(pack, x[:, :30])


def test_no_rows_is_a_quiet_return():
    x, _ = _inputs()
    d = _dist(_pack(), x[:0])
    assert d.z.shape == (0, 32) and d.taus.shape == (0, 32) and d.all.shape == (0, 32, A) and d.greedy.shape == (0,)
    assert d.q.shape == (0, A)
