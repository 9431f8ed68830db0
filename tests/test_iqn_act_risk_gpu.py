"""GPU: the IQN act pass under a risk level per row (asvrl_iqn_act_risk, critic kernel mode IQN_ACT_RISK): the level
as an f32 tensor, one value per row, or computed in the kernel from the row by fused_iqn.AdaptiveCvar.

The inputs are tests/test_iqn_act_ex_gpu.py's -- the same net (seed 100), the same CPU generator (seed 5) drawing x
then taus, n = 185 rows so the last 16-wave workgroup is partial -- with object 0 of row i overwritten: rho = 0.4 +
0.137 i, theta = 0.7 i, (px, py) = rho (cos theta, sin theta), r = 0.5, mask[0] = 1, and on every 7th row the whole
mask 0. Under the default rule 27 rows have no object, 77 are at or beyond `near`, 57 on the linear part and 24 at the
floor; no row is closer than 0.022 m to the `near` boundary or than 0.0073 in level to the floor boundary; the torch
reference under the per-row levels has output scale 0.2226, top-two gaps of at least 2.5e-4 of it, every row below
level 1 moves by at least 1.1 % of it against level 1 and the arg-max changes on 8.6 % of the rows
(test_the_reference_itself_depends_on_the_rule asserts all of it, so a kernel that ignores the rule cannot pass)."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

A = 25
N_ROWS, R = 185, 5
SEED = 99
EPS_HALF = (1.0, 1.0, 1.0, 0.5, 0.5)
EPS_ZERO = (1.0, 1.0, 1.0, 0.0, 0.0)
LINEAR_ROWS = (29, 36, 50, 60, 71, 80, 92, 94)
OTHER = dict(near=6.0, margin=1.0, floor=0.25)


@functools.lru_cache(maxsize=None)
def _net():
    from distributional_rl_decision_and_control_amd.policy.IQN_model import IQN_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    return IQN_Policy(**DEFAULT_NET, action_size=A, device="cuda", seed=100).cuda()


@functools.lru_cache(maxsize=None)
def _pack(operands="bf16"):
    from distributional_rl_decision_and_control_amd.fused_iqn import IqnPack
    return IqnPack(_net(), operands)


def _rule(**kw):
    from distributional_rl_decision_and_control_amd.fused_iqn import AdaptiveCvar
    return AdaptiveCvar(**kw)


@functools.lru_cache(maxsize=None)
def _inputs():
    g = torch.Generator().manual_seed(5)
    n = N_ROWS
    x = torch.zeros(n, 40)
    x[:, 0:7] = torch.randn(n, 7, generator=g) * 3
    x[:, 7:32] = torch.randn(n, 25, generator=g) * 3
    x[:, 32:37] = (torch.rand(n, 5, generator=g) > 0.4).float()
    taus = torch.rand(n, 32, generator=g)
    for i in range(n):
        rho, th = 0.4 + 0.137 * i, 0.7 * i
        x[i, 7], x[i, 8], x[i, 11], x[i, 32] = rho * math.cos(th), rho * math.sin(th), 0.5, 1.0
        if i % 7 == 0:
            x[i, 32:37] = 0.0
    return x.cuda(), taus.cuda()


def _split(x):
    n = x.shape[0]
    return x[:, 0:7], x[:, 7:32].reshape(n, 5, 5), x[:, 32:37]


@functools.lru_cache(maxsize=None)
def _levels():
    return _rule().levels(_inputs()[0])


@functools.lru_cache(maxsize=None)
def _reference(per_row=True):
    """quantiles.mean(dim=1) of IQN_Policy.forward under the per-row levels (or level 1), torch fp32: [n, A]."""
    x, taus = _inputs()
    cvar = _levels().view(N_ROWS, 1, 1) if per_row else 1.0
    with torch.no_grad():
        return _net()(_split(x), 32, cvar, taus=taus)[0].mean(1)


def _act(pack, eps, step=0, taus=None, x=None, **kw):
    from distributional_rl_decision_and_control_amd.fused_iqn import iqn_act
    x = _inputs()[0] if x is None else x
    out = torch.full((N_ROWS, 2), -1.0, dtype=torch.float64, device="cuda")
    step_dev = torch.full((1,), step, dtype=torch.int64, device="cuda")
    iqn_act(pack, None, out, step_dev, *eps, SEED, taus=taus, obs=x, **kw)
    assert int(step_dev.item()) == step, "the step counter is only read"
    return out


def _groups(lev, rule):
    """(no object, far, linear, floor) row masks of the rule on the inputs."""
    x = _inputs()[0]
    none = x[:, 32] < 0.5
    floor = ~none & (lev == torch.tensor(rule.floor, dtype=torch.float32, device="cuda"))
    far = ~none & (lev == 1.0)
    return none, far, ~(none | far | floor), floor


def test_the_reference_itself_depends_on_the_rule():
    x, _ = _inputs()
    lev = _levels()
    none, far, linear, floor = _groups(lev, _rule())
    assert [int(m.sum()) for m in (none, far, linear, floor)] == [27, 77, 57, 24]
    # the margins to the rule's two boundaries, in f64 on the f32 inputs. The nearest row to `near` is i = 94:
    # rho = 13.278, 0.022 from 13.3 exactly; the inputs are rounded to f32 (ulp 9.5e-7 at 13 m, twice: px and py), so
    # the bound is 0.022 less 4 ulp
    xd = x.double()
    d = torch.sqrt(xd[:, 7] ** 2 + xd[:, 8] ** 2) - xd[:, 11] - 2.8
    margin_near, margin_floor = float((d[~none] - 10.0).abs().min()), float((d[~none] / 10.0 - 0.1).abs().min())
    print(f"closest to near: {margin_near:.6f} m; closest to the floor in level: {margin_floor:.6f}")
    assert margin_near >= 0.022 - 4 * 9.5e-7
    assert margin_floor >= 0.0073
    q, q1 = _reference(True), _reference(False)
    scale = float(q.abs().max())
    top2 = q.topk(2, dim=1).values
    gap = float((top2[:, 0] - top2[:, 1]).min())
    below = lev < 1.0
    moved = float((q - q1)[below].abs().max(1).values.min())
    changed = float((q.argmax(1) != q1.argmax(1)).float().mean())
    print(f"scale {scale:.4f}; top-two gap {gap / scale:.3e} of it; rows below level 1 move by at least "
          f"{moved / scale:.3e} of it; arg-max changes on {100 * changed:.1f} % of the rows")
    assert abs(scale - 0.2226) < 2e-3, scale
    assert gap >= 2.5e-4 * scale
    assert int(below.sum()) == 81
    assert moved >= 1.1e-2 * scale
    assert changed >= 0.08
    assert torch.equal(q[~below], q1[~below]), "level 1 is the risk-neutral reference, bit for bit"
    for i in LINEAR_ROWS:
        assert bool(linear[i]), i


@pytest.mark.parametrize("ops", ["bf16", "f32"])
@pytest.mark.parametrize("kw", [{}, OTHER], ids=["default", "near6_margin1_floor0.25"])
def test_rule(kw, ops):
    """cvar_out against AdaptiveCvar.levels: 1e-6 absolute covers four f32 roundings at the distance's magnitude (at
    most 26 m: ulp 1.9e-6) divided by near; the ends are the constants themselves."""
    rule = _rule(**kw)
    want = rule.levels(_inputs()[0])
    got = torch.full((N_ROWS,), -3.0, device="cuda")
    _act(_pack(ops), EPS_ZERO, taus=_inputs()[1], cvar=rule, cvar_out=got)
    err = float((got - want).abs().max())
    print(f"{ops} {kw}: max |cvar_out - levels| = {err:.3e}")
    assert err <= 1e-6
    none, far, linear, floor = _groups(want, rule)
    assert int(linear.sum()) > 0 and int(floor.sum()) > 0 and int(far.sum()) > 0
    assert bool((got[none | far] == 1.0).all())
    assert bool((got[floor] == torch.tensor(rule.floor, dtype=torch.float32)).all())
    assert bool(((got[linear] > rule.floor) & (got[linear] < 1.0)).all())


@pytest.mark.parametrize("ops", ["bf16", "f32"])
@pytest.mark.parametrize("drawn", [False, True], ids=["given_taus", "drawn_taus_eps0.5"])
def test_adaptive_is_rows(drawn, ops):
    """The adaptive pass is the per-row pass fed the kernel's own levels, bit for bit."""
    pack = _pack(ops)
    kw = dict(eps=EPS_HALF, step=3, step_add=4) if drawn else dict(eps=EPS_ZERO, taus=_inputs()[1])
    lev = torch.zeros(N_ROWS, device="cuda")
    qa = torch.full((N_ROWS, 32), -7.0, device="cuda")
    qr = torch.full((N_ROWS, 32), -7.0, device="cuda")
    a = _act(pack, cvar=_rule(), cvar_out=lev, q_out=qa, **kw)
    echo = torch.zeros(N_ROWS, device="cuda")
    r = _act(pack, cvar=lev, cvar_out=echo, q_out=qr, **kw)
    assert torch.equal(a, r) and torch.equal(qa, qr)
    assert torch.equal(echo, lev), "the rows mode reports the levels it was given"
    assert bool((qa[:, A:] == -7.0).all()) and bool(torch.isfinite(qa[:, :A]).all())
    if drawn:   # another step draws other taus: the offset reaches the draw
        other = _act(pack, EPS_HALF, step=3, step_add=5, cvar=lev)
        assert not torch.equal(other, a)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_rows_are_scalars(ops):
    """Row k of the per-row pass is row k of the scalar pass at float(cvar[k]): every floor row against 0.1, eight
    rows of the linear part each against its own level, every level-1 row against asvrl_iqn_act."""
    pack = _pack(ops)
    taus = _inputs()[1]
    lev = _levels()
    none, far, linear, floor = _groups(lev, _rule())
    q = torch.zeros((N_ROWS, A), device="cuda")
    got = _act(pack, EPS_ZERO, taus=taus, cvar=lev, q_out=q)

    def scalar(cvar):
        qs = torch.zeros((N_ROWS, A), device="cuda")
        return _act(pack, EPS_ZERO, taus=taus, cvar=cvar, q_out=qs), qs

    a, qs = scalar(float(lev[floor][0]))
    assert float(lev[floor][0]) == float(torch.tensor(0.1, dtype=torch.float32))
    assert torch.equal(got[floor], a[floor]) and torch.equal(q[floor], qs[floor])
    for i in LINEAR_ROWS:
        a, qs = scalar(float(lev[i]))
        assert torch.equal(got[i], a[i]) and torch.equal(q[i], qs[i]), i
    a, qs = scalar(1.0)
    one = none | far
    assert torch.equal(q[one], qs[one])
    plain = _act(pack, EPS_ZERO, taus=taus)   # asvrl_iqn_act
    assert torch.equal(got[one], plain[one]) and torch.equal(got[one], a[one])
    # and the level matters on the other rows
    assert not bool((q[~one] == qs[~one]).all(1).any())


@pytest.mark.parametrize("source", ["adaptive", "rows"])
def test_f32_build_against_torch(source):
    """f32 operands, the bars of the scalar test: the action values within 1e-5 of the output scale of
    IQN_Policy.forward(x, 32, levels.view(n, 1, 1), taus), the actions its arg-max on every row."""
    _, taus = _inputs()
    ref = _reference(True)
    scale = float(ref.abs().max())
    q = torch.zeros((N_ROWS, A), device="cuda")
    cvar = _rule() if source == "adaptive" else _levels()
    out = _act(_pack("f32"), EPS_ZERO, taus=taus, cvar=cvar, q_out=q)
    err = float((q - ref).abs().max())
    print(f"{source}: f32 build max |qmean - ref| = {err:.3e} = {err / scale:.3e} of the scale {scale:.4f}")
    assert err <= 1e-5 * scale, (err, scale)
    assert torch.equal(out[:, 0].long(), ref.argmax(1))


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_records(ops):
    """rec_row holds (index, level used) on the rows of stepping envs and its pre-fill elsewhere; the pair the env
    step takes keeps 0.0 (act_pair is the window's: here act_out's column 1 stays unwritten)."""
    pack = _pack(ops)
    mask = torch.ones(N_ROWS // R, dtype=torch.uint8, device="cuda")
    mask[::4] = 0
    mask[16:32] = 0   # a whole workgroup's rows and more
    mask[-1] = 0      # the partial workgroup's last env
    rec = torch.full((N_ROWS, 2), 3.25, dtype=torch.float64, device="cuda")
    lev = torch.zeros(N_ROWS, device="cuda")
    got = _act(pack, EPS_HALF, step=2, cvar=_rule(), cvar_out=lev, actions_rec=rec, env_mask=mask, robots_per_env=R)
    ref = _act(pack, EPS_HALF, step=2, cvar=_rule())
    assert torch.equal(got, ref) and bool((got[:, 1] == -1.0).all())
    on = (mask != 0).repeat_interleave(R)
    assert torch.equal(rec[on, 0], ref[on, 0])
    assert torch.equal(rec[on, 1], lev[on].double()), "the f32 level, widened exactly"
    assert bool((rec[~on] == 3.25).all()), "rows of envs that did not step are not written"
    assert bool((lev > 0).all()), "cvar_out is written for every row, masked or not"
    full = torch.full((N_ROWS, 2), 3.25, dtype=torch.float64, device="cuda")
    _act(pack, EPS_HALF, step=2, cvar=lev, actions_rec=full)
    assert torch.equal(full[:, 0], ref[:, 0]) and torch.equal(full[:, 1], lev.double())


def test_act_pair_keeps_zero():
    """Through the C call: ex.act_pair receives (index, 0.0) while ex.rec_row receives (index, level)."""
    import ctypes as C
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.fused_iqn import _io, risk_struct
    pack = _pack("bf16")
    x, taus = _inputs()
    pair = torch.full((N_ROWS, 2), 5.5, dtype=torch.float64, device="cuda")
    rec = torch.full((N_ROWS, 2), 5.5, dtype=torch.float64, device="cuda")
    lev = torch.zeros(N_ROWS, device="cuda")
    io = _io(None, 32, obs=x, taus=taus)
    _abi.fill_schedule(io, None, EPS_ZERO, SEED)
    ex = _abi.AsvIqnActEx()
    ex.cvar, ex.robots_per_env, ex.act_pair, ex.rec_row = 1.0, 1, pair.data_ptr(), rec.data_ptr()
    risk, _keep = risk_struct(_rule(), N_ROWS, "cuda", lev)
    _abi.check(pack.L.asvrl_iqn_act_risk(C.byref(pack.struct), C.byref(pack.head), C.byref(io), C.byref(ex),
                                         C.byref(risk), None), "asvrl_iqn_act_risk", pack.L)
    want = _act(pack, EPS_ZERO, taus=taus, cvar=_rule())
    assert torch.equal(pair[:, 0], want[:, 0]) and bool((pair[:, 1] == 0.0).all())
    assert torch.equal(rec[:, 0], want[:, 0]) and torch.equal(rec[:, 1], lev.double())
    assert float(lev.min()) < 1.0


def test_refusals():
    pack = _pack("bf16")
    x, taus = _inputs()
    lev = _levels().clone()
    for bad in (0.0, 1.5):
        t = lev.clone()
        t[7] = bad
        with pytest.raises(ValueError, match=r"cvar must be in \(0, 1\]"):
            _act(pack, EPS_ZERO, taus=taus, cvar=t)
    with pytest.raises(ValueError, match="f32"):
        _act(pack, EPS_ZERO, taus=taus, cvar=lev.double())
    with pytest.raises(ValueError, match="185 values"):
        _act(pack, EPS_ZERO, taus=taus, cvar=lev[:-1].contiguous())
    with pytest.raises(ValueError, match="must be on"):
        _act(pack, EPS_ZERO, taus=taus, cvar=lev.cpu())
    from distributional_rl_decision_and_control_amd.fused_iqn import AdaptiveCvar, iqn_act
    with pytest.raises(ValueError, match="floor"):
        AdaptiveCvar(floor=0.0)
    for near in (0.0, -2.0):
        with pytest.raises(ValueError, match="near"):
            AdaptiveCvar(near=near)
    # the rule reads the observation row: precomputed features carry none
    F = torch.zeros(N_ROWS, 256, device="cuda")
    out = torch.zeros((N_ROWS, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="observation rows"):
        iqn_act(pack, F, out, None, *EPS_ZERO, SEED, taus=taus, cvar=AdaptiveCvar())
    with pytest.raises(ValueError, match="cvar_out"):
        _act(pack, EPS_ZERO, taus=taus, cvar=0.5, cvar_out=torch.zeros(N_ROWS, device="cuda"))
    # check_cvar=False skips the host check (graph capture): nothing is read back, the call is launched
    _act(pack, EPS_ZERO, taus=taus, cvar=lev, check_cvar=False)
