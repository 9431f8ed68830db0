"""GPU: the window form of the IQN act pass (asvrl_iqn_act_ex, critic kernel mode IQN_ACT_EX) against
asvrl_iqn_act (bit for bit at cvar = 1, step_add = 0), against itself under a step offset, against
policy_actions_kernel's record semantics, and -- its CVaR distortion and action values -- against
IQN_Policy.forward(x, 32, cvar, taus=taus) in torch fp32.

n = 185 rows = 37 envs x 5 robots: 185 tiles, so the last 16-wave workgroup is partial. The CVaR inputs come from the
CPU generator (seed 5), where they were checked: the reference's output scale is 0.182; at cvar 1, 0.5, 0.25 and 0.1
no row's two best action values are closer than 1e-4 of the scale (so the f32 build must agree with the reference
arg-max on every row); every row's values move by more than 2 % of the scale between cvar = 1 and the three others;
the reference arg-max changes on 19.5 %, 20.5 % and 23.8 % of the rows."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

A = 25
N_ROWS, R = 185, 5
SEED = 99
EPS_HALF = (1.0, 1.0, 1.0, 0.5, 0.5)
EPS_ZERO = (1.0, 1.0, 1.0, 0.0, 0.0)
CVARS = (1.0, 0.5, 0.25, 0.1)


@functools.lru_cache(maxsize=None)
def _net():
    from distributional_rl_decision_and_control_amd.policy.IQN_model import IQN_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    return IQN_Policy(**DEFAULT_NET, action_size=A, device="cuda", seed=100).cuda()


@functools.lru_cache(maxsize=None)
def _pack(operands="bf16"):
    from distributional_rl_decision_and_control_amd.fused_iqn import IqnPack
    return IqnPack(_net(), operands)


def _obs_rows(n, g, ld=40):
    """tests/test_fused_iqn_gpu.py's rows, drawn on the CPU generator g."""
    x = torch.zeros(n, ld)
    x[:, 0:7] = torch.randn(n, 7, generator=g) * 3
    x[:, 7:32] = torch.randn(n, 25, generator=g) * 3
    x[:, 32:37] = (torch.rand(n, 5, generator=g) > 0.4).float()
    return x


def _split(x):
    n = x.shape[0]
    return x[:, 0:7], x[:, 7:32].reshape(n, 5, 5), x[:, 32:37]


@functools.lru_cache(maxsize=None)
def _inputs():
    g = torch.Generator().manual_seed(5)
    x = _obs_rows(N_ROWS, g)
    taus = torch.rand(N_ROWS, 32, generator=g)
    return x.cuda(), taus.cuda()


@functools.lru_cache(maxsize=None)
def _reference(cvar):
    """quantiles.mean(dim=1) of IQN_Policy.forward at this cvar, torch fp32: [n, A]."""
    x, taus = _inputs()
    with torch.no_grad():
        return _net()(_split(x), 32, cvar, taus=taus)[0].mean(1)


def _act(pack, eps, step=0, taus=None, **kw):
    from distributional_rl_decision_and_control_amd.fused_iqn import iqn_act
    x, _ = _inputs()
    out = torch.full((N_ROWS, 2), -1.0, dtype=torch.float64, device="cuda")
    step_dev = torch.full((1,), step, dtype=torch.int64, device="cuda")
    iqn_act(pack, None, out, step_dev, *eps, SEED, taus=taus, obs=x, **kw)
    assert int(step_dev.item()) == step, "the step counter is only read"
    return out


@pytest.mark.parametrize("ops", ["bf16", "f32"])
@pytest.mark.parametrize("eps", [EPS_ZERO, EPS_HALF], ids=["greedy", "eps0.5"])
@pytest.mark.parametrize("inject", [True, False], ids=["given_taus", "drawn_taus"])
def test_unchanged_at_the_defaults(inject, eps, ops):
    """cvar = 1 and step_add = 0 through the new entry (taken because q_out is set): asvrl_iqn_act's bits."""
    pack = _pack(ops)
    taus = _inputs()[1] if inject else None
    old = _act(pack, eps, step=3, taus=taus)
    q = torch.full((N_ROWS, 32), -7.0, device="cuda")
    new = _act(pack, eps, step=3, taus=taus, q_out=q)
    assert torch.equal(new, old)
    assert bool((new[:, 1] == -1.0).all()), "act_out's column 1 is not written (ld_act = 2)"
    assert bool((q[:, A:] == -7.0).all()), "columns >= n_actions are not written"
    assert bool(torch.isfinite(q[:, :A]).all()) and bool((q[:, :A] != -7.0).all())
    if eps is EPS_ZERO:   # the action is the first arg-max of the values the kernel reports
        assert torch.equal(new[:, 0].long(), q[:, :A].argmax(1))
    else:                 # epsilon 0.5: both branches are taken
        share = float((new[:, 0].long() == q[:, :A].argmax(1)).float().mean())
        assert 0.25 <= share <= 0.75, share


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_step_offset(ops):
    """(step_dev = s, step_add = t) is (step_dev = s + t, step_add = 0): drawn taus, epsilon 0.5."""
    pack = _pack(ops)
    outs = []
    for s, t in ((7, 5), (12, 0), (0, 12)):
        outs.append(_act(pack, EPS_HALF, step=s, step_add=t) if t else _act(pack, EPS_HALF, step=s))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[1])
    other = _act(pack, EPS_HALF, step=7, step_add=4)
    assert not torch.equal(other, outs[0]), "another step draws other taus and exploration"


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_record_row_semantics(ops):
    """The record row holds (index, 0.0) for every robot slot of a stepping env and keeps its pre-fill behind a
    masked env: what policy_actions_kernel copies out of the step's action buffer."""
    pack = _pack(ops)
    mask = torch.ones(N_ROWS // R, dtype=torch.uint8, device="cuda")
    mask[::4] = 0
    mask[16:32] = 0   # a whole workgroup's rows and more
    mask[-1] = 0      # the partial workgroup's last env
    rec = torch.full((N_ROWS, 2), 3.25, dtype=torch.float64, device="cuda")
    got = _act(pack, EPS_HALF, step=2, actions_rec=rec, env_mask=mask, robots_per_env=R)
    ref = _act(pack, EPS_HALF, step=2)
    assert torch.equal(got, ref)
    on = (mask != 0).repeat_interleave(R)
    assert torch.equal(rec[on, 0], ref[on, 0]) and bool((rec[on, 1] == 0.0).all())
    assert bool((rec[~on] == 3.25).all()), "rows of envs that did not step are not written"
    full = torch.full((N_ROWS, 2), 3.25, dtype=torch.float64, device="cuda")
    _act(pack, EPS_HALF, step=2, actions_rec=full)
    assert torch.equal(full[:, 0], ref[:, 0]) and bool((full[:, 1] == 0.0).all())


def test_the_reference_itself_depends_on_cvar():
    """The inputs were chosen so that a kernel that ignores cvar cannot pass: the reference's own arg-max changes on
    at least 10 % of the rows between cvar = 1 and 0.25, and no row's top-two gap is below 1e-4 of the scale."""
    q1, q4 = _reference(1.0), _reference(0.25)
    assert float((q1.argmax(1) != q4.argmax(1)).float().mean()) >= 0.10
    assert abs(float(q1.abs().max()) - 0.182) < 2e-3
    for cvar in CVARS:
        q = _reference(cvar)
        top2 = q.topk(2, dim=1).values
        assert float((top2[:, 0] - top2[:, 1]).min()) >= 1e-4 * float(q.abs().max()), cvar
        if cvar != 1.0:
            assert float((q - q1).abs().max(1).values.min()) > 2e-2 * float(q1.abs().max()), cvar


@pytest.mark.parametrize("cvar", CVARS)
def test_cvar_f32_build_against_torch(cvar):
    """f32 operands: the action values within 1e-5 of the output scale, the actions the reference arg-max on every
    row."""
    _, taus = _inputs()
    ref = _reference(cvar)
    scale = float(ref.abs().max())
    q = torch.zeros((N_ROWS, A), device="cuda")
    out = _act(_pack("f32"), EPS_ZERO, taus=taus, cvar=cvar, q_out=q)
    err = float((q - ref).abs().max())
    print(f"cvar={cvar}: f32 build max |qmean - ref| = {err:.3e} = {err / scale:.3e} of the scale {scale:.4f}")
    assert err <= 1e-5 * scale, (err, scale)
    assert torch.equal(out[:, 0].long(), ref.argmax(1))


@pytest.mark.parametrize("cvar", CVARS)
def test_cvar_bf16_build_against_torch(cvar):
    """bf16 operands, the bars of tests/test_fused_iqn_gpu.py: values within 2 % of the output scale, the chosen
    action's mean within 1e-2 of the scale of the reference's best."""
    _, taus = _inputs()
    ref = _reference(cvar)
    scale = float(ref.abs().max())
    q = torch.zeros((N_ROWS, A), device="cuda")
    out = _act(_pack("bf16"), EPS_ZERO, taus=taus, cvar=cvar, q_out=q)
    err = float((q - ref).abs().max())
    act = out[:, 0].long()
    gap = float((ref.max(1).values - ref.gather(1, act.view(-1, 1)).squeeze(1)).max())
    print(f"cvar={cvar}: bf16 build max |qmean - ref| = {err / scale:.3e} of the scale, chosen-action gap "
          f"{gap / scale:.3e} of the scale")
    assert err <= 2e-2 * scale, (err, scale)
    assert gap <= 1e-2 * scale, (gap, scale)
    assert torch.equal(act, q.argmax(1))


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_cvar_applies_to_drawn_taus_too(ops):
    """Drawn taus at cvar = 0.25 differ from cvar = 1 (same step, same draws), and cvar reaches both tau sources."""
    pack = _pack(ops)
    q1 = torch.zeros((N_ROWS, A), device="cuda")
    q4 = torch.zeros((N_ROWS, A), device="cuda")
    a1 = _act(pack, EPS_ZERO, step=3, q_out=q1)
    a4 = _act(pack, EPS_ZERO, step=3, cvar=0.25, q_out=q4)
    assert float((a1[:, 0] != a4[:, 0]).float().mean()) >= 0.05
    assert float((q1 - q4).abs().max(1).values.min()) > 0.0
