"""GPU: the DQN kernels (csrc/asvrl_dqn.hip, fused_dqn.py) against the reference's own train_DQN / act_dqn outputs
(tests/golden/learn_dqn.npz) and torch-autograd restatements of agent.py:518-545.

The f32 build is held to the bars tests/test_agent_gpu.py holds the torch path to (loss 1e-5, gradient norm 1e-4,
weights rtol 1e-4 / atol 2e-6), gradients to 1e-5 of the gradient scale; the bf16 build to the bars
tests/test_fused_mlp_gpu.py holds the bf16 Actor (the same trunk and operand precision) to, against the f32 build."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import env_oracle as eo

pytestmark = pytest.mark.gpu

GAMMA = 0.99


def _z():
    return np.load(eo.GOLDEN + "/learn_dqn.npz")


def _net(z=None, prefix="init/"):
    from distributional_rl_decision_and_control_amd.policy.DQN_model import DQN_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    net = DQN_Policy(**DEFAULT_NET, action_size=25, device="cuda", seed=100).to("cuda")
    if z is not None:
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(torch.tensor(z[prefix + k]))
    return net


def _golden_rows(z, p):
    from distributional_rl_decision_and_control_amd.learn_ops import rows_from_batch
    t = lambda k: torch.tensor(z[p + k], dtype=torch.float32, device="cuda")  # noqa: E731
    return rows_from_batch((t("s_self"), t("s_obj"), t("s_mask")), t("a").view(-1, 1), t("r"),
                           (t("ns_self"), t("ns_obj"), t("ns_mask")), t("d"))


def _split(x):
    n = x.shape[0]
    return x[:, 0:7], x[:, 7:32].reshape(n, 5, 5), x[:, 32:37]


def _obs_rows(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.zeros(n, 40, device="cuda")
    x[:, 0:7] = torch.randn(n, 7, generator=g, device="cuda") * 3
    x[:, 7:32] = torch.randn(n, 25, generator=g, device="cuda") * 3
    x[:, 32:37] = (torch.rand(n, 5, generator=g, device="cuda") > 0.4).float()
    return x


def _rows(B, seed, done=0.3, r_std=1.0):
    """Replay rows with random observations; row 0 sees no object, row 1 all five (in s and s')."""
    g = torch.Generator(device="cuda").manual_seed(seed + 1000)
    rows = torch.zeros(B, 88, device="cuda")
    rows[:, 0:40] = _obs_rows(B, seed)
    rows[:, 40:80] = _obs_rows(B, seed + 500)
    for c in (0, 40):
        rows[0, c + 32:c + 37] = 0.0
        rows[1, c + 32:c + 37] = 1.0
    rows[:, 80] = torch.randint(0, 25, (B,), generator=g, device="cuda").float()
    rows[:, 82] = torch.randn(B, generator=g, device="cuda") * r_std
    rows[:, 83] = (torch.rand(B, generator=g, device="cuda") < done).float()
    return rows


def _cos(x, y):
    x, y = x.reshape(-1).double(), y.reshape(-1).double()
    return float((x @ y) / (x.norm() * y.norm() + 1e-30))


def _cmp_sd(module, z, prefix):
    for k, v in module.state_dict().items():
        np.testing.assert_allclose(v.detach().cpu().numpy(), z[prefix + k], rtol=1e-4, atol=2e-6, err_msg=prefix + k)


def _ref_loss(local, target, rows):
    s, ns = _split(rows[:, 0:40]), _split(rows[:, 40:80])
    with torch.no_grad():
        q_next = target(ns).max(dim=1, keepdim=True)[0]
        y = rows[:, 82:83] + (1 - rows[:, 83:84]) * GAMMA * q_next
    q = local(s).gather(1, rows[:, 80:81].long())
    return F.smooth_l1_loss(q, y), (q - y).detach()


# ------------------------------------------------------------------ the reference's two steps
def test_golden_update_f32():
    from distributional_rl_decision_and_control_amd.fused_dqn import FusedDQNState, dqn_update_fused
    from distributional_rl_decision_and_control_amd.learner import FusedAdam
    z = _z()
    local, target = _net(), _net()
    for k, v in local.state_dict().items():
        np.testing.assert_array_equal(v.cpu().numpy(), z["init/" + k])
    opt = FusedAdam(local.parameters(), lr=1e-4, operands="f32")
    st = FusedDQNState(local, target, 64, "f32")
    for step in range(2):
        loss, gn = dqn_update_fused(st, local, opt, opt.grads, _golden_rows(z, f"step{step}/"), gamma=GAMMA)
        print(f"step {step}: loss {loss.item():.9g} ref {float(z[f'step{step}/loss']):.9g}; "
              f"grad norm {gn.item():.9g} ref {float(z[f'step{step}/grad_norms'][0]):.9g}")
        np.testing.assert_allclose(loss.item(), z[f"step{step}/loss"], rtol=1e-5)
        np.testing.assert_allclose(gn.item(), z[f"step{step}/grad_norms"][0], rtol=1e-4)
    _cmp_sd(local, z, "after1/")


def test_agent_fused_learner_golden():
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.fused_dqn import FusedDQNState
    from distributional_rl_decision_and_control_amd.learner import FusedAdam
    from distributional_rl_decision_and_control_amd.learn_ops import split_rows
    z = _z()
    ag = Agent(seed=100, agent_type="DQN")
    assert ag.learner == "torch" and isinstance(ag.optimizer, torch.optim.Adam)   # the default did not change
    ag.set_learner("fused-f32")
    assert isinstance(ag.optimizer, FusedAdam)
    for step in range(2):
        b = split_rows(_golden_rows(z, f"step{step}/"))
        ag.memory.sample = (lambda b=b: b)
        loss = ag.train()
        np.testing.assert_allclose(loss, z[f"step{step}/loss"], rtol=1e-5)
    assert isinstance(ag._fused[1], FusedDQNState)
    _cmp_sd(ag.policy_local, z, "after1/")
    st = (z["act/state_self"].tolist(), z["act/state_obj"].tolist())
    assert ag.act_dqn(st, eps=0.0) == int(z["act/action"])
    ag.soft_update()   # re-packs the target images of the fused state
    ag.set_learner("torch")
    assert isinstance(ag.optimizer, torch.optim.Adam) and ag._fused is None


def test_agent_unsupported_batch_warns_and_falls_back():
    """B = 48 is not a shape the kernels take: a fused learner says so and runs the autograd update with its fused
    optimiser, which follows the torch learner's step."""
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.learn_ops import split_rows
    b = split_rows(_rows(48, seed=3))
    ag, ref = Agent(seed=100, agent_type="DQN"), Agent(seed=100, agent_type="DQN")
    ag.set_learner("fused-f32")
    ag.memory.sample = ref.memory.sample = (lambda: b)
    with pytest.warns(RuntimeWarning, match="torch-autograd"):
        loss = ag.train()
    assert ag._fused[1] is None
    np.testing.assert_allclose(loss, ref.train(), rtol=1e-5)
    for (n, p), q in zip(ag.policy_local.named_parameters(), ref.policy_local.parameters()):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=1e-4, atol=2e-6, err_msg=n)


# ------------------------------------------------------------------ gradients against autograd
@pytest.mark.parametrize("B", [32, 96])
@pytest.mark.parametrize("case", ["linear", "quadratic"])
def test_gradients_match_autograd_f32(B, case):
    """linear: the seeded nets (|Q| ~ 17) against a target whose output bias is 1e6: every non-terminal row sits far
    in the linear branch, every d = 1 row must not see the bias. quadratic: output layers scaled by 0.01, every row
    terminal (y = r) under the same 1e6 target bias: |q - y| < 1 on most rows, and the bias must not reach the loss."""
    from distributional_rl_decision_and_control_amd.fused_dqn import FusedDQNState, dqn_grads
    from distributional_rl_decision_and_control_amd.learner import FlatGrads
    local, target = _net(), _net()
    with torch.no_grad():
        if case == "quadratic":
            for n in (local, target):
                n.output_layer.weight.mul_(0.01)
                n.output_layer.bias.mul_(0.01)
        target.output_layer.bias.add_(1e6)
    rows = _rows(B, seed=B, done=1.0 if case == "quadratic" else 0.3, r_std=0.4 if case == "quadratic" else 1.0)
    assert rows[0, 32:37].sum() == 0 and rows[1, 32:37].sum() == 5 and bool((rows[:, 83] == 1).any())
    ref = copy.deepcopy(local)
    loss_ref, diff = _ref_loss(ref, target, rows)
    if case == "quadratic":
        assert bool((diff.abs() < 1).any()) and loss_ref.item() < 10.0
    else:
        assert bool((diff.abs() >= 1).any())
    grads_ref = torch.autograd.grad(loss_ref, list(ref.parameters()))
    FlatGrads(local.parameters())
    st = FusedDQNState(local, target, B, "f32")
    dqn_grads(st, local, rows, GAMMA)
    torch.cuda.synchronize()
    print(f"{case} B={B}: loss {st.loss.item():.9g} ref {loss_ref.item():.9g}")
    np.testing.assert_allclose(st.loss.item(), loss_ref.item(), rtol=1e-5)
    for (name, p), gr in zip(local.named_parameters(), grads_ref):
        err, scale = (p.grad - gr).abs().max().item(), max(1.0, gr.abs().max().item())
        print(f"  {name}: max abs err {err:.3g}, max |ref| {gr.abs().max().item():.3g}")
        assert err <= 1e-5 * scale, (name, err, scale)
    # dQ: exactly zero off the chosen action (the padded columns included), clamp(q - y, -1, 1) / B on it
    a = rows[:, 80].long()
    dz = st.dz_out.float()
    on = torch.zeros_like(dz, dtype=torch.bool)
    on[torch.arange(B, device="cuda"), a] = True
    assert bool((dz[~on] == 0).all())
    torch.testing.assert_close(dz[on], diff.reshape(-1).clamp(-1, 1) / B, rtol=1e-4, atol=1e-9)
    # terminal rows: the target is the reward alone
    d1 = rows[:, 83] == 1
    torch.testing.assert_close((st.q_sel - diff.reshape(-1))[d1], rows[:, 82][d1], rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------ padding and ties
def _bias_only(bias):
    net = _net()
    with torch.no_grad():
        net.output_layer.weight.zero_()
        net.output_layer.bias.copy_(torch.as_tensor(bias, device="cuda", dtype=torch.float32))
    return net


def _greedy(pack_or_state, x, q_out=None):
    out = torch.full((x.shape[0], 2), -7.0, dtype=torch.float64, device="cuda")
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    pack_or_state.act(x, out, step, 1, 1e6, 0.25, 0.0, 0.0, 3, q_out=q_out)
    torch.cuda.synchronize()
    assert bool((out[:, 1] == 0).all())
    return out[:, 0].long()


@pytest.mark.parametrize("ops", ["f32", "bf16"])
def test_padded_columns_never_win(ops):
    """Zero output weights and biases of -5: every real Q is -5, the seven padded columns hold 0. q_next must be -5
    and no row may pick an index >= 25."""
    from distributional_rl_decision_and_control_amd.fused_dqn import FusedDQNState, dqn_grads
    from distributional_rl_decision_and_control_amd.learner import FlatGrads
    local, target = _bias_only([-5.0] * 25), _bias_only([-5.0] * 25)
    FlatGrads(local.parameters())
    st = FusedDQNState(local, target, 64, ops)
    rows = _rows(64, seed=7)
    dqn_grads(st, local, rows, GAMMA)
    torch.cuda.synchronize()
    assert bool((st.q_next == -5.0).all()) and bool((st.q_sel == -5.0).all())
    assert bool((st.dz_out[:, 25:] == 0).all())
    x = _obs_rows(100, 9)   # not a multiple of the tile: the last tile is partial
    q = torch.zeros(100, 25, device="cuda")
    a = _greedy(st, x, q)
    assert bool((a < 25).all()) and bool((a == 0).all()) and bool((q == -5.0).all())


@pytest.mark.parametrize("ops", ["f32", "bf16"])
def test_ties_go_to_the_lowest_index(ops):
    from distributional_rl_decision_and_control_amd.fused_dqn import DqnPack, dqn_act
    x = _obs_rows(64, 11)
    for bias, want in (([0.25] * 25, 0), ([1.0 if k in (7, 19) else -1.0 for k in range(25)], 7),
                       ([1.0 if k in (19, 24) else 0.5 for k in range(25)], 19)):
        pack = DqnPack(_bias_only(bias), ops)
        out = torch.zeros(64, 2, dtype=torch.float64, device="cuda")
        dqn_act(pack, x, out, None, 1, 1e6, 0.25, 0.0, 0.0, 3)
        assert bool((out[:, 0] == want).all()), (bias, want)
        assert int(np.argmax(np.asarray(bias, dtype=np.float32))) == want


# ------------------------------------------------------------------ act
def _golden_obs(z):
    return torch.cat([_golden_rows(z, p)[:, c:c + 40] for p in ("step0/", "step1/") for c in (0, 40)]).contiguous()


def test_act_greedy_f32_matches_torch():
    from distributional_rl_decision_and_control_amd.fused_dqn import DqnPack
    z = _z()
    net = _net()
    x = _golden_obs(z)
    assert x.shape == (256, 40)
    with torch.no_grad():
        q_ref = net(_split(x))
    pack = DqnPack(net, "f32")
    q = torch.zeros(256, 25, device="cuda")
    a = _greedy(_PackAct(pack), x, q)
    assert torch.equal(a, q_ref.argmax(1))   # every row: the smallest top-2 gap of this set is 5.3e-3
    assert (q - q_ref).abs().max().item() <= 1e-5 * q_ref.abs().max().item()
    assert torch.equal(a, q.argmax(1))
    # the reference's act_dqn state (two objects) under the weights it acted with
    net2 = _net(z, "after1/")
    row = torch.zeros(1, 40, device="cuda")
    row[0, 0:7] = torch.tensor(z["act/state_self"], dtype=torch.float32)
    row[0, 7:17] = torch.tensor(z["act/state_obj"], dtype=torch.float32).reshape(-1)
    row[0, 32:34] = 1.0
    q1 = torch.zeros(1, 25, device="cuda")
    a1 = _greedy(_PackAct(DqnPack(net2, "f32")), row, q1)
    assert int(a1[0]) == int(z["act/action"])
    np.testing.assert_allclose(q1.cpu().numpy(), z["act/q"], rtol=1e-4, atol=1e-4)


class _PackAct:
    """A DqnPack behind FusedDQNState.act's signature."""

    def __init__(self, pack):
        self.pack = pack

    def act(self, *a, **kw):
        from distributional_rl_decision_and_control_amd.fused_dqn import dqn_act
        dqn_act(self.pack, *a, **kw)


@pytest.mark.parametrize("ops", ["f32", "bf16"])
def test_action_is_argmax_of_q_out(ops):
    from distributional_rl_decision_and_control_amd.fused_dqn import DqnPack
    x = torch.cat([_golden_obs(_z()), _obs_rows(77, 5)])   # 333 rows: a partial last tile
    q = torch.zeros(x.shape[0], 25, device="cuda")
    a = _greedy(_PackAct(DqnPack(_net(), ops)), x, q)
    assert torch.equal(a, q.argmax(1))


def test_act_exploring():
    """20,480 rows at a pinned epsilon. A row whose action differs from its greedy one explored; an exploring row
    draws the greedy action itself with probability 1/25."""
    from distributional_rl_decision_and_control_amd.fused_dqn import DqnPack, dqn_act
    n = 20480
    x = _obs_rows(n, 21)
    pack = DqnPack(_net(), "bf16")
    step = torch.zeros(1, dtype=torch.int64, device="cuda")

    def run(eps, p=pack, s=step):
        out = torch.zeros(n, 2, dtype=torch.float64, device="cuda")
        dqn_act(p, x, out, s, 4096, 6e6, 0.25, eps, eps, 5)
        torch.cuda.synchronize()
        assert bool(((out[:, 0] >= 0) & (out[:, 0] < 25) & (out[:, 1] == 0)).all())
        return out[:, 0].long()

    greedy = run(0.0)
    assert torch.equal(run(0.0), greedy)   # epsilon 0 explores no row
    a = run(0.6)
    share = (a != greedy).float().mean().item() * 25.0 / 24.0
    assert abs(share - 0.6) < 0.02, share
    p = 0.6 / 25.0
    for k in range(25):   # action k among the rows whose greedy action is another one: only explorers pick it
        rk = greedy != k
        m = int(rk.sum())
        cnt = int((a[rk] == k).sum())
        assert abs(cnt - m * p) < 5.0 * np.sqrt(m * p * (1 - p)), (k, cnt, m * p)
    # epsilon 1: every row explores -- the draw does not depend on the network at all
    a1 = run(1.0)
    assert torch.equal(a1, run(1.0, p=DqnPack(_bias_only([0.0] * 24 + [1.0]), "bf16")))
    assert abs((a1 != greedy).float().mean().item() * 25.0 / 24.0 - 1.0) < 0.02
    # another step-counter value: other draws
    a2 = run(1.0, s=torch.ones(1, dtype=torch.int64, device="cuda"))
    assert (a2 != a1).float().mean().item() > 0.9


# ------------------------------------------------------------------ bf16 build against the f32 build
def test_bf16_q_and_gradients_track_f32():
    from distributional_rl_decision_and_control_amd.fused_dqn import FusedDQNState, dqn_grads
    from distributional_rl_decision_and_control_amd.learner import FlatGrads
    B = 512
    rows = _rows(B, seed=31)
    res = {}
    for ops in ("f32", "bf16"):
        local, target = _net(), _net()
        FlatGrads(local.parameters())
        st = FusedDQNState(local, target, B, ops)
        dqn_grads(st, local, rows, GAMMA)
        q = torch.zeros(B, 25, device="cuda")
        _greedy(st, rows[:, 0:40], q)
        res[ops] = (q, [p.grad.clone() for p in local.parameters()], st.loss.item())
    qf, gf, lf = res["f32"]
    qb, gb, lb = res["bf16"]
    assert (qb - qf).abs().max().item() < 2e-2 * qf.abs().max().item()
    np.testing.assert_allclose(lb, lf, rtol=3e-2, atol=2e-3)
    for (name, _), a, b in zip(_net().named_parameters(), gb, gf):
        c, ratio = _cos(a, b), a.norm().item() / max(b.norm().item(), 1e-30)
        print(f"  {name}: cosine {c:.5f}, norm ratio {ratio:.4f}")
        assert c > 0.99 and abs(ratio - 1) < 0.05, (name, c, ratio)


def test_bf16_ten_updates_track_f32():
    from distributional_rl_decision_and_control_amd.fused_dqn import FusedDQNState, dqn_update_fused
    from distributional_rl_decision_and_control_amd.learner import FusedAdam
    B = 512
    runs = {}
    for ops in ("f32", "bf16"):
        local, target = _net(), _net()
        opt = FusedAdam(local.parameters(), lr=1e-4, operands=ops)
        st = FusedDQNState(local, target, B, ops)
        losses = [dqn_update_fused(st, local, opt, opt.grads, _rows(B, seed=100 + k), gamma=GAMMA)[0].item()
                  for k in range(10)]
        runs[ops] = (losses, {n: p.detach().clone() for n, p in local.named_parameters()})
    np.testing.assert_allclose(runs["bf16"][0], runs["f32"][0], rtol=3e-2, atol=2e-3)
    init = dict(_net().named_parameters())
    for n, p in runs["f32"][1].items():
        c = _cos(runs["bf16"][1][n] - init[n].detach(), p - init[n].detach())
        assert c > 0.9, (n, c)


# ------------------------------------------------------------------ graph capture
@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_captured_update_equals_eager(ops):
    """One captured dqn_update_fused replayed twice from a restored state equals two eager calls bit for bit:
    parameters, Adam moments, step count, weight images, loss."""
    from distributional_rl_decision_and_control_amd.fused_dqn import FusedDQNState, dqn_update_fused
    from distributional_rl_decision_and_control_amd.learner import FusedAdam
    B = 64
    rows = _rows(B, seed=41)

    def make():
        local, target = _net(), _net()
        opt = FusedAdam(local.parameters(), lr=1e-4, operands=ops)
        return local, opt, FusedDQNState(local, target, B, ops)

    def state(opt, st):
        t = st.local.sets[0]
        return [opt.flat, opt.exp_avg, opt.exp_avg_sq, opt.step_t, st.loss] + \
            [t[k] for k in ("enc", "b_enc", "w1", "w1t", "w2", "w2t", "head")]

    la, oa, sa = make()
    for _ in range(2):
        dqn_update_fused(sa, la, oa, oa.grads, rows, gamma=GAMMA)
    torch.cuda.synchronize()
    lb, ob, sb = make()
    saved = [t.clone() for t in state(ob, sb)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dqn_update_fused(sb, lb, ob, ob.grads, rows, gamma=GAMMA)   # warm-up
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dqn_update_fused(sb, lb, ob, ob.grads, rows, gamma=GAMMA)
    for t, s in zip(state(ob, sb), saved):
        t.copy_(s)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert ob.step_t.item() == 2.0
    for k, (x, y) in enumerate(zip(state(oa, sa), state(ob, sb))):
        assert torch.equal(x, y), k
    assert not torch.equal(saved[0], ob.flat)
