"""Shared by the SAC tests: the fixtures (tests/golden/learn_sac_init.npz, learn_sac.npz, captured from the
reference's train_SAC by tools/capture_oracle.py capture_sac), random replay rows shaped as the DDPG tests' and torch
restatements of agent.py:547-595 on the project's SAC_Policy."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import env_oracle as eo

GAMMA = 0.99
ALPHA = 0.078
TWO = [[-1.0, 1.0], [-1.0, 1.0]]
NETS = ("actor", "critic_1", "critic_2")


def golden():
    return np.load(eo.GOLDEN + "/learn_sac_init.npz"), np.load(eo.GOLDEN + "/learn_sac.npz")


def policy(device="cuda", seed=100):
    from distributional_rl_decision_and_control_amd.policy.SAC_model import SAC_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    return SAC_Policy(**DEFAULT_NET, value_ranges_of_action=TWO, device=device, seed=seed)


def load_sd(pol, z, prefix):
    for kind in NETS:
        p = prefix + kind + "/"
        sd = {k[len(p):]: torch.tensor(z[k]) for k in z.files if k.startswith(p)}
        getattr(pol, kind).load_state_dict(sd)   # strict: the reference's keys, all of them and no others


def golden_rows(z, p):
    from distributional_rl_decision_and_control_amd.learn_ops import rows_from_batch
    t = lambda k: torch.tensor(z[p + k], dtype=torch.float32, device="cuda")  # noqa: E731
    return rows_from_batch((t("s_self"), t("s_obj"), t("s_mask")), t("a"), t("r"),
                           (t("ns_self"), t("ns_obj"), t("ns_mask")), t("d"))


def split(x):
    n = x.shape[0]
    return x[:, 0:7], x[:, 7:32].reshape(n, 5, 5), x[:, 32:37]


def obs_rows(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.zeros(n, 40, device="cuda")
    x[:, 0:7] = torch.randn(n, 7, generator=g, device="cuda") * 3
    x[:, 7:32] = torch.randn(n, 25, generator=g, device="cuda") * 3
    x[:, 32:37] = (torch.rand(n, 5, generator=g, device="cuda") > 0.4).float()
    return x


def rows(B, seed, done=0.3, r_std=1.0):
    """Replay rows with random observations and actions in (-1, 1); row 0 sees no object, row 1 all five (in s and
    s')."""
    g = torch.Generator(device="cuda").manual_seed(seed + 1000)
    r = torch.zeros(B, 88, device="cuda")
    r[:, 0:40] = obs_rows(B, seed)
    r[:, 40:80] = obs_rows(B, seed + 500)
    for c in (0, 40):
        r[0, c + 32:c + 37] = 0.0
        r[1, c + 32:c + 37] = 1.0
    r[:, 80:82] = torch.rand(B, 2, generator=g, device="cuda") * 2 - 1
    r[:, 82] = torch.randn(B, generator=g, device="cuda") * r_std
    r[:, 83] = (torch.rand(B, generator=g, device="cuda") < done).float()
    return r


def normals(B, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(B, 2, generator=g, device="cuda")


def cos(x, y):
    x, y = x.reshape(-1).double(), y.reshape(-1).double()
    return float((x @ y) / (x.norm() * y.norm() + 1e-30))


def opts(pol, ops):
    """Three FusedAdam (built before anything caches parameter pointers): actor, [critic_1, critic_2]."""
    from distributional_rl_decision_and_control_amd.learner import FusedAdam
    return (FusedAdam(pol.actor.parameters(), lr=1e-4, operands=ops),
            [FusedAdam(c.parameters(), lr=1e-4, operands=ops) for c in (pol.critic_1, pol.critic_2)])


def flat_grads(pol):
    from distributional_rl_decision_and_control_amd.learner import FlatGrads
    for kind in NETS:
        FlatGrads(getattr(pol, kind).parameters())


def target_ref(target, r, eps_target):
    """(na, logp', y) of agent.py:556-561 for replay rows r."""
    ns = split(r[:, 40:80])
    with torch.no_grad():
        na, lpn = target.actor(ns, eps=eps_target)
        tv = torch.min(target.critic_1(ns, na), target.critic_2(ns, na)) - ALPHA * lpn
        y = r[:, 82:83] + GAMMA * tv * (1.0 - r[:, 83:84])
    return na, lpn, y


def critic_losses_ref(local, r, y):
    s = split(r[:, 0:40])
    return [F.mse_loss(c(s, r[:, 80:82]), y) for c in (local.critic_1, local.critic_2)]


def actor_loss_ref(local, r, eps_local, actor=None):
    """agent.py:582-587 with the pieces the tests look at: (loss, a, logp, q1, q2)."""
    s = split(r[:, 0:40])
    a, lp = (actor or local.actor)(s, eps=eps_local)
    q1, q2 = local.critic_1(s, a), local.critic_2(s, a)
    return (ALPHA * lp - torch.min(q1, q2)).mean(), a, lp, q1, q2


def own_scale(name, err, ref):
    """The DDPG tests' bar and reasoning: beside 1e-5 of max(1, scale), each tensor is held to 1e-4 of its OWN largest
    reference entry. Both sides are f32: an entry is a sum of at most 256 (layer width) x 160 (rows) products, each
    carrying a few roundings of 2^-24 = 6e-8; even if every rounding of the longer of the two sums lined up,
    (256 + 160) x 6e-8 = 2.5e-5 of the largest entry, under the bar."""
    assert err <= 1e-4 * ref.abs().max().item(), (name, err, ref.abs().max().item())


def check_grads(named, grads_ref):
    for (name, p), gr in zip(named, grads_ref):
        err, scale = (p.grad - gr).abs().max().item(), max(1.0, gr.abs().max().item())
        print(f"  {name}: max abs err {err:.3g}, max |ref| {gr.abs().max().item():.3g}")
        assert err <= 1e-5 * scale, (name, err, scale)
        own_scale(name, err, gr)
