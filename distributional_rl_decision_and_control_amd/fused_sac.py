"""The SAC update (Agent.train_SAC, agent.py:547-595) and act_sac (agent.py:289-306) on the gfx950 kernels of
csrc/asvrl_sac.hip, csrc/asvrl_wgrad.hip and csrc/asvrl_optim.hip.

SAC_model.Critic is DDPG_model.Critic, so each twin is a fused_ddpg.DdpgCriticPack on the one-scalar critic tile.
SAC_model.Actor is the Actor's trunk under a mean and a log-standard-deviation head; its pack is the Actor's image
set plus the f32 head. Per step, on a replay batch `rows` ([B][88]: obs | next obs | action | reward | done):

    local actor(s) saving activations -> a_pi, logp; target actor(s') -> na, logp_next   asvrl_sac_actor_forward
  critics (agent.py:556-579)
    local 1, 2 on (s, a) (activations kept), target 1, 2 on (s', na)      asvrl_sac_grad, launch 1
    y = r + gamma (1 - d) (min q_next - alpha logp_next), both MSE losses, dq and backwards
                                                                          asvrl_sac_grad, launch 2
    per critic: weight-gradient partials of its five layers               asvrl_linear_wgrad_multi
                every .grad (encoders folded), its loss and ITS OWN gradient norm   asvrl_partial_sums_norm
                clip + Adam + re-pack of its weight images                asvrl_adam_step_pack
  actor (agent.py:582-593), through the UPDATED critics
    Q1, Q2(s, a_pi); each critic's share of d(-min)/da                    asvrl_sac_actor_grad (two launches)
    the head's backward, dz2, dz1, dz0, the actor-loss partials           asvrl_sac_actor_backward
    weight-gradient partials (the head as four 128-vectors)               asvrl_linear_wgrad_multi
    every actor .grad, the actor loss, the norm                           asvrl_partial_sums_norm
    clip + Adam + re-pack                                                 asvrl_adam_step_pack

Fifteen launches from given rows, sixteen with the replay draw; no host synchronisation, no torch autograd. The noise
is given by the caller (eps_target / eps_local, the parity tests) or drawn in the kernels by Philox on the device
learn counter, so nothing depends on the host RNG and the update is capturable in a HIP graph.

The closed-loop windows (csrc/asvrl_env.hip, asvrl_sac_rollout / asvrl_sac_rollout_ar) run act_sac inside the env
kernel from a SacActorPack: the head, its noise and its sample live in csrc/asvrl_sac_tile.h, which both files
include, so a row's action does not depend on which kernel computed it (FusedSACState.window_pack,
DeviceEnvBatch.policy_rollout(..., deterministic=False), DeviceEvaluator.run(..., policy_seed=0, deterministic=False)).

Arithmetic: bf16 MFMA operands with f32 accumulation, f32 master weights / Adam, the head and the sample in f32
(operands="f32": the same kernels from libasvrl_f32.so, the parity build).
"""
import ctypes as C

import torch

from . import _abi
from .fused_critic import PartialArena, arena_floats
from .fused_ddpg import DdpgCriticPack
from .fused_mlp import ENC, HID, OBSK, MlpPack, default_net
from .fused_update import _reduce_and_step
from .learner import target_step

OBS = 40
ALPHA = 0.078   # agent.py:95, fixed
CRITIC_ARRAYS = ("xb", "h0", "h1", "p", "h2", "q", "q_next", "dq", "dz2", "dz1", "dzG", "dz0")


def supported(policy, B):
    """The shapes the kernels take: the default network dims, 2 actions and a batch that is a positive multiple
    of 32."""
    return B >= 32 and B % 32 == 0 and all(default_net(n) and n.action_dimension == 2
                                           for n in (policy.actor, policy.critic_1, policy.critic_2))


class SacActorPack(MlpPack):
    """Packed images of one SAC Actor: the Actor's set (encoder image, both hidden layers and their transposes),
    f32 copies of the hidden biases, and the f32 head -- `head` [4][128] (output_layer_mu.weight, then
    output_layer_log_std.weight) and `bhead` [4]. adam_segments(opt) lets FusedAdam's step write all of it, as
    DdpgCriticPack does for `wo` / `bo`. double=True (the batched loop): two sets, the step writing the one the act
    kernel does not read (MlpPack).

    As a window policy (MlpPack; asvrl_sac_rollout): the rounds are sac_act(pack, obs, act64, eps_out, step, *eps,
    policy_seed) -- the action noise drawn in the kernel on (global row, step, policy_seed) -- and step(act64, ...),
    the act inside the env kernel. deterministic=True (this pack only): the mean action, the rounds'
    sac_act(..., eps_in=zeros); nothing is drawn for the sample, the epsilon schedule still applies."""
    rollout, policy_struct = _abi.ROLLOUTS["sac"]
    takes_deterministic = True
    _policy_w = "sw"

    def __init__(self, net, operands="bf16", double=False):
        super().__init__(net, "actor", operands, double)

    def policy(self, cvar=1.0, deterministic=False):
        pi = super().policy()
        pi.deterministic = int(bool(deterministic))
        return pi

    @staticmethod
    def _make_set(net, kind, operands, copies):
        t = MlpPack._make_set(net, "encoders", operands, False)
        dev = t["enc"].device
        bf = dict(dtype=_abi.operand_dtype(operands), device=dev)
        f = dict(dtype=torch.float32, device=dev)
        for k, n in (("w1", HID * ENC), ("w2", HID * HID), ("w2t", HID * HID), ("w1t", ENC * HID)):
            t[k] = torch.zeros(n, **bf)
        t["b1"], t["b2"] = torch.zeros(HID, **f), torch.zeros(HID, **f)
        t["head"], t["bhead"] = torch.zeros(4 * HID, **f), torch.zeros(4, **f)
        w = t["w"]
        w.w1_frag, w.w2_frag, w.w2t_frag, w.w1t_frag = (t["w1"].data_ptr(), t["w2"].data_ptr(),
                                                       t["w2t"].data_ptr(), t["w1t"].data_ptr())
        w.b1, w.b2 = t["b1"].data_ptr(), t["b2"].data_ptr()
        w.wout, w.bout = t["head"].data_ptr(), t["bhead"].data_ptr()   # the Actor's staging reads two rows
        w.out_scale = float(net.atan_scale.float().item())
        sw = _abi.AsvSacActorWeights()
        sw.trunk = w   # by value: every pointer of the set is in place
        sw.head, sw.bhead = t["head"].data_ptr(), t["bhead"].data_ptr()
        t["sw"] = sw
        return t

    def _f32_copies(self, t):
        """(parameter, its f32 image) pairs of set t behind the MFMA images."""
        n = self.net
        mu, ls = n.output_layer_mu, n.output_layer_log_std
        return ((n.hidden_layer.bias, t["b1"]), (n.hidden_layer_2.bias, t["b2"]),
                (mu.weight, t["head"][:2 * HID]), (ls.weight, t["head"][2 * HID:]),
                (mu.bias, t["bhead"][:2]), (ls.bias, t["bhead"][2:]))

    @property
    def sw(self):
        """The AsvSacActorWeights of the current image set."""
        return self.sets[self.parity]["sw"]

    def adam_segments(self, opt):
        dst = self.parity ^ 1 if self.double else 0
        if dst not in self._segs:
            t = self.sets[dst]
            self._segs[dst] = self._trunk_segments(opt, t) + [opt.pack_seg(p.reshape(-1), img, f32=True)
                                                              for p, img in self._f32_copies(t)]
        return self._segs[dst]

    def refresh(self, stream=None):
        src = self.src()
        for t in self.sets:
            _abi.check(self.L.asvrl_mlp_pack(C.byref(src), C.byref(t["w"]), _abi.stream_ptr(stream)),
                       "asvrl_mlp_pack", self.L)
            with torch.no_grad():
                for p, img in self._f32_copies(t):
                    img.copy_(p.reshape(-1))


class _CriticBufs:
    """One critic's saved activations and backward outputs over B rows."""

    def __init__(self, B, dev, operands):
        bf = dict(dtype=_abi.operand_dtype(operands), device=dev)
        f = dict(dtype=torch.float32, device=dev)
        self.xb = torch.zeros(B, OBSK, **bf)
        self.h0, self.dz0 = torch.zeros(B, ENC, **bf), torch.zeros(B, ENC, **bf)
        self.h1, self.dz1 = torch.zeros(B, HID, **bf), torch.zeros(B, HID, **bf)
        self.h2, self.dz2 = torch.zeros(B, HID, **bf), torch.zeros(B, HID, **bf)
        self.p = torch.zeros(B, HID, **bf)
        self.dzG = torch.zeros(B, HID, **f)
        self.q, self.q_next, self.dq = torch.zeros(B, **f), torch.zeros(B, **f), torch.zeros(B, **f)


class FusedSACState:
    """Packs and buffers of the fused SAC update (allocated once, pointer-stable for graph replay).
    operands="f32": every kernel from libasvrl_f32.so (the parity build; the optimisers must be FusedAdam of the
    same operands). double_actor (the batched loop): two actor image sets, as FusedDDPGState. window_pack and
    eval_pack are the local actor's SacActorPack; policy_pack and actor_pack stay None, so VecTrainer.policy_pack(),
    collect, greedy_episodes and evaluate still refuse a SAC trainer."""

    policy_pack = actor_pack = None

    def __init__(self, policy_local, policy_target, B, operands="bf16", double_actor=False, alpha=ALPHA):
        if not supported(policy_local, B):
            raise ValueError(f"SAC learner kernels: B={B} (a positive multiple of 32), the default network, 2 actions")
        dev = policy_local.actor.output_layer_mu.weight.device
        self.B, self.device, self.operands, self.alpha = B, dev, operands, float(alpha)
        self.local = [DdpgCriticPack(policy_local.critic_1, operands), DdpgCriticPack(policy_local.critic_2, operands)]
        self.target = [DdpgCriticPack(policy_target.critic_1, operands),
                       DdpgCriticPack(policy_target.critic_2, operands)]
        self.actor = self.window_pack = self.eval_pack = SacActorPack(policy_local.actor, operands,
                                                                      double=double_actor)
        self.target_actor = SacActorPack(policy_target.actor, operands)
        self.L = self.actor.L
        bf = dict(dtype=_abi.operand_dtype(operands), device=dev)
        f = dict(dtype=torch.float32, device=dev)
        self.cb = [_CriticBufs(B, dev, operands), _CriticBufs(B, dev, operands)]
        # the actor's pass (AsvSacActorIO)
        self.xb = torch.zeros(B, OBSK, **bf)
        self.h0, self.dz0 = torch.zeros(B, ENC, **bf), torch.zeros(B, ENC, **bf)
        self.h1, self.dz1 = torch.zeros(B, HID, **bf), torch.zeros(B, HID, **bf)
        self.h2, self.dz2 = torch.zeros(B, HID, **bf), torch.zeros(B, HID, **bf)
        for k in ("mu", "ls", "sigma", "z", "a", "eps", "na", "eps_next"):
            setattr(self, k, torch.zeros(B, 2, **f))
        self.logp, self.logp_next, self.y = torch.zeros(B, **f), torch.zeros(B, **f), torch.zeros(B, **f)
        self.dA, self.q_pi, self.dhead = torch.zeros(2, B, 2, **f), torch.zeros(2, B, **f), torch.zeros(4, B, **f)
        self.tile_loss = torch.zeros(3, B // 32, **f)   # critic 1, critic 2, actor
        self.losses = torch.zeros(3, **f)
        self.act_eps = None   # act()'s eps_out, sized at the first call
        layers = ((HID, HID), (HID, ENC), (ENC, OBSK))
        # one arena per network: each reduction forms that network's own squared gradient norm
        self.carena = [PartialArena(arena_floats(self.L, B, layers, 1, small=True), dev, operands) for _ in range(2)]
        self.aarena = PartialArena(arena_floats(self.L, B, layers, 4), dev, operands)

    def target_changed(self):
        """Re-pack the target networks after a hard/soft update (eager, outside graphs)."""
        for p in self.target:
            p.refresh()
        self.target_actor.refresh()

    def target_step(self, tr):
        """The device-side target update behind a learn step (VecTrainer target_update="device"): blend and
        re-pack of the target actor and both target critics, one launch each, predicated on tr's learn counter."""
        target_step(tr, (self.target_actor, self.target[0], self.target[1]))

    def refresh_local(self):
        """Re-pack the local networks after their parameters were loaded (eager, outside graphs)."""
        for p in self.local:
            p.refresh()
        self.actor.refresh()

    def act(self, obs_rows, actions64, step_dev, steps_per_count, total, fraction, initial, final, seed, eps_in=None):
        n = obs_rows.shape[0]
        if self.act_eps is None or self.act_eps.shape[0] != n:
            self.act_eps = torch.zeros(n, 2, dtype=torch.float32, device=self.device)
        sac_act(self.actor, obs_rows, actions64, self.act_eps, step_dev, steps_per_count, total, fraction, initial,
                final, seed, eps_in=eps_in)

    def learn(self, tr, state=None, guard=0, actor_wait=None, target_wait=None, actor_done=None):
        """VecTrainer.learn: the draw from tr's ring into tr's buffers (no quantile fractions), then the update on
        tr's optimisers, the noise drawn in the kernels on tr's learn counter."""
        rows = tr.replay.sample(tr.B, seed=tr.seed + 777, counter_dev=tr.learn_counter, out=tr.batch_rows,
                                state=state, guard=guard)
        return sac_update_fused(self, tr.local, tr.actor_opt, tr.critic_opts, rows, gamma=tr.gamma, sync=tr.sync,
                                actor_wait=actor_wait, counter=tr.learn_counter, seed=tr.seed + 999,
                                counter_dev=tr.learn_counter)


def sac_act(pack, x, actions64, eps_out, step_dev, steps_per_count, total, fraction, initial, final, seed, eps_in=None,
            stream=None):
    """act_sac on every row of x (agent.py:289-306) into f64 actions [n][2]: the sampled action, or uniform per
    dimension with the scheduled probability. eps_out [n][2] receives the eps of the sample."""
    assert x.dtype == torch.float32 and x.stride(-1) == 1 and eps_out.shape == (x.shape[0], 2)
    io = _abi.AsvSacActIO()
    io.x, io.ldx, io.n = x.data_ptr(), x.stride(0), x.shape[0]
    io.a_out64, io.eps_out = actions64.data_ptr(), eps_out.data_ptr()
    io.eps_in = eps_in.data_ptr() if eps_in is not None else None
    _abi.fill_schedule(io, step_dev, (steps_per_count, total, fraction, initial, final), seed)
    _abi.check(pack.L.asvrl_sac_act(C.byref(pack.sw), C.byref(io), _abi.stream_ptr(stream)), "asvrl_sac_act", pack.L)


def _actor_io(st, rows=None):
    io = _abi.AsvSacActorIO()
    if rows is not None:
        assert rows.dtype == torch.float32 and rows.shape[0] == st.B and rows.stride(1) == 1
        io.rows, io.ld_rows = rows.data_ptr(), rows.stride(0)
    io.B, io.alpha = st.B, st.alpha
    for k in _abi.SAC_ACTOR_ARRAYS:
        setattr(io, k, (st.tile_loss[2] if k == "tile_loss" else getattr(st, k)).data_ptr())
    return io


def sac_actor_forward(st, rows, eps_target=None, eps_local=None, seed=0, counter=0, counter_dev=None, stream=None):
    """One launch: the local actor on s (activations and the head's values kept in st: mu, ls before the clamp,
    sigma, z, a, eps, logp) and the target actor on s' (st.na, st.logp_next, st.eps_next). eps_* [B][2]: used as
    is; None: drawn in the kernel on (row, counter + counter_dev, seed)."""
    io = _actor_io(st, rows)
    for name, e in (("eps_target_in", eps_target), ("eps_local_in", eps_local)):
        if e is not None:
            assert e.dtype == torch.float32 and e.shape == (st.B, 2) and e.is_contiguous()
            setattr(io, name, e.data_ptr())
    io.seed, io.counter = int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter) & 0xFFFFFFFFFFFFFFFF
    io.counter_dev = counter_dev.data_ptr() if counter_dev is not None else None
    _abi.check(st.L.asvrl_sac_actor_forward(C.byref(st.actor.sw), C.byref(st.target_actor.sw), C.byref(io),
                                            _abi.stream_ptr(stream)), "asvrl_sac_actor_forward", st.L)


def sac_critic_grads(st, policy, rows, gamma=0.99, flush=True, stream=None):
    """train_SAC's critic backwards (agent.py:556-579) for replay rows [B][88], the target action st.na and
    st.logp_next: every .grad of both critics (each one's four observation-encoder gradients contiguous: FusedAdam /
    FlatGrads), st.losses[0:2], st.y. flush=False leaves each critic's weight-gradient partials queued on its
    arena (the update reduces them together with that critic's gradient norm)."""
    assert rows.dtype == torch.float32 and rows.shape[0] == st.B and rows.stride(1) == 1
    io = _abi.AsvSacGradIO()
    for k, cb in enumerate(st.cb):
        c = io.c[k]
        c.rows, c.ld_rows, c.B, c.gamma = rows.data_ptr(), rows.stride(0), st.B, float(gamma)
        c.na, c.ld_na = st.na.data_ptr(), st.na.stride(0)
        for name in CRITIC_ARRAYS:
            setattr(c, name, getattr(cb, name).data_ptr())
        c.tile_loss = st.tile_loss[k].data_ptr()
    io.logp_next, io.y, io.alpha = st.logp_next.data_ptr(), st.y.data_ptr(), st.alpha
    _abi.check(st.L.asvrl_sac_grad(C.byref(st.local[0].dw), C.byref(st.local[1].dw), C.byref(st.target[0].dw),
                                   C.byref(st.target[1].dw), C.byref(io), _abi.stream_ptr(stream)),
               "asvrl_sac_grad", st.L)
    for k, critic in enumerate((policy.critic_1, policy.critic_2)):
        arena, cb, ae = st.carena[k], st.cb[k], critic.action_encoder[0]
        with arena.batch():   # every layer in one launch; every .grad is overwritten (no zeroing)
            arena.vec(cb.dq, cb.h2, critic.output_layer.weight.grad, critic.output_layer.bias.grad)
            arena.linear(cb.dz2, cb.p, critic.hidden_layer_2.weight.grad, critic.hidden_layer_2.bias.grad)
            arena.linear(cb.dz1, cb.h0, critic.hidden_layer.weight.grad, critic.hidden_layer.bias.grad)
            arena.small(cb.dzG, rows[:, 2 * OBS:2 * OBS + 2], ae.weight.grad, ae.bias.grad)
            arena.fold(cb.dz0, cb.xb, critic)
        arena.scalar(st.tile_loss[k], st.losses[k:k + 1])
        if flush:
            arena.flush()


def sac_actor_grad(st, obs_rows, act, stream=None):
    """asvrl_sac_actor_grad: Q1, Q2(s, act) through the local critics into st.q_pi and each critic's share of
    d(-min(Q1, Q2))/d act into st.dA (the gradient goes to the smaller critic, half and half on an exact tie)."""
    assert obs_rows.dtype == torch.float32 and obs_rows.stride(1) == 1 and act.dtype == torch.float32
    io = _abi.AsvSacActorGradIO()
    io.x, io.ldx = obs_rows.data_ptr(), obs_rows.stride(0)
    io.act, io.lda, io.B = act.data_ptr(), act.stride(0), st.B
    io.q_pi, io.dA = st.q_pi.data_ptr(), st.dA.data_ptr()
    _abi.check(st.L.asvrl_sac_actor_grad(C.byref(st.local[0].dw), C.byref(st.local[1].dw), C.byref(io),
                                         _abi.stream_ptr(stream)), "asvrl_sac_actor_grad", st.L)


def sac_actor_backward(st, actor, flush=True, stream=None):
    """asvrl_sac_actor_backward from st.dA / st.q_pi and what sac_actor_forward kept, then every actor .grad
    through st.aarena (the head as four 128-vectors: st.dhead's rows are dmu_0, dmu_1, dls_0, dls_1) and
    st.losses[2] = mean(alpha logp - min(Q1, Q2))."""
    io = _actor_io(st)
    _abi.check(st.L.asvrl_sac_actor_backward(C.byref(st.actor.sw), C.byref(io), _abi.stream_ptr(stream)),
               "asvrl_sac_actor_backward", st.L)
    arena, mu, ls = st.aarena, actor.output_layer_mu, actor.output_layer_log_std
    with arena.batch():
        for k, lin in enumerate((mu, mu, ls, ls)):
            arena.vec(st.dhead[k], st.h2, lin.weight.grad[k % 2], lin.bias.grad[k % 2:k % 2 + 1])
        arena.linear(st.dz2, st.h1, actor.hidden_layer_2.weight.grad, actor.hidden_layer_2.bias.grad)
        arena.linear(st.dz1, st.h0, actor.hidden_layer.weight.grad, actor.hidden_layer.bias.grad)
        arena.fold(st.dz0, st.xb, actor)
    arena.scalar(st.tile_loss[2], st.losses[2:3])
    if flush:
        arena.flush()


def sac_update_fused(st, policy, actor_opt, critic_opts, rows, gamma=0.99, eps_target=None, eps_local=None, sync=None,
                     max_norm=0.5, actor_wait=None, counter=None, seed=0, noise_counter=0, counter_dev=None):
    """One SAC update from replay rows [B][88]. eps_target / eps_local: the two standard normal draws [B][2]
    (None: drawn in the kernel on (row, noise_counter + counter_dev, seed)). critic_opts: the two critics'
    FusedAdam. actor_wait: event to wait for before the actor's weights change (a concurrent act kernel).
    counter: an int64 device scalar incremented by the last optimiser launch (the learn counter).
    Returns (critic_1_loss, critic_2_loss, actor_loss, c1_norm, c2_norm, actor_norm) as device scalars."""
    s_rows = rows[:, 0:OBS]
    # both sampled actors first: they read s, s' and the (not yet updated) actor only
    sac_actor_forward(st, rows, eps_target, eps_local, seed, noise_counter, counter_dev)
    # ---- critics (agent.py:556-579): each clipped by its own norm, each its own Adam step
    sac_critic_grads(st, policy, rows, gamma, flush=False)
    norms = [_reduce_and_step(st.carena[k], critic_opts[k], critic_opts[k].grads, sync, max_norm, pack=st.local[k])
             for k in range(2)]
    # ---- actor through the updated critics (agent.py:582-593)
    sac_actor_grad(st, s_rows, st.a)
    sac_actor_backward(st, policy.actor, flush=False)
    # a concurrent act kernel reads the current actor images: with two sets the step writes the other one
    st.actor._adam_segs = st.actor.adam_segments(actor_opt)
    agn = _reduce_and_step(st.aarena, actor_opt, actor_opt.grads, sync, max_norm,
                           wait=None if st.actor.double else actor_wait, pack=st.actor, counter=counter)
    st.actor.flip()
    return st.losses[0], st.losses[1], st.losses[2], norms[0], norms[1], agn
