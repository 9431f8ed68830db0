"""The DDPG update (Agent.train_DDPG, agent.py:478-516) on the gfx950 kernels of csrc/asvrl_ddpg.hip,
csrc/asvrl_mlp.hip, csrc/asvrl_wgrad.hip and csrc/asvrl_optim.hip.

DDPG_model.Actor is the AC-IQN Actor layer for layer, so the actor half is AC-IQN's own calls on MlpPack(kind
"actor"). DDPG_model.Critic is the AC-IQN critic without the cosine embedding and with one scalar per sample; it
runs the Actor's one-wave tile (asvrl_ddpg_tile.h) on the Actor's image set, with the action encoder read as f32.
Per step, on a replay batch `rows` ([B][88]: obs | next obs | action | reward | done):

    replay draw, actor(s) saving activations, target actor(s') -> na     asvrl_learn_prologue (ONE launch; without
                                                                          it: asvrl_actor_forward TRAIN and FWD)
  critic (agent.py:487-501)
    local critic on (s, a) (activations kept), target critic on (s', na) asvrl_ddpg_grad, launch 1
    y = r + gamma (1 - d) q_next, smooth-L1 (beta 1), dq, backward to every layer's pre-activation gradient
                                                                          asvrl_ddpg_grad, launch 2
    weight-gradient partials of the output layer, both hidden layers, the action encoder and the encoders
    (as the 256 x 32 image)                                               ONE asvrl_linear_wgrad_multi
    every .grad (encoders folded), the loss and the gradient norm        ONE asvrl_partial_sums_norm
    clip + Adam + re-pack of the weight images                           asvrl_adam_step_pack
  actor (agent.py:504-511), through the UPDATED critic
    forward Q(s, actor(s)), backward of -mean q to the action (dA)       asvrl_ddpg_actor_grad
    actor backward                                                       asvrl_actor_backward
    every actor .grad, the actor loss, the norm partials                 ONE asvrl_actor_grads
    clip + Adam + re-pack                                                asvrl_adam_step_pack

Ten launches with the prologue (the batched loop), eleven from given rows (the drop-in Agent: two actor
forwards, no draw); no host synchronisation, no torch autograd: capturable in a HIP graph.

Arithmetic: bf16 MFMA operands with f32 accumulation, f32 master weights / Adam (operands="f32": the same
kernels from libasvrl_f32.so, the parity build).
"""
import ctypes as C

import torch

from . import _abi
from .fused_critic import PartialArena, arena_floats
from .fused_mlp import (ENC, HID, OBSK, ActorBuffers, ActorGrads, MlpPack, actor_act, actor_backward, actor_forward,
                        actor_train_forward, default_net)
from .fused_update import _actor_step, _reduce_and_step, learn_prologue
from .learner import target_step

OBS = 40


def supported(policy, B):
    """The shapes the kernels take: the default network dims, 2 actions and a batch that is a positive multiple
    of 32."""
    return B >= 32 and B % 32 == 0 and all(default_net(n) and n.action_dimension == 2
                                           for n in (policy.critic, policy.actor))


class DdpgCriticPack(MlpPack):
    """Packed images of one DDPG Critic: the Actor's set (MlpPack kind "actor": encoder image, both hidden layers
    and their transposes), `wo` / `bo` -- f32 copies of the output layer padded to the two rows the tile's staging
    reads (row 1 stays zero) -- and the action encoder, read as f32 straight from the parameters. refresh()
    re-packs from the f32 parameters; adam_segments(opt) lets FusedAdam's step write the images itself."""

    def __init__(self, net, operands="bf16"):
        self._ddpg_segs = None
        super().__init__(net, "actor", operands, False)

    def _make_set(self, net, kind, operands, copies):
        t = MlpPack._make_set(net, kind, operands, copies)
        f = dict(dtype=torch.float32, device=t["enc"].device)
        t["wo"], t["bo"] = torch.zeros(2 * HID, **f), torch.zeros(2, **f)
        t["w"].wout, t["w"].bout = t["wo"].data_ptr(), t["bo"].data_ptr()
        dw = _abi.AsvDdpgWeights()
        dw.trunk = t["w"]   # by value: every pointer of the set is in place
        ae = net.action_encoder[0]
        dw.wae, dw.bae = ae.weight.data_ptr(), ae.bias.data_ptr()
        t["dw"] = dw
        return t

    def adam_segments(self, opt):
        """The Actor's segments and the padded output layer's leading row / element."""
        if self._ddpg_segs is None:
            n, t = self.net, self.sets[0]
            self._ddpg_segs = super().adam_segments(opt) + [
                opt.pack_seg(n.output_layer.weight.reshape(-1), t["wo"], f32=True),
                opt.pack_seg(n.output_layer.bias, t["bo"], f32=True)]
        return self._ddpg_segs

    def refresh(self, stream=None):
        super().refresh(stream)
        n = self.net
        with torch.no_grad():
            for t in self.sets:
                t["wo"][:HID].copy_(n.output_layer.weight.reshape(-1))
                t["bo"][:1].copy_(n.output_layer.bias)


class FusedDDPGState:
    """Packs and buffers of the fused DDPG update (allocated once, pointer-stable for graph replay).
    operands="f32": every kernel from libasvrl_f32.so (the parity build; the optimisers must be FusedAdam of the
    same operands). double_actor (the batched loop): two actor image sets, as FusedACIQNState."""

    def __init__(self, policy_local, policy_target, B, operands="bf16", double_actor=False):
        if not supported(policy_local, B):
            raise ValueError(f"DDPG learner kernels: B={B} (a positive multiple of 32), the default network, 2 actions")
        dev = policy_local.critic.output_layer.weight.device
        self.B, self.device, self.operands = B, dev, operands
        self.local = DdpgCriticPack(policy_local.critic, operands)
        self.target = DdpgCriticPack(policy_target.critic, operands)
        self.actor = MlpPack(policy_local.actor, "actor", operands, double=double_actor)
        self.actor_pack = self.policy_pack = self.window_pack = self.eval_pack = self.actor
        self.target_actor = MlpPack(policy_target.actor, "actor", operands)
        self.abufs = ActorBuffers(B, dev, operands)
        self.agrads = ActorGrads(B, dev, operands)
        bf = dict(dtype=_abi.operand_dtype(operands), device=dev)
        f = dict(dtype=torch.float32, device=dev)
        self.na = torch.zeros(B, 2, **f)
        self.xb = torch.zeros(B, OBSK, **bf)
        self.h0, self.dz0 = torch.zeros(B, ENC, **bf), torch.zeros(B, ENC, **bf)
        self.h1, self.dz1 = torch.zeros(B, HID, **bf), torch.zeros(B, HID, **bf)
        self.h2, self.dz2 = torch.zeros(B, HID, **bf), torch.zeros(B, HID, **bf)
        self.p = torch.zeros(B, HID, **bf)
        self.dzG = torch.zeros(B, HID, **f)
        self.q, self.q_next, self.dq = torch.zeros(B, **f), torch.zeros(B, **f), torch.zeros(B, **f)
        self.q_pi = torch.zeros(B, **f)
        self.tile_loss = torch.zeros(2, B // 32, **f)   # critic, actor
        self.losses = torch.zeros(2, **f)
        layers = ((HID, HID), (HID, ENC), (ENC, OBSK))
        self.arena = PartialArena(arena_floats(self.local.L, B, layers, vecs=1, small=True), dev, operands)

    def target_changed(self):
        """Re-pack the target networks after a hard/soft update (eager, outside graphs)."""
        self.target.refresh()
        self.target_actor.refresh()

    def target_step(self, tr):
        """The device-side target update behind a learn step (VecTrainer target_update="device"): blend and
        re-pack of the target actor and the target critic, one launch each, predicated on tr's learn counter."""
        target_step(tr, (self.target_actor, self.target))

    def refresh_local(self):
        """Re-pack the local networks after their parameters were loaded (eager, outside graphs)."""
        self.local.refresh()
        self.actor.refresh()

    def act(self, obs_rows, actions64, step_dev, steps_per_count, total, fraction, initial, final, seed):
        actor_act(self.actor, obs_rows, actions64, step_dev, steps_per_count, total, fraction, initial, final, seed)

    def learn(self, tr, state=None, guard=0, actor_wait=None, target_wait=None, actor_done=None):
        """VecTrainer.learn: the draw from tr's ring into tr's buffers, then the update on tr's optimisers."""
        # one launch: the draw (no quantile fractions), the actor's training forward and the target actor
        rows = learn_prologue(self, tr.replay, None, tr.seed + 777, counter_dev=tr.learn_counter, out=tr.batch_rows,
                              state=state, guard=guard)
        return ddpg_update_fused(self, tr.local, tr.actor_opt, tr.critic_opt, tr.critic_grads, tr.actor_grads, rows,
                                 gamma=tr.gamma, sync=tr.sync, actor_wait=actor_wait, counter=tr.learn_counter,
                                 prologue_done=True)


def ddpg_critic_grads(st, critic, rows, gamma=0.99, flush=True, stream=None):
    """train_DDPG's critic backward (agent.py:487-499) for replay rows [B][88] and the target actions st.na: every
    critic .grad (the four observation-encoder gradients contiguous: FusedAdam / FlatGrads) and st.losses[0].
    flush=False leaves the weight-gradient partials queued on st.arena (the update reduces them together with
    the gradient norm)."""
    assert rows.dtype == torch.float32 and rows.shape[0] == st.B and rows.stride(1) == 1
    io = _abi.AsvDdpgGradIO()
    io.rows, io.ld_rows, io.B, io.gamma = rows.data_ptr(), rows.stride(0), st.B, float(gamma)
    io.na, io.ld_na = st.na.data_ptr(), st.na.stride(0)
    for k in _abi.DDPG_GRAD_ARRAYS:
        setattr(io, k, (st.tile_loss[0] if k == "tile_loss" else getattr(st, k)).data_ptr())
    L = st.local.L
    _abi.check(L.asvrl_ddpg_grad(C.byref(st.local.dw), C.byref(st.target.dw), C.byref(io), _abi.stream_ptr(stream)),
               "asvrl_ddpg_grad", L)
    arena, ae = st.arena, critic.action_encoder[0]
    with arena.batch():   # every layer in one launch; every .grad is overwritten (no zeroing)
        arena.vec(st.dq, st.h2, critic.output_layer.weight.grad, critic.output_layer.bias.grad)
        arena.linear(st.dz2, st.p, critic.hidden_layer_2.weight.grad, critic.hidden_layer_2.bias.grad)
        arena.linear(st.dz1, st.h0, critic.hidden_layer.weight.grad, critic.hidden_layer.bias.grad)
        arena.small(st.dzG, rows[:, 2 * OBS:2 * OBS + 2], ae.weight.grad, ae.bias.grad)
        arena.fold(st.dz0, st.xb, critic)   # encoder image -> self / object encoder grads (folded over the slots)
    arena.scalar(st.tile_loss[0], st.losses[0:1])
    if flush:
        arena.flush()


def ddpg_actor_grad(st, obs_rows, act, q=None, stream=None):
    """asvrl_ddpg_actor_grad: Q(s, act) through the local critic, -mean q's gradient to the action into
    st.abufs.dA and its per-tile partials into st.tile_loss[1], in one launch."""
    assert obs_rows.dtype == torch.float32 and obs_rows.stride(1) == 1 and act.dtype == torch.float32
    io = _abi.AsvDdpgActorIO()
    io.x, io.ldx = obs_rows.data_ptr(), obs_rows.stride(0)
    io.act, io.lda, io.B = act.data_ptr(), act.stride(0), st.B
    io.q = q.data_ptr() if q is not None else None
    io.dA, io.tile_loss = st.abufs.dA.data_ptr(), st.tile_loss[1].data_ptr()
    L = st.local.L
    _abi.check(L.asvrl_ddpg_actor_grad(C.byref(st.local.dw), C.byref(io), _abi.stream_ptr(stream)),
               "asvrl_ddpg_actor_grad", L)


def ddpg_update_fused(st, policy_local, actor_opt, critic_opt, critic_grads, actor_grads, rows, gamma=0.99, sync=None,
                      max_norm=0.5, actor_wait=None, counter=None, prologue_done=False):
    """One DDPG update from replay rows [B][88]. actor_wait: event to wait for before the actor's weights change
    (a concurrent act kernel). counter: an int64 device scalar incremented after the step (the learn counter;
    in-kernel when the optimiser step is fused). prologue_done: learn_prologue already ran the actor's TRAIN
    forward and the target actor on these rows.
    Returns (critic_loss, actor_loss, critic_grad_norm, actor_grad_norm) as device scalars."""
    critic, actor = policy_local.critic, policy_local.actor
    s_rows, ab = rows[:, 0:OBS], st.abufs
    if not prologue_done:
        actor_train_forward(st.actor, s_rows, ab)   # reads only s and the (not yet updated) actor
        actor_forward(st.target_actor, rows[:, OBS:2 * OBS], st.na)
    # ---- critic (agent.py:487-501); every critic .grad is overwritten (no zeroing)
    ddpg_critic_grads(st, critic, rows, gamma, flush=False)
    cgn = _reduce_and_step(st.arena, critic_opt, critic_grads, sync, max_norm, pack=st.local)
    # ---- actor through the updated critic (agent.py:504-511)
    ddpg_actor_grad(st, s_rows, ab.a_out, q=st.q_pi)
    actor_backward(st.actor, ab)
    agn = _actor_step(st, actor, actor_opt, actor_grads, sync, max_norm, actor_wait, counter)
    return st.losses[0], st.losses[1], cgn, agn
