"""The DQN update (Agent.train_DQN, agent.py:518-545) and act_dqn (agent.py:271-287) on the gfx950 kernels of
csrc/asvrl_dqn.hip, csrc/asvrl_wgrad.hip and csrc/asvrl_optim.hip.

DQN_Policy (DQN_model.py) is the AC-IQN Actor's trunk layer for layer (both observation encoders, hidden_layer
256 -> 128, hidden_layer_2 128 -> 128) with a 128 -> 25 output layer and no squash, so it runs the Actor's
one-wave tile (asvrl_actor_tile.h) with the output layer as one padded 32 x 128 MFMA image. Per step, on a replay
batch `rows` ([B][88]: obs | next obs | action index | . | reward | done):

    local forward on s (activations kept), target forward on s' reduced to max_a Q   asvrl_dqn_grad, launch 1
    y = r + (1 - d) gamma q_next, smooth-L1 (beta 1), dQ at the taken action, backward to every layer's
    pre-activation gradient                                                          asvrl_dqn_grad, launch 2
    the four layers' weight-gradient partials (encoders as the 256 x 32 image)       ONE asvrl_linear_wgrad_multi
    every .grad (encoders folded, the 32-row output reduction into the 25-row layer), the loss and the
    gradient norm                                                                    ONE asvrl_partial_sums_norm
    clip + Adam + re-pack of the weight images                                       asvrl_adam_step_pack
      (with DP: asvrl_partial_sums, RCCL all-reduce, asvrl_partial_sums_norm over the averaged gradient)

Five launches, no host synchronisation, no torch autograd: capturable in a HIP graph. The batched act is one
kernel (Q, arg-max with np.argmax's first-maximum rule, epsilon-greedy on the device step counter).

Arithmetic: bf16 MFMA operands with f32 accumulation, f32 master weights / Adam (operands="f32": the same
kernels from libasvrl_f32.so, the parity build).
"""
import ctypes as C

import torch

from . import _abi
from .fused_critic import PartialArena, arena_floats
from .fused_mlp import ENC, HID, OBSK, MlpPack, default_net
from .fused_update import _reduce_and_step
from .learner import target_step

OBS = 40
QPAD = _abi.DQN_MAX_ACTIONS
ACTIONS = 25


def supported(net, B):
    """The shapes the kernels take: the default network (vec_trainer.DEFAULT_NET) with 25 actions and a batch
    that is a positive multiple of 32."""
    return B >= 32 and B % 32 == 0 and net.action_size == ACTIONS and default_net(net)


class DqnPack(MlpPack):
    """Packed images of one DQN_Policy: the Actor's set (MlpPack kind "actor": encoder image, hidden layers and
    their transposes) plus the output layer padded to 32 rows (`head`, rows 25.. zero). refresh() re-packs from
    the f32 parameters in one call; adam_segments(opt) lets FusedAdam's step write the images itself.
    double=True: two image sets as MlpPack(double=True).

    As a window policy (MlpPack; asvrl_dqn_rollout): the rounds are dqn_act(pack, obs, act64, step, *eps, policy_seed)
    and step(act64, is_continuous=False, ...), the act inside the env kernel; the "actions" record holds
    (action index, 0.0)."""
    rollout, policy_struct = _abi.ROLLOUTS["dqn"]
    continuous = False
    _policy_w = "dw"

    def __init__(self, net, operands="bf16", double=False):
        self._dqn_segs = {}
        super().__init__(net, "actor", operands, double)

    def _make_set(self, net, kind, operands, copies):
        t = MlpPack._make_set(net, kind, operands, copies)
        t["head"] = torch.zeros(QPAD * HID, dtype=_abi.operand_dtype(operands), device=t["enc"].device)
        dw = _abi.AsvDqnWeights()
        dw.trunk = t["w"]   # by value: every pointer of the set is in place
        dw.head_frag, dw.n_actions = t["head"].data_ptr(), net.action_size
        t["dw"] = dw
        return t

    def adam_segments(self, opt):
        """The Actor's segments and the head's leading rows (the padding rows stay zero)."""
        dst = self.parity ^ 1 if self.double else 0
        if dst not in self._dqn_segs:
            self._dqn_segs[dst] = super().adam_segments(opt) + [
                opt.pack_seg(self.net.output_layer.weight, self.sets[dst]["head"], K=HID, chained=True)]
        return self._dqn_segs[dst]

    def refresh(self, stream=None):
        src, n = self.src(), self.net
        for t in self.sets:
            _abi.check(self.L.asvrl_dqn_pack(C.byref(src), _abi.ptr(n.output_layer.weight), C.byref(t["dw"]),
                                             _abi.stream_ptr(stream)), "asvrl_dqn_pack", self.L)
            if self.double:
                with torch.no_grad():
                    for k, p in (("b1", n.hidden_layer.bias), ("b2", n.hidden_layer_2.bias),
                                 ("wout", n.output_layer.weight), ("bout", n.output_layer.bias)):
                        t[k].copy_(p.reshape(-1))


def dqn_act(pack, obs, actions64, step_dev, steps_per_count, total, fraction, initial, final, seed, q_out=None,
            stream=None):
    """act_dqn for every observation row into actions64[:, 0] (f64 action index; column 1 set to 0).
    q_out (optional, f32 [rows, 25]): the Q rows the arg-max was taken over."""
    assert obs.dtype == torch.float32 and obs.stride(-1) == 1 and actions64.dtype == torch.float64
    io = _abi.AsvDqnActIO()
    io.x, io.ldx, io.n = obs.data_ptr(), obs.stride(0), obs.shape[0]
    io.act_out, io.ld_act = actions64.data_ptr(), actions64.stride(0)
    if q_out is not None:
        assert q_out.dtype == torch.float32 and q_out.is_contiguous() and tuple(q_out.shape) == (obs.shape[0],
                                                                                                 pack.net.action_size)
        io.q_out = q_out.data_ptr()
    _abi.fill_schedule(io, step_dev, (steps_per_count, total, fraction, initial, final), seed)
    _abi.check(pack.L.asvrl_dqn_act(C.byref(pack.dw), C.byref(io), _abi.stream_ptr(stream)), "asvrl_dqn_act", pack.L)


class FusedDQNState:
    """Packs and buffers of the fused DQN update (allocated once, pointer-stable for graphs).
    operands="f32": every kernel from libasvrl_f32.so (the parity build; the optimiser must be a FusedAdam of the
    same operands)."""

    def __init__(self, net_local, net_target, B, operands="bf16"):
        if not supported(net_local, B):
            raise ValueError(f"DQN learner kernels: B={B} (a positive multiple of 32), the default network, 25 actions")
        dev = net_local.output_layer.weight.device
        self.B, self.device, self.operands = B, dev, operands
        # the closed-loop windows and the device evaluation run the Q network
        self.local = self.policy_pack = self.window_pack = self.eval_pack = DqnPack(net_local, operands)
        self.actor_pack = None
        self.target = DqnPack(net_target, operands)
        bf = dict(dtype=_abi.operand_dtype(operands), device=dev)
        f = dict(dtype=torch.float32, device=dev)
        self.xb = torch.zeros(B, OBSK, **bf)
        self.h0, self.dz0 = torch.zeros(B, ENC, **bf), torch.zeros(B, ENC, **bf)
        self.h1, self.dz1 = torch.zeros(B, HID, **bf), torch.zeros(B, HID, **bf)
        self.h2, self.dz2 = torch.zeros(B, HID, **bf), torch.zeros(B, HID, **bf)
        self.dz_out = torch.zeros(B, QPAD, **bf)
        self.q_sel, self.q_next = torch.zeros(B, **f), torch.zeros(B, **f)
        self.tile_loss = torch.zeros(B // 32, **f)
        self.loss = torch.zeros(1, **f)
        layers = ((QPAD, HID), (HID, HID), (HID, ENC), (ENC, OBSK))
        self.arena = PartialArena(arena_floats(self.local.L, B, layers), dev, operands)

    def target_changed(self):
        """Re-pack the target network after a hard/soft update (eager, outside graphs)."""
        self.target.refresh()

    def target_step(self, tr):
        """The device-side target update behind a learn step (VecTrainer target_update="device"): blend and
        re-pack of the target network in one launch, predicated on tr's learn counter."""
        target_step(tr, (self.target,))

    def refresh_local(self):
        """Re-pack the local network after its parameters were loaded (eager, outside graphs)."""
        self.local.refresh()

    def act(self, obs_rows, actions64, step_dev, steps_per_count, total, fraction, initial, final, seed, q_out=None):
        dqn_act(self.local, obs_rows, actions64, step_dev, steps_per_count, total, fraction, initial, final, seed,
                q_out=q_out)

    def learn(self, tr, state=None, guard=0, actor_wait=None, target_wait=None, actor_done=None):
        """VecTrainer.learn: the draw from tr's ring into tr's buffers (no quantile fractions), then the update on
        tr's optimiser."""
        rows = tr.replay.sample(tr.B, seed=tr.seed + 777, counter_dev=tr.learn_counter, out=tr.batch_rows,
                                state=state, guard=guard)
        return dqn_update_fused(self, tr.local, tr.opt, tr.grads, rows, gamma=tr.gamma, sync=tr.sync,
                                act_wait=actor_wait, counter=tr.learn_counter)


def dqn_grads(st, net, rows, gamma=0.99, flush=True):
    """train_DQN's backward (agent.py:531-540) for replay rows [B][88]: every parameter .grad (the four encoder
    gradients contiguous: FusedAdam / FlatGrads) and st.loss. flush=False leaves the weight-gradient partials
    queued on st.arena (the update reduces them together with the gradient norm)."""
    assert rows.dtype == torch.float32 and rows.shape[0] == st.B and rows.stride(1) == 1
    io = _abi.AsvDqnGradIO()
    io.rows, io.ld_rows, io.B, io.gamma = rows.data_ptr(), rows.stride(0), st.B, float(gamma)
    for k in _abi.DQN_GRAD_ARRAYS:
        setattr(io, k, getattr(st, k).data_ptr())
    L = st.local.L
    _abi.check(L.asvrl_dqn_grad(C.byref(st.local.dw), C.byref(st.target.dw), C.byref(io), _abi.stream_ptr(None)),
               "asvrl_dqn_grad", L)
    arena = st.arena
    with arena.batch():   # the four layers in one launch; every .grad is overwritten (no zeroing)
        # the padded 32-row output reduction fills the 25-row output layer directly
        arena.linear(st.dz_out, st.h2, net.output_layer.weight.grad, net.output_layer.bias.grad)
        arena.linear(st.dz2, st.h1, net.hidden_layer_2.weight.grad, net.hidden_layer_2.bias.grad)
        arena.linear(st.dz1, st.h0, net.hidden_layer.weight.grad, net.hidden_layer.bias.grad)
        arena.fold(st.dz0, st.xb, net)   # encoder image -> self / object encoder grads (the masked sum over objects)
    arena.scalar(st.tile_loss, st.loss)
    if flush:
        arena.flush()


def dqn_update_fused(st, net, opt, grads, rows, gamma=0.99, sync=None, max_norm=0.5, act_wait=None, counter=None):
    """One DQN update from replay rows [B][88]. act_wait: event to wait for before the weights change (a
    concurrent act kernel). Returns (loss, grad_norm) as device scalars."""
    dqn_grads(st, net, rows, gamma, flush=False)
    gn = _reduce_and_step(st.arena, opt, grads, sync, max_norm, wait=act_wait, pack=st.local, counter=counter)
    return st.loss[0], gn
