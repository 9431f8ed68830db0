"""The IQN update (Agent.train_IQN, agent.py:434-476) and act_iqn (agent.py:227-256) on the
gfx950 kernels of csrc/asvrl_critic.hip, csrc/asvrl_mlp.hip and csrc/asvrl_wgrad.hip.

IQN_Policy (IQN_model.py:74-108) is the AC-IQN critic trunk without the action encoder and
with a 128 -> 25 output layer, so it runs on the critic kernels' IQN modes. Per step, on a
replay batch `rows` ([B][88]: obs | next obs | action | reward | done):

    target encoders(ns) + trunk, max over actions per tau -> q_next
                                                          asvrl_iqn_forward_max    (agent.py:451-452)
                                                          (bf16 build, FusedIQNState.target_in_fused: inside
                                                          the next launch, ABI 24 asvrl_iqn_train_fused_tq)
    local encoders(s) + forward, gather at a, quantile-Huber vs r + g q_next (1-d), backward,
    and the per-workgroup weight-gradient partials of the four layers
                                                          asvrl_iqn_train_fused (ONE launch, agent.py:455-468)
    encoder gradients                                     asvrl_linear_wgrad_multi (the fold image),
                                                          ONE asvrl_partial_sums_norm: every .grad
                                                          (encoders folded, the 32-row output
                                                          reduction into the 25-row layer), the
                                                          loss and the gradient norm
    clip + Adam                                           asvrl_adam_step          (agent.py:471-472)
      (with DP: asvrl_partial_sums, RCCL all-reduce, asvrl_adam_clip)
    (B*N not a multiple of the 64-row round: asvrl_iqn_train's two launches + the weight-gradient launch over the
    saved activations, the round-1 path)
    re-pack trunk and head                                asvrl_iqn_pack

The encoders run inside the trunk kernels' prologue (f32, from the parameters). act_iqn for
every robot row is one kernel (encoders, K = 32 quantile samples per state, mean over them,
argmax, epsilon-greedy on the device step counter).

The closed-loop windows (csrc/asvrl_env.hip, asvrl_iqn_rollout / asvrl_iqn_rollout_ar) take an IqnPack: per step
they launch the window form of the act pass (asvrl_iqn_act_ex: the same tile with the step offset, the (index, 0.0)
pair, its masked record row and act_iqn's cvar), then the env step; the act is not fused into the env kernel (its
150 KB LDS image and 16 waves per CU do not fit beside the env's carve). FusedIQNState.window_pack,
DeviceEnvBatch.policy_rollout(..., cvar=1.0), DeviceEvaluator.run(..., policy_seed=0, cvar=1.0).

Arithmetic: bf16 MFMA operands with f32 accumulation, f32 master weights / Adam.
"""
import collections
import ctypes as C
import dataclasses
import math

import torch

from . import _abi
from .fused_critic import CriticPack, PartialArena, TrainBuffers, fused_groups, fused_train_supported
from .fused_mlp import default_net
from .fused_update import ENC_IN_KERNEL, _reduce_and_step
from .learner import target_step

OBS = 40
K_ACT = 32


# the IQN step's forward / loss / backward and weight gradients in ONE launch (asvrl_iqn_train_fused)
# wherever it takes the shape (B*N a multiple of its 64-row round); otherwise asvrl_iqn_train's two
# launches + the batched weight-gradient launch over saved activations (tests toggle it)
FUSED_TRAIN = True
# the target network's max over the actions inside that launch (ABI 24, asvrl_iqn_train_fused_tq: each workgroup
# forms q_next for the samples it updates, bit-identical to asvrl_iqn_forward_max); bf16 build. The default of
# FusedIQNState.target_in_fused. Off for the batched loop, whose act pass runs beside the learner: there the longer
# update launch runs beside the act pass instead of the env step, 0.2982 -> 0.3153 ms per IQN step; on for the
# drop-in Agent (nothing beside its update; bf16 learner): 55.5 -> 54.0 us per B = 64 step (profiles/r06j_*, r06k_*)
TARGET_IN_FUSED = False


@dataclasses.dataclass(frozen=True)
class AdaptiveCvar:
    """The risk level chosen per robot and per act from what the robot sees (the reference's adjust_cvar,
    agent.py:326-343, with a floor): on the packed observation row (self 7 | objects 5 x 5 (px, py, vx, vy, r),
    nearest first | mask 5), 1 when mask[0] is 0 (no object); otherwise d = sqrt(px0^2 + py0^2) - r0 - margin and the
    level is 1 for d >= near, else max(d / near, floor). f32 arithmetic, inside the act kernel. near and margin default
    to the reference's constants; floor keeps the level in (0, 1] (the reference's d / 10 is unclamped and can go
    negative), 0.1 by default."""
    near: float = 10.0
    margin: float = 2.8
    floor: float = 0.1

    def __post_init__(self):
        for name in ("near", "margin", "floor"):
            object.__setattr__(self, name, float(getattr(self, name)))
        if not (math.isfinite(self.near) and self.near > 0.0):
            raise ValueError("AdaptiveCvar: near must be > 0")
        if not math.isfinite(self.margin):
            raise ValueError("AdaptiveCvar: margin must be finite")
        if not 0.0 < self.floor <= 1.0:
            raise ValueError("AdaptiveCvar: floor must be in (0, 1]")

    def levels(self, obs_rows):
        """The rule in torch f32 on packed observation rows [..., >= 37]: the level of every row."""
        x = obs_rows.to(torch.float32)
        px, py, r, m0 = x[..., 7], x[..., 8], x[..., 11], x[..., 32]
        d = torch.sqrt(px * px + py * py) - r - x.new_tensor(self.margin)
        lev = torch.clamp(d / x.new_tensor(self.near), min=self.floor)
        one = torch.ones_like(lev)
        return torch.where((m0 < 0.5) | (d >= x.new_tensor(self.near)), one, lev)

    def as_dict(self):
        return dataclasses.asdict(self)


def risk_struct(cvar, rows, device, cvar_out=None, check=True, who="iqn_act"):
    """The AsvIqnRisk of a risk level that is not a float: an f32 device tensor [rows] of levels in (0, 1] (checked on
    the host unless check is False: one sync) or an AdaptiveCvar. Returns (struct, what it must keep alive)."""
    rk = _abi.AsvIqnRisk()
    if isinstance(cvar, AdaptiveCvar):
        rk.mode, rk.near, rk.margin, rk.floor = _abi.IQN_RISK_ADAPTIVE, cvar.near, cvar.margin, cvar.floor
    else:
        if cvar.dtype != torch.float32 or cvar.dim() != 1 or not cvar.is_contiguous():
            raise ValueError(f"{who}: a per-row cvar must be a contiguous f32 tensor of one value per row")
        if cvar.shape[0] != rows:
            raise ValueError(f"{who}: a per-row cvar needs {rows} values, one per row; got {cvar.shape[0]}")
        dev = torch.device(device)
        if cvar.device.type != dev.type or (dev.index is not None and cvar.device.index != dev.index):
            raise ValueError(f"{who}: a per-row cvar must be on {device}")
        if check and rows and not bool(((cvar > 0) & (cvar <= 1)).all().item()):
            raise ValueError(f"{who}: cvar must be in (0, 1]")
        rk.mode, rk.cvar_rows = _abi.IQN_RISK_ROWS, cvar.data_ptr()
    if cvar_out is not None:
        assert cvar_out.dtype == torch.float32 and cvar_out.is_contiguous() and cvar_out.numel() >= rows
        rk.cvar_out = cvar_out.data_ptr()
    return rk, (cvar, cvar_out)


def is_risk(cvar):
    """A risk level that is decided per row: a tensor or an AdaptiveCvar (not a float)."""
    return isinstance(cvar, AdaptiveCvar) or torch.is_tensor(cvar)


def supported(net, B, N):
    return (default_net(net) and net.n == 64 and 1 <= net.action_size <= _abi.IQN_MAX_ACTIONS and N in (8, 16, 32)
            and (B * N) % 32 == 0)


class IqnPack(CriticPack):
    """bf16 images of one IQN_Policy: the trunk (CriticPack's five) and the padded output head,
    one refresh launch; the observation encoders are read in f32 by the kernels themselves.
    operands="f32": the f32 images of libasvrl_f32.so (the parity build).

    As a window policy (the surface MlpPack describes; asvrl_iqn_rollout): the rounds are iqn_act(pack, None, act64,
    step, *eps, policy_seed, obs=obs, cvar=cvar) -- K = 32 taus per state drawn in the kernel on (global row, step,
    policy_seed) -- and step(act64, is_continuous=False, ...); "actions" holds (action index, 0.0). The act stays a
    launch of its own per step (it is not fused into the env kernel), all enqueued by the one call. cvar in (0, 1]
    (this pack only): act_iqn's risk distortion, every tau times cvar. cvar may also be an f32 device tensor [NT] (one
    level per robot slot, constant over the window) or an AdaptiveCvar (the level from the row the robot acts on, at
    every step): the rounds are then iqn_act(..., cvar=that) and the call is rollout_risk (asvrl_iqn_rollout_risk),
    which the windows pick from the policy struct's `risk`; "actions" then holds (action index, level used)."""
    rollout, policy_struct = _abi.ROLLOUTS["iqn"]
    rollout_risk = "asvrl_iqn_rollout_risk"
    continuous = False
    takes_cvar, takes_deterministic = True, False
    is_policy = True

    def __init__(self, net, operands="bf16"):
        dev = net.cos_embedding.weight.device
        self.head_img = torch.zeros(_abi.IQN_MAX_ACTIONS * 128, dtype=_abi.operand_dtype(operands), device=dev)
        hd = _abi.AsvIqnHead()
        hd.wo_frag, hd.wo, hd.bo = (self.head_img.data_ptr(), net.output_layer.weight.data_ptr(),
                                    net.output_layer.bias.data_ptr())
        hd.n_actions = net.action_size
        self.head = hd
        super().__init__(net, operands)

    def policy(self, cvar=1.0, deterministic=False):
        pi = self.policy_struct()
        if is_risk(cvar):   # validated by policy_options; the struct rides on pi (a Python attribute, not a member)
            pi.w, pi.head, pi.cvar = self.struct, self.head, 1.0
            pi.risk, pi.risk_keep = risk_struct(cvar, cvar.shape[0] if torch.is_tensor(cvar) else 0,
                                                self.head_img.device, check=False, who="policy")
            return pi
        pi.w, pi.head, pi.cvar = self.struct, self.head, float(cvar)
        return pi

    def adam_segments(self, opt):
        """The trunk images and the head's leading rows (the padding rows stay zero)."""
        return super().adam_segments(opt) + [opt.pack_seg(self.critic.output_layer.weight, self.head_img, K=128,
                                                          chained=True)]

    def refresh(self, stream=None):
        n = self.critic
        rc = self.L.asvrl_iqn_pack(_abi.ptr(n.cos_embedding.weight), _abi.ptr(n.hidden_layer.weight),
                                   _abi.ptr(n.hidden_layer_2.weight), _abi.ptr(n.output_layer.weight),
                                   C.byref(self.struct), C.byref(self.head), _abi.stream_ptr(stream))
        _abi.check(rc, "asvrl_iqn_pack", self.L)


def _io(F, N, obs=None, xb=None, **kw):
    """AsvIqnIO for one launch: features F [B][256], or packed observation rows `obs` (any row
    stride; the kernels run the encoders)."""
    io = _abi.AsvIqnIO()
    io.F = F.data_ptr() if F is not None else None
    io.B, io.N = (F if F is not None else obs).shape[0], N
    if obs is not None:
        assert obs.dtype == torch.float32 and obs.stride(-1) == 1
        io.obs, io.ld_obs = obs.data_ptr(), obs.stride(0)
    io.xb = xb.data_ptr() if xb is not None else None
    for k in ("Np", "kappa", "gamma", "ld_rd", "loss_scale", "ld_act"):
        if k in kw:
            setattr(io, k, kw.pop(k))
    for k, v in kw.items():
        setattr(io, k, v.data_ptr() if v is not None else None)
    return io


def iqn_forward_max(pack, F, taus, N, q, stream=None, obs=None):
    """q[b*N + n] = max_a Q(s_b, tau_bn, a) (the target of train_IQN)."""
    io = _io(F, N, obs=obs, taus=taus, q=q)
    _abi.check(pack.L.asvrl_iqn_forward_max(C.byref(pack.struct), C.byref(pack.head), C.byref(io),
                                            _abi.stream_ptr(stream)), "asvrl_iqn_forward_max", pack.L)
    return q


def iqn_train(pack, F, taus, bufs, dz_out, q_next, actions, rewards, dones, gamma, dzF, tile_loss=None, kappa=1.0,
              q=None, stream=None, obs=None, xb=None):
    """Forward + loss + backward of the local net. actions / rewards / dones are column views of
    the replay rows (one stride). Writes bufs' activations, dz_out, dzF and, with tile_loss,
    the per-tile loss partials (loss = their sum)."""
    B, N = (F if F is not None else obs).shape[0], bufs.N
    Np = q_next.shape[1]
    assert actions.stride(0) == rewards.stride(0) == dones.stride(0)
    io = _io(F, N, obs=obs, xb=xb, taus=taus, Np=Np, kappa=float(kappa), q_next=q_next, actions=actions, rewards=rewards,
             dones=dones, ld_rd=rewards.stride(0), gamma=float(gamma), q=q, row_loss=bufs.row_loss, dzF=dzF,
             dz_out=dz_out, tile_loss=tile_loss, loss_scale=1.0 / float(B * Np))
    _abi.check(pack.L.asvrl_iqn_train(C.byref(pack.struct), C.byref(pack.head), C.byref(io),
                                      C.byref(bufs.struct), _abi.stream_ptr(stream)), "asvrl_iqn_train", pack.L)


def iqn_train_fused(pack, net, taus, N, q_next, actions, rewards, dones, gamma, obs, arena, dzF=None, xb=None,
                    tile_loss=None, kappa=1.0, q=None, row_loss=None, stream=None, encoders=False, target=None):
    """asvrl_iqn_train_fused: train_IQN's local pass (agent.py:455-468) -- forward, gather at the
    taken action, quantile-Huber loss, backward -- AND the weight gradients of the trunk and the
    output layer in one launch; the per-workgroup partials land in `arena` as segments of net's
    cos_embedding / hidden_layer / hidden_layer_2 / output_layer .grad.
    encoders=True: also the observation encoders' gradients (ABI 16 parts.enc; their .grad contiguous
    [self_w | self_b | obj_w | obj_b]); dzF / xb are then not needed.
    target=(target_pack, target_taus, next_obs): q_next is first computed inside the launch
    (asvrl_iqn_train_fused_tq) from the target network, as iqn_forward_max would."""
    B = obs.shape[0]
    groups = fused_groups(pack, B, N)
    assert groups > 0 and fused_train_supported(pack, B, N), (B, N)
    assert actions.stride(0) == rewards.stride(0) == dones.stride(0)
    shapes = ((net.cos_embedding, 256, 64), (net.hidden_layer, 128, 256), (net.hidden_layer_2, 128, 128),
              (net.output_layer, _abi.IQN_MAX_ACTIONS, 128))
    regions = [arena._take(groups * (M * K + M)) for _, M, K in shapes]
    parts = _abi.AsvCriticParts()
    parts.cos_emb, parts.hidden, parts.hidden2, parts.out = (t.data_ptr() for t in regions)
    if encoders:
        se, oe = net.self_encoder[0], net.object_encoder[0]
        gs = [se.weight.grad, se.bias.grad, oe.weight.grad, oe.bias.grad]
        if not all(gs[k].data_ptr() + 4 * gs[k].numel() == gs[k + 1].data_ptr() for k in range(3)):
            raise RuntimeError("iqn_train_fused(encoders=True) needs the encoder gradients contiguous (FusedAdam)")
        enc_part = arena._take(groups * 688)
        parts.enc = enc_part.data_ptr()
    io = _io(None, N, obs=obs, xb=xb, taus=taus, Np=N, kappa=float(kappa), q_next=q_next, actions=actions,
             rewards=rewards, dones=dones, ld_rd=rewards.stride(0), gamma=float(gamma), q=q, row_loss=row_loss,
             dzF=dzF, tile_loss=tile_loss, loss_scale=1.0 / float(B * N))
    if target is not None:
        tpack, ttaus, next_obs = target
        tio = _io(None, N, obs=next_obs, taus=ttaus)
        _abi.check(pack.L.asvrl_iqn_train_fused_tq(C.byref(pack.struct), C.byref(pack.head), C.byref(io),
                                                   C.byref(parts), C.byref(tpack.struct), C.byref(tpack.head),
                                                   C.byref(tio), _abi.stream_ptr(stream)),
                   "asvrl_iqn_train_fused_tq", pack.L)
    else:
        _abi.check(pack.L.asvrl_iqn_train_fused(C.byref(pack.struct), C.byref(pack.head), C.byref(io),
                                                C.byref(parts), _abi.stream_ptr(stream)), "asvrl_iqn_train_fused",
                   pack.L)
    for (layer, M, K), part in zip(shapes, regions):
        arena.groups(part, groups, M, K, layer.weight.grad, layer.bias.grad)
    if encoders:
        arena._seg(enc_part, gs[0], None, groups, 688, 0, False)


def iqn_act(pack, F, actions64, step_dev, steps_per_count, total, fraction, initial, final, seed, taus=None,
            stream=None, obs=None, cvar=1.0, step_add=0, q_out=None, actions_rec=None, env_mask=None,
            robots_per_env=1, cvar_out=None, check_cvar=True):
    """act_iqn for every row of F (or of the observation rows `obs`) into actions64[:, 0] (f64 action index).
    The window form (asvrl_iqn_act_ex, taken only when one of these is set): cvar in (0, 1] multiplies every tau,
    drawn or given (act_iqn's risk distortion, IQN_model.py:68); step_add is added to the step counter's value;
    q_out (f32 [rows, >= A]) receives the action values quantiles.mean(dim=1); actions_rec (f64 [rows, 2]) receives
    (index, 0.0) for the rows of envs with env_mask != 0 (u8, one per robots_per_env rows; None: every row).
    cvar may also be decided per row (asvrl_iqn_act_risk): an f32 device tensor [rows], row b's 32 taus times cvar[b]
    (its range is checked on the host, which is one synchronisation; check_cvar=False skips it, for graph capture),
    or an AdaptiveCvar, the level computed in the kernel from observation row b (needs obs). actions_rec then
    receives (index, level used) and cvar_out (f32 [rows]) the level of every row. A ValueError for a level outside
    (0, 1], a tensor of another dtype, length or device, and an AdaptiveCvar without obs."""
    io = _io(F, K_ACT, obs=obs, taus=taus, act_out=actions64, ld_act=actions64.stride(0))
    _abi.fill_schedule(io, step_dev, (steps_per_count, total, fraction, initial, final), seed)
    risk = None
    if is_risk(cvar):
        if isinstance(cvar, AdaptiveCvar) and obs is None:
            raise ValueError("iqn_act: an AdaptiveCvar reads the observation rows (obs=); features alone carry none")
        risk, _keep = risk_struct(cvar, io.B, actions64.device, cvar_out, check_cvar)
        cvar = 1.0
    elif cvar_out is not None:
        raise ValueError("iqn_act: cvar_out is the per-row level of a tensor or AdaptiveCvar cvar")
    if (risk is None and float(cvar) == 1.0 and int(step_add) == 0 and q_out is None and actions_rec is None
            and env_mask is None):
        _abi.check(pack.L.asvrl_iqn_act(C.byref(pack.struct), C.byref(pack.head), C.byref(io),
                                        _abi.stream_ptr(stream)), "asvrl_iqn_act", pack.L)
        return
    ex = _abi.AsvIqnActEx()
    ex.cvar, ex.robots_per_env, ex.step_add = float(cvar), int(robots_per_env), int(step_add)
    if q_out is not None:
        assert q_out.dtype == torch.float32 and q_out.stride(-1) == 1 and q_out.shape[0] == io.B
        assert q_out.shape[1] >= pack.head.n_actions
        ex.qmean_out, ex.ld_q = q_out.data_ptr(), q_out.stride(0)
    if actions_rec is not None:
        assert actions_rec.dtype == torch.float64 and actions_rec.is_contiguous()
        assert tuple(actions_rec.shape) == (io.B, 2)
        ex.rec_row = actions_rec.data_ptr()
    if env_mask is not None:
        assert env_mask.dtype == torch.uint8 and env_mask.is_contiguous()
        assert env_mask.numel() * int(robots_per_env) >= io.B
        ex.env_mask = env_mask.data_ptr()
    if risk is not None:
        _abi.check(pack.L.asvrl_iqn_act_risk(C.byref(pack.struct), C.byref(pack.head), C.byref(io), C.byref(ex),
                                             C.byref(risk), _abi.stream_ptr(stream)), "asvrl_iqn_act_risk", pack.L)
        return
    _abi.check(pack.L.asvrl_iqn_act_ex(C.byref(pack.struct), C.byref(pack.head), C.byref(io), C.byref(ex),
                                       _abi.stream_ptr(stream)), "asvrl_iqn_act_ex", pack.L)


IqnDistribution = collections.namedtuple("IqnDistribution", "z taus all greedy q")


def iqn_dist(pack, obs, *, rows_per_step=None, step0=0, seed=0, cvar=1.0, levels=None, taus=None, actions=None,
             z_out=None, tau_out=None, all_out=None, greedy_out=None, q_out=None, stream=None):
    """The quantile samples behind act_iqn's decisions on the observation rows `obs` [M, >= 37] f32 (asvrl_iqn_dist:
    the act pass's tile, so its action values bit for bit; nothing is drawn for exploration and no action is written).
    The rows are [steps][rows_per_step] (default: one step of M rows): row m is robot slot m % rows_per_step at step
    step0 + m // rows_per_step, and its 32 fractions are `taus` [M, 32] or the Philox draws of the act launch over
    rows_per_step rows at that step under `seed` (iqn_act(..., step_add=t) with a null or zero step counter). Every
    fraction is multiplied by cvar in (0, 1], or by the row's entry of levels (f32 [M], each in (0, 1], not checked:
    no synchronisation; cvar must then be 1. The device evaluation passes the recorded levels of every slot, acted
    or not: a slot that did not act carries 0.0 or a stale value, which only scales that row's fractions, and the row
    is never read). actions (f64 [M, 2], the windows' record): the selected action is column
    0, otherwise the first arg-max of the 32-sample sums; an index outside 0..A-1 gives a NaN row of z.
    Returns IqnDistribution(z [M, 32] the selected action's quantile values in sample order, taus [M, 32] the
    fractions used, all [M, 32, A] every action's values (what act_iqn returns as quantiles), greedy [M] i32 the
    arg-max, q [M, A] the action values); each is the tensor given (all_out / q_out may have a wider last stride) or
    allocated here."""
    if obs.dtype != torch.float32 or obs.dim() != 2 or obs.stride(-1) != 1 or obs.shape[1] < 37:
        raise ValueError("iqn_dist: obs must be f32 rows [M, >= 37] with unit column stride")
    M, A, dev = obs.shape[0], pack.head.n_actions, obs.device
    rows_per_step = max(M, 1) if rows_per_step is None else int(rows_per_step)
    if rows_per_step < 1:
        raise ValueError("iqn_dist: rows_per_step must be >= 1")
    if int(step0) < 0:
        raise ValueError("iqn_dist: step0 must be >= 0")
    if not 0.0 < float(cvar) <= 1.0:
        raise ValueError("iqn_dist: cvar must be in (0, 1]")
    if levels is not None and float(cvar) != 1.0:
        raise ValueError("iqn_dist: one level, cvar or levels, not both")

    def given(t, name, dtype, shape):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"iqn_dist: {name} must be a contiguous {dtype} tensor {shape} on {dev}")
        return t

    def out2(t, name, dtype, lead):   # outputs whose last dimension may be padded: [lead..., >= A]
        if t is None:
            return torch.empty(lead + (A,), dtype=dtype, device=dev)
        if (t.dtype != dtype or tuple(t.shape[:-1]) != lead or t.shape[-1] < A or t.device != dev
                or not t.is_contiguous()):
            raise ValueError(f"iqn_dist: {name} must be a contiguous {dtype} tensor {lead + ('>= %d' % A,)} on {dev}")
        return t
    f32 = torch.float32
    z = torch.empty((M, K_ACT), dtype=f32, device=dev) if z_out is None else given(z_out, "z_out", f32, (M, K_ACT))
    tu = torch.empty((M, K_ACT), dtype=f32, device=dev) if tau_out is None else given(tau_out, "tau_out", f32,
                                                                                       (M, K_ACT))
    gr = torch.empty(M, dtype=torch.int32, device=dev) if greedy_out is None else given(greedy_out, "greedy_out",
                                                                                        torch.int32, (M,))
    al = out2(all_out, "all_out", f32, (M, K_ACT))
    qm = out2(q_out, "q_out", f32, (M,))
    if taus is not None:
        given(taus, "taus", f32, (M, K_ACT))
    if levels is not None:
        given(levels, "levels", f32, (M,))
    if actions is not None:
        given(actions, "actions", torch.float64, (M, 2))
    if M:   # no rows: nothing to launch (an empty tensor has no address to hand over)
        iqn_dist_launch(pack, obs, rows_per_step, step0, seed, cvar, levels, taus, actions, z, tu, al, gr, qm, stream)
    return IqnDistribution(z, tu, al, gr, qm)


def iqn_dist_launch(pack, obs, rows_per_step, step0, seed, cvar, levels, taus, actions, z, tau, all_, greedy, q,
                    stream=None):
    """asvrl_iqn_dist on checked tensors (iqn_dist's, or the evaluator's planes); an output that is None is not
    written, so a caller that wants the samples alone moves no [M, 32, A] block."""
    io = _io(None, K_ACT, obs=obs, taus=taus)
    io.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    d = _abi.AsvIqnDist()
    d.rows_per_step, d.cvar, d.step0 = int(rows_per_step), float(cvar), int(step0)
    for name, t in (("level_rows", levels), ("actions", actions), ("z_out", z), ("tau_out", tau),
                    ("greedy_out", greedy)):
        setattr(d, name, t.data_ptr() if t is not None else None)
    if all_ is not None:
        d.all_out, d.ld_a = all_.data_ptr(), all_.shape[-1]
    if q is not None:
        d.qmean_out, d.ld_q = q.data_ptr(), q.shape[-1]
    _abi.check(pack.L.asvrl_iqn_dist(C.byref(pack.struct), C.byref(pack.head), C.byref(io), C.byref(d),
                                     _abi.stream_ptr(stream)), "asvrl_iqn_dist", pack.L)


class FusedIQNState:
    """Packs and buffers of the fused IQN update (allocated once, pointer-stable for graphs).
    operands="f32": every kernel from libasvrl_f32.so (the parity build; the optimiser must be a
    FusedAdam of the same operands). window_pack and eval_pack are the local IqnPack; policy_pack and actor_pack stay
    None, so VecTrainer.policy_pack(), collect, greedy_episodes and evaluate still refuse an IQN trainer."""
    actor_pack = policy_pack = None   # act_iqn runs in its own launch (the windows compose it per step, window_pack)

    def __init__(self, net_local, net_target, B, N, operands="bf16", target_in_fused=None):
        dev = net_local.cos_embedding.weight.device
        self.B, self.N, self.device = B, N, dev
        self.operands = operands
        # the target's max inside the fused launch (bf16 build; module default TARGET_IN_FUSED)
        self.target_in_fused = TARGET_IN_FUSED if target_in_fused is None else bool(target_in_fused)
        self.A = net_local.action_size
        self.local = self.window_pack = self.eval_pack = IqnPack(net_local, operands)
        self.target = IqnPack(net_target, operands)
        self.bufs = TrainBuffers(B, N, dev, operands)
        f = dict(dtype=torch.float32, device=dev)
        bf = dict(dtype=_abi.operand_dtype(operands), device=dev)
        self.xb = torch.empty(B, 32, **bf)
        self.q_next = torch.empty(B * N, **f)
        self.dzF = torch.empty(B, 256, **bf)
        self.dz_out = torch.empty(B * N, _abi.IQN_MAX_ACTIONS, **bf)
        self.arena = PartialArena(32 << 20, dev, operands)
        self.loss = torch.zeros(1, **f)
        self.tile_loss = torch.zeros(B * N // 32, **f)

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

    def act(self, obs_rows, actions64, step_dev, steps_per_count, total, fraction, initial, final, seed):
        iqn_act(self.local, None, actions64, step_dev, steps_per_count, total, fraction, initial, final, seed,
                obs=obs_rows)

    def learn(self, tr, state=None, guard=0, actor_wait=None, target_wait=None, actor_done=None):
        """VecTrainer.learn: the draw from tr's ring into tr's buffers, then the update on tr's optimiser."""
        # the update's quantile fractions are drawn by the sampling launch
        rows = tr.replay.sample(tr.B, seed=tr.seed + 777, counter_dev=tr.learn_counter, out=tr.batch_rows,
                                state=state, guard=guard, taus=tr.taus)
        return iqn_update_fused(self, tr.local, tr.opt, tr.grads, rows, gamma=tr.gamma, sync=tr.sync,
                                act_wait=actor_wait, taus=tr.taus[:2], counter=tr.learn_counter)


def iqn_grads(st, net, rows, taus, gamma=0.99, flush=True):
    """train_IQN's backward (agent.py:449-468) for replay rows [B][88] and taus (2, B, N) =
    (target, local): every parameter .grad and st.loss. flush=False leaves the weight-gradient
    partials queued on st.arena (the update reduces them together with the gradient norm)."""
    B, N = st.B, st.N
    s_rows, ns_rows = rows[:, 0:OBS], rows[:, OBS:2 * OBS]
    a_col, r_col, d_col = rows[:, 80], rows[:, 82], rows[:, 83]
    bufs, arena = st.bufs, st.arena
    # every .grad is overwritten below (no zeroing); the trunk kernels run the encoders on the rows
    fused = FUSED_TRAIN and fused_train_supported(st.local, B, N)
    target_in = fused and ENC_IN_KERNEL and st.target_in_fused and st.operands == "bf16"
    if not target_in:
        iqn_forward_max(st.target, None, taus[0], N, st.q_next, obs=ns_rows)
    if fused:
        # forward, loss, backward and the four layers' weight-gradient partials in one launch
        if ENC_IN_KERNEL:   # ... and the encoders' gradient partials (and, target_in, the target's max first)
            iqn_train_fused(st.local, net, taus[1], N, st.q_next.view(B, N), a_col, r_col, d_col, gamma, s_rows,
                            arena, tile_loss=st.tile_loss, encoders=True,
                            target=(st.target, taus[0], ns_rows) if target_in else None)
        else:
            iqn_train_fused(st.local, net, taus[1], N, st.q_next.view(B, N), a_col, r_col, d_col, gamma, s_rows,
                            arena, dzF=st.dzF, xb=st.xb, tile_loss=st.tile_loss)
            with arena.batch():
                arena.fold(st.dzF, st.xb, net)   # encoder image -> self/object encoder grads
        arena.scalar(st.tile_loss, st.loss)
        if flush:
            arena.flush()
        return
    iqn_train(st.local, None, taus[1], bufs, st.dz_out, st.q_next.view(B, N), a_col, r_col, d_col, gamma, st.dzF,
              tile_loss=st.tile_loss, obs=s_rows, xb=st.xb)
    with arena.batch():   # the five layers in one launch
        # the padded 32-row output reduction fills the A-row output layer directly
        arena.linear(st.dz_out, bufs.h2, net.output_layer.weight.grad, net.output_layer.bias.grad)
        arena.linear(bufs.dzc, bufs.cos, net.cos_embedding.weight.grad, net.cos_embedding.bias.grad)
        arena.fold(st.dzF, st.xb, net)   # encoder image -> self/object encoder grads
        arena.linear(bufs.dz1, bufs.h0, net.hidden_layer.weight.grad, net.hidden_layer.bias.grad)
        arena.linear(bufs.dz2, bufs.h1g, net.hidden_layer_2.weight.grad, net.hidden_layer_2.bias.grad)
    arena.scalar(st.tile_loss, st.loss)
    if flush:
        arena.flush()


def iqn_update_fused(st, net, opt, grads, rows, gamma=0.99, taus=None, sync=None, max_norm=0.5, act_wait=None,
                     counter=None):
    """One IQN update from replay rows [B][88]; taus: (2, B, N) (target, local) or None (drawn).
    act_wait: event to wait for before the weights change (a concurrent act kernel).
    Returns (loss, grad_norm) as device scalars."""
    if taus is None:
        taus = torch.rand(2, st.B, st.N, device=st.device)
    iqn_grads(st, net, rows, taus, gamma, flush=False)
    gn = _reduce_and_step(st.arena, opt, grads, sync, max_norm, wait=act_wait, pack=st.local, counter=counter)
    return st.loss[0], gn
