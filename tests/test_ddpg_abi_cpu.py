"""CPU: the binding of the DDPG entry points (asvrl_ddpg_grad / asvrl_ddpg_actor_grad). The three new structs have
the same size in ctypes and in both compiled libraries, the ABI version did not move, every argument error comes back
as a status with an asvrl_last_error text "<entry point>: <argument>", and fused_ddpg.supported refuses the shapes the
kernels do not take. The checks fail before anything is launched: no pointer is dereferenced."""
import ctypes as C

import pytest

WEIGHT_ARRAYS = ("enc_frag", "b_enc", "w1_frag", "w2_frag", "b1", "b2", "wout", "bout", "wae", "bae")
BACKWARD_ARRAYS = ("w2t_frag", "w1t_frag")
FAKE = 0x1000   # never dereferenced: every call below is refused


def test_ddpg_struct_sizes_and_abi_version():
    from distributional_rl_decision_and_control_amd import _abi
    assert C.sizeof(_abi.AsvDdpgWeights) == C.sizeof(_abi.AsvMlpWeights) + 16
    assert C.sizeof(_abi.AsvDdpgGradIO) == 40 + len(_abi.DDPG_GRAD_ARRAYS) * 8
    assert C.sizeof(_abi.AsvDdpgActorIO) == 8 * 8
    for ops in ("bf16", "f32"):
        L = _abi.lib(ops)
        assert L.asvrl_ddpg_weights_struct_size() == C.sizeof(_abi.AsvDdpgWeights)
        assert L.asvrl_ddpg_grad_struct_size() == C.sizeof(_abi.AsvDdpgGradIO)
        assert L.asvrl_ddpg_actor_struct_size() == C.sizeof(_abi.AsvDdpgActorIO)
        assert L.asvrl_abi_version() == 29
    # no existing struct changed size
    assert C.sizeof(_abi.AsvMlpWeights) == 12 * 8 + 8 and C.sizeof(_abi.AsvMlpIO) == 216
    assert C.sizeof(_abi.AsvDqnWeights) == C.sizeof(_abi.AsvMlpWeights) + 16
    assert C.sizeof(_abi.AsvDqnGradIO) == 24 + len(_abi.DQN_GRAD_ARRAYS) * 8


def _weights(missing=None):
    from distributional_rl_decision_and_control_amd import _abi
    w = _abi.AsvDdpgWeights()
    for name in WEIGHT_ARRAYS + BACKWARD_ARRAYS:
        tgt = w if name in ("wae", "bae") else w.trunk
        setattr(tgt, name, None if name == missing else FAKE)
    return w


def _grad(L, null=None, local_missing=None, target_missing=None, missing=None, B=64, ld_rows=88, rows=FAKE, ld_na=2,
          dzG=FAKE):
    from distributional_rl_decision_and_control_amd import _abi
    lw, tw = _weights(local_missing), _weights(target_missing)
    io = _abi.AsvDdpgGradIO()
    io.rows, io.ld_rows, io.B, io.gamma = (None if missing == "rows" else rows), ld_rows, B, 0.99
    io.na, io.ld_na = (None if missing == "na" else FAKE), ld_na
    for name in _abi.DDPG_GRAD_ARRAYS:
        setattr(io, name, None if name == missing else (dzG if name == "dzG" else FAKE))
    return L.asvrl_ddpg_grad(None if null == "local" else C.byref(lw), None if null == "target" else C.byref(tw),
                             None if null == "io" else C.byref(io), None)


def _actor(L, null=None, local_missing=None, missing=None, B=64, ldx=40, x=FAKE, lda=2):
    from distributional_rl_decision_and_control_amd import _abi
    lw = _weights(local_missing)
    io = _abi.AsvDdpgActorIO()
    io.x, io.ldx = (None if missing == "x" else x), ldx
    io.act, io.lda, io.B = (None if missing == "act" else FAKE), lda, B
    io.dA = None if missing == "dA" else FAKE
    io.tile_loss = None if missing == "tile_loss" else FAKE
    return L.asvrl_ddpg_actor_grad(None if null == "local" else C.byref(lw), None if null == "io" else C.byref(io), None)


GRAD_ARRAYS = ("rows", "na", "xb", "h0", "h1", "p", "h2", "q", "q_next", "dq", "dz2", "dz1", "dzG", "dz0", "tile_loss")
CASES = [(_grad, dict(null="local"), b"asvrl_ddpg_grad: null struct local"),
         (_grad, dict(null="target"), b"asvrl_ddpg_grad: null struct target"),
         (_grad, dict(null="io"), b"asvrl_ddpg_grad: null struct io"),
         (_grad, dict(B=0), b"asvrl_ddpg_grad: B must be a positive multiple of 32"),
         (_grad, dict(B=-32), b"asvrl_ddpg_grad: B must be a positive multiple of 32"),
         (_grad, dict(B=48), b"asvrl_ddpg_grad: B must be a positive multiple of 32"),
         (_grad, dict(ld_rows=80), b"asvrl_ddpg_grad: rows must be 16-byte aligned replay rows"),
         (_grad, dict(ld_rows=90), b"asvrl_ddpg_grad: rows must be 16-byte aligned replay rows"),
         (_grad, dict(rows=FAKE + 4), b"asvrl_ddpg_grad: rows must be 16-byte aligned replay rows"),
         (_grad, dict(ld_na=1), b"asvrl_ddpg_grad: ld_na must be >= 2"),
         (_grad, dict(dzG=FAKE + 4), b"asvrl_ddpg_grad: dzG must be 16-byte aligned"),
         (_actor, dict(null="local"), b"asvrl_ddpg_actor_grad: null struct local"),
         (_actor, dict(null="io"), b"asvrl_ddpg_actor_grad: null struct io"),
         (_actor, dict(B=0), b"asvrl_ddpg_actor_grad: B must be a positive multiple of 32"),
         (_actor, dict(B=48), b"asvrl_ddpg_actor_grad: B must be a positive multiple of 32"),
         (_actor, dict(ldx=36), b"asvrl_ddpg_actor_grad: x rows must be 16-byte aligned"),
         (_actor, dict(ldx=42), b"asvrl_ddpg_actor_grad: x rows must be 16-byte aligned"),
         (_actor, dict(x=FAKE + 8), b"asvrl_ddpg_actor_grad: x rows must be 16-byte aligned"),
         (_actor, dict(lda=1), b"asvrl_ddpg_actor_grad: lda must be >= 2")]
CASES += [(_grad, dict(local_missing=n), b"asvrl_ddpg_grad: null array local." + n.encode())
          for n in WEIGHT_ARRAYS + BACKWARD_ARRAYS]
CASES += [(_grad, dict(target_missing=n), b"asvrl_ddpg_grad: null array target." + n.encode()) for n in WEIGHT_ARRAYS]
CASES += [(_grad, dict(missing=n), b"asvrl_ddpg_grad: null array " + n.encode()) for n in GRAD_ARRAYS]
CASES += [(_actor, dict(local_missing=n), b"asvrl_ddpg_actor_grad: null array local." + n.encode())
          for n in WEIGHT_ARRAYS + BACKWARD_ARRAYS]
CASES += [(_actor, dict(missing=n), b"asvrl_ddpg_actor_grad: null array " + n.encode())
          for n in ("x", "act", "dA", "tile_loss")]


@pytest.mark.parametrize("ops", ["bf16", "f32"])
@pytest.mark.parametrize("call,kw,text", CASES, ids=[c.__name__ + str(sorted(kw.items())[0]) for c, kw, _ in CASES])
def test_ddpg_argument_errors(ops, call, kw, text):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    assert call(L, **kw) != 0
    assert L.asvrl_last_error() == text   # the whole message: the entry point, then the argument's own name


def test_target_does_not_need_the_backward_images():
    """Only the local critic's transposed images are read (the backward); the target's may be absent: the call gets
    past the target's weights to the next refusal."""
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib()
    assert _grad(L, target_missing="w2t_frag", B=48) != 0
    assert L.asvrl_last_error() == b"asvrl_ddpg_grad: B must be a positive multiple of 32"


def test_actor_q_output_is_optional():
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib()
    assert _actor(L, B=48) != 0   # q is NULL in every _actor call: only B is refused
    assert L.asvrl_last_error() == b"asvrl_ddpg_actor_grad: B must be a positive multiple of 32"


def test_supported_shapes():
    import torch  # noqa: F401
    from distributional_rl_decision_and_control_amd import fused_ddpg
    from distributional_rl_decision_and_control_amd.policy.DDPG_model import DDPG_Policy
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    two = [[-1.0, 1.0], [-1.0, 1.0]]
    net = DDPG_Policy(**DEFAULT_NET, value_ranges_of_action=two)
    for B in (32, 64, 96, 160, 4096):
        assert fused_ddpg.supported(net, B)
    for B in (0, -32, 16, 48, 65):
        assert not fused_ddpg.supported(net, B)
    assert not fused_ddpg.supported(DDPG_Policy(**DEFAULT_NET, value_ranges_of_action=two + [[-1.0, 1.0]]), 64)
    assert not fused_ddpg.supported(DDPG_Policy(**dict(DEFAULT_NET, hidden_dimension=64), value_ranges_of_action=two),
                                    64)
    assert not fused_ddpg.supported(DDPG_Policy(**dict(DEFAULT_NET, self_feature_dimension=64,
                                                       concat_feature_dimension=264), value_ranges_of_action=two), 64)
