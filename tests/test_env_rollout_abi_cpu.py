"""CPU: the binding of asvrl_env_rollout (ABI 27). sizeof(AsvRollout) agrees between ctypes and the compiled
library, and every argument error comes back as a status with an asvrl_last_error text. The checks fail
before anything is launched, so no device memory is touched (all array pointers are null)."""
import ctypes as C

import pytest


def test_rollout_struct_size():
    from distributional_rl_decision_and_control_amd import _abi
    assert C.sizeof(_abi.AsvRollout) == 8 + 10 * 8
    for ops in ("bf16", "f32"):
        assert _abi.lib(ops).asvrl_rollout_struct_size() == C.sizeof(_abi.AsvRollout)


def _call(L, n_steps=3, actions=0x1000, hold_done=0, trainer_deactivate=0, noise_mode=1, noise=None, do_dynamics=1,
          ro=True):
    from distributional_rl_decision_and_control_amd import _abi
    p = _abi.params_from()
    st = _abi.AsvEnvState()
    st.n_envs, st.max_robots, st.max_obs, st.max_cores = 4, 5, 4, 0
    ctl = _abi.AsvStepCtl()
    ctl.is_continuous, ctl.do_dynamics, ctl.trainer_deactivate, ctl.noise_mode = 1, do_dynamics, trainer_deactivate, noise_mode
    out = _abi.AsvStepOut()
    r = _abi.AsvRollout()
    r.n_steps, r.hold_done = n_steps, hold_done
    r.actions = actions   # never dereferenced: every call below fails its argument checks first
    r.noise = noise
    return L.asvrl_env_rollout(C.byref(p), C.byref(st), C.byref(ctl), C.byref(out), C.byref(r) if ro else None, None,
                               None)


@pytest.mark.parametrize("kw,text", [
    (dict(n_steps=0), b"n_steps"),
    (dict(n_steps=-2), b"n_steps"),
    (dict(actions=None), b"actions"),
    (dict(hold_done=1, trainer_deactivate=0), b"hold_done"),
    (dict(noise_mode=0, noise=None), b"noise"),
    (dict(do_dynamics=0), b"do_dynamics"),
    (dict(ro=False), b"null"),
    (dict(), b"null"),   # well-formed control, but the state and output arrays are null
])
def test_rollout_argument_errors(kw, text):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib()
    rc = _call(L, **kw)
    assert rc != 0
    msg = L.asvrl_last_error()
    assert b"asvrl_env_rollout" in msg and text in msg, msg
