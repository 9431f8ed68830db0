"""CPU: the auto-reset ABI (AsvAutoReset, asvrl_env_rollout_ar, asvrl_policy_rollout_ar, asvrl_replay_push_window).
The ctypes struct matches the compiled one in both libraries, AsvRollout keeps its 88 bytes, and every refusal comes
back non-zero with a text that names the call and the argument -- all array pointers are null, nothing is launched."""
import ctypes as C

import pytest


def _args(**over):
    """Arguments that pass every auto-reset check (and then fail on the first null array: nothing is launched)."""
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.device_env import reset_cfg
    a = dict(params=_abi.params_from(), state=_abi.AsvEnvState(), ctl=_abi.AsvStepCtl(), out=_abi.AsvStepOut(),
             ro=_abi.AsvRollout(), pi=_abi.AsvPolicy(), ar=_abi.AsvAutoReset())
    a["state"].n_envs, a["state"].max_robots, a["state"].max_obs, a["state"].max_cores = 4, 5, 4, 2
    a["ctl"].is_continuous, a["ctl"].do_dynamics, a["ctl"].trainer_deactivate, a["ctl"].noise_mode = 1, 1, 1, 2
    a["out"].env_done = 0x1000   # never dereferenced: the call stops at the first null array
    a["ro"].n_steps = 3
    a["ar"].cfg = reset_cfg(5, 4, 2)
    for k, v in over.items():
        obj, field = k.split("__")
        setattr(a[obj], field, v)
    return a


def _call(L, closed, a, ar_null=False):
    ar = None if ar_null else C.byref(a["ar"])
    if closed:
        return L.asvrl_policy_rollout_ar(C.byref(a["params"]), C.byref(a["state"]), C.byref(a["ctl"]), C.byref(a["out"]),
                                         C.byref(a["ro"]), C.byref(a["pi"]), ar, None, None)
    return L.asvrl_env_rollout_ar(C.byref(a["params"]), C.byref(a["state"]), C.byref(a["ctl"]), C.byref(a["out"]),
                                  C.byref(a["ro"]), ar, None, None)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_struct_sizes(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    assert L.asvrl_autoreset_struct_size() == C.sizeof(_abi.AsvAutoReset) == 96 + 16 + 4 * 8
    assert L.asvrl_rollout_struct_size() == C.sizeof(_abi.AsvRollout) == 88
    assert L.asvrl_policy_struct_size() == C.sizeof(_abi.AsvPolicy)
    assert L.asvrl_abi_version() == 29


REFUSALS = [
    # (overrides, ar NULL, open loop only, words the error text carries)
    ({}, True, False, ["null ar"]),
    ({"ro__hold_done": 1}, False, False, ["hold_done"]),
    ({"ctl__trainer_deactivate": 0}, False, False, ["trainer_deactivate", "env_done"]),
    ({"out__env_done": None}, False, False, ["trainer_deactivate", "env_done"]),
    ({"ctl__noise_mode": 0}, False, False, ["noise_mode 0"]),
    ({"ar__obs_prev": 0x2000}, False, True, ["obs_prev", "obs_in"]),
    ({"state__max_robots": 33}, False, False, ["num_robots"]),
    ({"state__max_obs": 33}, False, False, ["num_obs"]),
    ({"state__max_cores": 17}, False, False, ["num_cores"]),
]


@pytest.mark.parametrize("closed", [False, True], ids=["env_rollout_ar", "policy_rollout_ar"])
@pytest.mark.parametrize("over,ar_null,open_only,words", REFUSALS)
def test_refusals_name_the_call_and_the_argument(over, ar_null, open_only, words, closed):
    from distributional_rl_decision_and_control_amd import _abi
    if open_only and closed:
        over = {}   # the closed loop takes pi->obs_in: this combination is accepted there (checked below)
    L = _abi.lib()
    rc = _call(L, closed, _args(**over), ar_null)
    assert rc != 0
    msg = L.asvrl_last_error().decode()
    name = "asvrl_policy_rollout_ar" if closed else "asvrl_env_rollout_ar"
    assert msg.startswith(name + ":"), msg
    if open_only and closed:
        assert "obs_prev" not in msg, msg
        return
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("closed", [False, True], ids=["env_rollout_ar", "policy_rollout_ar"])
def test_cfg_counts_beyond_the_reset_tables(closed):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib()
    for field, word in (("num_robots", "num_robots"), ("num_obs", "num_obs"), ("num_cores", "num_cores")):
        a = _args()
        setattr(a["ar"].cfg, field, 33 if field != "num_cores" else 17)
        assert _call(L, closed, a) != 0
        assert word in L.asvrl_last_error().decode()


@pytest.mark.parametrize("closed", [False, True], ids=["env_rollout_ar", "policy_rollout_ar"])
def test_what_the_plain_calls_refuse_is_still_refused(closed):
    """Past the auto-reset checks the two calls' own checks run, under the new call's name."""
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib()
    name = "asvrl_policy_rollout_ar" if closed else "asvrl_env_rollout_ar"
    assert _call(L, closed, _args(ro__n_steps=0)) != 0
    assert L.asvrl_last_error().decode() == f"{name}: n_steps must be >= 1"
    assert _call(L, closed, _args()) != 0   # null actions (open loop) / null obs_in (closed loop)
    msg = L.asvrl_last_error().decode()
    assert msg.startswith(name + ": null"), msg
    assert L.asvrl_env_rollout_ar(None, None, None, None, None, None, None, None) != 0
    assert b"asvrl_env_rollout_ar: null argument" in L.asvrl_last_error()


def test_push_window_refusals():
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib()
    P = 0x1000   # never dereferenced
    rc = L.asvrl_replay_push_window(None, None, None, None, 2, 2, None, None, 8, 2, None, None, 64, None, None, None,
                                    None, 2, None)
    assert rc != 0 and b"asvrl_replay_push_window: null argument" in L.asvrl_last_error()
    rc = L.asvrl_replay_push_window(P, P, P, P, 2, 2, P, P, 33, 2, None, P, 64, P, P, None, None, 2, None)
    assert rc != 0
    msg = L.asvrl_last_error().decode()
    assert msg.startswith("asvrl_replay_push_window:") and "capacity" in msg, msg
    rc = L.asvrl_replay_push_window(P, P, P, P, 3, 3, P, P, 8, 2, None, P, 64, P, P, None, None, 2, None)
    assert rc != 0 and b"action_dim" in L.asvrl_last_error()
