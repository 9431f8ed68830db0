"""CPU: the binding of asvrl_sac_rollout / asvrl_sac_rollout_ar (new entry points, ABI 29). sizeof(AsvSacPolicy)
agrees between ctypes and both compiled libraries, and every refusal comes back non-zero as
"<entry point>: <argument>". The checks fail before anything is launched: the pointers below are made-up
addresses that are never dereferenced."""
import ctypes as C

import pytest

P = 0x1000   # a made-up, 16-byte aligned address
NAMES = ("asvrl_sac_rollout", "asvrl_sac_rollout_ar")
IMAGES = ("enc_frag", "b_enc", "w1_frag", "w2_frag", "b1", "b2", "wout", "bout")


def _args(**over):
    """Arguments that pass every check of both calls up to the launch (nothing is launched: every test overrides
    one of them into a refusal). Overrides are obj__field=value; w__<image> sets a trunk image, sw__<name> the
    head's weight or bias."""
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.device_env import reset_cfg
    a = dict(params=_abi.params_from(), state=_abi.AsvEnvState(), ctl=_abi.AsvStepCtl(), out=_abi.AsvStepOut(),
             ro=_abi.AsvRollout(), pi=_abi.AsvSacPolicy(), ar=_abi.AsvAutoReset())
    st = a["state"]
    st.n_envs, st.max_robots, st.max_obs, st.max_cores = 4, 5, 4, 2
    for n in ("rs", "rflags", "n_robots", "n_obs", "n_cores", "ep_ts", "obstacles", "cores"):
        setattr(st, n, P)
    ctl = a["ctl"]
    ctl.is_continuous, ctl.do_dynamics, ctl.trainer_deactivate, ctl.noise_mode = 1, 1, 1, 2
    for n in ("obs", "obj_cnt", "reward", "done", "info", "env_done"):
        setattr(a["out"], n, P)
    a["ro"].n_steps = 3
    pi = a["pi"]
    pi.obs_in = P
    for n in IMAGES:
        setattr(pi.w.trunk, n, P)
    pi.w.head, pi.w.bhead = P, P
    a["ar"].cfg = reset_cfg(5, 4, 2)
    for k, v in over.items():
        obj, field = k.split("__")
        setattr(a["pi"].w.trunk if obj == "w" else (a["pi"].w if obj == "sw" else a[obj]), field, v)
    return a


def _call(L, name, a, null=()):
    order = ["params", "state", "ctl", "out", "ro", "pi"] + (["ar"] if name.endswith("_ar") else [])
    return getattr(L, name)(*[None if k in null else C.byref(a[k]) for k in order], None, None)


def _refused(L, name, text, null=(), **over):
    assert _call(L, name, _args(**over), null) != 0, (name, text)
    assert L.asvrl_last_error().decode() == f"{name}: {text}"


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_struct_size_and_abi_version(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    # the weights, obs_in and step_dev, the five schedule doubles, seed, actions, deterministic and its padding
    assert C.sizeof(_abi.AsvSacPolicy) == C.sizeof(_abi.AsvSacActorWeights) + 2 * 8 + 5 * 8 + 8 + 8 + 4 + 4
    assert L.asvrl_sac_policy_struct_size() == C.sizeof(_abi.AsvSacPolicy)
    assert L.asvrl_sac_actor_weights_struct_size() == C.sizeof(_abi.AsvSacActorWeights)
    assert L.asvrl_abi_version() == 29 == _abi.ABI_VERSION
    # no existing struct changed
    assert L.asvrl_policy_struct_size() == C.sizeof(_abi.AsvPolicy)
    assert L.asvrl_dqn_policy_struct_size() == C.sizeof(_abi.AsvDqnPolicy)
    assert L.asvrl_sac_act_struct_size() == C.sizeof(_abi.AsvSacActIO)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_refusals_of_both_entry_points(name, ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    for k in ("params", "state", "ctl", "out", "ro"):
        _refused(L, name, "null argument", null=(k,))
    _refused(L, name, "null policy", null=("pi",))
    _refused(L, name, "null obs_in", pi__obs_in=None)
    _refused(L, name, "is_continuous must be 1 (SAC's actions are continuous)", ctl__is_continuous=0)
    _refused(L, name, "ro->actions must be null (the policy supplies the actions)", ro__actions=P)
    for img in IMAGES:
        _refused(L, name, "null SAC actor image", **{"w__" + img: None})
    _refused(L, name, "null pi->w.head", sw__head=None)
    _refused(L, name, "null pi->w.bhead", sw__bhead=None)
    _refused(L, name, "observation rows must be 16-byte aligned", pi__obs_in=P + 4)
    _refused(L, name, "observation rows must be 16-byte aligned", out__obs=P + 8)
    # the rollout's own members, under the new call's name
    _refused(L, name, "n_steps must be >= 1", ro__n_steps=0)
    _refused(L, name, "do_dynamics must be 1", ctl__do_dynamics=0)
    _refused(L, name, "null output", out__reward=None)
    _refused(L, name, "null state array", state__rs=None)
    _refused(L, name, "max_robots must be in [1, 256]", state__max_robots=0)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_plain_call_only_refusals(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    name = "asvrl_sac_rollout"
    _refused(L, name, "hold_done needs trainer_deactivate", ro__hold_done=1, ctl__trainer_deactivate=0)
    _refused(L, name, "noise_mode 0 needs injected noise", ctl__noise_mode=0)
    _refused(L, name, "hold_done and the env_done record need trainer_deactivate and out->env_done", ro__hold_done=1,
             out__env_done=None)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_auto_reset_refusals(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    name = "asvrl_sac_rollout_ar"
    _refused(L, name, "null ar (the auto-reset description)", null=("ar",))
    _refused(L, name, "ro->hold_done cannot be combined with the auto-reset", ro__hold_done=1)
    _refused(L, name, "noise_mode 0 (recorded noise) cannot cover a sampled reset; Philox noise only (mode 1 or 2)",
             ctl__noise_mode=0)
    need = "the auto-reset needs ctl->trainer_deactivate and last->env_done"
    _refused(L, name, need, out__env_done=None)
    _refused(L, name, need, ctl__trainer_deactivate=0)
    _refused(L, name, "observation rows must be 16-byte aligned", ar__obs_prev=P + 4)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_the_actor_call_is_unchanged(ops):
    """asvrl_policy_rollout keeps its struct, its checks and their texts: the SAC dispatch is a call of its own."""
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)

    def call(pol, **over):
        a = _args(**over)
        return L.asvrl_policy_rollout(C.byref(a["params"]), C.byref(a["state"]), C.byref(a["ctl"]), C.byref(a["out"]),
                                      C.byref(a["ro"]), None if pol is None else C.byref(pol), None, None)

    def policy(**over):
        pol = _abi.AsvPolicy()
        pol.obs_in = P
        for n in IMAGES:
            setattr(pol.w, n, P)
        for k, v in over.items():
            setattr(pol.w if k in IMAGES else pol, k, v)
        return pol

    for pol, over, text in ((None, {}, "null policy"), (policy(obs_in=None), {}, "null obs_in"),
                            (policy(), dict(ctl__is_continuous=0),
                             "is_continuous must be 1 (the Actor is the continuous agent)"),
                            (policy(wout=None), {}, "null actor image"),
                            (policy(), dict(ro__actions=P), "ro->actions must be null (the policy supplies the actions)"),
                            (policy(obs_in=P + 4), {}, "observation rows must be 16-byte aligned")):
        assert call(pol, **over) != 0, text
        assert L.asvrl_last_error().decode() == f"asvrl_policy_rollout: {text}"
