"""CPU: the checks the twelve rollout calls share. The two open-loop calls (asvrl_env_rollout, asvrl_env_rollout_ar)
and the ten closed-loop ones (the Actor, DQN_Policy, SAC's sampled actor, IQN_Policy and Rainbow_Policy, each plain
and with the auto-reset) go through one host path, so a refusal that applies to several of them comes back as
"<call name>: <text>" with the same text from each. The checks fail before anything is launched: the pointers below
are made-up addresses that are never dereferenced."""
import ctypes as C

import pytest

P = 0x1000   # a made-up, 16-byte aligned address
MLP_IMAGES = ("enc_frag", "b_enc", "w1_frag", "w2_frag", "b1", "b2", "wout", "bout")


def _actor(_abi):
    pi = _abi.AsvPolicy()
    for n in MLP_IMAGES:
        setattr(pi.w, n, P)
    return pi, 1


def _dqn(_abi):
    pi = _abi.AsvDqnPolicy()
    for n in MLP_IMAGES:
        setattr(pi.w.trunk, n, P)
    pi.w.head_frag, pi.w.n_actions = P, 25
    return pi, 0


def _sac(_abi):
    pi = _abi.AsvSacPolicy()
    for n in MLP_IMAGES:
        setattr(pi.w.trunk, n, P)
    pi.w.head, pi.w.bhead = P, P
    return pi, 1


def _iqn(_abi):
    pi = _abi.AsvIqnPolicy()
    for n in ("wc_frag", "w1_frag", "w2_frag", "bc", "b1", "b2", "self_w", "self_b", "obj_w", "obj_b"):
        setattr(pi.w, n, P)
    pi.head.wo_frag, pi.head.bo, pi.head.n_actions, pi.cvar = P, P, 9, 1.0
    return pi, 0


def _rainbow(_abi):
    pi = _abi.AsvRainbowPolicy()
    for n in ("enc", "v1", "a1", "v2", "a2", "vo", "mo", "ao", "b_enc", "b_v1p", "b_a1p", "b_v2p", "b_a2p", "b_vop",
              "b_mop", "b_aop"):
        setattr(pi.w, n, P)
    pi.support = P
    pi.eps_steps_per_count, pi.eps_total, pi.eps_fraction = 1.0, 1.0, 1.0
    return pi, 0


# call name -> its policy (None: the open loop)
POLICIES = {"asvrl_env_rollout": None, "asvrl_policy_rollout": _actor, "asvrl_dqn_rollout": _dqn,
            "asvrl_sac_rollout": _sac, "asvrl_iqn_rollout": _iqn, "asvrl_rainbow_rollout": _rainbow}
PLAIN = tuple(POLICIES)
RESET = tuple(n + "_ar" for n in PLAIN)
ALL = PLAIN + RESET
CLOSED = tuple(n for n in ALL if POLICIES[n.removesuffix("_ar")] is not None)


def _args(name, **over):
    """Arguments that pass every check of the call `name` up to the launch (nothing is launched: every test overrides
    one of them into a refusal). Overrides are obj__field=value."""
    from distributional_rl_decision_and_control_amd import _abi
    from distributional_rl_decision_and_control_amd.device_env import reset_cfg
    a = dict(params=_abi.params_from(), state=_abi.AsvEnvState(), ctl=_abi.AsvStepCtl(), out=_abi.AsvStepOut(),
             ro=_abi.AsvRollout(), ar=_abi.AsvAutoReset(), launch=_abi.AsvEnvLaunch())
    st = a["state"]
    st.n_envs, st.max_robots, st.max_obs, st.max_cores = 4, 5, 4, 2
    for n in ("rs", "rflags", "n_robots", "n_obs", "n_cores", "ep_ts", "obstacles", "cores"):
        setattr(st, n, P)
    ctl = a["ctl"]
    ctl.do_dynamics, ctl.trainer_deactivate, ctl.noise_mode = 1, 1, 2
    for n in ("obs", "obj_cnt", "reward", "done", "info", "env_done"):
        setattr(a["out"], n, P)
    a["ro"].n_steps = 3
    make = POLICIES[name.removesuffix("_ar")]
    if make is None:
        a["ro"].actions = P
    else:
        a["pi"], ctl.is_continuous = make(_abi)
        a["pi"].obs_in = P
    a["ar"].cfg = reset_cfg(5, 4, 2)
    for k, v in over.items():
        obj, field = k.split("__")
        setattr(a[obj], field, v)
    return a


def _refused(L, name, text, null=(), **over):
    a = _args(name, **over)
    order = ["params", "state", "ctl", "out", "ro"] + (["pi"] if "pi" in a else []) + \
        (["ar"] if name.endswith("_ar") else []) + ["launch"]
    rc = getattr(L, name)(*[None if k in null else C.byref(a[k]) for k in order], None)
    assert rc != 0, (name, text)
    assert L.asvrl_last_error().decode() == f"{name}: {text}"


@pytest.fixture(params=["bf16", "f32"])
def L(request):
    from distributional_rl_decision_and_control_amd import _abi
    return _abi.lib(request.param)


def test_the_twelve_calls():
    assert len(ALL) == 12 and len(CLOSED) == 10 and len(RESET) == 6


@pytest.mark.parametrize("name", ALL)
def test_every_rollout_call(L, name):
    _refused(L, name, "null argument", null=("params",))
    _refused(L, name, "n_steps must be >= 1", ro__n_steps=0)
    _refused(L, name, "do_dynamics must be 1", ctl__do_dynamics=0)
    _refused(L, name, "layout must be 0 (auto), 1 (pairs) or 2 (sweep)", launch__layout=3)


@pytest.mark.parametrize("name", CLOSED)
def test_every_closed_loop_call(L, name):
    _refused(L, name, "ro->actions must be null (the policy supplies the actions)", ro__actions=P)
    _refused(L, name, "null policy", null=("pi",))
    _refused(L, name, "null obs_in", pi__obs_in=None)
    _refused(L, name, "observation rows must be 16-byte aligned", pi__obs_in=P + 4)


@pytest.mark.parametrize("name", RESET)
def test_every_auto_reset_call(L, name):
    _refused(L, name, "null ar (the auto-reset description)", null=("ar",))
    _refused(L, name, "ro->hold_done cannot be combined with the auto-reset", ro__hold_done=1)
    _refused(L, name, "noise_mode 0 (recorded noise) cannot cover a sampled reset; Philox noise only (mode 1 or 2)",
             ctl__noise_mode=0)


def test_the_open_loop_auto_reset_takes_its_rows_from_ar(L):
    """The one call whose obs_in is the auto-reset's own: its misaligned rows are refused under that member's name."""
    _refused(L, "asvrl_env_rollout_ar", "ar->obs_in / ar->obs_prev rows must be 16-byte aligned", ar__obs_in=P + 4,
             ar__obs_prev=P)
