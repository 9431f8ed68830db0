"""CPU: the binding of asvrl_rainbow_net_act_ex, asvrl_rainbow_rollout, asvrl_rainbow_rollout_ar and
asvrl_per_push_window (new entry points, ABI 29). sizeof(AsvRainbowActEx) and sizeof(AsvRainbowPolicy) agree between
ctypes and both compiled libraries, and every refusal comes back non-zero with its exact text. The checks fail before
anything is launched: the pointers below are made-up addresses that are never dereferenced."""
import ctypes as C

import pytest

import rollout_abi_cases
from rollout_abi_cases import P

RO = rollout_abi_cases.Rollout("rainbow")
NAMES, IMAGES = RO.names, RO.images
_refused = RO.refused


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_exports_struct_sizes_and_abi_version(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    for name in NAMES + ("asvrl_rainbow_net_act_ex", "asvrl_rainbow_act_ex_struct_size",
                         "asvrl_rainbow_policy_struct_size", "asvrl_per_push_window"):
        assert hasattr(L, name), name
    # robots_per_env and its padding, step_add, the four pointers, ld_q
    assert C.sizeof(_abi.AsvRainbowActEx) == 4 + 4 + 8 + 4 * 8 + 8
    assert L.asvrl_rainbow_act_ex_struct_size() == C.sizeof(_abi.AsvRainbowActEx)
    # the images, support, obs_in and step_dev, the five schedule doubles, seed, actions
    assert C.sizeof(_abi.AsvRainbowPolicy) == C.sizeof(_abi.AsvRainbowImg) + 3 * 8 + 5 * 8 + 8 + 8
    assert L.asvrl_rainbow_policy_struct_size() == C.sizeof(_abi.AsvRainbowPolicy)
    assert L.asvrl_abi_version() == 29 == _abi.ABI_VERSION
    # no existing struct changed: the sizes of the parent commit
    assert C.sizeof(_abi.AsvRainbowImg) == 23 * 8 and C.sizeof(_abi.AsvRainbowNetIO) == 272
    assert C.sizeof(_abi.AsvPer) == 6 * 8 + 2 * 8 + 2 * 4 + 8 + 2 * 4 + 2 * 4
    assert L.asvrl_iqn_policy_struct_size() == C.sizeof(_abi.AsvIqnPolicy)
    assert L.asvrl_iqn_act_ex_struct_size() == C.sizeof(_abi.AsvIqnActEx) == 56


@pytest.mark.parametrize("ops", ["bf16", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_refusals_of_both_rollout_entry_points(name, ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    for k in ("params", "state", "ctl", "out", "ro"):
        _refused(L, name, "null argument", null=(k,))
    _refused(L, name, "null policy", null=("pi",))
    _refused(L, name, "null obs_in", pi__obs_in=None)
    _refused(L, name, "is_continuous must be 0 (Rainbow's actions are indices)", ctl__is_continuous=1)
    _refused(L, name, "ro->actions must be null (the policy supplies the actions)", ro__actions=P)
    for img in IMAGES:
        _refused(L, name, "null Rainbow image", **{"w__" + img: None})
    _refused(L, name, "null pi->support", pi__support=None)
    _refused(L, name, "pi->eps_total and pi->eps_fraction must be > 0", pi__eps_total=0.0)
    _refused(L, name, "pi->eps_total and pi->eps_fraction must be > 0", pi__eps_fraction=0.0)
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
    name = "asvrl_rainbow_rollout"
    _refused(L, name, "hold_done needs trainer_deactivate", ro__hold_done=1, ctl__trainer_deactivate=0)
    _refused(L, name, "noise_mode 0 needs injected noise", ctl__noise_mode=0)
    _refused(L, name, "hold_done and the env_done record need trainer_deactivate and out->env_done", ro__hold_done=1,
             out__env_done=None)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_auto_reset_refusals(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    name = "asvrl_rainbow_rollout_ar"
    _refused(L, name, "null ar (the auto-reset description)", null=("ar",))
    _refused(L, name, "ro->hold_done cannot be combined with the auto-reset", ro__hold_done=1)
    _refused(L, name, "noise_mode 0 (recorded noise) cannot cover a sampled reset; Philox noise only (mode 1 or 2)",
             ctl__noise_mode=0)
    need = "the auto-reset needs ctl->trainer_deactivate and last->env_done"
    _refused(L, name, need, out__env_done=None)
    _refused(L, name, need, ctl__trainer_deactivate=0)
    _refused(L, name, "observation rows must be 16-byte aligned", ar__obs_prev=P + 4)


ACT = rollout_abi_cases.WindowAct("rainbow")
_act_refused = ACT.refused


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_refusals_of_the_window_act(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    for k in ("w", "io"):
        _act_refused(L, "asvrl_rainbow_net: null argument", null=(k,))
    _act_refused(L, "asvrl_rainbow_net_act_ex: null ex", null=("ex",))
    for img in IMAGES:
        _act_refused(L, "asvrl_rainbow_net: null weight image", **{"w__" + img: None})
    for over in (dict(io__x=None), dict(io__ldx=36), dict(io__ldx=42), dict(io__x=P + 4)):
        _act_refused(L, "asvrl_rainbow_net: obs rows must be 16-byte aligned with ldx >= 40", **over)
    _act_refused(L, "asvrl_rainbow_net: null support", io__support=None)
    need = "asvrl_rainbow_net_act_ex: needs act_out with ld_act (or act_pair / rec_row) and the epsilon schedule"
    _act_refused(L, need, io__act_out=None)
    _act_refused(L, need, io__ld_act=0)
    _act_refused(L, need, io__eps_total=0.0)
    _act_refused(L, need, io__eps_fraction=0.0)
    for rpe in (0, -1):
        _act_refused(L, "asvrl_rainbow_net_act_ex: robots_per_env must be >= 1", ex__robots_per_env=rpe)
    for ld in (24, 0, -25):
        _act_refused(L, "asvrl_rainbow_net_act_ex: ld_q must be >= 25", ex__q_out=P, ex__ld_q=ld)


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_the_existing_act_call_is_unchanged(ops):
    """asvrl_rainbow_net_act keeps its struct, its checks and their texts: the window form is a call of its own."""
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    for over, text in ((dict(io__act_out=None), "asvrl_rainbow_net_act: needs act_out"),
                       (dict(io__step_dev=P, io__eps_total=0.0), "asvrl_rainbow_net_act: bad epsilon schedule"),
                       (dict(io__support=None), "asvrl_rainbow_net: null support")):
        ACT.plain_refused(L, text, **over)


def _per(**over):
    from distributional_rl_decision_and_control_amd import _abi
    per = _abi.AsvPer()
    for n in ("rows", "tree", "state", "t", "maxp", "dirty"):
        setattr(per, n, P)
    per.capacity, per.tree_leaves, per.stride, per.n_step, per.discount = 185 * 40, 8192, 185, 3, 0.99
    per.priority_weight, per.priority_exponent, per.deferred = 0.4, 0.5, 1
    for k, v in over.items():
        setattr(per, k, v)
    return per


def _push_refused(L, text, per=None, n=185 * 5, counter_by=5, null=()):
    args = dict(obs=P, obj_cnt=P, actions=P, reward=P, done=P)
    for k in null:
        args[k] = None
    rc = L.asvrl_per_push_window(C.byref(per if per is not None else _per()), args["obs"], args["obj_cnt"],
                                 args["actions"], 2, args["reward"], args["done"], n, P, counter_by, None)
    assert rc != 0, text
    assert L.asvrl_last_error().decode() == text


def test_refusals_of_the_window_push():
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib()
    for by in (0, -1):
        _push_refused(L, "asvrl_per_push_window: counter_by must be >= 1", counter_by=by)
    stride = "asvrl_per_push: n must be a multiple of stride and <= capacity"
    _push_refused(L, stride, n=185 * 5 + 1)
    _push_refused(L, stride, n=184)
    _push_refused(L, stride, n=185 * 41)
    _push_refused(L, stride, n=-185)
    for k in ("obs", "obj_cnt", "actions", "reward", "done"):
        _push_refused(L, "asvrl_per_push: null argument", null=(k,))
    _push_refused(L, "asvrl_per_push: null AsvPer member", per=_per(tree=None))
    _push_refused(L, "asvrl_per_push: capacity must be a multiple of stride", per=_per(stride=7))
    # n = 0 pushes nothing and launches nothing: the early return of asvrl_per_push_ex
    assert L.asvrl_per_push_window(C.byref(_per()), P, P, P, 2, P, P, 0, P, 5, None) == 0
