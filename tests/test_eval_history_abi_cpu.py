"""CPU: the binding of asvrl_eval_history_count / asvrl_eval_history_pack. Both builds export the four new symbols,
sizeof(AsvEvalHistory) and the step tile agree between ctypes and the compiled libraries, the ABI version and the
pinned struct sizes have not moved, and every argument error comes back as a status with an asvrl_last_error text
that names the call and the argument. The checks fail before anything is launched: the array pointers are null or
never dereferenced."""
import ctypes as C

import pytest

SYMBOLS = ("asvrl_eval_history_count", "asvrl_eval_history_pack", "asvrl_eval_history_struct_size",
           "asvrl_eval_history_step_tile")
COUNT_ARRAYS = ("info", "length", "n_robots", "counts")
PACK_ARRAYS = ("counts", "offsets", "rs0", "rs", "actions", "obs0", "obs", "cnt0", "obj_cnt", "traj", "act", "obs_out",
               "cnt_out")


@pytest.mark.parametrize("ops", ["bf16", "f32"])
def test_eval_history_exports_and_struct_size(ops):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    exported = {name for name, _, _ in _abi.EXPORTS}
    for name in SYMBOLS:
        assert name in exported and getattr(L, name) is not None, name
    arrays = [n for n, _ in _abi.AsvEvalHistory._fields_[4:-3]]
    assert arrays == list(_abi.HISTORY_ARRAYS) and set(COUNT_ARRAYS + PACK_ARRAYS) == set(arrays)
    assert C.sizeof(_abi.AsvEvalHistory) == 4 * 4 + len(arrays) * 8 + 3 * 8
    assert L.asvrl_eval_history_struct_size() == C.sizeof(_abi.AsvEvalHistory)
    assert L.asvrl_eval_history_step_tile() == _abi.HISTORY_STEP_TILE
    # additive: nothing else moved
    assert L.asvrl_abi_version() == 29 == _abi.ABI_VERSION
    assert C.sizeof(_abi.AsvRollout) == 88 == L.asvrl_rollout_struct_size()
    assert C.sizeof(_abi.AsvAutoReset) == 144 and C.sizeof(_abi.AsvParams) == 480
    assert L.asvrl_eval_metrics_struct_size() == C.sizeof(_abi.AsvEvalMetrics)


def test_trajectory_fields_are_the_reference_order():
    """wamv.py:191-193: x, y, theta, velocity_r, velocity, left_pos, right_pos, left_thrust, right_thrust."""
    from distributional_rl_decision_and_control_amd import _abi
    assert _abi.TRAJ_FIELDS == (0, 1, 2, 3, 4, 5, 6, 7, 8, _abi.F_LP, _abi.F_RP, _abi.F_TL, _abi.F_TR)
    assert len(_abi.TRAJ_FIELDS) == _abi.TRAJ_DIM == 13 and (_abi.F_LP, _abi.F_TL) == (11, 9)


def _call(L, entry, null_struct=False, n_steps=13, n_envs=11, max_robots=5, act_steps=13, missing=None, rows=7,
          misaligned=None):
    from distributional_rl_decision_and_control_amd import _abi
    h = _abi.AsvEvalHistory()
    h.n_steps, h.n_envs, h.max_robots, h.act_steps = n_steps, n_envs, max_robots, act_steps
    for name in _abi.HISTORY_ARRAYS:   # never dereferenced: every call below is refused
        setattr(h, name, None if name == missing else (0x1004 if name == misaligned else 0x1000))
    h.traj_rows = h.act_rows = h.obs_rows = rows
    return getattr(L, entry)(None if null_struct else C.byref(h), None)


COMMON = [(dict(null_struct=True), b"null struct"), (dict(n_steps=0), b"n_steps"), (dict(n_steps=-3), b"n_steps"),
          (dict(max_robots=0), b"max_robots"), (dict(max_robots=33), b"max_robots"), (dict(n_envs=0), b"n_envs")]
CASES = [("asvrl_eval_history_count", kw, text) for kw, text in COMMON]
CASES += [("asvrl_eval_history_count", dict(missing=n), n.encode()) for n in COUNT_ARRAYS]
CASES += [("asvrl_eval_history_pack", kw, text) for kw, text in COMMON]
CASES += [("asvrl_eval_history_pack", dict(missing=n), n.encode()) for n in PACK_ARRAYS]
CASES += [("asvrl_eval_history_pack", dict(act_steps=0), b"act_steps"),
          ("asvrl_eval_history_pack", dict(rows=-1), b"traj_rows"),
          ("asvrl_eval_history_pack", dict(misaligned="obs"), b"16-byte aligned"),
          ("asvrl_eval_history_pack", dict(misaligned="obs_out"), b"16-byte aligned")]


@pytest.mark.parametrize("ops", ["bf16", "f32"])
@pytest.mark.parametrize("entry,kw,text", CASES,
                         ids=[e.rsplit("_", 1)[1] + "-" + str(sorted(kw.items())[0]) for e, kw, _ in CASES])
def test_eval_history_argument_errors(ops, entry, kw, text):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    rc = _call(L, entry, **kw)
    assert rc != 0
    msg = L.asvrl_last_error()
    assert msg.startswith(entry.encode() + b": ") and text in msg, msg
    if "missing" in kw:
        assert msg.endswith(b" " + text), msg   # the array's own name, not one that contains it
