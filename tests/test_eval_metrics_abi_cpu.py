"""CPU: the binding of asvrl_eval_metrics. sizeof(AsvEvalMetrics) agrees between ctypes and both compiled libraries,
and every argument error comes back as a status with an asvrl_last_error text that names the call and the argument.
The checks fail before anything is launched: the array pointers are null or never dereferenced."""
import ctypes as C

import pytest

ARRAYS = ("reward", "info", "rs", "steps_run", "n_robots", "dt", "N", "pc", "length", "ended", "alive", "deact",
          "outcome", "ret", "time", "energy")


def test_eval_metrics_struct_size():
    from distributional_rl_decision_and_control_amd import _abi
    assert C.sizeof(_abi.AsvEvalMetrics) == 4 * 4 + 8 + len(ARRAYS) * 8
    assert [n for n, _ in _abi.AsvEvalMetrics._fields_[5:]] == list(ARRAYS)
    for ops in ("bf16", "f32"):
        assert _abi.lib(ops).asvrl_eval_metrics_struct_size() == C.sizeof(_abi.AsvEvalMetrics)
    # nothing else moved
    assert _abi.lib().asvrl_abi_version() == 29
    assert C.sizeof(_abi.AsvRollout) == 88 and C.sizeof(_abi.AsvAutoReset) == 144 and C.sizeof(_abi.AsvParams) == 480


def _call(L, null_struct=False, n_steps=5, n_envs=11, max_robots=5, missing=None):
    from distributional_rl_decision_and_control_amd import _abi
    m = _abi.AsvEvalMetrics()
    m.n_steps, m.n_envs, m.max_robots, m.episode_limit, m.gamma = n_steps, n_envs, max_robots, 1000, 0.99
    for name in ARRAYS:
        setattr(m, name, None if name == missing else 0x1000)   # never dereferenced: every call below is refused
    return L.asvrl_eval_metrics(None if null_struct else C.byref(m), None)


CASES = [(dict(null_struct=True), b"null struct"), (dict(n_steps=0), b"n_steps"), (dict(n_steps=-3), b"n_steps"),
         (dict(max_robots=0), b"max_robots"), (dict(max_robots=33), b"max_robots"), (dict(n_envs=0), b"n_envs")]
CASES += [(dict(missing=name), name.encode()) for name in ARRAYS]


@pytest.mark.parametrize("ops", ["bf16", "f32"])
@pytest.mark.parametrize("kw,text", CASES, ids=[str(sorted(kw.items())[0]) for kw, _ in CASES])
def test_eval_metrics_argument_errors(ops, kw, text):
    from distributional_rl_decision_and_control_amd import _abi
    L = _abi.lib(ops)
    rc = _call(L, **kw)
    assert rc != 0
    msg = L.asvrl_last_error()
    assert msg.startswith(b"asvrl_eval_metrics: ") and text in msg, msg
    if "missing" in kw:
        assert msg.endswith(b" " + text), msg   # the array's own name, not one that contains it
