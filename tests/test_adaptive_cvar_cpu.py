"""CPU: the adaptive risk level on the host. Agent.adjust_cvar (the reference's commented-out rule, agent.py:342-358,
with a floor) on hand-built (self, objects) states, Agent.act_adaptive_iqn over act_iqn, fused_iqn.AdaptiveCvar's
validation, and AdaptiveCvar.levels -- the same rule in torch f32 on the packed rows -- against adjust_cvar.

The Agent here is a bare instance around a CPU IQN_Policy: its constructor insists on the GPU, the two methods under
test do not need one."""
import random
import types

import numpy as np
import pytest
import torch

MARGIN, RADIUS = 2.8, 0.5
SELF = [1.0, -2.0, 0.5, 0.1, 0.0, 0.3, -0.2]


def _state(d=None, angle=0.9, extra=()):
    """A robot whose nearest object's surface is d + margin away (d None: no object at all)."""
    if d is None:
        return (list(SELF), [])
    rho = d + MARGIN + RADIUS
    objs = [[rho * np.cos(angle), rho * np.sin(angle), 0.4, -0.3, RADIUS]]
    return (list(SELF), objs + [list(o) for o in extra])


FAR = [30.0, 5.0, 0.0, 0.1, 1.0]
# (state, the level): no object, beyond near, the linear part, under the floor, inside the margin
CASES = [(_state(None), 1.0), (_state(12.0), 1.0), (_state(5.0, extra=[FAR]), 0.5), (_state(0.3), 0.1),
         (_state(-1.0, extra=[FAR, FAR]), 0.1)]


def _agent():
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.policy.IQN_model import IQN_Policy
    from distributional_rl_decision_and_control_amd.utils.replay_buffer import ReplayBuffer
    from distributional_rl_decision_and_control_amd.vec_trainer import DEFAULT_NET
    ag = object.__new__(Agent)
    ag.device, ag.action_size, ag.agent_type = torch.device("cpu"), 25, "IQN"
    ag.policy_local = IQN_Policy(**DEFAULT_NET, action_size=25, device="cpu", seed=100)
    shape = types.SimpleNamespace(obj_len=5, max_obj_num=5)
    ag.memory = types.SimpleNamespace(state_batch=lambda states: ReplayBuffer.state_batch(shape, states))
    return ag


@pytest.mark.parametrize("state, level", CASES)
def test_adjust_cvar(state, level):
    from distributional_rl_decision_and_control_amd.agent import Agent
    got = Agent.adjust_cvar(None, state)
    assert isinstance(got, float) and got == pytest.approx(level, abs=1e-12)
    if level in (1.0, 0.1):
        assert got == level   # the ends are the constants themselves


def test_adjust_cvar_parameters():
    from distributional_rl_decision_and_control_amd.agent import Agent
    s = _state(5.0)   # d = 5 under the default margin: 6.8 under margin 1
    assert Agent.adjust_cvar(None, s, near=20.0) == pytest.approx(0.25, abs=1e-12)
    assert Agent.adjust_cvar(None, s, near=6.0, margin=1.0, floor=0.25) == 1.0
    assert Agent.adjust_cvar(None, _state(0.3), floor=0.25) == 0.25
    with pytest.raises(AssertionError):
        Agent.adjust_cvar(None, (SELF, [], []))


def test_act_adaptive_iqn_is_act_iqn_at_that_level():
    ag = _agent()
    taus = torch.rand(1, ag.policy_local.K, generator=torch.Generator().manual_seed(3))
    for state, level in CASES:
        random.seed(1)
        out = ag.act_adaptive_iqn(state, taus=taus)
        assert len(out) == 4
        action, quantiles, used, cvar = out
        assert cvar == pytest.approx(level, abs=1e-12) and cvar == ag.adjust_cvar(state)
        random.seed(1)
        a2, q2, t2 = ag.act_iqn(state, cvar=cvar, taus=taus)
        assert action == a2 and np.array_equal(quantiles, q2) and np.array_equal(used, t2)
        assert quantiles.shape == (1, ag.policy_local.K, 25)
    # the level matters: the floor state's quantiles differ from its risk-neutral ones
    _, q_floor, _, _ = ag.act_adaptive_iqn(CASES[3][0], taus=taus)
    _, q_one, _ = ag.act_iqn(CASES[3][0], cvar=1.0, taus=taus)
    assert not np.array_equal(q_floor, q_one)


def test_levels_on_packed_rows_agree_with_adjust_cvar():
    from distributional_rl_decision_and_control_amd.agent import Agent
    from distributional_rl_decision_and_control_amd.fused_iqn import AdaptiveCvar
    from distributional_rl_decision_and_control_amd.utils.replay_buffer import pack_state
    rows = np.zeros((len(CASES), 40), np.float32)
    for i, (state, _) in enumerate(CASES):
        pack_state(state, 5, 5, rows[i])
    x = torch.from_numpy(rows)
    assert x[:, 32].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0]
    lev = AdaptiveCvar().levels(x)
    assert lev.dtype == torch.float32 and tuple(lev.shape) == (len(CASES),)
    want = [Agent.adjust_cvar(None, s) for s, _ in CASES]
    assert np.abs(lev.numpy().astype(np.float64) - np.array(want)).max() <= 1e-6
    assert lev[0] == 1.0 and lev[1] == 1.0 and lev[3] == np.float32(0.1) and lev[4] == np.float32(0.1)
    other = AdaptiveCvar(near=6.0, margin=1.0, floor=0.25)
    want = [Agent.adjust_cvar(None, s, near=6.0, margin=1.0, floor=0.25) for s, _ in CASES]
    assert np.abs(other.levels(x).numpy().astype(np.float64) - np.array(want)).max() <= 1e-6
    # any leading shape: [K, rows, 40] as the windows record it
    assert torch.equal(AdaptiveCvar().levels(x.expand(3, -1, -1)), lev.expand(3, -1))


@pytest.mark.parametrize("kw", [dict(near=0.0), dict(near=-1.0), dict(near=float("nan")), dict(near=float("inf")),
                                dict(margin=float("inf")), dict(margin=float("nan")), dict(floor=0.0),
                                dict(floor=-0.5), dict(floor=1.5), dict(floor=float("nan"))])
def test_adaptive_cvar_refuses(kw):
    from distributional_rl_decision_and_control_amd.fused_iqn import AdaptiveCvar
    with pytest.raises(ValueError):
        AdaptiveCvar(**kw)


def test_adaptive_cvar_is_a_frozen_value():
    import dataclasses
    from distributional_rl_decision_and_control_amd.fused_iqn import AdaptiveCvar
    a = AdaptiveCvar()
    assert (a.near, a.margin, a.floor) == (10.0, 2.8, 0.1)
    assert a == AdaptiveCvar(10, 2.8, 0.1) and hash(a) == hash(AdaptiveCvar(10, 2.8, 0.1))
    assert a.as_dict() == {"near": 10.0, "margin": 2.8, "floor": 0.1}
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.floor = 0.5
    assert AdaptiveCvar(floor=1.0).floor == 1.0
