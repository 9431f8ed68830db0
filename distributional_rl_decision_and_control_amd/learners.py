"""The learner table: one entry per agent_type with the facts VecTrainer and the drop-in Agent need -- the policy
class, one network or actor + critic, the replay kind, the shapes the kernels take and how the fused state (packs and
buffers) is built. The Fused*State classes share one surface, so neither front end tests for the type:

    act(obs, actions, step, E, total, fraction, initial, final, seed)      the batched epsilon-greedy act kernel
    learn(tr, state, guard, actor_wait, target_wait, actor_done)           VecTrainer's sample + update
    target_changed() / refresh_local()                                     re-pack the target / local weight images
    target_step(tr)                                                        VecTrainer target_update="device": one
                                                                           asvrl_target_update_pack per target network
                                                                           (blend + re-pack, predicated on the device
                                                                           learn counter; Rainbow: the blend alone)
    window_pack                                                            the training-mode pack of the closed-loop
                                                                           windows (VecTrainer._collect_window)
    eval_pack                                                              what DeviceEvaluator.run takes (Rainbow: the
                                                                           mu-only images, re-packed on every read;
                                                                           every other learner: window_pack itself)
    policy_pack, actor_pack                                                what VecTrainer.policy_pack() and collect /
                                                                           greedy_episodes / evaluate go by: None
                                                                           where they refuse the agent type
"""
from dataclasses import dataclass
from typing import Callable, Optional

from . import fused_ddpg, fused_dqn, fused_iqn, fused_rainbow, fused_sac, fused_update
from .policy.AC_IQN_model import AC_IQN_Policy
from .policy.DDPG_model import DDPG_Policy
from .policy.DQN_model import DQN_Policy
from .policy.IQN_model import IQN_Policy
from .policy.Rainbow_model import Rainbow_Policy
from .policy.SAC_model import SAC_Policy


@dataclass(frozen=True)
class Learner:
    policy: type
    field: str              # VecTrainer's attribute that holds the state (the other five stay None)
    supported: Callable     # (policy, B, N) -> the kernels take this network and batch
    state: Callable         # (local, target, B, N, operands, support, batched) -> the Fused*State; batched: VecTrainer's
                            # (graphs, unroll), None for the drop-in Agent (nothing runs beside its update)
    refusal: Optional[str] = None   # VecTrainer's ValueError for an unsupported shape (None: not checked there)
    actor_critic: bool = False      # actor + critic with an optimiser each and a continuous 2-d action; otherwise one
                                    # network, one optimiser, an action index
    twin: bool = False              # actor_critic with two critics (critic_1, critic_2), an optimiser each (SAC)
    policy_args: tuple = ()         # constructor arguments behind action_size
    per: bool = False               # the prioritised n-step tree instead of the uniform ring

    @property
    def continuous(self):
        return self.actor_critic

    @property
    def action_dim(self):
        return 2 if self.actor_critic else 1

    def make_policy(self, net_args, device, seed, value_ranges_of_action=((-1.0, 1.0), (-1.0, 1.0)), action_size=25):
        """net_args: the seven network dimensions in constructor order (vec_trainer.DEFAULT_NET's values)."""
        if self.actor_critic:
            return self.policy(*net_args, value_ranges_of_action, device, seed)
        return self.policy(*net_args, action_size, *self.policy_args, device, seed).to(device)


def _ddpg_state(local, target, B, N, operands, support=None, batched=None):
    # two actor image sets flip at every update, host-side: a captured graph of an odd number of iterations
    # would replay on the set it was captured on and never see the other one written -- one set there, and
    # the update waits for the act kernel instead (fused_update._actor_step's actor_wait)
    double = batched is not None and (not batched[0] or batched[1] % 2 == 0)
    return fused_ddpg.FusedDDPGState(local, target, B, operands, double_actor=double)


def _sac_state(local, target, B, N, operands, support=None, batched=None):
    double = batched is not None and (not batched[0] or batched[1] % 2 == 0)   # the same odd-unroll rule
    return fused_sac.FusedSACState(local, target, B, operands, double_actor=double)


LEARNERS = {
    "AC-IQN": Learner(
        AC_IQN_Policy, "fused2", fused_update.supported,
        lambda l, t, B, N, ops, support=None, batched=None:
            fused_update.FusedACIQNState(l, t, B, N, ops, double_actor=batched is not None),
        "AC-IQN learner kernels: B={B}, N={N} (B a multiple of 32, N in 8, 16, 32)", actor_critic=True),
    "IQN": Learner(
        IQN_Policy, "fused_iqn", fused_iqn.supported,
        # nothing runs beside the drop-in's update: the target's max inside the fused launch (bf16 build)
        lambda l, t, B, N, ops, support=None, batched=None:
            fused_iqn.FusedIQNState(l, t, B, N, ops, target_in_fused=True if batched is None else None),
        "IQN learner kernels: B={B}, N={N}"),
    # Rainbow_Policy (dueling NoisyNet C51, 51 atoms on [-1, 1]) with the prioritised n-step replay in HBM, one
    # stream per robot (agent.py:597-641, replay_memory_rainbow.py)
    "Rainbow": Learner(
        Rainbow_Policy, "fused_rb", lambda p, B, N: fused_rainbow.supported(p, B),
        lambda l, t, B, N, ops, support=None, batched=None: fused_rainbow.FusedRainbow(l, t, B, support, ops),
        policy_args=(51,), per=True),
    # DQN_Policy: the Actor's trunk with a 25-wide head (fused_dqn.py); the uniform ring, one optimiser
    "DQN": Learner(
        DQN_Policy, "fused_dqn", lambda p, B, N: fused_dqn.supported(p, B),
        lambda l, t, B, N, ops, support=None, batched=None: fused_dqn.FusedDQNState(l, t, B, ops),
        "DQN learner kernels: B={B} (a positive multiple of 32)"),
    # DDPG_Policy: AC-IQN's Actor and a one-scalar critic (fused_ddpg.py)
    "DDPG": Learner(
        DDPG_Policy, "fused_ddpg", lambda p, B, N: fused_ddpg.supported(p, B), _ddpg_state,
        "DDPG learner kernels: B={B} (a positive multiple of 32)", actor_critic=True),
    # SAC_Policy: the Actor's trunk under a sampled head and two DDPG critics (fused_sac.py); the batched loop, and the
    # closed-loop windows / device evaluation through fused_sac.window_pack
    "SAC": Learner(
        SAC_Policy, "fused_sac", lambda p, B, N: fused_sac.supported(p, B), _sac_state,
        "SAC learner kernels: B={B} (a positive multiple of 32)", actor_critic=True, twin=True),
}


def policy_modules(policy):
    """[actor, critic] of an actor-critic policy ([actor, critic_1, critic_2] of SAC's), [policy] of a single
    network."""
    if hasattr(policy, "critic_1"):
        return [policy.actor, policy.critic_1, policy.critic_2]
    return [policy.actor, policy.critic] if hasattr(policy, "actor") else [policy]


def policy_parameters(policy):
    return [p for m in policy_modules(policy) for p in m.parameters()]
