"""VecTrainer -- the fused rollout + learn loop of rfarl's Trainer.learn (trainer.py:85-255),
batched over E envs on one GPU, data-parallel over ranks.

One iteration (= one `step` of bench.py):
  1. act: the local actor on every robot of every env (E*R rows), epsilon-greedy on device
     (trainer.py:106-135, agent.py:207-225; linear epsilon schedule trainer.py:257-264)
  2. env step kernel with the trainer bookkeeping fused (asvrl_env_step)
  3. replay push of the transitions of robots that acted (asvrl_replay_push, trainer.py:157-166)
  4. device reset of finished envs + their first observation (asvrl_env_reset, trainer.py:212-245)
  5. learn: sample B transitions (asvrl_replay_sample) and one distributional update
     (AC-IQN and DDPG: two dependent optimizer steps, critic then actor; SAC: three, both critics then the
     actor; IQN, Rainbow and DQN: one)
  6. target update every `target_update_interval` learn steps (agent.py:643-679): the hard copy (tau = 1, the
     default) or the Polyak blend (tau < 1), issued by the host between iterations (target_update="host") or as
     launches of the learn step predicated on the device learn counter (target_update="device")

Cadence in the batched setting: one learn step of batch B per iteration (after
`learning_starts` transitions) replaces the reference's one B=64 step per 4 single-env
timesteps; target updates count learn steps (2500 = 10000 timesteps / UPDATE_EVERY 4).
With `graphs=True` steps 1-5 are captured once into a HIP graph and replayed; with target_update="device" step 6
is captured with them.
"""
import time

import torch

from . import streams
from .learn_ops import DevicePER, DeviceReplay
from .learner import FlatParams, FusedAdam
from .learners import LEARNERS, policy_modules, policy_parameters
from .vec_env import VecMarineNavEnv

DEFAULT_NET = dict(self_dimension=7, object_dimension=5, max_object_num=5, self_feature_dimension=56,
                   object_feature_dimension=40, concat_feature_dimension=256, hidden_dimension=128)


class VecTrainer:
    def __init__(self, n_envs=4096, agent_type="AC-IQN", num_robots=5, num_obs=4, num_cores=0, min_start_goal_dis=40.0,
                 width=55.0, batch_size=4096, num_tau=32, buffer_size=4_000_000, lr=1e-4, gamma=0.99,
                 learning_starts=None, target_update_interval=2500, total_timesteps=6_000_000,
                 exploration_fraction=0.25, initial_eps=0.6, final_eps=0.05, seed=0,
                 device="cuda", sync=None, graphs=False, schedule=None, net_seed=100, overlap=True, unroll=1,
                 chain=None, operands="bf16", target_after_env=False, push_after_actor=None, tau=1.0,
                 target_update="host"):
        """Every learner (learners.LEARNERS) runs on the hand-written kernels with FusedAdam; operands="f32" takes
        them from the f32-operand parity build (libasvrl_f32.so). Shapes the kernels do not take raise ValueError.
        tau: soft_update's TAU, 0 < tau <= 1 (1: the hard copy). target_update: "host" -- the update is issued by
        iteration() every target_update_interval host-counted learn steps, between graph replays; "device" -- every
        learn step ends with one asvrl_target_update_pack launch per target network, which fires when the device
        learn counter is a multiple of target_update_interval (captured with the rest of the iteration)."""
        if not 0.0 < float(tau) <= 1.0:
            raise ValueError(f"tau must be in (0, 1], not {tau!r}")
        if target_update not in ("host", "device"):
            raise ValueError(f"target_update must be 'host' or 'device', not {target_update!r}")
        self.tau, self.target_update = float(tau), target_update
        if agent_type not in LEARNERS:
            raise NotImplementedError(f"VecTrainer agent_type {agent_type!r} (AC-IQN, IQN, Rainbow, DQN, DDPG and SAC "
                                      "are batched)")
        spec = LEARNERS[agent_type]
        self.device = torch.device(device)
        self.agent_type = agent_type
        # chained schedule knob: the AC-IQN learner's target critic waits for the same iteration's env step
        # (the two then run one after the other instead of side by side; results unchanged). With the target pass
        # inside the fused critic launch (fused_update.TARGET_IN_FUSED, the default) that wait gates the whole
        # fused critic update, not only the target forward
        self.target_after_env = bool(target_after_env)
        # schedule knob: the rollout's replay push (and the reset behind it) waits for the learner's ACTOR pass
        # of the same iteration instead of running beside it (None: wherever the chained AC-IQN graph runs)
        self._paa_arg = push_after_actor
        self.push_after_actor = bool(push_after_actor)
        self.continuous = spec.continuous
        self.env = VecMarineNavEnv(n_envs, num_robots, num_obs, num_cores, min_start_goal_dis, width, seed=seed,
                                   device=self.device, is_continuous=self.continuous, gamma=gamma, schedule=schedule)
        self.E, self.R = n_envs, self.env.max_robots
        self.B, self.num_tau, self.gamma = batch_size, num_tau, gamma
        self.operands = operands
        self.sync = sync
        self.seed = seed
        self.target_update_interval = target_update_interval
        self.total_timesteps = total_timesteps
        self.exploration_fraction, self.initial_eps, self.final_eps = exploration_fraction, initial_eps, final_eps
        self.learning_starts = learning_starts if learning_starts is not None else batch_size
        self.local = spec.make_policy(DEFAULT_NET.values(), self.device, net_seed)
        self.target = spec.make_policy(DEFAULT_NET.values(), self.device, net_seed)
        for p in policy_parameters(self.target):
            p.requires_grad_(False)
        if spec.refusal is not None and not spec.supported(self.local, batch_size, num_tau):
            raise ValueError(spec.refusal.format(B=batch_size, N=num_tau))
        # clip + Adam over flat buffers (must precede the packs, which cache parameter pointers)
        if spec.actor_critic:
            self.actor_opt = FusedAdam(self.local.actor.parameters(), lr=lr, operands=operands)
            self.actor_grads = self.actor_opt.grads
            if spec.twin:   # SAC: each critic is clipped by its own norm and takes its own Adam step
                self.critic_opts = [FusedAdam(c.parameters(), lr=lr, operands=operands)
                                    for c in (self.local.critic_1, self.local.critic_2)]
            else:
                self.critic_opt = FusedAdam(self.local.critic.parameters(), lr=lr, operands=operands)
                self.critic_grads = self.critic_opt.grads
        else:
            self.opt = FusedAdam(self.local.parameters(), lr=lr, operands=operands)
            self.grads = self.opt.grads
        # target_update="device": each target network in one flat buffer of its local optimiser's order (before the
        # packs, for the same reason); None otherwise -- the targets stay as they were built
        self._target_flat = None
        if target_update == "device":
            self._target_flat = [FlatParams(m.parameters(), operands) for m in policy_modules(self.target)]
            assert [f.n for f in self._target_flat] == [o.n for o in self.local_opts()]
        self.action_dim = spec.action_dim
        self.n_step = 3 if spec.per else None
        self.support = torch.linspace(-1.0, 1.0, 51, device=self.device) if spec.per else None
        # the learner's packs and buffers on the hand-written kernels: the one fused field that is not None
        self.fused2 = self.fused_iqn = self.fused_rb = self.fused_dqn = self.fused_ddpg = self.fused_sac = None
        self.learner = spec.state(self.local, self.target, batch_size, num_tau, operands, support=self.support,
                                  batched=(graphs, max(1, int(unroll))))
        setattr(self, spec.field, self.learner)
        NT = self.E * self.R
        self.per = None
        if spec.per:
            slots = max(min(buffer_size, 1 << 22) // NT, self.n_step + 3)
            self.per = DevicePER(slots * NT, stride=NT, n_step=self.n_step, discount=gamma, deferred=True,
                                 device=self.device)
            self.replay = None
            self.per_idx = torch.zeros(self.B, dtype=torch.int64, device=self.device)
            # the tree holds complete windows once n + 1 pushes are in
            self.learning_starts = max(self.learning_starts, (self.n_step + 1) * NT + self.B)
        else:
            self.replay = DeviceReplay(max(buffer_size, 2 * NT), device=self.device)
        self.actions = torch.zeros((NT, 2), dtype=torch.float64, device=self.device)
        self.learn_counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.loss_mean = torch.zeros(1, dtype=torch.float32, device=self.device)   # PER: the update's mean loss
        self.batch_rows = torch.zeros((self.B, 88), dtype=torch.float32, device=self.device)
        # the fused updates' quantile fractions (AC-IQN: target, local, actor step; IQN: the first two)
        self.taus = torch.zeros((3, self.B, self.num_tau), dtype=torch.float32, device=self.device)
        self.learn_steps = 0
        self.iterations = 0
        self.last_losses = None
        self.graphs = graphs
        self._graph = None
        # iterations per captured graph: one replay enqueues `unroll` whole iterations (the host
        # calls iteration() once per iteration; every unroll-th call replays): 10 with the chained
        # schedule at the bench shape (profiles/r02_unroll_chain_ab.txt)
        self.unroll = max(1, int(unroll))
        # observation double buffer by parity flip (no copy) unless a graph of an odd number of iterations
        # has to find the same buffers at every replay
        self.env.swap = not graphs or self.unroll % 2 == 0
        self._phase = 0
        self._graph_learn = None
        # rollout / learn on two streams (fused learners): the learner samples against a
        # snapshot of the ring state taken before this iteration's push, skipping the oldest
        # E*R entries the push may overwrite, and waits for the act kernel before the actor
        # weights change
        self.overlap = bool(overlap)
        self.ring_snap = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._streams = None
        # inside a captured graph of an even number of iterations, the two streams are ordered by the
        # exact dependencies instead of a join per iteration: act(i) after learn(i-1) (new weights),
        # learn(i) after the snapshot of the ring taken right behind push(i-1) (double-buffered, the
        # same state the joined schedule samples against), learn(i)'s weight updates after act(i).
        # Same operations on the same data as the joined schedule (tested bit for bit); the next
        # learner no longer waits for the rollout's tail (reset, observation pass, copies). chain=None:
        # AC-IQN only (measured 0.346 -> 0.340 ms/step; IQN, whose act kernel fills the GPU, 0.363 ->
        # 0.366: profiles/r02_chain_schedule_ab.txt)
        self.chain = (agent_type == "AC-IQN") if chain is None else bool(chain)
        if self.chain and agent_type in ("DDPG", "SAC"):
            # not built for DDPG or SAC: refused rather than silently run as the joined schedule
            raise ValueError(f"the dependency-chained schedule is not available for {agent_type} (chain=None or "
                             "False: the joined schedule)")
        paa_ok = agent_type == "AC-IQN" and self.graphs and self._chained()
        if self.target_after_env and not paa_ok:
            # the knob orders two nodes of the chained AC-IQN graph; anywhere else it would be silently ignored
            # and a bench config recording it would be mislabelled
            raise ValueError("target_after_env applies only to the chained, graph-captured AC-IQN schedule")
        if self._paa_arg is None:
            self.push_after_actor = paa_ok
        elif self.push_after_actor and not paa_ok:
            raise ValueError("push_after_actor applies only to the chained, graph-captured AC-IQN schedule")
        self.ring_snap2 = torch.zeros((2, 2), dtype=torch.int64, device=self.device)
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(seed + 12345)
        self.env.reset()

    # ------------------------------------------------------------------ pieces
    def epsilon(self):
        """trainer.py:257-264 as a device scalar of the device step counter (graph-safe)."""
        steps = self.env.counter.to(torch.float32) * float(self.E)
        progress = steps / float(self.total_timesteps)
        r = progress / self.exploration_fraction
        eps = self.initial_eps + r * (self.final_eps - self.initial_eps)
        return torch.where(progress < self.exploration_fraction, eps, torch.full_like(eps, self.final_eps))

    @torch.no_grad()
    def act(self):
        """The local policy on every robot row with the epsilon-greedy schedule on the device step counter
        (trainer.py:106-135, agent.py:207-250,308-324), one kernel per agent type."""
        args = (self.env.obs_cur, self.actions, self.env.counter, self.E, self.total_timesteps,
                self.exploration_fraction, self.initial_eps, self.final_eps, self.seed + 4242)
        self.learner.act(*args)

    def _eval_env(self):
        """A fresh env batch of the training env's shape, parameters and current curriculum stage, with its own
        seed, reset and observed (greedy_episodes)."""
        from . import _abi
        src = self.env
        c = src.cfg
        env = VecMarineNavEnv(self.E, c.num_robots, c.num_obs, c.num_cores, c.min_start_goal_dis, c.width, c.height,
                              seed=self.seed + 7919, device=self.device, is_continuous=True, gamma=self.gamma,
                              max_robots=src.max_robots, max_obs=src.batch.max_obs, max_cores=src.batch.max_cores)
        env.batch.params = _abi.AsvParams.from_buffer_copy(src.batch.params)
        env.reset()
        return env

    @torch.no_grad()
    def greedy_episodes(self, max_steps=1000, chunk=64):
        """Greedy evaluation of the current local actor: one episode per env of a fresh batch (_eval_env), run in
        closed-loop windows of `chunk` steps, one launch each (VecMarineNavEnv.policy_rollout with epsilon 0 and
        hold_done; an env that ended stays out of the later windows), until every env has ended or after
        max_steps. Returns that batch's episode_stats() plus steps_run, the steps every env took. The training
        env, the replay and the step counter are not touched. AC-IQN and DDPG only."""
        if self.learner.actor_pack is None:
            raise NotImplementedError("greedy_episodes runs the AC-IQN / DDPG actor; IQN, Rainbow and DQN act inside "
                                      "their own kernels (the learner's window_pack / eval_pack with "
                                      "device_evaluator(...).run is the route for IQN and Rainbow)")
        env = self._eval_env()
        alive = torch.ones(self.E, dtype=torch.uint8, device=self.device)
        steps_run = torch.zeros(self.E, dtype=torch.int32, device=self.device)
        done = 0
        while done < max_steps:
            k = min(int(chunk), max_steps - done)
            rec = env.policy_rollout(self.learner.actor_pack, k, hold_done=True, keep=("env_done",), env_mask=alive)
            env.advance_device(counted=True)   # the next window acts on this one's last observation
            steps_run += rec.steps_run
            alive *= (rec.env_done.sum(0) == 0).to(torch.uint8)
            done += k
            if not bool(alive.any().item()):   # one host sync per window
                break
        return dict(env.episode_stats(), steps_run=steps_run.cpu().numpy())

    @torch.no_grad()
    def evaluate(self, configs, chunk=64, template_env=None, **kw):
        """Trainer.evaluation's schedule on the device (policy/device_eval.DeviceEvaluator): the eval `configs`
        (MarineNavEnv3.episode_data) are loaded into env batches once and cached; every call restores them, runs the
        current local actor greedily in closed-loop windows of `chunk` steps and reduces the windows to the
        reference's per-config rewards / successes / times / energies / lengths on the device. kw: run()'s seed,
        episode_limit, sync, perception ("numpy": the robots' own RandomState streams, as the other paths draw) and
        histories (True: the result's "history" holds every robot's observation, action and trajectory history as
        packed arrays; device_eval.history_lists turns them into the reference's lists) and distribution (True: the
        result's "distribution", an EvalDistribution, holds the local critic's 32 quantile samples at every recorded
        decision reduced against the return each robot then collected; AC-IQN only, a ValueError for DDPG. An IQN
        trainer's route is device_evaluator(cfgs).run(fused_iqn.window_pack, distribution=True)). The actor's packed images are the learner's own, so no copy into a drop-in agent is
        needed; the training env, the replay and the step counter are not touched. AC-IQN and DDPG only."""
        if self.learner.actor_pack is None:
            raise NotImplementedError("evaluate runs the AC-IQN / DDPG actor; IQN, Rainbow and DQN act inside their "
                                      "own kernels (device_evaluator(...).run(policy_pack()) for DQN, "
                                      "run(fused_iqn.window_pack) for IQN, run(fused_rb.eval_pack) for Rainbow)")
        if kw.get("distribution") is True:   # the critic whose quantiles are read out at the recorded actions
            if self.fused2 is None:
                raise ValueError(f"evaluate: distribution=True reads the AC-IQN critic's return distribution; "
                                 f"{self.agent_type}'s critic has none")
            kw["distribution"] = self.fused2.local_trunk
        return self.device_evaluator(configs, chunk, template_env).run(self.learner.actor_pack, **kw)

    def policy_pack(self):
        """The pack the closed-loop windows take (DeviceEnvBatch.policy_rollout, DeviceEvaluator.run): the learner's
        own local images -- AC-IQN's or DDPG's actor or DQN's local net. IQN and Rainbow act inside their own
        kernels: the windows take fused_iqn.window_pack, and for Rainbow fused_rb.window_pack (training mode, the noisy
        images) or fused_rb.eval_pack (evaluation, mu only)."""
        if self.learner.policy_pack is not None:
            return self.learner.policy_pack
        raise NotImplementedError(f"policy_pack: the closed-loop windows run the AC-IQN / DDPG actor or DQN_Policy, not "
                                  f"{self.agent_type} (its learner's window_pack, and Rainbow's eval_pack, go to "
                                  "policy_rollout / DeviceEvaluator.run / _collect_window directly)")

    def device_evaluator(self, configs, chunk=64, template_env=None):
        """The DeviceEvaluator of the eval `configs`, built once and cached (one per configs list, chunk and
        template env): device_evaluator(...).run(policy_pack()) is an evaluation that touches neither the training
        env nor the replay nor the step counter."""
        from .policy.device_eval import DeviceEvaluator
        cached = getattr(self, "_dev_eval", None)
        if cached is None or cached[0] is not configs or cached[1] != (len(configs), int(chunk), template_env):
            ev = DeviceEvaluator(configs, template_env=template_env, device=self.device, chunk=chunk,
                                 gamma=self.gamma)
            cached = self._dev_eval = (configs, (len(configs), int(chunk), template_env), ev)
        return cached[2]

    def _push(self, snap=None):
        """The replay push of every robot that acted; for the uniform ring it is one launch that also
        increments the env step counter (and writes the new ring state to `snap` when given). Returns
        whether the counter was incremented."""
        env = self.env
        if self.per is not None:   # ReplayMemory.append of every robot that acted (trainer.py:163-164), and the
            # step counter advanced in the push's last launch
            self.per.push(env.obs_cur, env.cnt_next, self.actions[:, :1], env.batch.reward, env.batch.done,
                          step_counter=env.counter)
            return True
        self.replay.push(env.obs_cur, env.obs_next, env.cnt_next, self.actions[:, :self.action_dim],
                         env.batch.reward, env.batch.done, snap=snap, counter_inc=env.counter)
        return True

    def rollout(self, snap=None):
        """act, env step, replay push, device reset and the step counter (trainer.py:142-172)."""
        self.act()
        self.env.step(self.actions)
        counted = self._push(snap)
        self.env.auto_reset(counted)
        self.env.advance_device(counted)

    def _collect_buffers(self, K):
        """collect(K)'s records, allocated once per window length."""
        bufs = getattr(self, "_collect_bufs", None)
        if bufs is None:
            bufs = self._collect_bufs = {}
        if K not in bufs:
            NT, dev = self.E * self.R, self.device
            bufs[K] = dict(
                obs=torch.zeros((K, NT, 40), dtype=torch.float32, device=dev),
                obs_prev=torch.zeros((K, NT, 40), dtype=torch.float32, device=dev),
                obj_cnt=torch.full((K, NT), -1, dtype=torch.int8, device=dev),
                reward=torch.zeros((K, NT), dtype=torch.float64, device=dev),
                done=torch.ones((K, NT), dtype=torch.uint8, device=dev),
                actions=torch.zeros((K, NT, 2), dtype=torch.float64, device=dev),
                steps_run=torch.zeros(self.E, dtype=torch.int32, device=dev),
                pushed=torch.zeros(K, dtype=torch.int32, device=dev),
                resets=torch.zeros(self.E, dtype=torch.int32, device=dev))
        return bufs[K]

    @torch.no_grad()
    def collect(self, K, snap=None):
        """K calls of rollout() in two launches, bit for bit: one closed-loop window of K steps with the training
        epsilon schedule and seed of act(), ended envs restarting inside it (VecMarineNavEnv.policy_rollout with
        auto_reset), recorded into persistent buffers, then one push of the whole window into the uniform ring
        (DeviceReplay.push_window), which also advances the step counter by K. No host sync: the call can be
        graph-captured. Returns the window's records (views of the persistent buffers: obs, obs_prev, obj_cnt,
        reward, done, actions, steps_run, pushed, resets). AC-IQN and DDPG (the uniform ring) only; the caller accounts
        for the host-side step count (env.advance_host() per step) as iteration() does."""
        if self.learner.actor_pack is None or self.per is not None:
            raise NotImplementedError("collect runs the AC-IQN / DDPG actor and pushes into the uniform ring; IQN, "
                                      "Rainbow and DQN act inside their own kernels (_collect_window takes the "
                                      "learner's window_pack for SAC, IQN and Rainbow)")
        return self._collect_window(self.learner.actor_pack, K, snap)

    @torch.no_grad()
    def _collect_window(self, pack, K, snap=None):
        """collect()'s two launches under `pack`: the learner's actor_pack, or a SAC trainer's
        fused_sac.window_pack, whose ring rows are DDPG's (K calls of rollout(), bit for bit, there too), or an IQN
        trainer's fused_iqn.window_pack: its "actions" record holds (index, 0.0), and the push stores the pair as
        rollout()'s one-column push stores the index and a zero; or a Rainbow trainer's fused_rb.window_pack: the pack
        is refreshed once (the compose and pack act() does first: the online noise is never resampled, so K act()
        calls pack the same images K times), the window runs under the seed and step counter act() gives
        FusedRainbow.act, and the whole window goes into the prioritised replay in one push (DevicePER.push_window)."""
        K = int(K)
        buf = self._collect_buffers(K)
        buf["obj_cnt"].fill_(-1)   # a row no env took is never pushed (PER: it becomes a blank slot, as in push())
        if self.per is not None:
            pack.refresh()
        keep = {k: buf[k] for k in ("obs", "obs_prev", "obj_cnt", "reward", "done", "actions", "steps_run")}
        rec = self.env.policy_rollout(pack, K, hold_done=False, keep=keep,
                                      eps=(self.E, self.total_timesteps, self.exploration_fraction, self.initial_eps,
                                           self.final_eps), policy_seed=self.seed + 4242,
                                      auto_reset=dict(pushed=buf["pushed"], resets=buf["resets"]), count=False)
        if self.per is not None:
            self.per.push_window(buf, K, counter_inc=self.env.counter, counter_by=K)
        else:
            self.replay.push_window(buf, K, pushed=buf["pushed"], snap=snap, counter_inc=self.env.counter,
                                    counter_by=K)
        self.env.advance_device(True)
        return rec

    def learn(self, state=None, guard=0, actor_wait=None, target_wait=None, actor_done=None, target_step=True):
        """One learn step of batch B: sample (uniform ring, or the prioritised tree for Rainbow) and the
        agent's fused update. state / guard: the ring snapshot to sample against and the newest entries to
        skip (the overlapped schedule); actor_wait: an event to wait for before the actor's weights change.
        With target_update="device" the target step follows the learner's last launch (target_step=False: the
        caller enqueues it itself, _target_step())."""
        out = self.learner.learn(self, state, guard, actor_wait, target_wait, actor_done)
        if target_step:
            self._target_step()
        return out

    def local_opts(self):
        """The local networks' optimisers in policy_modules order."""
        if not LEARNERS[self.agent_type].actor_critic:
            return [self.opt]
        return [self.actor_opt] + (list(self.critic_opts) if LEARNERS[self.agent_type].twin else [self.critic_opt])

    def _target_step(self):
        """target_update="device": the target update of the learn step just enqueued, on the current stream. The
        learner's last launch has incremented the learn counter, so the launches fire when it is a multiple of
        target_update_interval and write nothing otherwise."""
        if self._target_flat is not None:
            self.learner.target_step(self)

    def hard_update(self):
        """soft_update with TAU = 1.0 (agent.py:643-679): target <- local."""
        with torch.no_grad():
            torch._foreach_copy_(policy_parameters(self.target), policy_parameters(self.local))
            self.learner.target_changed()   # eager, outside any captured graph

    def soft_update(self):
        """soft_update (agent.py:643-679) with this trainer's tau, in Agent.soft_update's own expression per
        parameter: target <- tau * local + (1 - tau) * target, then the target's weight images re-packed."""
        tau = self.tau
        with torch.no_grad():
            for t, l in zip(policy_parameters(self.target), policy_parameters(self.local)):
                t.copy_(tau * l + (1.0 - tau) * t)
            self.learner.target_changed()   # eager, outside any captured graph

    @torch.no_grad()
    def load_policies(self, local, target):
        """Start from the given networks (a drop-in Agent's policy_local / policy_target, e.g. after its
        load_model): their weights are copied in place into this trainer's networks (whose parameters
        are views of the optimisers' flat buffers) and every weight image is re-packed. Eager, before
        the first captured graph."""
        assert self._graph is None, "load_policies before the first captured iteration"
        for dst, src in ((self.local, local), (self.target, target)):
            for d, s in zip(policy_modules(dst), policy_modules(src)):
                sd = s.state_dict()
                for name, t in d.state_dict(keep_vars=True).items():
                    t.data.copy_(sd[name].to(device=t.device, dtype=t.dtype))
        self.learner.refresh_local()
        self.learner.target_changed()

    # ------------------------------------------------------------------ iteration
    def _iteration_body(self, do_learn):
        if not (do_learn and self.overlap and self.per is None):
            # the learner samples after the push: only the act -> push order of rollout() matters
            self.rollout()
            return self.learn() if do_learn else None
        # the learner runs on the current stream and the rollout on a side stream: HIP graph
        # capture (ROCm 7) segfaults at capture end on a stream forked from an already forked
        # stream, and the learner forks side streams of its own (fused_update.SideStreams)
        main = torch.cuda.current_stream(self.device)
        if self._streams is None:
            self._streams = (self.roll_stream(),) + self._roll_events()
        s_roll, ev_snap, ev_act = self._streams
        # the replay state the learner samples against (after the previous iteration's push, which
        # the caller's stream joined), copied on the learner's own stream: the learner's chain then
        # starts without a cross-stream wait (each costs ~10 us in a replayed graph)
        self.ring_snap.copy_(self.replay.state)
        s_roll.wait_stream(main)
        with torch.cuda.stream(s_roll):
            self.act()
            ev_act.record(s_roll)
            env = self.env
            env.step(self.actions)
            counted = self._push()
            env.auto_reset(counted)
            env.advance_device(counted)
        out = self.learn(state=self.ring_snap, guard=self.E * self.R, actor_wait=ev_act)
        main.wait_stream(s_roll)
        return out

    def iteration(self, timing=None):
        """One fused rollout+learn iteration. Returns losses (device tensors) or None."""
        do_learn = self.replay_size_host() >= self.learning_starts
        if self.graphs and do_learn and self._graph is None:
            try:
                self._capture()
            except RuntimeError as e:   # a capture the runtime refuses: keep going eagerly, loudly
                import sys
                print(f"VecTrainer: HIP graph capture failed ({e}); continuing without graphs", file=sys.stderr)
                self.graphs, self._graph = False, None
        if self.graphs and do_learn:
            if self._phase == 0:
                self._graph.replay()
            self._phase = (self._phase + 1) % self.unroll
            out = self._graph_out
        else:
            out = self._iteration_body(do_learn)
        self.env.advance_host()
        self.iterations += 1
        if do_learn:
            self.learn_steps += 1
            if self._target_flat is None and self.learn_steps % self.target_update_interval == 0:
                if self.tau == 1.0:
                    self.hard_update()
                else:
                    self.soft_update()
        self.last_losses = out
        return out

    def replay_size_host(self):
        # host-side estimate avoids a device sync every iteration: exact once the buffer
        # has been observed >= learning_starts (it only grows until full)
        if getattr(self, "_replay_ready", False):
            return self.learning_starts
        n = self.per.pushed if self.per is not None else self.replay.size()
        if n >= self.learning_starts:
            self._replay_ready = True
        return n

    def roll_stream(self):
        """The rollout's stream: a dedicated one (streams.py), never an alias of the capture stream or
        of the learner's side streams."""
        return streams.stream(self.device, "roll")

    def _roll_events(self):
        return torch.cuda.Event(), torch.cuda.Event()

    def _chained(self):
        return self.chain and self.overlap and self.per is None and self.unroll % 2 == 0

    def _chain_body(self):
        """self.unroll iterations with per-dependency stream ordering (captured only; see __init__)."""
        main = torch.cuda.current_stream(self.device)
        if self._streams is None:
            self._streams = (self.roll_stream(),) + self._roll_events()
        s_roll = self._streams[0]
        U = self.unroll
        ev_act = [torch.cuda.Event() for _ in range(U)]
        ev_snap = [torch.cuda.Event() for _ in range(U)]
        ev_learn = [torch.cuda.Event() for _ in range(U)]
        ev_env = [torch.cuda.Event() for _ in range(U)]
        ev_actor = [torch.cuda.Event() for _ in range(U)]
        # the events live as long as the graph: the captured cross-stream waits may refer to them at replay
        self._chain_events = (ev_act, ev_snap, ev_learn, ev_env, ev_actor)
        tae, paa = self.target_after_env, self.push_after_actor   # AC-IQN only (__init__)
        s_roll.wait_stream(main)
        out = None

        def push_reset(k):
            self._push(snap=self.ring_snap2[k % 2])   # + the ring state learn(k+1) samples against
            ev_snap[k].record(s_roll)
            self.env.auto_reset(True)
            self.env.advance_device(True)

        for k in range(U):
            with torch.cuda.stream(s_roll):
                if k > 0:
                    s_roll.wait_event(ev_learn[k - 1])   # the weights learn(k-1) wrote
                self.act()
                ev_act[k].record(s_roll)
                self.env.step(self.actions)
                if tae:
                    ev_env[k].record(s_roll)
                if not paa:
                    push_reset(k)
            if k > 0:
                main.wait_event(ev_snap[k - 1])
            out = self.learn(state=self.ring_snap2[(k - 1) % 2], guard=self.E * self.R, actor_wait=ev_act[k],
                             target_wait=ev_env[k] if tae else None, actor_done=ev_actor[k] if paa else None,
                             target_step=False)
            ev_learn[k].record(main)
            # behind the event the next act waits for: nothing on the rollout stream reads a target
            self._target_step()
            if paa:
                with torch.cuda.stream(s_roll):
                    s_roll.wait_event(ev_actor[k])
                    push_reset(k)
        main.wait_stream(s_roll)
        return out

    def _capture(self):
        # warm up the captured region on a side stream (allocator + autograd state)
        s = streams.stream(self.device, "warmup")
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(3):
                self._iteration_body(True)
                self.env.advance_host()
        torch.cuda.current_stream(self.device).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        # thread_local: the RCCL process group's watchdog thread queries its work events while this
        # thread captures; under the default global mode that query invalidates the capture and the
        # watchdog aborts the process
        chained = self._chained()
        if chained:   # the ring state after the last eager push: what the graph's first learner samples against
            self.ring_snap2[(self.unroll - 1) % 2].copy_(self.replay.state)
        # captured on the dedicated capture stream: torch.cuda.graph's default is a pool stream that a
        # long process also hands out as "another" stream (streams.py)
        with torch.cuda.graph(g, stream=streams.capture_stream(self.device), capture_error_mode="thread_local"):
            if chained:
                self._graph_out = self._chain_body()
            else:
                for _ in range(self.unroll):
                    self._graph_out = self._iteration_body(True)
        self._graph = g

    def run(self, iterations):
        t0 = time.time()
        for _ in range(iterations):
            self.iteration()
        torch.cuda.synchronize(self.device)
        return time.time() - t0
