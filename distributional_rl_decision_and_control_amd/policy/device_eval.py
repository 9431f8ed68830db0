"""Trainer.evaluation (trainer.py:266-392) resident on the device.

policy/batched_eval.evaluate_configs advances every eval config together, but through the Python MarineNavEnv3
objects: per step one torch policy call, one env-step launch with an upload and a download, one host wait and the
per-robot bookkeeping in Python. DeviceEvaluator keeps the same episodes in DeviceEnvBatches:

  * the configs are parsed once, exactly as evaluate_configs parses them (MarineNavEnv3.reset_with_eval_config on a
    copy of the template env's curriculum attributes), grouped by env_key(), and each group's host image (robot
    state, flags, counts, obstacles, cores; set_batch_params for the launch parameters) is loaded into one batch;
    a device copy of that state is kept, so every later evaluation restores by copy;
  * an evaluation is the observation pass and then closed-loop windows of `chunk` steps, one launch each
    (DeviceEnvBatch.policy_rollout with hold_done, the greedy Actor of an MlpPack, the greedy DQN_Policy of a
    DqnPack, SAC's actor of a SacActorPack, sampled as act_sac samples or its mean action, or the greedy IQN_Policy
    of an IqnPack at a risk level cvar or the greedy Rainbow_Policy of a RainbowPack (eval mode: mu-only images), the
    act launch and the step of these two enqueued per step by the one call), or, teacher-forced, open-loop windows over a caller's action table (DeviceEnvBatch.rollout);
  * behind every window one asvrl_eval_metrics launch folds the window's records into the evaluation's carried
    state by trainer.py:286-303: discounted return, time, energy, deactivation, and the evaluation's end rule (the
    step limit, ANY collision, or every robot deactivated). Its `alive` output is the next window's env_mask;
  * one copy at the end brings the per-robot sums, outcomes and lengths to the host.

Perception noise has two modes. perception="philox" (the default): the rollout's Philox stream (seed, env, robot,
step; f32 draws), not each robot's numpy RandomState; the results agree with evaluate_configs in distribution, and
exactly under teacher forcing with the noise given (tests/test_device_eval_gpu.py). perception="numpy": every robot's
own numpy.random.RandomState(seed) stream continued on the device (noise_streams.NoiseStreams, asvrl_noise_streams):
one launch in front of every step draws the step's rows for the robots that are still active, and the windows are one
step long, because which robots draw depends on the deactivations of the step before. The episodes are then the ones
the reference, Trainer.evaluation and evaluate_configs produce for the same configs and actions
(tests/test_eval60_reference_noise_gpu.py). In both modes SAC's action noise is Philox + Box-Muller on (row, step,
policy_seed + group), not torch's generator, and IQN's quantile fractions and the exploration draw are Philox too.

Observation, action and trajectory histories (trainer.py:347-365; what visualize_eval_episode.py plays back) are kept
on request, run(histories=True): every group then records its windows into episode-long buffers of
T = episode_limit + 1 steps (the window at t0 of length k takes the slices [t0:t0 + k] as its keep= tensors: no copy
and no launch per window), 322 bytes per robot-step -- reward 8, info 1, rs 136, actions 16, obs 160, obj_cnt 1 --
which is 97 MB for the 300 robot rows of the shipped schedule at the limit of 1000, allocated once and reused. At the
end of the run asvrl_eval_history_count cuts them by the evaluation's rules (an env's records stop at its evaluation
length L, a robot's actions and trajectory at its own collision or goal), and one asvrl_eval_history_pack launch per
group writes four packed arrays in which every robot's history is contiguous (EvalHistory); history_lists turns them
into the reference's nested lists. Observation values are the packed f32 rows the policy was fed, not the f64 the host
paths keep. Without histories nothing of this is allocated or launched.
"""
import ctypes as C

import numpy as np
import torch

from .. import _abi
from ..device_env import DeviceEnvBatch, policy_options
from ..envs.marinenav.env import MarineNavEnv3, set_batch_params
from ..noise_streams import NoiseStreams

RECORDS = ("reward", "info", "rs")
PERCEPTIONS = ("philox", "numpy")
OBS_COUNTER = 0x80000000   # the observation pass's Philox counter (VecMarineNavEnv.reset's); step t draws at t


def eval_metrics(L, K, E, R, rec, n_robots, dt, N, pc, state, gamma, episode_limit, stream=None):
    """asvrl_eval_metrics of library L on one window: rec has reward [K, NT] f64, info [K, NT] u8, rs [K, 17, NT]
    f64 and steps_run [E] i32; state has length, ended, alive, deact, outcome, ret, time, energy (updated in
    place)."""
    NT = E * R
    m = _abi.AsvEvalMetrics()
    m.n_steps, m.n_envs, m.max_robots, m.episode_limit = int(K), int(E), int(R), int(episode_limit)
    m.gamma = float(gamma)
    shapes = dict(reward=((K, NT), torch.float64), info=((K, NT), torch.uint8),
                  rs=((K, _abi.NUM_FIELDS, NT), torch.float64), steps_run=((E,), torch.int32),
                  n_robots=((E,), torch.int32), dt=((NT,), torch.float64), N=((NT,), torch.float64),
                  pc=((NT,), torch.float64), length=((E,), torch.int32), ended=((E,), torch.uint8),
                  alive=((E,), torch.uint8), deact=((NT,), torch.uint8), outcome=((NT,), torch.uint8),
                  ret=((NT,), torch.float64), time=((NT,), torch.float64), energy=((NT,), torch.float64))
    given = dict(n_robots=n_robots, dt=dt, N=N, pc=pc)
    for name, (shape, dtype) in shapes.items():
        t = given[name] if name in given else (rec[name] if name in ("reward", "info", "rs", "steps_run")
                                               else state[name])
        assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape, name
        setattr(m, name, t.data_ptr())
    rc = L.asvrl_eval_metrics(C.byref(m), _abi.stream_ptr(stream))
    _abi.check(rc, "asvrl_eval_metrics", L)


def new_metrics_state(E, R, device):
    """The carried state of asvrl_eval_metrics before the first window."""
    NT = E * R
    u8 = dict(dtype=torch.uint8, device=device)
    f64 = dict(dtype=torch.float64, device=device)
    return dict(length=torch.zeros(E, dtype=torch.int32, device=device), ended=torch.zeros(E, **u8),
                alive=torch.ones(E, **u8), deact=torch.zeros(NT, **u8), outcome=torch.zeros(NT, **u8),
                ret=torch.zeros(NT, **f64), time=torch.zeros(NT, **f64), energy=torch.zeros(NT, **f64))


HISTORY_RECORDS = ("reward", "info", "rs", "actions", "obs", "obj_cnt")   # the episode-long records of histories=True
HISTORY_BYTES = 8 + 1 + 8 * _abi.NUM_FIELDS + 16 + 4 * _abi.OBS_DIM + 1   # per robot-step: 322


def _history_struct(T, E, R, act_steps=1):
    h = _abi.AsvEvalHistory()
    h.n_steps, h.n_envs, h.max_robots, h.act_steps = int(T), int(E), int(R), int(act_steps)
    return h


def _set(h, name, t, shape, dtype):
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape), name
    setattr(h, name, t.data_ptr() if t.numel() else None)


def history_count(L, T, E, R, info, length, n_robots, counts=None, stream=None):
    """asvrl_eval_history_count of library L: info [T, NT] u8 (episode-long), length [E] i32 (the evaluation's
    lengths), n_robots [E] i32. Returns counts [3, NT] i32: per robot row its trajectory rows (n_act + 1), actions
    (n_act) and observations (L + 1); zeros for an absent slot."""
    NT = E * R
    if counts is None:
        counts = torch.zeros((3, NT), dtype=torch.int32, device=info.device)
    h = _history_struct(T, E, R)
    _set(h, "info", info, (T, NT), torch.uint8)
    _set(h, "length", length, (E,), torch.int32)
    _set(h, "n_robots", n_robots, (E,), torch.int32)
    _set(h, "counts", counts, (3, NT), torch.int32)
    _abi.check(L.asvrl_eval_history_count(C.byref(h), _abi.stream_ptr(stream)), "asvrl_eval_history_count", L)
    return counts


def history_offsets(counts):
    """The exclusive scans of the three count planes, [3, NT] i64: where every robot row's history starts."""
    return (torch.cumsum(counts, dim=1) - counts).contiguous()


def history_pack(L, T, E, R, counts, offsets, src, out, stream=None):
    """asvrl_eval_history_pack of library L. src: rs0 [17, NT] f64, rs [T, 17, NT] f64, actions [Ta, NT, 2] f64,
    obs0 [NT, 40] f32, obs [T, NT, 40] f32, cnt0 [NT] i8, obj_cnt [T, NT] i8; out: traj [n, 13] f64, act [n, 2] f64,
    obs [n, 32] f32, cnt [n] i8 with at least the sums of the count planes as their n (a smaller n drops what does
    not fit, it is never written past)."""
    NT = E * R
    Ta = int(src["actions"].shape[0])
    h = _history_struct(T, E, R, Ta)
    _set(h, "counts", counts, (3, NT), torch.int32)
    _set(h, "offsets", offsets, (3, NT), torch.int64)
    _set(h, "rs0", src["rs0"], (_abi.NUM_FIELDS, NT), torch.float64)
    _set(h, "rs", src["rs"], (T, _abi.NUM_FIELDS, NT), torch.float64)
    _set(h, "actions", src["actions"], (Ta, NT, 2), torch.float64)
    _set(h, "obs0", src["obs0"], (NT, _abi.OBS_DIM), torch.float32)
    _set(h, "obs", src["obs"], (T, NT, _abi.OBS_DIM), torch.float32)
    _set(h, "cnt0", src["cnt0"], (NT,), torch.int8)
    _set(h, "obj_cnt", src["obj_cnt"], (T, NT), torch.int8)
    h.traj_rows, h.act_rows, h.obs_rows = int(out["traj"].shape[0]), int(out["act"].shape[0]), int(out["obs"].shape[0])
    _set(h, "traj", out["traj"], (h.traj_rows, _abi.TRAJ_DIM), torch.float64)
    _set(h, "act", out["act"], (h.act_rows, 2), torch.float64)
    _set(h, "obs_out", out["obs"], (h.obs_rows, _abi.HISTORY_OBS_DIM), torch.float32)
    _set(h, "cnt_out", out["cnt"], (h.obs_rows,), torch.int8)
    _abi.check(L.asvrl_eval_history_pack(C.byref(h), _abi.stream_ptr(stream)), "asvrl_eval_history_pack", L)


class EvalHistory:
    """The histories of one evaluation as four packed host arrays -- traj [sum(n_act + 1), 13] f64, act
    [sum n_act, 2] f64, obs [sum(L + 1), 32] f32 and cnt [sum(L + 1)] i8 -- in which the history of every robot is
    contiguous (robots in batch order: group by group, config by config; time fastest), and slices[c][i], the
    (trajectory, action, observation) slices of config c's robot i into them. Everything the accessors return is a
    view of those arrays, except a discrete policy's int64 action indices."""

    def __init__(self, traj, act, obs, cnt, slices, continuous, levels=False):
        self.traj, self.act, self.obs, self.cnt = traj, act, obs, cnt
        self.slices = slices
        self.continuous = bool(continuous)
        self.levels = bool(levels)   # the run's risk level was decided per robot (an AdaptiveCvar)

    def trajectory(self, c, i):
        """[n_act + 1, 13] f64: the reset row and the row after every step the robot acted in (wamv.py:191-193)."""
        return self.traj[self.slices[c][i][0]]

    def action(self, c, i):
        """[n_act, 2] f64, the pairs the env was given; of a discrete policy [n_act] int64, the action indices."""
        a = self.act[self.slices[c][i][1]]
        return a if self.continuous else a[:, 0].astype(np.int64)

    def cvar(self, c, i):
        """[n_act] f64: the risk level the robot acted on at every act of a run under an AdaptiveCvar (the second
        column of its packed action pairs, the f32 level widened exactly). A ValueError after a run at a float
        level, whose pairs carry 0.0 there."""
        if not self.levels:
            raise ValueError("EvalHistory.cvar: the run had one float risk level (its result's \"cvar\"); the level "
                             "per act is recorded under run(..., cvar=AdaptiveCvar())")
        return self.act[self.slices[c][i][1]][:, 1]

    def observation(self, c, i):
        """(self [L + 1, 7], objects [L + 1, 5, 5], count [L + 1]): the reset observation and the one after every
        step of the episode; count < 0 is the reference's [None, None], else the first `count` objects hold."""
        sl = self.slices[c][i][2]
        o = self.obs[sl]
        return o[:, :_abi.SELF_DIM], o[:, _abi.SELF_DIM:].reshape(-1, _abi.MAX_OBJ, _abi.OBJ_DIM), self.cnt[sl]

    def _nested(self, get):
        return [[get(c, i) for i in range(len(robots))] for c, robots in enumerate(self.slices)]

    @property
    def trajectories(self):
        return self._nested(self.trajectory)

    @property
    def actions(self):
        return self._nested(self.action)

    @property
    def observations(self):
        return self._nested(self.observation)


def history_lists(result):
    """Fill observations / actions / trajectories of a run(histories=True) result with the reference's nested Python
    lists (trainer.py:347-365): per config and robot the trajectory rows as lists of 13 floats, the actions as
    [left, right] float pairs or, of a discrete policy, ints, and the observations as [self, objects] with self 7
    floats and objects one list of 5 floats per perceived object, or [None, None]. Costs host time the arrays do not,
    so it is a call of its own. Returns result."""
    h = result.get("history")
    if h is None:
        raise ValueError("history_lists: the result has no histories (run(..., histories=True))")
    for c, robots in enumerate(h.slices):
        obs_c, act_c, traj_c = [], [], []
        for i in range(len(robots)):
            traj_c.append(h.trajectory(c, i).tolist())
            act_c.append(h.action(c, i).tolist())
            s, o, n = (a.tolist() for a in h.observation(c, i))
            obs_c.append([[None, None] if k < 0 else [s[q], o[q][:k]] for q, k in enumerate(n)])
        result["observations"][c], result["actions"][c], result["trajectories"][c] = obs_c, act_c, traj_c
    return result


# ------------------------------------------------------------------ return distributions
DIST_OUTPUTS = (("g0", torch.float64, ()), ("pred0", torch.float64, ()), ("pinball", torch.float64, ()),
                ("bias", torch.float64, ()), ("steps", torch.int32, ()), ("pit", torch.int32, (_abi.DIST_SAMPLES + 1,)))


def new_dist_outputs(NT, device):
    """The per-robot outputs of asvrl_eval_dist_stats at their pre-fill (zeros; absent slots keep it)."""
    return {n: torch.zeros((NT,) + tail, dtype=dt, device=device) for n, dt, tail in DIST_OUTPUTS}


def eval_dist_stats(L, T, E, R, z, tau, reward, n_act, n_robots, gamma, out, G, block=0, stream=None):
    """asvrl_eval_dist_stats of library L for one group: z, tau [T, NT, 32] f32 (the quantile samples and fractions
    behind the decision of robot row n at step t), reward [T, NT] f64, n_act [NT] i32 (plane 1 of history_count's
    counts), n_robots [E] i32; out: new_dist_outputs' tensors, G [T, NT] f64 the return-to-go plane (rows at or behind
    a robot's n_act are not written). block: threads per block of the two launches (0: 256); the results do not
    depend on it. Two launches, no atomics: the same bits from run to run."""
    NT = E * R
    s = _abi.AsvEvalDistStats()
    s.n_steps, s.n_envs, s.max_robots, s.block, s.gamma = int(T), int(E), int(R), int(block), float(gamma)
    S = _abi.DIST_SAMPLES
    shapes = dict(z=((T, NT, S), torch.float32), tau=((T, NT, S), torch.float32), reward=((T, NT), torch.float64),
                  n_act=((NT,), torch.int32), n_robots=((E,), torch.int32), g_plane=((T, NT), torch.float64))
    given = dict(z=z, tau=tau, reward=reward, n_act=n_act, n_robots=n_robots, g_plane=G)
    for n, dt, tail in DIST_OUTPUTS:
        shapes[n], given[n] = ((NT,) + tail, dt), out[n]
    for name, (shape, dtype) in shapes.items():
        t = given[name]
        assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape, name
        setattr(s, name, t.data_ptr())
    _abi.check(L.asvrl_eval_dist_stats(C.byref(s), _abi.stream_ptr(stream)), "asvrl_eval_dist_stats", L)
    return out, G


class EvalDistribution:
    """What run(distribution=...) adds as result["distribution"]: per config c and robot i, as arrays indexed [c][i],
    g0 (the discounted return the robot collected from step 0: robot_rewards by a backward scan), pred0 (the mean of
    the 32 quantile samples at its first decision), pit ([33]: how often u of the 32 samples lay at or below the
    return-to-go, over its decisions), pinball (the quantile loss summed over its decisions and samples), bias (the
    sum over its decisions of sample mean - return-to-go), steps (its decisions) and truncated (its outcome is 0: the
    episode ended at the limit or by another robot's collision while it was running, so its returns are cut short).
    mismatches (an IqnPack only, else None): acted robot-steps whose recomputed greedy action differs from the
    recorded one. The samples themselves stay on the device, in planes the evaluator reuses at its next run with a
    distribution: quantiles / taus / returns_to_go copy a robot's rows on demand."""
    ARRAYS = ("g0", "pred0", "pit", "pinball", "bias", "steps", "truncated")

    def __init__(self, arrays, where, planes, mismatches, kind):
        for name in self.ARRAYS:
            setattr(self, name, arrays[name])
        self._where, self._planes = where, planes
        self.mismatches, self.kind = mismatches, kind

    def _rows(self, name, c, i):
        g, row0 = self._where[c]
        return self._planes[g][name][:int(self.steps[c][i]), row0 + i].cpu().numpy()

    def quantiles(self, c, i):
        """[steps, 32] f32: the quantile values of the action robot i of config c took, in sample order."""
        return self._rows("z", c, i)

    def taus(self, c, i):
        """[steps, 32] f32: their fractions (after the risk level)."""
        return self._rows("tau", c, i)

    def returns_to_go(self, c, i):
        """[steps] f64: G_t, the discounted return from step t on."""
        return self._rows("G", c, i)

    def summary(self, terminated_only=True):
        """Calibration per config and overall (host numpy over the per-robot arrays): "pit" the normalised PIT
        histogram [33] (uniform for a calibrated distribution up to the samples' own spread), "pinball" the quantile
        loss per sample, "bias" the mean of sample mean - return-to-go per decision, "pred0_minus_g0" the mean over
        robots of pred0 - g0, "robots" and "steps" what entered. terminated_only drops the truncated robots. Values
        with nothing behind them are NaN. Returns {"configs": {name: array over configs}, "overall": {name: value}}."""
        S = _abi.DIST_SAMPLES

        def reduce(sel):
            steps = sum(int(self.steps[c][m].sum()) for c, m in sel)
            robots = sum(int((self.steps[c][m] > 0).sum()) for c, m in sel)
            pit = sum((self.pit[c][m].sum(axis=0) for c, m in sel), np.zeros(S + 1))
            pin = sum(float(self.pinball[c][m].sum()) for c, m in sel)
            bias = sum(float(self.bias[c][m].sum()) for c, m in sel)
            gap = sum(float((self.pred0[c][m] - self.g0[c][m])[self.steps[c][m] > 0].sum()) for c, m in sel)
            nan = float("nan")
            return dict(pit=pit / steps if steps else np.full(S + 1, nan), pinball=pin / (steps * S) if steps else nan,
                        bias=bias / steps if steps else nan, pred0_minus_g0=gap / robots if robots else nan,
                        robots=robots, steps=steps)
        masks = [(~t if terminated_only else np.ones_like(t)) for t in self.truncated]
        per = [reduce([(c, m)]) for c, m in enumerate(masks)]
        return dict(configs={k: np.array([p[k] for p in per]) for k in per[0]}, overall=reduce(list(enumerate(masks))),
                    terminated_only=bool(terminated_only))


def distribution_source(who, pack, distribution):
    """The refusals of run(distribution=...): None -> None; else ("iqn", pack) for an IqnPack with True, or
    ("critic", CriticPack) for the Actor's pack with the AC-IQN critic's CriticPack."""
    from ..fused_critic import CriticPack
    from ..fused_iqn import IqnPack
    from ..fused_mlp import MlpPack
    if distribution is None or distribution is False:
        return None
    if pack is None:
        raise ValueError(f"{who}: distribution reads the quantiles of the policy that acted; an action table has none")
    if isinstance(pack, IqnPack):
        if distribution is not True:
            raise ValueError(f"{who}: an IqnPack's distribution is its own (distribution=True)")
        return "iqn", pack
    if type(pack) is MlpPack and getattr(pack, "kind", None) == "actor":   # not DQN's or SAC's packs, its subclasses
        if type(distribution) is CriticPack and distribution.struct.ae_w:
            if distribution.L is not pack.L:
                raise ValueError(f"{who}: the critic's pack and the actor's are of different operand builds")
            return "critic", distribution
        raise ValueError(f"{who}: with the Actor's pack, distribution must be the AC-IQN critic's CriticPack (a "
                         "trainer's fused2.local_trunk); DDPG's critic has no return distribution")
    raise ValueError(f"{who}: distribution is offered for an IqnPack (True) and for AC-IQN's Actor with its critic's "
                     f"CriticPack, not for a {type(pack).__name__} (Rainbow's C51 atoms are not read out yet)")


def _check_perception(who, perception, *noises):
    if perception not in PERCEPTIONS:
        raise ValueError(f"{who}: perception must be one of {PERCEPTIONS}, not {perception!r}")
    if perception == "numpy" and any(n is not None for n in noises):
        raise ValueError(f"{who}: perception='numpy' draws the noise from the robots' RandomState streams; "
                         "explicit noise (noise= / obs_noise=) goes with perception='philox'")


class _Group:
    """The configs that share env-level parameters: one DeviceEnvBatch, its initial state and carried metrics."""

    def __init__(self, members, envs, device):
        self.members = members
        self.envs = envs
        E = len(envs)
        R = max(max(len(env.robots) for env in envs), 1)
        O = max(max(len(env.obstacles) for env in envs), 1)
        Cm = max(max(len(env.cores) for env in envs), 1)
        b = self.batch = DeviceEnvBatch(E, R, O, Cm, device=device, obs64=True)
        set_batch_params(b, envs)
        NT = E * R
        rs = np.zeros((_abi.NUM_FIELDS, NT))
        fl = np.zeros(NT, np.uint8)
        cnt = np.zeros((3, E), np.int32)
        obst = np.zeros((E, O, 3))
        cores = np.zeros((E, Cm, 4))
        per = np.zeros((3, NT))
        for e, env in enumerate(envs):
            pk = env._pack(None, True, R, O, Cm)   # the host image one env-step launch uploads
            sl = slice(e * R, (e + 1) * R)
            rs[:, sl], fl[sl] = pk["rs"], pk["fl"]
            cnt[:, e] = (pk["n"], pk["n_obs"], pk["n_cores"])
            obst[e], cores[e] = pk["obst"], pk["cores"]
            for i, rob in enumerate(env.robots):
                per[:, e * R + i] = (rob.dt, rob.N, rob.power_coefficient)
        self.host = dict(rs=rs, rflags=fl, n_robots=cnt[0], n_obs=cnt[1], n_cores=cnt[2], obstacles=obst,
                         cores=cores)
        for name, a in self.host.items():
            getattr(b, name).copy_(torch.from_numpy(np.ascontiguousarray(a)))
        b.ep_ts.zero_()
        self.initial = dict(rs=b.rs.clone(), rflags=b.rflags.clone())
        self.dt, self.N, self.pc = (torch.from_numpy(per[k].copy()).to(device) for k in range(3))
        self.state = new_metrics_state(E, R, device)
        self.step = torch.zeros(1, dtype=torch.int64, device=device)
        self._rec = {}
        self._hist = {}
        self._dist = {}
        self._streams = None

    def streams(self):
        """Every robot row's RandomState(rob.perception.seed) stream as the robot's Perception held it before
        reset_with_eval_config's observation pass (built on first use, restored by observe)."""
        if self._streams is None:
            R = self.batch.max_robots
            seeds = [None] * (self.batch.n_envs * R)
            for e, env in enumerate(self.envs):
                for i, rob in enumerate(env.robots):
                    seeds[e * R + i] = rob.perception.seed
            self._streams = NoiseStreams(seeds, device=self.batch.device)
        return self._streams

    def restore(self):
        b = self.batch
        b.rs.copy_(self.initial["rs"])
        b.rflags.copy_(self.initial["rflags"])
        b.ep_ts.zero_()
        b.stats.zero_()
        for name, t in self.state.items():
            t.fill_(1) if name == "alive" else t.zero_()

    def records(self, K):
        """The window's records, allocated once per window length. Rows an env does not take keep whatever an
        earlier window left: asvrl_eval_metrics reads no row at or behind steps_run."""
        rec = self._rec.get(K)
        if rec is None:
            b = self.batch
            specs = b._record_specs()
            rec = {n: torch.full((K,) + specs[n][0], specs[n][2], dtype=specs[n][1], device=b.device)
                   for n in RECORDS}
            rec["steps_run"] = torch.zeros(b.n_envs, dtype=torch.int32, device=b.device)
            self._rec[K] = rec
        return rec

    def history(self, T):
        """The episode-long records of run(histories=True), allocated once per T = episode_limit + 1 and reused by
        later runs: HISTORY_RECORDS as [T, ...] at the records' pre-fill, steps_run, the observation pass's rows
        (obs0, cnt0; rs0 is initial["rs"]) and the counts of asvrl_eval_history_count. Rows at or behind an env's
        evaluation end keep whatever an earlier window or run left there: nothing reads them."""
        H = self._hist.get(T)
        if H is None:
            b = self.batch
            specs = b._record_specs()
            specs["actions"] = ((b.n_envs * b.max_robots, 2), torch.float64, 0)
            H = {n: torch.full((T,) + specs[n][0], specs[n][2], dtype=specs[n][1], device=b.device)
                 for n in HISTORY_RECORDS}
            H["steps_run"] = torch.zeros(b.n_envs, dtype=torch.int32, device=b.device)
            H["obs0"], H["cnt0"] = torch.zeros_like(b.obs), torch.zeros_like(b.obj_cnt)
            H["counts"] = torch.zeros((3, b.n_envs * b.max_robots), dtype=torch.int32, device=b.device)
            self._hist[T] = H
        return H

    def distribution(self, T, kind):
        """The planes of run(distribution=...), allocated once per T and reused: z, tau [T, NT, 32] f32 and G [T, NT]
        f64, the per-robot outputs of asvrl_eval_dist_stats, and what the readout of `kind` needs beside them."""
        D = self._dist.get(T)
        if D is None:
            b = self.batch
            NT, dev = b.n_envs * b.max_robots, b.device
            D = dict(z=torch.zeros((T, NT, _abi.DIST_SAMPLES), dtype=torch.float32, device=dev),
                     tau=torch.zeros((T, NT, _abi.DIST_SAMPLES), dtype=torch.float32, device=dev),
                     G=torch.zeros((T, NT), dtype=torch.float64, device=dev), out=new_dist_outputs(NT, dev))
            self._dist[T] = D
        if kind == "iqn" and "greedy" not in D:
            D["greedy"] = torch.zeros(D["G"].shape, dtype=torch.int32, device=D["G"].device)
        if kind == "critic" and "act32" not in D:
            D["act32"] = torch.zeros(D["G"].shape + (2,), dtype=torch.float32, device=D["G"].device)
        return D

    @staticmethod
    def window(H, t0, k, names):
        """The window at t0 of length k as keep= tensors: the slices [t0:t0 + k] of the episode-long records."""
        rec = {n: H[n][t0:t0 + k] for n in names}
        rec["steps_run"] = H["steps_run"]
        return rec


class DeviceEvaluator:
    def __init__(self, configs, template_env=None, device=None, chunk=64, gamma=0.99):
        """configs: the eval configs (MarineNavEnv3.episode_data); template_env: the eval env whose current
        curriculum attributes seed the robots (evaluate_configs' argument); chunk: steps per window; gamma: the
        discount of the returns (agent.GAMMA)."""
        dev = torch.device(device) if device is not None else (template_env._device if template_env is not None
                                                               else torch.device("cuda"))
        if int(chunk) < 1:
            raise ValueError("chunk must be >= 1")
        self.device, self.chunk, self.gamma = dev, int(chunk), float(gamma)
        self.envs, self.initial_states = [], []
        for cfg in configs:
            env = MarineNavEnv3(seed=0, is_eval_env=True, device=dev)
            if template_env is not None:   # evaluate_configs: env.py:569 seeds robots from the CURRENT attributes
                for k in ("num_robots", "num_cores", "num_obs", "min_start_goal_dis"):
                    setattr(env, k, getattr(template_env, k))
            st, _, _ = env.reset_with_eval_config(cfg)
            self.envs.append(env)
            self.initial_states.append(st)
        self.n_robots = [len(env.robots) for env in self.envs]
        by_key = {}
        for e, env in enumerate(self.envs):
            by_key.setdefault(env.env_key(), []).append(e)
        self.groups = [_Group(members, [self.envs[e] for e in members], dev) for members in by_key.values()]
        self.windows = 0       # windows of the last run
        self.steps = 0         # env-steps the last run enqueued per env, at most

    # ------------------------------------------------------------------ pieces
    def rows(self, config):
        """(group index, first row) of a config's robots in its group's batch."""
        for g, grp in enumerate(self.groups):
            if config in grp.members:
                return g, grp.members.index(config) * grp.batch.max_robots
        raise IndexError(config)

    def zero_noise(self, T=None):
        """Explicit zero perception noise for every group: [T, NT, O + R, 5] f64 (T None: one pass)."""
        out = []
        for grp in self.groups:
            b = grp.batch
            shape = (b.n_envs * b.max_robots, b.max_obs + b.max_robots, 5)
            out.append(torch.zeros(shape if T is None else (int(T),) + shape, dtype=torch.float64, device=self.device))
        return out

    def _per_group(self, x, what):
        if x is None:
            return [None] * len(self.groups)
        if torch.is_tensor(x):
            if len(self.groups) != 1:
                raise ValueError(f"{what}: {len(self.groups)} parameter groups need a list, one tensor per group")
            return [x]
        if len(x) != len(self.groups):
            raise ValueError(f"{what}: {len(x)} tensors for {len(self.groups)} parameter groups")
        return list(x)

    def observe(self, noise=None, seed=0, perception="philox"):
        """Restore the initial state, zero the carried metrics and run the observation pass (the do_dynamics = 0
        step of VecMarineNavEnv.reset) into every batch's obs / obs64 / obj_cnt. noise: explicit draws per group
        ([NT, O + R, 5] f64) instead of the Philox stream. perception="numpy": the pass's rows come from the robots'
        RandomState streams, restored to their seeds first (noise must be None); the streams then stand where each
        robot's Perception stands after reset_with_eval_config, and their draw counters are zeroed behind the pass."""
        _check_perception("observe", perception, noise)
        noise = self._per_group(noise, "observe noise")
        for g, grp in enumerate(self.groups):
            grp.restore()
            if perception == "numpy":
                ns = grp.streams()
                ns.restore()
                grp.batch.step(None, do_dynamics=False, noise=ns.fill(grp.batch))
                ns.zero_counters()
                continue
            grp.batch.step(None, do_dynamics=False, noise=noise[g], seed=seed + g, counter=OBS_COUNTER,
                           fast_noise=True)

    @torch.no_grad()
    def run(self, pack=None, *, actions=None, noise=None, obs_noise=None, seed=0, episode_limit=1000, sync=True,
            is_continuous=None, policy_seed=0, deterministic=False, cvar=1.0, perception="philox", histories=False,
            distribution=None):
        """One evaluation of every config. pack: the Actor's MlpPack or DQN's DqnPack, greedy in closed-loop
        windows, or SAC's SacActorPack, which samples its action as act_sac does in evaluation too (group g draws
        under policy_seed + g: rows are batch-local, so two groups share no draws) or, with deterministic=True (a
        ValueError for any other pack), takes its mean action, or IQN's IqnPack, greedy over the mean of K = 32
        quantile samples whose fractions are drawn per act (group g under policy_seed + g, as for SAC) and, with
        cvar in (0, 1] (a ValueError for any other pack and outside the range), distorted as act_iqn(cvar=) does -- or
        with cvar a fused_iqn.AdaptiveCvar, at the level the rule gives every robot at every act from the row it acts
        on (with histories, EvalHistory.cvar(c, i); a per-row tensor is not offered: the rows are regrouped per
        config batch); the result's "cvar" is the float or the rule's three parameters --, or
        Rainbow's RainbowPack, greedy on the images of its last refresh() (FusedRainbow.eval_pack: mu only, as the
        reference's policy_local.eval(); group g under policy_seed + g as well, though at epsilon 0 nothing is drawn); or actions: a [T, NT, 2] f64 table per group (a tensor when there is one group, else a list)
        applied open loop, with noise ([T, NT, O + R, 5] f64 per group) or the Philox stream. is_continuous: what
        the table's rows are -- True (also None, the default) thrust commands, False column 0 is the action index;
        with a pack it follows the pack (None) and a value that contradicts it is a ValueError. obs_noise: the observation pass's explicit
        draws. sync: one host wait per window to stop once every episode has ended; False enqueues the
        ceil((episode_limit + 1) / chunk) windows without a host wait. Returns evaluate_configs' per-config lists
        (rewards, successes, times, energies, lengths; observations / actions / trajectories / relations empty per
        robot) and the per-robot arrays robot_rewards, robot_times, robot_energies, robot_outcomes (0 running at
        the end, 1 goal, 2 collision).
        perception: "philox" (the default: the noise described above) or "numpy": the perception noise of the
        observation pass and of every step is drawn from each robot's own RandomState(rob.perception.seed) stream, as
        the reference, Trainer.evaluation and evaluate_configs draw it. Every step is then one asvrl_noise_streams
        launch under env_mask = alive, a window of length 1 on its rows and asvrl_eval_metrics with K = 1 (`chunk`
        only sets how many steps lie between two host waits of sync=True). seed does not enter the perception noise;
        noise= or obs_noise= with it, and any other value of perception, is a ValueError. policy_seed, IQN's tau
        draws, SAC's action noise and the exploration draw stay Philox in both modes. The result then also carries
        draws_n, draws_sum and draws_sq: per config, an array per robot of the count, sum and sum of squares of its
        step draws in draw order (the observation pass's are not counted); in the Philox mode the three are None.
        histories: True keeps the episode's records (the module docstring: 322 bytes per robot-step over
        episode_limit + 1 steps, allocated once) and adds "history", an EvalHistory: the packed trajectory, action,
        observation and object-count arrays and every robot's slices of them; the action history is the `actions`
        record of the windows or, teacher-forced, the caller's table, read as is_continuous says. observations /
        actions / trajectories stay empty per robot until history_lists(result) fills them with the reference's
        lists. False (the default) allocates and launches nothing for them.
        distribution: None (the default: nothing allocated, launched or added), True with an IqnPack, or the AC-IQN
        critic's CriticPack (a trainer's fused2.local_trunk) with its Actor's pack; a ValueError for anything else
        (distribution_source). Keeps the episode-long records of histories=True (packed into "history" only if that is
        set too) and, after the last window, reads out per group the 32 quantile samples behind every recorded
        decision -- IQN: fused_iqn.iqn_dist on the rows the robots acted on, at the recorded action, under the act
        launches' own Philox keys (policy_seed + g, step t) and the run's cvar, or under an AdaptiveCvar the level
        recorded with every action; AC-IQN: fused_critic.critic_dist at the recorded thrust pair, its fractions a
        Philox stream of their own -- and reduces them against the return each robot then collected
        (asvrl_eval_dist_stats). Adds "distribution", an EvalDistribution."""
        if (pack is None) == (actions is None):
            raise ValueError("run takes the Actor's pack or an action table, not both")
        if pack is not None and not pack.is_policy:
            raise ValueError("run: pack must be an MlpPack of kind 'actor'")
        if pack is not None and is_continuous is not None and bool(is_continuous) != pack.continuous:
            raise ValueError("run: is_continuous=%s does not match the pack (a DqnPack, IqnPack or RainbowPack picks "
                             "discrete actions, the Actor continuous ones)" % bool(is_continuous))
        cvar = policy_options("run", pack, cvar, deterministic)   # a float or an AdaptiveCvar (no per-row tensor)
        dist = distribution_source("run", pack, distribution)
        record = bool(histories) or dist is not None   # the episode-long records
        _check_perception("run", perception, noise, obs_noise)
        is_continuous = True if is_continuous is None else bool(is_continuous)
        episode_limit = int(episode_limit)
        actions = self._per_group(actions, "actions")
        noise = self._per_group(noise, "noise")
        total = episode_limit + 1
        if pack is None:
            T = min(int(a.shape[0]) for a in actions)
            total = min(total, T)
        L = pack.L if pack is not None else _abi.lib()
        self.observe(obs_noise, seed, perception)
        hist = names = None
        if record:   # the episode-long records, and what stands in front of step 0
            hist = [grp.history(episode_limit + 1) for grp in self.groups]
            names = HISTORY_RECORDS if pack is not None else tuple(n for n in HISTORY_RECORDS if n != "actions")
            for grp, H in zip(self.groups, hist):
                H["obs0"].copy_(grp.batch.obs)
                H["cnt0"].copy_(grp.batch.obj_cnt)
        numpy_noise = perception == "numpy"
        t0 = self.windows = 0
        while t0 < total:
            k = 1 if numpy_noise else min(self.chunk, total - t0)
            for g, grp in enumerate(self.groups):
                b, st = grp.batch, grp.state
                rec = grp.window(hist[g], t0, k, names) if record else grp.records(k)
                if numpy_noise:   # this step's rows from the streams of the robots still active
                    noise[g] = grp.streams().fill(b, env_mask=st["alive"])[None]
                if pack is not None:
                    grp.step.fill_(t0)
                    b.policy_rollout(pack, k, b.obs, noise=noise[g] if numpy_noise else None, keep=rec,
                                     hold_done=True, trainer_deactivate=True,
                                     step_dev=grp.step, env_mask=st["alive"], seed=seed + g, counter=t0,
                                     fast_noise=True, policy_seed=policy_seed + g, deterministic=deterministic,
                                     cvar=cvar)
                else:
                    nz = noise[g]
                    b.rollout(actions[g][t0:t0 + k], nz if nz is None or numpy_noise else nz[t0:t0 + k], keep=rec,
                              hold_done=True, is_continuous=is_continuous, trainer_deactivate=True,
                              env_mask=st["alive"], seed=seed + g, counter=t0, fast_noise=True)
                eval_metrics(L, k, b.n_envs, b.max_robots, rec, b.n_robots, grp.dt, grp.N, grp.pc, st, self.gamma,
                             episode_limit)
            t0 += k
            self.windows += 1
            if numpy_noise and t0 % self.chunk and t0 < total:
                continue   # one-step windows: the host waits every `chunk` steps
            if sync and not any(bool(grp.state["alive"].any().item()) for grp in self.groups):
                break   # one host wait per window
        self.steps = t0
        if record:   # the records, the action source per group and how to read it
            hist = dict(L=L, T=episode_limit + 1, records=hist,
                        actions=[H["actions"] for H in hist] if pack is not None else actions,
                        continuous=pack.continuous if pack is not None else is_continuous,
                        levels=not isinstance(cvar, float), pack=bool(histories))
        if dist is not None:
            dist = dict(kind=dist[0], pack=dist[1], seed=int(policy_seed), cvar=cvar)
        out = self._result(check_ended=pack is None and total < episode_limit + 1, draws=numpy_noise, hist=hist,
                           dist=dist)
        out["cvar"] = cvar if isinstance(cvar, float) else cvar.as_dict()
        return out

    def _history(self, hist, counts):
        """The EvalHistory of a run: counts the host image of every group's count planes ([3, NT] each), read in
        _result's one copy. Allocates the four packed outputs for all groups together, packs every group into its
        part with one launch and brings each array over in one copy."""
        counts = [c.astype(np.int64) for c in counts]
        base = np.zeros((len(counts) + 1, 3), np.int64)
        for g, c in enumerate(counts):
            base[g + 1] = base[g] + c.sum(axis=1)
        n_traj, n_act, n_obs = (int(v) for v in base[-1])
        dev = self.device
        out = dict(traj=torch.empty((n_traj, _abi.TRAJ_DIM), dtype=torch.float64, device=dev),
                   act=torch.empty((n_act, 2), dtype=torch.float64, device=dev),
                   obs=torch.empty((n_obs, _abi.HISTORY_OBS_DIM), dtype=torch.float32, device=dev),
                   cnt=torch.empty(n_obs, dtype=torch.int8, device=dev))
        slices = [None] * len(self.envs)
        for g, grp in enumerate(self.groups):
            b, H = grp.batch, hist["records"][g]
            lo, hi = base[g], base[g + 1]
            part = dict(traj=out["traj"][lo[0]:hi[0]], act=out["act"][lo[1]:hi[1]], obs=out["obs"][lo[2]:hi[2]],
                        cnt=out["cnt"][lo[2]:hi[2]])
            src = dict(rs0=grp.initial["rs"], rs=H["rs"], actions=hist["actions"][g], obs0=H["obs0"], obs=H["obs"],
                       cnt0=H["cnt0"], obj_cnt=H["obj_cnt"])
            history_pack(hist["L"], hist["T"], b.n_envs, b.max_robots, H["counts"], H["offsets"], src, part)
            c = counts[g]
            start = np.cumsum(c, axis=1) - c + lo[:, None]
            R = b.max_robots
            for le, cfg in enumerate(grp.members):
                rows = range(le * R, le * R + self.n_robots[cfg])
                slices[cfg] = [tuple(slice(int(start[q, r]), int(start[q, r] + c[q, r])) for q in range(3))
                               for r in rows]
        host = {n: t.cpu().numpy() for n, t in out.items()}
        return EvalHistory(host["traj"], host["act"], host["obs"], host["cnt"], slices, hist["continuous"],
                           hist["levels"])

    def _distribution_pass(self, g, hist, dist):
        """Group g's readout and reduction behind the last window (the count launch has run): the quantile samples of
        the steps that ran -- obs0 and the recorded action of step 0, then obs[0 : steps - 1] and the actions of the
        steps 1 .. steps - 1 -- into the group's planes, then asvrl_eval_dist_stats. Returns the planes."""
        from ..fused_critic import critic_dist
        from ..fused_iqn import iqn_dist_launch
        grp, H = self.groups[g], hist["records"][g]
        b = grp.batch
        NT, T, S = b.n_envs * b.max_robots, hist["T"], _abi.DIST_SAMPLES
        D = grp.distribution(T, dist["kind"])
        act = H["actions"]
        for t0, t1, obs in ((0, 1, H["obs0"]), (1, self.steps, H["obs"][:max(self.steps - 1, 0)])):
            if t1 <= t0:
                continue
            M = (t1 - t0) * NT
            rows, a64 = obs.reshape(M, _abi.OBS_DIM), act[t0:t1].reshape(M, 2)
            z, tau = D["z"][t0:t1].view(M, S), D["tau"][t0:t1].view(M, S)
            if dist["kind"] == "iqn":
                per_robot = not isinstance(dist["cvar"], float)   # the level recorded with every action
                levels = a64[:, 1].to(torch.float32).contiguous() if per_robot else None
                iqn_dist_launch(dist["pack"], rows, NT, t0, dist["seed"] + g, 1.0 if per_robot else dist["cvar"], levels,
                                None, a64, z, tau, None, D["greedy"][t0:t1].view(M), None)
            else:
                critic_dist(dist["pack"], rows, a64, rows_per_step=NT, step0=t0, seed=dist["seed"] + g, z_out=z,
                            tau_out=tau, act32=D["act32"][t0:t1].view(M, 2))
        for t in D["out"].values():
            t.zero_()
        eval_dist_stats(hist["L"], T, b.n_envs, b.max_robots, D["z"], D["tau"], H["reward"], H["counts"][1],
                        b.n_robots, self.gamma, D["out"], D["G"])
        return D

    def _result(self, check_ended=False, draws=False, hist=None, dist=None):
        # one copy: every group's lengths, ended flags, outcomes and sums in one f64 tensor
        parts = []
        for grp in self.groups:
            st = grp.state
            parts += [st["length"].double(), st["ended"].double(), st["outcome"].double(), st["ret"], st["time"],
                      st["energy"]]
        if hist is not None:   # behind them every group's history counts; their scans stay on the device
            for grp, H in zip(self.groups, hist["records"]):
                b = grp.batch
                history_count(hist["L"], hist["T"], b.n_envs, b.max_robots, H["info"], grp.state["length"],
                              b.n_robots, counts=H["counts"])
                H["offsets"] = history_offsets(H["counts"])
                parts.append(H["counts"].double().reshape(-1))
        planes = []
        if dist is not None:   # behind those every group's per-robot distribution outputs (and IQN's mismatch count)
            for g, (grp, H) in enumerate(zip(self.groups, hist["records"])):
                D = self._distribution_pass(g, hist, dist)
                planes.append(D)
                parts += [D["out"][n].double().reshape(-1) for n, _, _ in DIST_OUTPUTS]
                if dist["kind"] == "iqn":
                    k = self.steps
                    acted = torch.arange(k, device=self.device)[:, None] < H["counts"][1][None, :]
                    parts.append(((D["greedy"][:k].double() != H["actions"][:k, :, 0]) & acted).sum().double()[None])
        flat = torch.cat(parts).cpu().numpy()
        n = len(self.envs)
        out = dict(observations=[None] * n, actions=[None] * n, trajectories=[None] * n, rewards=[None] * n,
                   successes=[None] * n, times=[None] * n, energies=[None] * n, relations=[None] * n,
                   lengths=[None] * n, robot_rewards=[None] * n, robot_times=[None] * n, robot_energies=[None] * n,
                   robot_outcomes=[None] * n, draws_n=None, draws_sum=None, draws_sq=None)
        if draws:
            for name in ("draws_n", "draws_sum", "draws_sq"):
                out[name] = [None] * n
            for grp in self.groups:
                R = grp.batch.max_robots
                for name, a in zip(("draws_n", "draws_sum", "draws_sq"), grp.streams().counters()):
                    for le, c in enumerate(grp.members):
                        out[name][c] = a[le * R:le * R + self.n_robots[c]].copy()
        at = 0
        for grp in self.groups:
            E, R = grp.batch.n_envs, grp.batch.max_robots
            NT = E * R
            length, ended = flat[at:at + E], flat[at + E:at + 2 * E]
            at += 2 * E
            outcome, ret, tim, en = (flat[at + q * NT:at + (q + 1) * NT].reshape(E, R) for q in range(4))
            at += 4 * NT
            if check_ended and not ended.all():
                raise ValueError("the action table ran out before every episode ended")
            for le, c in enumerate(grp.members):
                k = self.n_robots[c]
                out["robot_rewards"][c] = ret[le, :k].copy()
                out["robot_times"][c] = tim[le, :k].copy()
                out["robot_energies"][c] = en[le, :k].copy()
                out["robot_outcomes"][c] = outcome[le, :k].astype(np.uint8)
                out["rewards"][c] = np.mean(ret[le, :k])          # trainer.py:347-365
                out["successes"][c] = bool((outcome[le, :k] == 1).all())
                out["times"][c] = np.mean(tim[le, :k])
                out["energies"][c] = np.mean(en[le, :k])
                out["lengths"][c] = int(length[le])
                for name in ("observations", "actions", "trajectories", "relations"):
                    out[name][c] = [[] for _ in range(k)]
        if hist is not None:
            counts = []
            for grp in self.groups:
                NT = grp.batch.n_envs * grp.batch.max_robots
                counts.append(flat[at:at + 3 * NT].reshape(3, NT))
                at += 3 * NT
            if hist["pack"]:
                out["history"] = self._history(hist, counts)
        if dist is not None:
            arrays = {name: [None] * n for name in EvalDistribution.ARRAYS}
            where, mismatches = [None] * n, 0
            for g, grp in enumerate(self.groups):
                R = grp.batch.max_robots
                NT = grp.batch.n_envs * R
                got = {}
                for name, dt, tail in DIST_OUTPUTS:
                    w = NT * int(np.prod(tail, dtype=np.int64))
                    got[name] = flat[at:at + w].reshape((NT,) + tail)
                    at += w
                if dist["kind"] == "iqn":
                    mismatches += int(flat[at])
                    at += 1
                for le, c in enumerate(grp.members):
                    sl = slice(le * R, le * R + self.n_robots[c])
                    where[c] = (g, le * R)
                    for name, dt, _ in DIST_OUTPUTS:
                        arrays[name][c] = got[name][sl].astype(np.int32 if dt == torch.int32 else np.float64)
                    arrays["truncated"][c] = out["robot_outcomes"][c] == 0
            out["distribution"] = EvalDistribution(arrays, where, planes, mismatches if dist["kind"] == "iqn" else None,
                                                   dist["kind"])
        return out
