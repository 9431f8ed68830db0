"""Device-resident env batch: the HBM layout of E ASV envs and the launches on it.

One DeviceEnvBatch owns the SoA state of `n_envs` MarineNavEnv3 scenes (include/asvrl.h
AsvEnvState) as torch tensors on the GPU and calls the gfx950 kernels through the C ABI.
Both the vectorised training env (vec_env.VecMarineNavEnv) and the drop-in single-env
MarineNavEnv3 (envs/marinenav/env.py) sit on top of it.
"""
import ctypes as C
import types

import torch

from . import _abi
from ._abi import OBS_DIM, NUM_FIELDS


class DeviceEnvBatch:
    def __init__(self, n_envs, max_robots, max_obs, max_cores=0, device="cuda", params=None, obs64=False):
        _abi.lib()  # fail loudly before allocating anything
        if max_robots < 1 or max_robots > 256:
            raise ValueError("max_robots must be in [1, 256]")
        self.n_envs, self.max_robots, self.max_obs, self.max_cores = n_envs, max_robots, max_obs, max_cores
        self.device = torch.device(device)
        self.params = params if params is not None else _abi.params_from()
        E, R, O, Cc = n_envs, max_robots, max(max_obs, 0), max(max_cores, 0)
        NT = E * R
        dev = self.device
        f64 = dict(dtype=torch.float64, device=dev)
        self.rs = torch.zeros((NUM_FIELDS, NT), **f64)
        self.rflags = torch.zeros(NT, dtype=torch.uint8, device=dev)
        self.n_robots = torch.zeros(E, dtype=torch.int32, device=dev)
        self.n_obs = torch.zeros(E, dtype=torch.int32, device=dev)
        self.n_cores = torch.zeros(E, dtype=torch.int32, device=dev)
        self.ep_ts = torch.zeros(E, dtype=torch.int32, device=dev)
        self.obstacles = torch.zeros((E, max(O, 1), 3), **f64)
        self.cores = torch.zeros((E, max(Cc, 1), 4), **f64)
        # outputs
        self.obs = torch.zeros((NT, OBS_DIM), dtype=torch.float32, device=dev)
        self.obs64 = torch.zeros((NT, 32), **f64) if obs64 else None
        self.obj_cnt = torch.zeros(NT, dtype=torch.int8, device=dev)
        self.reward = torch.zeros(NT, **f64)
        self.done = torch.zeros(NT, dtype=torch.uint8, device=dev)
        self.info = torch.zeros(NT, dtype=torch.uint8, device=dev)
        self.env_done = torch.zeros(E, dtype=torch.uint8, device=dev)
        self.stats = torch.zeros(8, **f64)
        # optional per-robot AsvParams table (AsvEnvState.robot_params; set_robot_params)
        self.robot_params = None

    def set_robot_params(self, table):
        """Every robot slot's own vehicle / perception parameters: a sequence of n_envs * max_robots
        AsvParams (reset_with_eval_config, env.py:553-607), or None for `params` everywhere. The
        table's env-level members are ignored (the kernel takes those from `params`)."""
        if table is None:
            self.robot_params = None
            return
        NT = self.n_envs * self.max_robots
        if len(table) != NT:
            raise ValueError(f"robot parameter table: {len(table)} entries for {NT} robot slots")
        arr = (_abi.AsvParams * NT)(*table)
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        if self.robot_params is None or self.robot_params.numel() != host.numel():
            self.robot_params = torch.empty(host.numel(), dtype=torch.uint8, device=self.device)
        self.robot_params.copy_(host)

    # ------------------------------------------------------------------ ABI structs
    def state_struct(self):
        s = _abi.AsvEnvState()
        s.n_envs, s.max_robots, s.max_obs, s.max_cores = self.n_envs, self.max_robots, self.max_obs, self.max_cores
        s.rs = self.rs.data_ptr()
        s.rflags = self.rflags.data_ptr()
        s.n_robots = self.n_robots.data_ptr()
        s.n_obs = self.n_obs.data_ptr()
        s.n_cores = self.n_cores.data_ptr()
        s.ep_ts = self.ep_ts.data_ptr()
        s.obstacles = self.obstacles.data_ptr()
        s.cores = self.cores.data_ptr()
        s.robot_params = self.robot_params.data_ptr() if self.robot_params is not None else None
        return s

    def out_struct(self, obs=None, obj_cnt=None, with_env_done=True):
        o = _abi.AsvStepOut()
        o.obs = (obs if obs is not None else self.obs).data_ptr()
        o.obs64 = self.obs64.data_ptr() if self.obs64 is not None else None
        o.obj_cnt = (obj_cnt if obj_cnt is not None else self.obj_cnt).data_ptr()
        o.reward = self.reward.data_ptr()
        o.done = self.done.data_ptr()
        o.info = self.info.data_ptr()
        o.env_done = self.env_done.data_ptr() if with_env_done else None
        o.stats = self.stats.data_ptr() if with_env_done else None
        return o

    # ------------------------------------------------------------------ launches
    def step(self, actions, is_continuous=True, noise=None, do_dynamics=True, trainer_deactivate=False,
             seed=0, counter=0, counter_dev=None, gamma=0.0, env_mask=None, obs=None, obj_cnt=None, stream=None,
             fast_noise=False, launch=None):
        """asvrl_env_step. actions: f64 [E*R, 2] device tensor. noise: f64 [E*R, O+R, 5] or None (Philox;
        fast_noise: f32 draws, noise_mode 2). launch: (layout, block, envs_per_block) of the kernel
        (asvrl_env_step_ex; _abi.ENV_LAYOUT_*), None = automatic."""
        ctl = _abi.AsvStepCtl()
        ctl.is_continuous = int(bool(is_continuous))
        ctl.do_dynamics = int(bool(do_dynamics))
        ctl.trainer_deactivate = int(bool(trainer_deactivate))
        ctl.noise_mode = 0 if noise is not None else (2 if fast_noise else 1)
        ctl.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        ctl.counter = int(counter) & 0xFFFFFFFFFFFFFFFF
        ctl.counter_dev = counter_dev.data_ptr() if counter_dev is not None else None
        ctl.gamma = float(gamma)
        ctl.env_mask = env_mask.data_ptr() if env_mask is not None else None
        if actions is not None:
            assert actions.dtype == torch.float64 and actions.is_contiguous()
            assert actions.numel() >= 2 * self.n_envs * self.max_robots
        if noise is not None:
            assert noise.dtype == torch.float64 and noise.is_contiguous()
            assert noise.numel() >= self.n_envs * self.max_robots * (self.max_obs + self.max_robots) * 5
        st = self.state_struct()
        out = self.out_struct(obs, obj_cnt, with_env_done=trainer_deactivate)
        if launch is None:
            rc = _abi.lib().asvrl_env_step(C.byref(self.params), C.byref(st), _abi.ptr(actions), _abi.ptr(noise),
                                           C.byref(ctl), C.byref(out), _abi.stream_ptr(stream))
        else:
            ln = _abi.AsvEnvLaunch(*(int(v) for v in launch))
            rc = _abi.lib().asvrl_env_step_ex(C.byref(self.params), C.byref(st), _abi.ptr(actions), _abi.ptr(noise),
                                              C.byref(ctl), C.byref(out), C.byref(ln), _abi.stream_ptr(stream))
        _abi.check(rc, "asvrl_env_step")

    # per-step records of rollout(): name -> (row shape, dtype, pre-fill of rows the env did not take)
    def _record_specs(self):
        NT, E = self.n_envs * self.max_robots, self.n_envs
        return {"reward": ((NT,), torch.float64, 0), "done": ((NT,), torch.uint8, 1),
                "info": ((NT,), torch.uint8, _abi.INFO_ABSENT), "env_done": ((E,), torch.uint8, 0),
                "obs": ((NT, OBS_DIM), torch.float32, 0), "obj_cnt": ((NT,), torch.int8, 0),
                "rs": ((NUM_FIELDS, NT), torch.float64, 0)}

    def _records(self, who, keep, K, specs, trainer_deactivate):
        """The kept records of a K-step rollout: allocated at their pre-fill, or the caller's own tensors (keep a
        dict name -> tensor). Returns (name -> tensor, steps_run)."""
        given = dict(keep) if isinstance(keep, dict) else {}
        rec = {}
        for name in keep:
            if name == "steps_run":
                continue
            if name not in specs:
                raise ValueError(f"{who}: unknown record {name!r}; choose from {sorted(specs)}")
            if name == "env_done" and not trainer_deactivate:
                raise ValueError(f"{who}: the env_done record needs trainer_deactivate")
            shape, dtype, fill = specs[name]
            t = given.get(name)
            if t is None:
                t = torch.full((K,) + shape, fill, dtype=dtype, device=self.device)
            assert t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == (K,) + shape, name
            rec[name] = t
        steps_run = given.get("steps_run")
        if steps_run is None:
            steps_run = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        assert steps_run.dtype == torch.int32 and steps_run.numel() == self.n_envs
        return rec, steps_run

    def _auto_reset(self, who, auto_reset, K, specs):
        """The AsvAutoReset of rollout(auto_reset=...) / policy_rollout(auto_reset=...): a dict or namespace with
        cfg (AsvResetCfg), reset_counter, obs_counter and, for the open loop's obs_prev record, obs_in; optionally
        the caller's own pushed [K] / resets [E] i32 tensors (graph capture). Adds the obs_prev record to specs.
        Returns (struct, pushed, resets); pushed is zeroed here."""
        get = auto_reset.get if isinstance(auto_reset, dict) else (lambda k, d=None: getattr(auto_reset, k, d))
        NT = self.n_envs * self.max_robots
        specs["obs_prev"] = ((NT, OBS_DIM), torch.float32, 0)
        ar = _abi.AsvAutoReset()
        cfg = get("cfg")
        if cfg is None:
            raise ValueError(f"{who}: auto_reset needs cfg (an AsvResetCfg)")
        ar.cfg = cfg
        ar.reset_counter = int(get("reset_counter", 0)) & 0xFFFFFFFFFFFFFFFF
        ar.obs_counter = int(get("obs_counter", 0)) & 0xFFFFFFFFFFFFFFFF
        obs_in = get("obs_in")
        if obs_in is not None:
            assert obs_in.dtype == torch.float32 and obs_in.is_contiguous() and tuple(obs_in.shape) == (NT, OBS_DIM)
            ar.obs_in = obs_in.data_ptr()
        pushed, resets = get("pushed"), get("resets")
        if pushed is None:
            pushed = torch.zeros(K, dtype=torch.int32, device=self.device)
        else:
            assert pushed.dtype == torch.int32 and pushed.numel() == K and pushed.is_contiguous()
            pushed.zero_()
        if resets is None:
            resets = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        assert resets.dtype == torch.int32 and resets.numel() == self.n_envs and resets.is_contiguous()
        ar.pushed, ar.resets = pushed.data_ptr(), resets.data_ptr()
        return ar, pushed, resets

    def _rollout_args(self, who, K, extra_specs, *, noise, keep, hold_done, is_continuous, trainer_deactivate, seed,
                      counter, counter_dev, gamma, env_mask, obs, obj_cnt, fast_noise, launch, auto_reset):
        """What rollout() and policy_rollout() build alike: a namespace of the AsvStepCtl (ctl), the AsvRollout
        without its actions (ro), the AsvAutoReset or None (ar, with pushed / resets), the kept records (specs, rec,
        steps_run), the state and output structs (st, out) and the launch (ln)."""
        if noise is not None:
            assert noise.dtype == torch.float64 and noise.is_contiguous()
            assert noise.numel() == K * self.n_envs * self.max_robots * (self.max_obs + self.max_robots) * 5
        specs = self._record_specs()
        specs.update(extra_specs)
        ar = pushed = resets = None
        if auto_reset is not None:
            ar, pushed, resets = self._auto_reset(who, auto_reset, K, specs)
        rec, steps_run = self._records(who, keep, K, specs, trainer_deactivate)
        ctl = _abi.AsvStepCtl()
        ctl.is_continuous = int(bool(is_continuous))
        ctl.do_dynamics = 1
        ctl.trainer_deactivate = int(bool(trainer_deactivate))
        ctl.noise_mode = 0 if noise is not None else (2 if fast_noise else 1)
        ctl.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        ctl.counter = int(counter) & 0xFFFFFFFFFFFFFFFF
        ctl.counter_dev = counter_dev.data_ptr() if counter_dev is not None else None
        ctl.gamma = float(gamma)
        ctl.env_mask = env_mask.data_ptr() if env_mask is not None else None
        ro = _abi.AsvRollout()
        ro.n_steps, ro.hold_done = K, int(bool(hold_done))
        ro.noise = noise.data_ptr() if noise is not None else None
        for name, t in rec.items():
            if name not in ("actions", "obs_prev"):   # (AsvPolicy's and AsvAutoReset's records)
                setattr(ro, name, t.data_ptr())
        ro.steps_run = steps_run.data_ptr()
        if ar is not None:
            ar.obs_prev = rec["obs_prev"].data_ptr() if "obs_prev" in rec else None
        ln = C.byref(_abi.AsvEnvLaunch(*(int(v) for v in launch))) if launch is not None else None
        return types.SimpleNamespace(ctl=ctl, ro=ro, ar=ar, pushed=pushed, resets=resets, specs=specs, rec=rec,
                                     steps_run=steps_run, st=self.state_struct(), ln=ln,
                                     out=self.out_struct(obs, obj_cnt, with_env_done=trainer_deactivate))

    def _rollout_call(self, b, L, name, extra, stream):
        """Call `name` of library L on _rollout_args' b (its _ar form under auto_reset), `extra` the arguments between
        the AsvRollout and the auto-reset; returns the namespace of the kept records and counts."""
        args = [C.byref(self.params), C.byref(b.st), C.byref(b.ctl), C.byref(b.out), C.byref(b.ro)] + extra
        counts = {}
        if b.ar is not None:
            name += "_ar"
            args.append(C.byref(b.ar))
            counts = dict(resets=b.resets, pushed=b.pushed)
        rc = getattr(L, name)(*args, b.ln, _abi.stream_ptr(stream))
        _abi.check(rc, name, L)
        return types.SimpleNamespace(steps_run=b.steps_run, **counts, **{n: b.rec.get(n) for n in b.specs})

    def rollout(self, actions, noise=None, *, keep=("reward", "done", "info"), hold_done=False, is_continuous=True,
                trainer_deactivate=False, seed=0, counter=0, counter_dev=None, gamma=0.0, env_mask=None, obs=None,
                obj_cnt=None, fast_noise=False, launch=None, stream=None, auto_reset=None):
        """asvrl_env_rollout: K = actions.shape[0] open-loop steps in one launch, bit for bit the K calls
        step(actions[t], noise[t], counter=counter + t). actions: f64 [K, E*R, 2]; noise: f64 [K, E*R, O+R, 5]
        or None (Philox). keep: the per-step records to return, names out of reward, done, info, env_done, obs,
        obj_cnt, rs (allocated here, [K, ...] each; rows of steps an env did not take -- masked, or after a
        hold -- stay at done = 1, info = INFO_ABSENT, zero elsewhere), or a dict name -> the caller's own
        pre-filled tensor (also "steps_run": nothing is allocated then and the call can be graph-captured).
        hold_done (needs trainer_deactivate): an env stops after the step that sets its env_done. The last
        step's outputs land where step() writes them (obs / obj_cnt, self.reward, ...). Returns a namespace of
        the kept records (None where not kept) and steps_run [E] i32. No host sync.
        auto_reset (asvrl_env_rollout_ar; see _auto_reset): an env whose episode ends in step t is reset inside the
        window (cfg at reset_counter + t) and observed (obs_counter + t) before step t + 1 -- the values of
        reset_observe(cfg, env_done & env_mask, counter=reset_counter + t, obs_counter=obs_counter + t) behind every
        step. Needs trainer_deactivate and Philox noise, not hold_done. keep then also takes "obs_prev"
        (f32 [K, E*R, 40]: the observation every robot row of a stepping env had in front of step t; needs
        auto_reset's obs_in), and the namespace gains resets [E] i32 and pushed [K] i32 (rows with obj_cnt >= 0)."""
        assert actions.dtype == torch.float64 and actions.is_contiguous() and actions.dim() == 3
        K, NT = int(actions.shape[0]), self.n_envs * self.max_robots
        assert tuple(actions.shape[1:]) == (NT, 2)
        b = self._rollout_args("rollout", K, {}, noise=noise, keep=keep, hold_done=hold_done,
                               is_continuous=is_continuous, trainer_deactivate=trainer_deactivate, seed=seed,
                               counter=counter, counter_dev=counter_dev, gamma=gamma, env_mask=env_mask, obs=obs,
                               obj_cnt=obj_cnt, fast_noise=fast_noise, launch=launch, auto_reset=auto_reset)
        b.ro.actions = actions.data_ptr()
        return self._rollout_call(b, _abi.lib(), "asvrl_env_rollout", [], stream)

    def policy_rollout(self, pack, K, obs_in, *, noise=None, keep=("reward", "done", "info"), hold_done=False,
                       step_dev=None, eps=(1.0, 1.0, 1.0, 0.0, 0.0), policy_seed=0, trainer_deactivate=False, seed=0,
                       counter=0, counter_dev=None, gamma=0.0, env_mask=None, obs=None, obj_cnt=None,
                       fast_noise=False, launch=None, stream=None, auto_reset=None, deterministic=False,
                       cvar=1.0):
        """K closed-loop steps in one launch: the policy of `pack` acts on every robot row and the env steps on its
        actions, bit for bit K rounds of the pack's own act call at step = step_dev + t followed by
        step(act64, is_continuous=pack.continuous, counter=counter + t), where round 0 acts on obs_in (f32 [E*R, 40];
        may be the tensor the step writes) and round t > 0 on the observation of round t - 1. pack: an MlpPack of kind
        "actor", a DqnPack, SacActorPack, IqnPack or RainbowPack -- anything with the window-policy surface MlpPack
        describes; each class says what its rounds are and which of cvar / deterministic it takes (a ValueError for
        the others, and for cvar outside (0, 1]; for an IqnPack cvar may also be an f32 tensor [E*R] on this device or
        a fused_iqn.AdaptiveCvar, and "actions" then holds (index, level used) -- a record for evaluation, not for
        a replay push). The call is pack.rollout of pack.L (its _ar form under auto_reset),
        so an f32 pack runs the f32-operand build. eps: (steps_per_count, total, fraction, initial, final) of the
        linear epsilon schedule (the default is greedy); step_dev: i64 device step counter (None: 0), only read. keep,
        noise, hold_done and the remaining arguments are rollout()'s; keep also takes "actions": f64 [K, E*R, 2], the
        action every robot slot of a stepping env was given (rows of steps an env did not take stay 0). No host sync;
        with every record passed in by the caller (and steps_run) the call can be graph-captured.
        auto_reset: as rollout()'s; the policy acts on a reset env's reset observation at the next step, and
        "obs_prev" records the rows it acted on at every step (obs_in comes from this call's own)."""
        K, NT = int(K), self.n_envs * self.max_robots
        assert pack.is_policy
        cvar = policy_options("policy_rollout", pack, cvar, deterministic, rows=NT, device=self.device)
        assert obs_in.dtype == torch.float32 and obs_in.is_contiguous() and tuple(obs_in.shape) == (NT, OBS_DIM)
        if step_dev is not None:
            assert step_dev.dtype == torch.int64 and step_dev.numel() >= 1
        b = self._rollout_args("policy_rollout", K, {"actions": ((NT, 2), torch.float64, 0)}, noise=noise, keep=keep,
                               hold_done=hold_done, is_continuous=pack.continuous, trainer_deactivate=trainer_deactivate,
                               seed=seed, counter=counter, counter_dev=counter_dev, gamma=gamma, env_mask=env_mask,
                               obs=obs, obj_cnt=obj_cnt, fast_noise=fast_noise, launch=launch, auto_reset=auto_reset)
        if b.ar is not None:
            b.ar.obs_in = None
        pi = pack.policy(cvar=cvar, deterministic=deterministic)
        pi.obs_in = obs_in.data_ptr()
        _abi.fill_schedule(pi, step_dev, eps, policy_seed)
        pi.actions = b.rec["actions"].data_ptr() if "actions" in b.rec else None
        risk = getattr(pi, "risk", None)   # IqnPack under a per-robot level: its _risk call, the AsvIqnRisk behind pi
        if risk is not None:
            return self._rollout_call(b, pack.L, pack.rollout_risk, [C.byref(pi), C.byref(risk)], stream)
        return self._rollout_call(b, pack.L, pack.rollout, [C.byref(pi)], stream)

    def reset(self, cfg, env_mask=None, seed=0, counter=0, counter_dev=None, stream=None):
        st = self.state_struct()
        rc = _abi.lib().asvrl_env_reset(C.byref(self.params), C.byref(st), C.byref(cfg), _abi.ptr(env_mask),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter) & 0xFFFFFFFFFFFFFFFF,
                                        _abi.ptr(counter_dev), _abi.stream_ptr(stream))
        _abi.check(rc, "asvrl_env_reset")


    def reset_observe(self, cfg, env_mask, seed=0, counter=0, counter_dev=None, obs_counter=0, obs=None,
                      obj_cnt=None, fast_noise=True, stream=None):
        """asvrl_env_reset_observe: reset the envs of env_mask (reset's sampler at (seed, counter)) and write
        their reset observations (the masked do_dynamics = 0 step at (seed, obs_counter)) in one launch --
        the same values as reset(...) followed by step(None, do_dynamics=False, env_mask=...)."""
        ctl = _abi.AsvStepCtl()
        ctl.is_continuous = 1
        ctl.do_dynamics = 0
        ctl.trainer_deactivate = 0
        ctl.noise_mode = 2 if fast_noise else 1
        ctl.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        ctl.counter = int(obs_counter) & 0xFFFFFFFFFFFFFFFF
        ctl.counter_dev = counter_dev.data_ptr() if counter_dev is not None else None
        ctl.gamma = 0.0
        ctl.env_mask = env_mask.data_ptr()
        st = self.state_struct()
        out = self.out_struct(obs, obj_cnt, with_env_done=False)
        rc = _abi.lib().asvrl_env_reset_observe(C.byref(self.params), C.byref(st), C.byref(cfg), _abi.ptr(env_mask),
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter) & 0xFFFFFFFFFFFFFFFF,
                                                _abi.ptr(counter_dev), C.byref(ctl), C.byref(out),
                                                _abi.stream_ptr(stream))
        _abi.check(rc, "asvrl_env_reset_observe")


def policy_options(who, pack, cvar, deterministic, rows=None, device=None):
    """The refusals of the per-policy options every front end of the closed-loop windows shares (`who`: its name):
    cvar must lie in (0, 1] and differ from 1 only for a pack that takes it, deterministic needs one that takes it.
    pack may be None (DeviceEvaluator.run's action table). Returns cvar as a float.
    A level decided per robot -- an f32 tensor of `rows` values on `device` (one per robot slot, each in (0, 1]:
    checked on the host, one synchronisation) or a fused_iqn.AdaptiveCvar -- is returned as it is, for a pack that
    takes cvar only."""
    from .fused_iqn import is_risk, risk_struct
    if is_risk(cvar):
        if not getattr(pack, "takes_cvar", False):
            raise ValueError(f"{who}: cvar is the risk distortion of IQN's quantile fractions (an IqnPack); "
                             "the other policies have no quantiles to distort")
        if deterministic and not getattr(pack, "takes_deterministic", False):
            raise ValueError(f"{who}: deterministic=True is the sampled actor's mean action (a SacActorPack); "
                             "the Actor and DQN_Policy have no sample to switch off")
        if torch.is_tensor(cvar):
            if rows is None:
                raise ValueError(f"{who}: a per-row cvar is not offered here (the rows are regrouped per batch); "
                                 "pass a float or an AdaptiveCvar")
            risk_struct(cvar, rows, device, who=who)   # dtype, length, device and range
        return cvar
    cvar = float(cvar)
    if not 0.0 < cvar <= 1.0:
        raise ValueError(f"{who}: cvar must be in (0, 1]")
    if cvar != 1.0 and not getattr(pack, "takes_cvar", False):
        raise ValueError(f"{who}: cvar is the risk distortion of IQN's quantile fractions (an IqnPack); "
                         "the other policies have no quantiles to distort")
    if deterministic and not getattr(pack, "takes_deterministic", False):
        raise ValueError(f"{who}: deterministic=True is the sampled actor's mean action (a SacActorPack); "
                         "the Actor and DQN_Policy have no sample to switch off")
    return cvar


def reset_cfg(num_robots=5, num_obs=4, num_cores=0, min_start_goal_dis=40.0, width=55.0, height=55.0,
              clear_r=10.0, obs_r_range=(1.0, 1.0), v_range=(3.0, 3.0), v_rel_max=1.0, p=0.8):
    """AsvResetCfg with the reference's env.py:33-54 defaults (curriculum values override)."""
    c = _abi.AsvResetCfg()
    c.num_robots, c.num_obs, c.num_cores = int(num_robots), int(num_obs), int(num_cores)
    c.min_start_goal_dis, c.width, c.height, c.clear_r = float(min_start_goal_dis), float(width), float(height), float(clear_r)
    c.obs_r_lo, c.obs_r_hi = float(obs_r_range[0]), float(obs_r_range[1])
    c.v_lo, c.v_hi = float(v_range[0]), float(v_range[1])
    c.v_rel_max, c.p_rel = float(v_rel_max), float(p)
    return c


def current_field(cores, core_r, xy, stream=None):
    """Ocean current (env.py:458-501) at points xy [n,2] (device f64) for cores [n_cores,4]."""
    n = xy.shape[0]
    out = torch.empty((n, 3), dtype=torch.float64, device=xy.device)
    nc = 0 if cores is None else int(cores.shape[0])
    rc = _abi.lib().asvrl_current_field(_abi.ptr(cores) if nc else None, nc, float(core_r), _abi.ptr(xy), n,
                                        _abi.ptr(out), _abi.stream_ptr(stream))
    _abi.check(rc, "asvrl_current_field")
    return out
