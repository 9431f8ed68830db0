"""Shared by the CPU tests of the rollout bindings (tests/test_*_rollout_abi_cpu.py): arguments that pass every check
of a policy's two rollout calls up to the launch, the call itself and the assertion that a call is refused with its
exact text. Driven by the policy's row of _abi.ROLLOUTS, which names the entry point and the policy struct. The
checks fail before anything is launched: the pointers are made-up addresses that are never dereferenced."""
import ctypes as C

P = 0x1000   # a made-up, 16-byte aligned address
TRUNK = ("enc_frag", "b_enc", "w1_frag", "w2_frag", "b1", "b2", "wout", "bout")
IMAGES = {"actor": TRUNK, "dqn": TRUNK, "sac": TRUNK,
          "iqn": ("wc_frag", "w1_frag", "w2_frag", "bc", "b1", "b2", "self_w", "self_b", "obj_w", "obj_b"),
          "rainbow": ("enc", "v1", "a1", "v2", "a2", "vo", "mo", "ao", "b_enc", "b_v1p", "b_a1p", "b_v2p", "b_a2p",
                      "b_vop", "b_mop", "b_aop")}
# where an override's prefix points inside the policy struct (any other prefix names one of the call's arguments)
MEMBERS = {"actor": dict(w=lambda pi: pi.w), "dqn": dict(w=lambda pi: pi.w.trunk, dw=lambda pi: pi.w),
           "sac": dict(w=lambda pi: pi.w.trunk, sw=lambda pi: pi.w),
           "iqn": dict(w=lambda pi: pi.w, hd=lambda pi: pi.head), "rainbow": dict(w=lambda pi: pi.w)}


def _fill(policy, pi):
    pi.obs_in = P
    for n in IMAGES[policy]:
        setattr(MEMBERS[policy]["w"](pi), n, P)
    if policy == "dqn":
        pi.w.head_frag, pi.w.n_actions = P, 25
    elif policy == "sac":
        pi.w.head, pi.w.bhead = P, P
    elif policy == "iqn":
        pi.cvar = 1.0
        pi.head.wo_frag, pi.head.bo, pi.head.n_actions = P, P, 9
    elif policy == "rainbow":
        pi.support = P
        pi.eps_steps_per_count, pi.eps_total, pi.eps_fraction = 1.0, 1.0, 1.0


def _override(a, members, over):
    for k, v in over.items():
        obj, field = k.split("__")
        setattr(members[obj](a["pi"]) if obj in members else a[obj], field, v)


class Rollout:
    """The two rollout entry points of one policy."""

    def __init__(self, policy):
        from distributional_rl_decision_and_control_amd import _abi
        self.policy = policy
        self.entry, self.struct = _abi.ROLLOUTS[policy]
        self.names = (self.entry, self.entry + "_ar")
        self.images = IMAGES[policy]

    def args(self, **over):
        """Arguments that pass every check of both calls up to the launch (nothing is launched: every test overrides
        one of them into a refusal). Overrides are obj__field=value; a prefix in MEMBERS[policy] (w__<image>, ...)
        sets a member inside the policy struct."""
        from distributional_rl_decision_and_control_amd import _abi
        from distributional_rl_decision_and_control_amd.device_env import reset_cfg
        a = dict(params=_abi.params_from(), state=_abi.AsvEnvState(), ctl=_abi.AsvStepCtl(), out=_abi.AsvStepOut(),
                 ro=_abi.AsvRollout(), pi=self.struct(), ar=_abi.AsvAutoReset())
        st = a["state"]
        st.n_envs, st.max_robots, st.max_obs, st.max_cores = 4, 5, 4, 2
        for n in ("rs", "rflags", "n_robots", "n_obs", "n_cores", "ep_ts", "obstacles", "cores"):
            setattr(st, n, P)
        ctl = a["ctl"]
        ctl.is_continuous = int(self.policy in ("actor", "sac"))
        ctl.do_dynamics, ctl.trainer_deactivate, ctl.noise_mode = 1, 1, 2
        for n in ("obs", "obj_cnt", "reward", "done", "info", "env_done"):
            setattr(a["out"], n, P)
        a["ro"].n_steps = 3
        _fill(self.policy, a["pi"])
        a["ar"].cfg = reset_cfg(5, 4, 2)
        _override(a, MEMBERS[self.policy], over)
        return a

    def call(self, L, name, a, null=()):
        order = ["params", "state", "ctl", "out", "ro", "pi"] + (["ar"] if name.endswith("_ar") else [])
        return getattr(L, name)(*[None if k in null else C.byref(a[k]) for k in order], None, None)

    def refused(self, L, name, text, null=(), **over):
        assert self.call(L, name, self.args(**over), null) != 0, (name, text)
        assert L.asvrl_last_error().decode() == f"{name}: {text}"


class WindowAct:
    """The window form of a K-launch policy's act pass (asvrl_iqn_act_ex, asvrl_rainbow_net_act_ex) beside the
    existing act call, which takes the same arguments without `ex`."""

    def __init__(self, policy):
        from distributional_rl_decision_and_control_amd import _abi
        self.policy = policy
        if policy == "iqn":
            self.entry, self.plain = "asvrl_iqn_act_ex", "asvrl_iqn_act"
            self.structs = dict(w=_abi.AsvCriticWeights, hd=_abi.AsvIqnHead, io=_abi.AsvIqnIO, ex=_abi.AsvIqnActEx)
        else:
            self.entry, self.plain = "asvrl_rainbow_net_act_ex", "asvrl_rainbow_net_act"
            self.structs = dict(w=_abi.AsvRainbowImg, io=_abi.AsvRainbowNetIO, ex=_abi.AsvRainbowActEx)

    def args(self, **over):
        """Arguments that pass every check (the tests override one member into a refusal, so nothing is launched)."""
        a = {k: t() for k, t in self.structs.items()}
        for n in IMAGES[self.policy]:
            setattr(a["w"], n, P)
        io = a["io"]
        if self.policy == "iqn":
            a["hd"].wo_frag, a["hd"].bo, a["hd"].n_actions = P, P, 9
            io.obs, io.ld_obs, io.B, io.N, io.act_out, io.ld_act = P, 40, 185, 32, P, 2
            a["ex"].cvar = 1.0
        else:
            io.x, io.ldx, io.N, io.support, io.act_out, io.ld_act = P, 40, 185, P, P, 2
        io.eps_steps_per_count, io.eps_total, io.eps_fraction = 1.0, 1.0, 1.0
        a["ex"].robots_per_env = 5
        for k, v in over.items():
            obj, field = k.split("__")
            setattr(a[obj], field, v)
        return a

    def refused(self, L, text, null=(), **over):
        a = self.args(**over)
        rc = getattr(L, self.entry)(*[None if k in null else C.byref(a[k]) for k in self.structs], None)
        assert rc != 0, text
        assert L.asvrl_last_error().decode() == text

    def plain_refused(self, L, text, **over):
        """The existing act call on the same arguments."""
        a = self.args(**over)
        assert getattr(L, self.plain)(*[C.byref(a[k]) for k in self.structs if k != "ex"], None) != 0
        assert L.asvrl_last_error().decode() == text
