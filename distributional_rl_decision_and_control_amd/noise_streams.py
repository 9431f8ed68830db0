"""The reference's perception-noise streams on the device (asvrl_noise_streams, csrc/asvrl_noise.hip).

Every robot of the reference draws its perception noise from its own numpy.random.RandomState(seed) (wamv.py:5-40).
NoiseStreams holds one such stream per robot row of a DeviceEnvBatch as numpy's own get_state() tuple -- the 624
MT19937 words, the position, the cached second normal -- in device tensors; fill() advances every drawing robot's
stream by one env step and returns the rows [NT, O + R, 5] f64 that step / rollout / policy_rollout take as explicit
noise. The states are made on the host by numpy itself (RandomState(seed).get_state()), so there is no seeding code on
the device, and a device copy of the initial states is kept to restore from.

On device "cpu" the tensors are host tensors and fill runs asvrl_noise_streams_host, the same draw functions compiled
for the CPU: the check against numpy that needs no GPU.
"""
import ctypes as C

import numpy as np
import torch

from . import _abi

KEY = _abi.RS_KEY_WORDS


def initial_state(seed):
    """(key u32[624], pos, has_gauss, gauss) of numpy.random.RandomState(seed); seed None: an empty stream (a
    padding row, which never draws)."""
    if seed is None:
        return np.zeros(KEY, np.uint32), KEY, 0, 0.0
    _, key, pos, has_gauss, gauss = np.random.RandomState(int(seed)).get_state()
    return key.astype(np.uint32), int(pos), int(has_gauss), float(gauss)


class NoiseStreams:
    def __init__(self, seeds, device="cuda", states=None):
        """seeds: one per robot row (None for a padding row), each the seed of that robot's RandomState; or states:
        one get_state()-like (key, pos, has_gauss, gauss) per row."""
        L = _abi.lib()
        if states is None:
            states = [initial_state(s) for s in seeds]
        self.device = torch.device(device)
        self.n = n = len(states)
        self._call = L.asvrl_noise_streams_host if self.device.type == "cpu" else L.asvrl_noise_streams
        key = np.zeros((n, KEY), np.uint32)
        pos = np.zeros(n, np.int32)
        has = np.zeros(n, np.int32)
        gauss = np.zeros(n, np.float64)
        for r, (k, p, h, g) in enumerate(states):
            key[r], pos[r], has[r], gauss[r] = np.asarray(k, np.uint32), p, h, g
        # torch has no uint32 arithmetic to speak of: the words travel as int32 bit patterns
        self._init = dict(key=torch.from_numpy(key.view(np.int32)).to(self.device),
                          pos=torch.from_numpy(pos).to(self.device),
                          has_gauss=torch.from_numpy(has).to(self.device),
                          gauss=torch.from_numpy(gauss).to(self.device))
        self.key, self.pos, self.has_gauss, self.gauss = (self._init[k].clone()
                                                          for k in ("key", "pos", "has_gauss", "gauss"))
        self.draws_n = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.draws_sum = torch.zeros(n, dtype=torch.float64, device=self.device)
        self.draws_sq = torch.zeros(n, dtype=torch.float64, device=self.device)
        self._rows = {}

    def restore(self):
        """Back to the initial states, counters zeroed."""
        for k, t in self._init.items():
            getattr(self, k).copy_(t)
        self.zero_counters()

    def zero_counters(self):
        self.draws_n.zero_()
        self.draws_sum.zero_()
        self.draws_sq.zero_()

    def state(self, row):
        """Row `row`'s stream as RandomState.get_state() returns it (one copy to the host)."""
        return ("MT19937", self.key[row].cpu().numpy().view(np.uint32).copy(), int(self.pos[row]),
                int(self.has_gauss[row]), float(self.gauss[row]))

    def counters(self):
        """(draws_n i64, draws_sum, draws_sq) as host arrays."""
        return self.draws_n.cpu().numpy(), self.draws_sum.cpu().numpy(), self.draws_sq.cpu().numpy()

    def fill_raw(self, params, n_envs, max_robots, max_obs, n_robots, n_obs, rflags, env_mask=None,
                 robot_params=None, out=None, stream=None):
        """asvrl_noise_streams on the tensors of a batch: n_robots / n_obs i32 [E], rflags u8 [NT], env_mask u8 [E]
        or None, robot_params the batch's per-robot AsvParams table (a u8 tensor) or None. Returns the rows
        [NT, O + R, 5] f64 (out, or a tensor kept per shape and overwritten by the next call)."""
        E, R, O = int(n_envs), int(max_robots), max(int(max_obs), 0)
        NT = E * R
        if NT != self.n:
            raise ValueError(f"NoiseStreams: {self.n} streams for {NT} robot rows")
        if out is None:
            out = self._rows.get((NT, O + R))
            if out is None:
                out = self._rows[(NT, O + R)] = torch.zeros((NT, O + R, 5), dtype=torch.float64, device=self.device)
        assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == NT * (O + R) * 5
        for t, dtype, numel in ((n_robots, torch.int32, E), (n_obs, torch.int32, E), (rflags, torch.uint8, NT)):
            assert t.dtype == dtype and t.is_contiguous() and t.numel() >= numel and t.device.type == self.device.type
        if env_mask is not None:
            assert env_mask.dtype == torch.uint8 and env_mask.numel() >= E and env_mask.is_contiguous()
        s = _abi.AsvNoiseStreams()
        s.n_envs, s.max_robots, s.max_obs = E, R, O
        s.n_robots, s.n_obs, s.rflags = n_robots.data_ptr(), n_obs.data_ptr(), rflags.data_ptr()
        s.env_mask = env_mask.data_ptr() if env_mask is not None else None
        s.robot_params = robot_params.data_ptr() if robot_params is not None else None
        s.key, s.pos, s.has_gauss, s.gauss = (self.key.data_ptr(), self.pos.data_ptr(), self.has_gauss.data_ptr(),
                                              self.gauss.data_ptr())
        s.noise_out = out.data_ptr()
        s.draws_n, s.draws_sum, s.draws_sq = self.draws_n.data_ptr(), self.draws_sum.data_ptr(), self.draws_sq.data_ptr()
        st = None if self.device.type == "cpu" else _abi.stream_ptr(stream)
        _abi.check(self._call(C.byref(params), C.byref(s), st), "asvrl_noise_streams")
        return out

    def fill(self, batch, env_mask=None, stream=None, out=None):
        """One env step's rows for `batch` (a DeviceEnvBatch) from its current rflags and counts: the robots of the
        envs of env_mask (None: all) that exist and are not deactivated draw, in MarineNavEnv3._pack's order."""
        return self.fill_raw(batch.params, batch.n_envs, batch.max_robots, batch.max_obs, batch.n_robots, batch.n_obs,
                             batch.rflags, env_mask=env_mask, robot_params=batch.robot_params, out=out, stream=stream)
