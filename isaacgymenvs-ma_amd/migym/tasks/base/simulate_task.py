"""The base of the tasks whose control step is three launches around ``mg_sim_simulate`` (FrankaReachMA, Anymal,
HumanoidAMP, Quadcopter): ``mg_<task>_pre``, ``mg_sim_simulate`` x ``controlFrequencyInv``,
``mg_<task>_post``, and ``mg_<task>_reset_idx`` for indexed resets.  A subclass builds its tensors, its params struct
and its views struct in ``create_sim`` and hands the two structs to ``_bind_task``; the launches, the step buffers,
indexed resets and the reset-noise check are here.
"""
from __future__ import annotations

import torch

from ... import _abi
from .vec_task import VecTask

# the tensors of VecTask.env_state_tensors that only the fused step kernels (and their domain randomization) keep
_FUSED_ONLY = ("potentials", "prev_potentials", "up_vec", "heading_vec", "env_props", "randomize_buf_actors")


def state_tensors(drop=(), add=()):
    """VecTask's tuple without the fused kernels' tensors and without ``drop``, then ``add``"""
    return tuple(k for k in VecTask.env_state_tensors if k not in _FUSED_ONLY and k not in drop) + tuple(add)


class SimulateTask(VecTask):
    supports_host_pipeline = False
    steps_through_simulate = True   # gym.simulate is mg_sim_simulate: link forces (apply_rigid_body_force_tensors)
    entry = None   # the prefix of the task's entry points: "mg_anymal" for mg_anymal_pre / _post / _reset_idx

    @classmethod
    def _refuse_randomize(cls, cfg):
        if bool((cfg.get("task", {}) or {}).get("randomize", False)):
            raise NotImplementedError(f"{cls.task_name}: task.randomize is not built for this task (domain "
                                      "randomization runs inside the fused step kernels, which this task does not use)")

    def _bind_task(self, params, views, noise_shape=None):
        """Name the task's params and views structs, once: every launch gets them by reference, so later writes into
        either struct are seen.  ``noise_shape``: the (rows, cols) ``set_reset_noise`` accepts."""
        self._task_views, self._noise_shape = views, noise_shape
        self._params_ref, self._views_ref = _abi.C.byref(params), _abi.C.byref(views)
        lib = self._lib
        self._pre, self._post = getattr(lib, self.entry + "_pre"), getattr(lib, self.entry + "_post")
        self._reset, self._simulate = getattr(lib, self.entry + "_reset_idx"), lib.mg_sim_simulate

    def allocate_buffers(self):
        self._allocate_step_buffers()

    # ---------------------------------------------------------------------------------- hot path
    def _launch_step(self, tb, stream):
        lib, sim, p, v, b = self._lib, self.sim, self._params_ref, self._views_ref, _abi.C.byref(tb)
        _abi.check(self._pre(sim, p, v, b, stream), lib)
        for _ in range(max(1, self.control_freq_inv)):
            _abi.check(self._simulate(sim, stream), lib)
        _abi.check(self._post(sim, p, v, b, None, stream), lib)

    # ---------------------------------------------------------------------------------- API
    def reset_idx(self, env_ids, goal_env_ids=None):
        """reset_idx(ids), one launch (``mg_<task>_reset_idx``) on the listed ids; its draws come from the injected
        noise rows (``set_reset_noise``) or the device RNG"""
        ids = torch.as_tensor(env_ids, device=self.device).flatten().to(torch.int32).contiguous()
        if ids.numel() == 0:
            return
        self._dyn_covered = None
        self._reset_ids = ids   # alive until the launch has consumed it
        tb = self._tb
        tb.step_counter = self.control_steps
        tb.noise = _abi.ptr(self._reset_noise(int(ids.numel())))
        _abi.check(self._reset(self.sim, self._params_ref, self._views_ref, _abi.C.byref(tb), ids.data_ptr(),
                               int(ids.numel()), self._stream()), self._lib)

    def _reset_noise(self, n):
        """the noise tensor of a reset_idx of n ids, or None for the device RNG: rows by env"""
        return self._noise

    def set_reset_noise(self, noise):
        want = self._noise_shape
        if noise is not None and tuple(noise.shape) != want:
            raise ValueError(f"reset noise must be {want}, got {tuple(noise.shape)}")
        super().set_reset_noise(noise)
