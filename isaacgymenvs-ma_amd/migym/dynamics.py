"""Jacobian / mass-matrix tensors and the fused operational-space controller of a fixed-base articulation.

The counterpart of ``gym.acquire_jacobian_tensor`` / ``acquire_mass_matrix_tensor`` / ``refresh_*`` and of the
reference's ``_compute_osc_torques`` (franka_reach_MA.py:564-565, 770-802, 891-911), on any sim handle of the HIP
library (``mg_dynamics_bind``, ``mg_dynamics_refresh``, ``mg_osc_torques``: include/migym.h).  ``VecTask`` wraps one
of these behind the gym-named calls; tests drive it directly on a sim created from a model table.
"""
from __future__ import annotations

import math

import torch

from . import _abi

# the reference's gains (franka_reach_MA.py:47-50: kp 150, kd 2 sqrt(kp), kp_null 10, kd_null 2 sqrt(kp_null))
DEFAULT_KP = 150.0
DEFAULT_KP_NULL = 10.0


def _vec(x, n, name):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().tolist()
    if isinstance(x, (int, float)):
        x = [float(x)] * n
    x = [float(v) for v in x]
    if len(x) < n:
        raise ValueError(f"{name} needs at least {n} values, got {len(x)}")
    return x[:n]


class DynamicsTensors:
    """Owns the (N*A, nB-1, 6, nD) Jacobian and (N*A, nD, nD) mass-matrix tensors of ``sim`` and launches the kernels.

    lib: the loaded library (``_abi.lib()``); sim: a bound ``mg_sim`` handle of a fixed-base model; spec: its
    ModelSpec; num_actors: N*A; device: the torch device of the sim's tensors."""

    def __init__(self, lib, sim, spec, num_actors, device):
        if not spec.fixed_base:
            # the library's own message (mg_dynamics_bind on a free-base sim)
            rc = lib.mg_dynamics_bind(sim, None)
            msg = lib.mg_last_error().decode() if rc else "dynamics tensors need a fixed-base model"
            raise NotImplementedError(msg)
        self._lib, self._sim, self.spec = lib, sim, spec
        self.num_actors, self.device = int(num_actors), device
        self.num_dofs, self.num_bodies = spec.num_dofs, len(spec.bodies)
        self.jacobian = None
        self.mass_matrix = None
        self._keep = None

    def _bind(self):
        v = _abi.DynamicsViews()
        v.jacobian, v.mass_matrix = _abi.ptr(self.jacobian), _abi.ptr(self.mass_matrix)
        _abi.check(self._lib.mg_dynamics_bind(self._sim, _abi.C.byref(v)), self._lib)

    def acquire_jacobian(self) -> torch.Tensor:
        if self.jacobian is None:
            self.jacobian = torch.zeros((self.num_actors, self.num_bodies - 1, 6, self.num_dofs), device=self.device,
                                        dtype=torch.float32)
            self._bind()
        return self.jacobian

    def acquire_mass_matrix(self) -> torch.Tensor:
        if self.mass_matrix is None:
            self.mass_matrix = torch.zeros((self.num_actors, self.num_dofs, self.num_dofs), device=self.device,
                                           dtype=torch.float32)
            self._bind()
        return self.mass_matrix

    def _stream(self, stream):
        return torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream

    def refresh(self, stream=None):
        """one launch: every acquired tensor from the sim's bound root_states / dof_state (asynchronous)"""
        _abi.check(self._lib.mg_dynamics_refresh(self._sim, self._stream(stream)), self._lib)

    def osc_torques(self, dpose, eef_vel, *, jac_body, arm_dofs=7, kp=DEFAULT_KP, kd=None, kp_null=DEFAULT_KP_NULL,
                    kd_null=None, default_dof_pos=None, effort_limit=None, out=None, out_cols=None, out_stride=None,
                    jac_in=None, mm_in=None, stream=None) -> torch.Tensor:
        """``_compute_osc_torques`` as one launch (mg_osc_torques).

        dpose: (n, 6) contiguous.  eef_vel: (n, 6), contiguous or a strided view whose rows are 6 contiguous floats a
        fixed number of floats apart (``rigid_body_states.view(n, nB, 13)[:, b, 7:13]``).  Gains: a scalar or one
        value per task-space axis (kp, kd: 6) / per arm DOF (kp_null, kd_null, default_dof_pos, effort_limit: arm_dofs);
        kd defaults to 2 sqrt(kp) as the reference's; effort_limit None = no clamp.  out: where actor a's first
        out_cols torques go, out_stride floats apart (default: a new (n, arm_dofs) tensor; ``out=dof_actuation``,
        ``out_stride=nD`` writes into the actuation tensor).  jac_in (n, 6, arm_dofs) / mm_in (n, arm_dofs, arm_dofs):
        injected tensors instead of the kernel's own J and M.  Returns ``out``."""
        n, na = self.num_actors, int(arm_dofs)
        if isinstance(jac_body, str):
            jac_body = self.spec.body_index(jac_body)
        if dpose.shape != (n, 6) or not dpose.is_contiguous() or dpose.dtype != torch.float32:
            raise ValueError(f"dpose must be a contiguous float32 {(n, 6)} tensor")
        if eef_vel.shape != (n, 6) or eef_vel.dtype != torch.float32 or eef_vel.stride(1) != 1:
            raise ValueError(f"eef_vel must be a float32 {(n, 6)} tensor with contiguous rows")
        a = _abi.OscArgs()
        a.arm_dofs, a.jac_body = na, int(jac_body)
        a.dpose, a.eef_vel, a.eef_vel_stride = _abi.ptr(dpose), _abi.ptr(eef_vel), eef_vel.stride(0)
        kp = _vec(kp, 6, "kp")
        kd = [2.0 * math.sqrt(v) for v in kp] if kd is None else _vec(kd, 6, "kd")
        kpn = _vec(kp_null, na, "kp_null")
        kdn = [2.0 * math.sqrt(v) for v in kpn] if kd_null is None else _vec(kd_null, na, "kd_null")
        dflt = [0.0] * na if default_dof_pos is None else _vec(default_dof_pos, na, "default_dof_pos")
        lim = [math.inf] * na if effort_limit is None else _vec(effort_limit, na, "effort_limit")
        pad = [0.0] * (7 - na)
        a.kp, a.kd = (_abi.C.c_float * 6)(*kp), (_abi.C.c_float * 6)(*kd)
        a.kp_null, a.kd_null = (_abi.C.c_float * 7)(*(kpn + pad)), (_abi.C.c_float * 7)(*(kdn + pad))
        a.default_dof_pos = (_abi.C.c_float * 7)(*(dflt + pad))
        a.effort_limit = (_abi.C.c_float * 7)(*(lim + pad))
        if out is None:
            out = torch.zeros((n, na), device=self.device, dtype=torch.float32)
        if out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor")
        cols = na if out_cols is None else int(out_cols)
        stride = (out.numel() // n if out_stride is None else int(out_stride))
        if out.numel() < (n - 1) * stride + cols:
            raise ValueError("out is too small for out_stride / out_cols")
        a.out, a.out_stride, a.out_cols = _abi.ptr(out), stride, cols
        if (jac_in is None) != (mm_in is None):
            raise ValueError("jac_in and mm_in are given together or not at all")
        if jac_in is not None:
            if (jac_in.shape != (n, 6, na) or mm_in.shape != (n, na, na) or not jac_in.is_contiguous()
                    or not mm_in.is_contiguous() or jac_in.dtype != torch.float32 or mm_in.dtype != torch.float32):
                raise ValueError(f"jac_in / mm_in must be contiguous float32 {(n, 6, na)} / {(n, na, na)} tensors")
            a.jac_in, a.mm_in = _abi.ptr(jac_in), _abi.ptr(mm_in)
        self._keep = (dpose, eef_vel, out, jac_in, mm_in)   # alive until the launch has consumed them
        _abi.check(self._lib.mg_osc_torques(self._sim, _abi.C.byref(a), self._stream(stream)), self._lib)
        return out
