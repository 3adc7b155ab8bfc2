#!/usr/bin/env python3
"""Operational-space control torques from the reference's own method.

Run in the build container only (needs the reference checkout, MIGYM_REFERENCE, and the built oracle):

    python tests/golden/make_osc_golden.py [franka] [edges]

``FrankaReachMA._compute_osc_torques`` (isaacgymenvs/tasks/franka_reach_MA.py:770-802) is plain torch, so it is
called here unmodified, bound to a minimal stand-in ``self`` (``_get_mm``, ``_get_j_eef``, ``_q``, ``_qd``,
``states["eef_vel"]``, the gains, ``franka_default_dof_pos``, ``_franka_effort_limits``, ``num_envs``,
``num_agents``, ``device``).  The gym tensors it would read are replaced by the fp64 oracle's on the Franka fixture
(tests/golden/franka_panda.json): M from ``orc_mass_matrix`` on a copy of the model with joint damping and stiffness
zeroed (the oracle adds their implicit terms to the diagonal otherwise), column j of the hand's Jacobian from
``orc_rigid_body_states`` with qd = e_j, shifted from the body's COM to its origin (v_o = v_com - w x R body_com).

Inputs: 64 actors (32 envs x 2 agents, the two base poses of ``_get_franka_start_poses_rots(0.45)``), a fixed seed,
q = clamp(default + U(-0.4, 0.4), limits) on the arm joints (fingers 0.035), qd ~ U(-1, 1) on the arm joints,
dpose ~ U(-1, 1) * cmd_limit, eef_vel = J qd; all rounded to fp32, as the reference holds them.  No draw is rejected:
cond(J M^-1 J^T) <= 5e4 is asserted for every sample (a failure is a bug in the model table).

Outputs: the method's result as the reference runs it (``u_ref32``: fp32 tensors) and the same unmodified method with
every tensor in double on the same fp32-rounded inputs (``u_ref64``; torch promotes the method's float32 ``eye``), each
with the URDF effort limits (87 x 4, 12 x 3) and with +inf limits (``*_free``: saturation on joints 5-7 would hide
errors), and ``ref_err`` = max |u_ref32_free - u_ref64_free|.  The fixture holds data only: tests/golden/osc_franka.npz.

A second fixture, tests/golden/osc_franka_edges.npz (``python tests/golden/make_osc_golden.py edges``), runs the same
method on the same 64 actors, J and M with the arguments the first leaves at the reference's defaults: six distinct
kp, six distinct kd (none 2 sqrt(kp)), seven distinct kp_null and kd_null, +inf effort limits, and a null-space wrap
that fires.  ``franka_default_dof_pos`` is one row for all actors and q stays within 0.4 of it, so the wrap is made to
fire through q itself: every arm joint is a hinge, and q + 2 pi k (k drawn from {-1, 0, 1} per actor and joint) is
the same pose with the same J and M, while default - q lands near -2 pi, 0 or +2 pi; the default row is shifted by
EDGE_SHIFT per joint on top.  |default - q - 2 pi k'| <= 0.4 + max |EDGE_SHIFT| = 1.9 for the nearest k', so
(default - q + pi) mod 2 pi stays 1.2 away from 0 and 2 pi by construction (asserted at 1e-3; no draw is rejected) and
fp32 and fp64 wrap alike.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "isaacgymenvs-ma_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refshim  # noqa: E402

_refshim.install()
from isaacgymenvs.tasks.franka_reach_MA import FrankaReachMA  # noqa: E402

from migym import model as M  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from dynamics_ref import oracle_jacobian, oracle_mass_matrix, oracle_model  # noqa: E402

N_ENV, A = 32, 2
HAND = "panda_hand"          # the body gym's 'panda_hand_joint' Jacobian row belongs to (franka_reach_MA.py:896)
START_Z = 1.0 + 0.05 / 2 + 0.1   # franka_start_z (franka_reach_MA.py:270-276, 415)
DEFAULT_DOF_POS = [0, 0.1963, 0, -2.6180, 0, 2.9416, 0.7854, 0.035, 0.035]   # franka_reach_MA.py:206-208
CMD_LIMIT = [0.1, 0.1, 0.1, 0.5, 0.5, 0.5]                                   # franka_reach_MA.py:219


EDGE_KP = [150.0, 90.0, 210.0, 60.0, 120.0, 30.0]
EDGE_KD = [11.0, 23.0, 17.0, 5.0, 29.0, 7.0]                  # 2 sqrt(kp) would be 24.5, 19.0, 29.0, 15.5, 21.9, 11.0
EDGE_KP_NULL = [10.0, 4.0, 16.0, 7.0, 13.0, 5.5, 19.0]
EDGE_KD_NULL = [3.0, 5.5, 2.0, 7.5, 1.5, 6.0, 4.5]
EDGE_SHIFT = [0.9, -1.3, 0.4, -0.7, 1.5, -1.1, 0.2]           # added to DEFAULT_DOF_POS[:7]


def stand_in(n_env, n_agents, mm, j_eef, q, qd, eef_vel, limits, dtype, gains=None):
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=dtype)   # noqa: E731
    s = types.SimpleNamespace(num_envs=n_env, num_agents=n_agents, device="cpu")
    s._get_mm = lambda: t(mm)
    s._get_j_eef = lambda: t(j_eef)
    s._q = t(q).view(n_env, n_agents, -1)
    s._qd = t(qd).view(n_env, n_agents, -1)
    s.states = {"eef_vel": t(eef_vel).view(n_env, n_agents, 6)}
    s.kp = t([150.0] * 6)                                   # franka_reach_MA.py:212-215
    s.kd = 2 * torch.sqrt(s.kp)
    s.kp_null = t([10.0] * 7)
    s.kd_null = 2 * torch.sqrt(s.kp_null)
    s.franka_default_dof_pos = t(DEFAULT_DOF_POS)
    s._franka_effort_limits = t(limits)
    if gains is not None:
        s.kp, s.kd, s.kp_null, s.kd_null = (t(gains[k]) for k in ("kp", "kd", "kp_null", "kd_null"))
        s.franka_default_dof_pos = t(gains["default_dof_pos"])
    return s


def inputs():
    """the 64 actors both fixtures share, and the names the reference runs need"""
    spec = M.load_json(os.path.join(HERE, "franka_panda.json"))
    mnp = oracle_model(spec)
    hand, nd = spec.body_index(HAND), spec.num_dofs
    n = N_ENV * A
    rng = np.random.default_rng(20261019)
    lo = np.array([nd_.lower for nd_ in spec.nodes[1:]])
    hi = np.array([nd_.upper for nd_ in spec.nodes[1:]])
    q = np.tile(np.array(DEFAULT_DOF_POS), (n, 1))
    q[:, :7] = np.clip(q[:, :7] + rng.uniform(-0.4, 0.4, (n, 7)), lo[:7], hi[:7])
    qd = np.zeros((n, nd))
    qd[:, :7] = rng.uniform(-1, 1, (n, 7))
    dpose = rng.uniform(-1, 1, (n, 6)) * np.array(CMD_LIMIT)
    f = types.SimpleNamespace(num_agents=A)
    p, r = FrankaReachMA._get_franka_start_poses_rots(f, 0.45)
    root = np.zeros((n, 13), np.float32)
    for a in range(n):
        root[a, 0:2], root[a, 2], root[a, 3:7] = p[a % A].numpy(), START_Z, r[a % A].numpy()
    q32 = q.astype(np.float32)
    mm = np.zeros((n, 7, 7))
    j_eef = np.zeros((n, 6, 7))
    cond = np.zeros(n)
    for a in range(n):
        mm[a] = oracle_mass_matrix(mnp, root[a], q32[a])[:7, :7]
        j_eef[a] = oracle_jacobian(spec, mnp, root[a], q32[a])[hand][:, :7]
        cond[a] = np.linalg.cond(j_eef[a] @ np.linalg.solve(mm[a], j_eef[a].T))
    assert cond.max() <= 5e4, f"cond(J M^-1 J^T) = {cond.max():.3g}: a bug in the model table, not a draw to reject"
    eef_vel = np.einsum("nij,nj->ni", j_eef, qd[:, :7])
    # fp32, as the reference holds every tensor
    mm32, j32, qd32 = mm.astype(np.float32), j_eef.astype(np.float32), qd.astype(np.float32)
    dpose32, eef32 = dpose.astype(np.float32), eef_vel.astype(np.float32)
    eff = np.array([nd_.effort_limit for nd_ in spec.nodes[1:]])
    assert list(eff[:7]) == [87, 87, 87, 87, 12, 12, 12]
    out = dict(root_states=root, q=q32, qd=qd32, dpose=dpose32, eef_vel=eef32, mm=mm32, j_eef=j32,
               effort_limit=eff.astype(np.float32), default_dof_pos=np.array(DEFAULT_DOF_POS, np.float32),
               kp=np.float32(150.0), kp_null=np.float32(10.0), cond=cond, jac_body=np.int32(hand))
    return out, eff, nd


def run_reference(out, cases, gains=None):
    """u_ref32 / u_ref64 (+ tag) from the unmodified method, fp32 and fp64, per (tag, limits) case; then ref_err"""
    n = N_ENV * A
    mm32, j32, q32, qd32, eef32, dpose32 = (out[k] for k in ("mm", "j_eef", "q", "qd", "eef_vel", "dpose"))
    for tag, limits in cases:
        for name, dt in (("u_ref32", torch.float32), ("u_ref64", torch.float64)):
            s = stand_in(N_ENV, A, mm32, j32, q32, qd32, eef32, limits, dt, gains)
            u = FrankaReachMA._compute_osc_torques(s, torch.as_tensor(dpose32, dtype=dt))
            assert u.dtype == dt and u.shape == (n, 7)
            out[name + tag] = u.numpy()
    out["ref_err"] = np.float64(np.abs(out["u_ref32_free"].astype(np.float64) - out["u_ref64_free"]).max())


def main():
    out, eff, nd = inputs()
    cond = out["cond"]
    run_reference(out, (("", eff), ("_free", np.full(nd, np.inf))))
    path = os.path.join(HERE, "osc_franka.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: np.shape(v) for k, v in out.items()})
    print(f"cond max {cond.max():.3g} median {np.median(cond):.3g}; |u| max {np.abs(out['u_ref64_free']).max():.4g}; "
          f"ref_err {out['ref_err']:.3g}")


def main_edges():
    out, eff, nd = inputs()
    n = N_ENV * A
    rng = np.random.default_rng(20261020)
    k = rng.integers(-1, 2, (n, 7))
    for j in range(7):
        assert (k[:, j] == -1).any() and (k[:, j] == 1).any(), "every joint wraps in both directions somewhere"
    q = out["q"].astype(np.float64)
    q[:, :7] += 2 * np.pi * k
    out["q_base"], out["turns"] = out["q"], k.astype(np.int32)
    out["q"] = q.astype(np.float32)
    dflt = np.array(DEFAULT_DOF_POS)
    dflt[:7] += EDGE_SHIFT
    gains = dict(kp=EDGE_KP, kd=EDGE_KD, kp_null=EDGE_KP_NULL, kd_null=EDGE_KD_NULL, default_dof_pos=dflt)
    y = np.mod(dflt[:7].astype(np.float32).astype(np.float64) - out["q"][:, :7] + np.pi, 2 * np.pi)
    assert np.minimum(y, 2 * np.pi - y).min() >= 1e-3
    for key, v in gains.items():
        out[key] = np.asarray(v, np.float32)
    out["effort_limit"] = np.full(nd, np.inf, np.float32)
    run_reference(out, (("_free", np.full(nd, np.inf)),), gains)
    path = os.path.join(HERE, "osc_franka_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k_: np.shape(v) for k_, v in out.items()})
    print(f"|u| max {np.abs(out['u_ref64_free']).max():.4g}; ref_err {out['ref_err']:.3g}; "
          f"wrap margin {np.minimum(y, 2 * np.pi - y).min():.3g}")


if __name__ == "__main__":
    # "franka" rewrites tests/golden/osc_franka.npz, "edges" tests/golden/osc_franka_edges.npz
    for which in sys.argv[1:] or ["franka", "edges"]:
        {"franka": main, "edges": main_edges}[which]()
