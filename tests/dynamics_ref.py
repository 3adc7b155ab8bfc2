"""fp64-oracle references of the dynamics tensors (shared by tests/test_gpu_dynamics.py, tests/test_dynamics_host.py
and tests/golden/make_osc_golden.py): the mass matrix and the body-origin Jacobian of a fixed-base model table."""
import copy
import os

import numpy as np

import pyoracle as O
from migym import _abi, model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRANKA_JSON = os.path.join(GOLDEN, "franka_panda.json")
OSC_NPZ = os.path.join(GOLDEN, "osc_franka.npz")


def oracle_model(spec):
    """the packed model with joint damping and stiffness zeroed: orc_mass_matrix adds their implicit terms
    (h b + h^2 k) to the diagonal, which the mass-matrix tensor does not carry"""
    s = copy.deepcopy(spec)
    for nd in s.nodes:
        nd.damping, nd.stiffness = 0.0, 0.0
    return M.pack_model(s)


def oracle_sim_params():
    sp = _abi.SimParams()
    sp.dt, sp.substeps = 1.0 / 60.0, 2
    return sp


def oracle_mass_matrix(mnp, root13, q):
    q = np.asarray(q, np.float32)
    dof = np.stack([q, np.zeros_like(q)], 1)
    return O.mass_matrix(mnp, oracle_sim_params(), np.asarray(root13, np.float32), dof)


def oracle_jacobian(spec, mnp, root13, q):
    """(nB, 6, nD) Jacobian of every body ORIGIN, [linear; angular], world frame: column j is the body's velocity
    under qd = e_j (orc_rigid_body_states reports the COM's: v_o = v_com - w x R body_com)"""
    nd, nb = spec.num_dofs, len(spec.bodies)
    J = np.zeros((nb, 6, nd))
    root13 = np.asarray(root13, np.float32)
    for j in range(nd):
        dof = np.zeros((nd, 2), np.float32)
        dof[:, 0] = q
        dof[j, 1] = 1.0
        rb = O.rigid_body_states(mnp, root13, dof, nb).astype(np.float64)
        for b in range(nb):
            w = rb[b, 10:13]
            J[b, 0:3, j] = rb[b, 7:10] - np.cross(w, M.qmat(rb[b, 3:7]) @ np.asarray(spec.bodies[b].com))
            J[b, 3:6, j] = w
    return J
