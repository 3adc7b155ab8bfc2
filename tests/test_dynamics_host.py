"""Host-side checks of the dynamics-tensor feature (no GPU): the hull mass integration behind the Franka fixture, the
fixture table itself, the OSC golden's internal consistency, and the new C-ABI exports."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from migym import _abi, model as M

import dynamics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def franka():
    return M.load_json(R.FRANKA_JSON)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(R.OSC_NPZ))


def _box(dx, dy, dz):
    return np.array([[x, y, z] for x in (-dx / 2, dx / 2) for y in (-dy / 2, dy / 2) for z in (-dz / 2, dz / 2)])


def test_hull_mass_properties_box_kat():
    from build_models import hull_mass_properties
    rho, (a, b, c) = 1000.0, (0.2, 0.4, 0.6)
    m, com, I = hull_mass_properties(_box(a, b, c), rho)
    m0 = rho * a * b * c
    I0 = np.diag([m0 * (b * b + c * c) / 12, m0 * (a * a + c * c) / 12, m0 * (a * a + b * b) / 12])
    assert abs(m - m0) <= 1e-9 * m0
    assert np.abs(com).max() <= 1e-9 * max(a, b, c)
    assert np.abs(I - I0).max() <= 1e-9 * I0.max()
    # the same box rotated and shifted: the COM moves with it, the inertia about the COM rotates (R I R^T), and
    # the inertia about the origin obeys the parallel-axis theorem
    Rm = M.qmat(M.quat_from_rpy(0.3, -0.7, 1.1))
    t = np.array([0.5, -0.25, 0.125])
    m2, com2, I2 = hull_mass_properties(_box(a, b, c) @ Rm.T + t, rho)
    assert abs(m2 - m0) <= 1e-9 * m0
    assert np.abs(com2 - t).max() <= 1e-9
    assert np.abs(I2 - Rm @ I0 @ Rm.T).max() <= 1e-9 * I0.max()
    # about the origin: the returned (mass, COM, inertia) compose to the analytic box's by the parallel-axis theorem
    Io = I2 + m2 * (np.dot(com2, com2) * np.eye(3) - np.outer(com2, com2))
    Io_ref = Rm @ I0 @ Rm.T + m0 * (np.dot(t, t) * np.eye(3) - np.outer(t, t))
    assert np.abs(Io - Io_ref).max() <= 1e-9 * Io_ref.max()


def test_franka_fixture_table(franka):
    assert franka.num_dofs == 9 and len(franka.nodes) == 10 and len(franka.bodies) == 16
    assert franka.dof_names == [f"panda_joint{i}" for i in range(1, 8)] + ["panda_finger_joint1", "panda_finger_joint2"]
    assert franka.body_index("panda_hand") == 8 and franka.body_index("panda_grip_site") == 15
    assert franka.fixed_base == 1 and franka.gravity_off == 1
    assert all(n.mass > 0 for n in franka.nodes[1:])
    assert 15.0 < franka.total_mass() < 25.0
    assert all(g.gtype != M.GT_CONVEX for g in franka.geoms)
    q = np.array([0, 0.1963, 0, -2.6180, 0, 2.9416, 0.7854, 0.035, 0.035])   # franka_reach_MA.py:206-208
    root = np.array([0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.float32)
    Mq = R.oracle_mass_matrix(R.oracle_model(franka), root, q)[:7, :7]
    assert np.abs(Mq - Mq.T).max() <= 1e-12 * np.abs(Mq).max()
    assert np.linalg.eigvalsh(Mq).min() > 0


def test_osc_golden_is_consistent(golden):
    g = golden
    for k in ("u_ref32", "u_ref64", "u_ref32_free", "u_ref64_free"):
        assert g[k].shape == (64, 7) and np.isfinite(g[k]).all(), k
    assert g["u_ref32"].dtype == np.float32 and g["u_ref64"].dtype == np.float64
    lim = g["effort_limit"][:7]
    assert list(lim) == [87, 87, 87, 87, 12, 12, 12]
    for k in ("u_ref32", "u_ref64"):
        assert np.array_equal(g[k], np.clip(g[k + "_free"], -lim.astype(g[k].dtype), lim.astype(g[k].dtype))), k
    # the unclamped set does saturate somewhere (else the clamped variant would check nothing)
    assert (np.abs(g["u_ref64_free"]) > lim).any()
    err = np.abs(g["u_ref32_free"].astype(np.float64) - g["u_ref64_free"]).max()
    assert float(g["ref_err"]) == err and 0 < err < 1e-2
    assert g["cond"].max() <= 5e4


def test_dynamics_entry_points_are_exported():
    lib = C.CDLL(_abi.LIB_PATH)
    for name in ("mg_dynamics_bind", "mg_dynamics_refresh", "mg_osc_torques"):
        assert hasattr(lib, name), name
    l = _abi.lib()
    assert l.mg_osc_args_sizeof() == C.sizeof(_abi.OscArgs)
    # argument checks that need no device: a null sim
    assert l.mg_dynamics_refresh(None, None) == -1 and b"mg_dynamics_refresh" in l.mg_last_error()
    assert l.mg_osc_torques(None, None, None) == -1 and b"mg_osc_torques" in l.mg_last_error()
