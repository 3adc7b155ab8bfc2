"""The quadcopter model (migym.model.quadcopter_model, taskdefs.quadcopter_spec) and the Quadcopter task layer's numpy
restatement (tests/quadcopter_ref.py) on the CPU.

The reference's Quadcopter task writes its MJCF at run time and ships no asset; tests/golden/quadcopter.json is the
table migym.model.load_mjcf makes of that file (tests/golden/make_quadcopter_golden.py).  The builder makes the same
table from the named dimensions.  The file is written with six significant digits ("%g"), so positions and
quaternions agree to 1e-6 and everything computed from the dimensions alone (masses, inertias, limits) to 1e-12.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import quadcopter_ref as R
from migym import _abi, model as M, taskdefs

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quadcopter.json")


def test_builder_matches_the_reference_models_table():
    got, ref = M.quadcopter_model(), M.load_json(FIXTURE)
    assert (len(got.nodes), len(got.bodies), len(got.geoms), got.fixed_base) == (9, 9, 9, 0)
    assert [b.name for b in got.bodies] == [b.name for b in ref.bodies]            # body order: the force tensor's rows
    assert got.dof_names == ref.dof_names and [n.name for n in got.nodes] == [n.name for n in ref.nodes]
    for a, b in zip(got.nodes, ref.nodes):
        assert (a.parent, a.jtype, a.body, a.limited) == (b.parent, b.jtype, b.body, b.limited)
        np.testing.assert_allclose(a.t, b.t, atol=1e-6)
        np.testing.assert_allclose(a.r0, b.r0, atol=1e-6)
        np.testing.assert_allclose(a.axis, b.axis, atol=1e-12)
        np.testing.assert_allclose([a.mass] + list(a.com) + list(a.inertia), [b.mass] + list(b.com) + list(b.inertia),
                                   rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose([a.lower, a.upper], [b.lower, b.upper], rtol=1e-12)
        assert (a.armature, a.damping, a.stiffness, a.drive_kp, a.frictionloss) == (0.0,) * 5
    for a, b in zip(got.bodies, ref.bodies):
        assert (a.node, a.parent_body) == (b.node, b.parent_body)
        np.testing.assert_allclose(list(a.pos) + list(a.quat) + [a.mass] + list(a.com),
                                   list(b.pos) + list(b.quat) + [b.mass] + list(b.com), rtol=1e-12, atol=1e-12)
    for a, b in zip(got.geoms, ref.geoms):
        assert (a.gtype, a.node, a.body, a.filter) == (b.gtype, b.node, b.body, b.filter)
        np.testing.assert_allclose(list(a.size) + list(a.pos) + list(a.quat), list(b.size) + list(b.pos) + list(b.quat),
                                   rtol=1e-12, atol=1e-12)
    assert got.pairs == ref.pairs == [] and got.sensors == ref.sensors == []
    assert abs(got.total_mass() - 0.25154) < 1e-5
    assert all(abs(n.upper - math.radians(30)) < 1e-12 and n.lower == -n.upper for n in got.nodes[1:])


def test_task_spec_and_instance():
    """the task's copy: stiffness 1000, damping 0, no effort limit, no angular damping, rates capped at 4 pi; the model
    runs on the (16, 9, 16, 16, 0) instance, and the thrust rows are the rotors"""
    base = M.quadcopter_model()
    spec = taskdefs.quadcopter_spec(base)
    assert base.nodes[1].drive_kp == 0.0, "the spec is configured on a copy"
    for n in spec.nodes[1:]:
        assert (n.drive_kp, n.damping, n.stiffness) == (1000.0, 0.0, 0.0) and n.effort_limit > 1e30
    assert spec.angular_damping == 0.0 and abs(spec.max_angular_velocity - 4 * math.pi) < 1e-12
    assert [spec.bodies[b].name for b in taskdefs.QUADCOPTER_ROTOR_BODIES] == [f"rotor{i}" for i in range(4)]
    lanes, lib, mnp = C.c_int32(-1), _abi.lib(), M.pack_model(spec)   # mnp: alive over the call
    _abi.check(lib.mg_model_team_lanes(mnp.ctypes.data, taskdefs.QUADCOPTER_MAX_CONTACTS, C.byref(lanes)), lib)
    assert lanes.value == 16


# ------------------------------------------------------------------------------------------------ the task layer
def test_struct_sizes_and_constants():
    lib = _abi.lib()
    assert lib.mg_quadcopter_params_sizeof() == C.sizeof(_abi.QuadcopterParams)
    assert lib.mg_quadcopter_views_sizeof() == C.sizeof(_abi.QuadcopterViews) == 24
    _, _, sp, qp = R.task_model(R.golden_cfg(6))
    dt = float(np.float32(0.01))
    assert qp.dof_step == np.float32(dt * 8 * math.pi) and qp.thrust_step == np.float32(dt * 200)
    assert list(qp.rotor_body) == [2, 4, 6, 8] and qp.max_episode_length == int(R.golden()["max_episode_length"])
    assert list(qp.init_root) == [0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0] and not any(qp.init_dof)
    assert (sp.substeps, sp.max_contacts, sp.pos_iters) == (2, 16, 4) and abs(sp.dt - 0.01) < 1e-9
    from migym import configs
    env = configs.task_config("Quadcopter")["env"]            # the reference YAML's values
    assert (env["numEnvs"], env["maxEpisodeLength"], env["clipObservations"], env["clipActions"]) == (8192, 500, 5.0, 1.0)


@pytest.mark.parametrize("N", [6, 67])
def test_numpy_restatement_replays_the_trace(N):
    """pre_step and post_step of tests/quadcopter_ref.py on the reference's trace: integers and every state tensor bit
    for bit, observations and rewards within the project's 1e-4"""
    g = R.golden()
    p = R.params_from(R.task_model(R.golden_cfg(N))[3])
    st = R.trace_state0(g, N)
    worst = 0.0
    for t in range(int(g["steps"])):
        k = lambda name: g[f"N{N}_t{t}_{name}"]   # noqa: E731
        st["reset"], st["progress"] = k("reset_in").copy(), k("progress_in").copy()
        R.pre_step(p, st, k("actions"), k("noise"))
        for name in R.STATE_KEYS:
            np.testing.assert_array_equal(st[name], k("pre_" + name), err_msg=f"step {t}: {name} after pre")
        np.testing.assert_array_equal(st["reset"], k("pre_reset_buf"))
        np.testing.assert_array_equal(st["progress"], k("pre_progress_buf"))
        st["root_states"], st["dof_states"] = k("sim_root_states").copy(), k("sim_dof_states").copy()
        obs, clamped, timeout = R.post_step(p, st)
        np.testing.assert_array_equal(st["reset"], k("reset"))
        np.testing.assert_array_equal(st["progress"], k("progress"))
        np.testing.assert_array_equal(timeout, k("timeout"))
        for got, ref in ((obs, k("obs")), (clamped, k("obs_clamped")), (st["rew"], k("rew"))):
            assert R.close(got, ref).all()
            worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max()))
    print(f"N={N}: largest float difference from the trace {worst:.3g}")
