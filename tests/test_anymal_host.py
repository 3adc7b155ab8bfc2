"""CPU tests of the Anymal task layer (no GPU): the URDF loader options, the model fixture and the kernel instance it
selects, the numpy restatement (tests/anymal_ref.py) against the reference's own output
(tests/golden/trace_anymal.npz), the host-side constants, the ABI additions, the constructor's error paths, and the
fp64 oracle's rollout of the task model from the reset distribution."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import anymal_ref as R
from migym import _abi, configs, model as M, taskdefs

SIZES = [6, 67]

SMALL_URDF = """<?xml version="1.0"?>
<robot name="small">
  <link name="trunk">
    <inertial><origin xyz="0 0 0.1"/><mass value="2.0"/><inertia ixx="0.1" iyy="0.1" izz="0.1"/></inertial>
    <collision><geometry><box size="0.4 0.2 0.1"/></geometry></collision>
  </link>
  <link name="lid">
    <inertial><origin xyz="0.1 0 0"/><mass value="1.0"/><inertia ixx="0.01" iyy="0.01" izz="0.01"/></inertial>
    <collision><origin xyz="0 0.05 0" rpy="1.5707963267948966 0 0"/><geometry><cylinder radius="0.03" length="0.2"/></geometry></collision>
  </link>
  <link name="knob">
    <inertial><origin xyz="0 0 0.02"/><mass value="0.5"/><inertia ixx="0.001" iyy="0.001" izz="0.001"/></inertial>
    <collision><geometry><sphere radius="0.02"/></geometry></collision>
  </link>
  <link name="arm">
    <inertial><origin xyz="0 0 -0.1"/><mass value="0.7"/><inertia ixx="0.01" iyy="0.01" izz="0.01"/></inertial>
    <collision><origin xyz="0 0 -0.1"/><geometry><cylinder radius="0.02" length="0.16"/></geometry></collision>
  </link>
  <link name="hand">
    <inertial><origin xyz="0.01 0 0"/><mass value="0.3"/><inertia ixx="0.001" iyy="0.001" izz="0.001"/></inertial>
    <collision><geometry><box size="0.04 0.04 0.04"/></geometry></collision>
  </link>
  <joint name="trunk_lid" type="fixed"><parent link="trunk"/><child link="lid"/>
    <origin xyz="0 0 0.2" rpy="0 0 1.5707963267948966"/></joint>
  <joint name="lid_knob" type="fixed"><parent link="lid"/><child link="knob"/><origin xyz="0.3 0 0"/></joint>
  <joint name="shoulder" type="revolute"><parent link="knob"/><child link="arm"/><origin xyz="0 0 0.05"/>
    <axis xyz="0 1 0"/><limit lower="-1" upper="2" effort="33" velocity="5"/></joint>
  <joint name="arm_hand" type="fixed"><parent link="arm"/><child link="hand"/><origin xyz="0 0 -0.2"/></joint>
</robot>
"""


@pytest.fixture(scope="module")
def small_urdf(tmp_path_factory):
    p = tmp_path_factory.mktemp("urdf") / "small.urdf"
    p.write_text(SMALL_URDF)
    return str(p)


# ------------------------------------------------------------------------------------------------ the loader
def test_loader_defaults_are_unchanged(small_urdf):
    s = M.load_urdf(small_urdf, "small", fix_base=False)
    assert [b.name for b in s.bodies] == ["trunk", "lid", "knob", "arm", "hand"]
    assert [g.gtype for g in s.geoms] == [M.GT_BOX, M.GT_CYLINDER, M.GT_SPHERE, M.GT_CYLINDER, M.GT_BOX]
    assert [g.body for g in s.geoms] == [0, 1, 2, 3, 4] and [n.effort_limit for n in s.nodes] == [0.0, 0.0]
    assert [b.mass for b in s.bodies] == [2.0, 1.0, 0.5, 0.7, 0.3]
    assert s == M.load_urdf(small_urdf, "small", fix_base=False, collapse_fixed=False,
                            replace_cylinder_with_capsule=False, effort_limits=False)


def test_loader_collapse_cylinder_effort(small_urdf):
    base = M.load_urdf(small_urdf, "small", fix_base=False)
    s = M.load_urdf(small_urdf, "small", fix_base=False, collapse_fixed=True, replace_cylinder_with_capsule=True,
                    effort_limits=True)
    # body rows: one per node, depth-first URDF order
    assert [b.name for b in s.bodies] == ["trunk", "arm"] and [b.node for b in s.bodies] == [0, 1]
    assert [b.parent_body for b in s.bodies] == [-1, 0]
    assert [g.body for g in s.geoms] == [0, 0, 0, 1, 1] and [g.node for g in s.geoms] == [0, 0, 0, 1, 1]
    # cylinders become capsules of the same radius, axis and segment half-length L / 2
    assert [g.gtype for g in s.geoms] == [M.GT_BOX, M.GT_CAPSULE, M.GT_SPHERE, M.GT_CAPSULE, M.GT_BOX]
    assert s.geoms[1].size[:2] == [0.03, 0.1] and s.geoms[3].size[:2] == [0.02, 0.08]
    # the node tables and the geoms' node-frame poses do not depend on the collapse
    assert s.nodes[1].effort_limit == 33.0 and s.nodes[0].effort_limit == 0.0
    for a, b in zip(s.nodes, base.nodes):
        b = copy.deepcopy(b)
        b.effort_limit, b.body = a.effort_limit, a.body
        assert a == b
    for a, b in zip(s.geoms, base.geoms):
        assert a.pos == b.pos and a.quat == b.quat and a.size == b.size
    # composed poses: lid = Rz(90 deg) at (0, 0, 0.2); its cylinder at lid (0, 0.05, 0) -> trunk (-0.05, 0, 0.2), its
    # axis (lid -y after the roll) -> trunk +x; knob at lid (0.3, 0, 0) -> trunk (0, 0.3, 0.2)
    assert np.allclose(s.geoms[1].pos, [-0.05, 0.0, 0.2], atol=1e-12)
    assert np.allclose(np.abs(M.qrot(np.array(s.geoms[1].quat), [0, 0, 1])), [1, 0, 0], atol=1e-12)
    assert np.allclose(s.geoms[2].pos, [0.0, 0.3, 0.2], atol=1e-12)
    assert np.allclose(s.geoms[4].pos, [0.0, 0.0, -0.2], atol=1e-12)
    # accumulated mass and COM, body frame: trunk 2 kg at (0, 0, 0.1), lid 1 kg at lid (0.1, 0, 0) -> (0, 0.1, 0.2),
    # knob 0.5 kg at knob (0, 0, 0.02) -> (0, 0.3, 0.22)
    assert s.bodies[0].mass == pytest.approx(3.5) and s.bodies[1].mass == pytest.approx(1.0)
    com0 = (2.0 * np.array([0, 0, 0.1]) + 1.0 * np.array([0, 0.1, 0.2]) + 0.5 * np.array([0, 0.3, 0.22])) / 3.5
    assert np.allclose(s.bodies[0].com, com0, atol=1e-12)
    com1 = (0.7 * np.array([0, 0, -0.1]) + 0.3 * np.array([0.01, 0, -0.2])) / 1.0
    assert np.allclose(s.bodies[1].com, com1, atol=1e-12)
    assert np.allclose(s.bodies[0].com, s.nodes[0].com, atol=1e-12) and s.total_mass() == pytest.approx(4.5)
    # each option alone
    only = M.load_urdf(small_urdf, "small", fix_base=False, replace_cylinder_with_capsule=True)
    assert len(only.bodies) == 5 and only.geoms[1].gtype == M.GT_CAPSULE and only.nodes[1].effort_limit == 0.0
    only = M.load_urdf(small_urdf, "small", fix_base=False, effort_limits=True)
    assert len(only.bodies) == 5 and only.geoms[1].gtype == M.GT_CYLINDER and only.nodes[1].effort_limit == 33.0


# ------------------------------------------------------------------------------------------------ the fixture
def test_fixture_model():
    s = M.load_json(R.ANYMAL_JSON)
    legs = ("LF", "RF", "LH", "RH")
    assert (len(s.nodes), len(s.bodies), s.num_dofs, s.fixed_base) == (13, 13, 12, 0)
    assert [b.name for b in s.bodies] == ["base"] + [f"{leg}_{p}" for leg in legs for p in ("HIP", "THIGH", "SHANK")]
    assert s.dof_names == [f"{leg}_{j}" for leg in legs for j in ("HAA", "HFE", "KFE")]
    assert sum("THIGH" in b.name for b in s.bodies) == 4 and len(s.geoms) == 37
    assert all(g.gtype in (M.GT_SPHERE, M.GT_CAPSULE, M.GT_BOX) for g in s.geoms)
    assert [n.effort_limit for n in s.nodes[1:]] == [80.0] * 12 and s.angular_damping == 0.0
    assert s.total_mass() == pytest.approx(52.13, abs=0.01)
    assert os.path.getsize(R.ANYMAL_JSON) < 1 << 20
    cfg = R.task_cfg(4)
    spec, mnp, sp, ap = R.task_model(cfg)
    assert int(mnp["num_nodes"]) == 13 and int(mnp["nv"]) == 18 and sp.max_contacts == 48
    assert list(mnp["drive_kp"][1:13]) == [85.0] * 12 and list(mnp["damping"][1:13]) == [2.0] * 12
    assert list(mnp["effort_limit"][1:13]) == [80.0] * 12 and float(mnp["link_ang_damping"]) == 0.0
    assert R.dispatch_team_size(spec, sp.max_contacts) == 32
    assert R.dispatch_team_size(M.load_builtin("ant"), 16) == 16
    assert R.dispatch_team_size(M.load_builtin("humanoid"), 32) == 32


REF_URDF = os.path.join(os.environ.get("MIGYM_REFERENCE", "/root/reference"), "assets/urdf/anymal_c/urdf/anymal.urdf")


@pytest.mark.skipif(not os.path.isfile(REF_URDF), reason="the reference's assets/ tree is only in the build container")
def test_fixture_equals_the_builder_output():
    urdf = REF_URDF
    s = M.load_urdf(urdf, "anymal_c", fix_base=False, collapse_fixed=True, replace_cylinder_with_capsule=True,
                    effort_limits=True)
    s.angular_damping = 0.0
    assert s == M.load_json(R.ANYMAL_JSON)
    full = M.load_urdf(urdf, "anymal_c", fix_base=False)
    assert len(full.bodies) == 78 and len(full.nodes) == 13 and len(full.geoms) == 37


# ------------------------------------------------------------------------------------------------ the restatement
def test_golden_covers_the_sizes():
    g = R.golden()
    assert list(g["sizes"]) == SIZES and int(g["steps"]) == 6 and os.path.getsize(R.GOLDEN) < 1 << 20


def test_params_match_the_reference_constants():
    g = R.golden()
    _, _, _, ap = R.task_model(R.golden_cfg(6))
    assert ap.max_episode_length == int(g["max_episode_length"]) == 12
    assert np.array_equal(np.array([ap.rew_lin_vel_xy, ap.rew_ang_vel_z, ap.rew_torque], np.float32), g["rew_scales"])
    assert np.array_equal(np.array(list(ap.default_dof_pos), np.float32), g["default_dof_pos"])
    assert np.array_equal(np.array(list(ap.base_init_state), np.float32), g["base_init_state"])
    assert list(ap.command_lo) == [-2.0, -1.0, -1.0] and list(ap.command_span) == [4.0, 2.0, 2.0]
    assert (ap.base_body, list(ap.knee_body), ap.num_bodies) == (0, [2, 5, 8, 11], 13)
    _, _, _, ap = R.task_model(R.task_cfg(6))
    assert ap.max_episode_length == 2500   # int(50 / float32(0.02) + 0.5)


@pytest.mark.parametrize("N", SIZES)
def test_restatement_reproduces_the_reference(N):
    g = R.golden()
    p = R.params_from(R.task_model(R.golden_cfg(N))[3])
    st = R.golden_state0(g, N)
    seen = dict(base=False, knee=False, timeout=False, none=False, reset=False, kept=False, clipped=False)
    worst_obs = worst_rew = 0.0
    for t in range(int(g["steps"])):
        pre = f"N{N}_s{t}_"
        st["reset"][:], st["progress"][:] = g[pre + "reset_in"], g[pre + "progress_in"]
        st["root"][:], st["dof"][:] = g[pre + "root_in"], g[pre + "dof_in"]
        a_out, tgt = R.pre_step(p, g[pre + "actions"])
        assert np.array_equal(tgt.reshape(-1), g[pre + "targets"].reshape(-1)), f"step {t}: targets"
        seen["clipped"] |= bool((np.abs(g[pre + "actions"]) > 1).any())
        out = R.post_step(p, st, g[pre + "torques"], g[pre + "ncf"], g[pre + "actions"], g[pre + "noise"])
        assert np.array_equal(st["reset"], g[pre + "reset"]) and np.array_equal(st["progress"], g[pre + "progress"])
        for k in R.STATE_KEYS:
            assert np.array_equal(st[k], g[pre + k]), f"step {t}: {k}"
        assert np.array_equal(out["obs"][:, 36:48], a_out)
        worst_obs = max(worst_obs, np.abs(out["obs"].astype(np.float64) - g[pre + "obs"]).max())
        worst_rew = max(worst_rew, np.abs(out["rew"].astype(np.float64) - g[pre + "rew"]).max())
        assert R.close(out["obs"], g[pre + "obs"]).all(), f"step {t}: obs"
        assert R.close(out["rew"], g[pre + "rew"]).all(), f"step {t}: reward"
        nrm = np.linalg.norm(g[pre + "ncf"].astype(np.float64), axis=-1)
        assert (np.abs(nrm[:, [0, 2, 5, 8, 11]] - 1) > 1e-3).all()
        fb, fk = nrm[:, 0] > 1, (nrm[:, [2, 5, 8, 11]] > 1).any(1)
        ft = g[pre + "progress"] >= p["max_episode_length"] - 1
        seen["base"] |= bool(fb.any())
        seen["knee"] |= bool(fk.any())
        seen["timeout"] |= bool(ft.any())
        seen["none"] |= bool((~fb & ~fk & ~ft).any())
        seen["reset"] |= bool((g[pre + "reset_in"] != 0).any())
        seen["kept"] |= bool((g[pre + "reset_in"] == 0).any())
        assert (np.abs(g[pre + "torques"]).max() == 80.0) and (g[pre + "rew"] > 0).any() and (g[pre + "rew"] == 0).any()
    print(f"N={N}: max |obs - ref| = {worst_obs:.3g}, max |rew - ref| = {worst_rew:.3g}")
    assert all(seen.values()), seen


# ------------------------------------------------------------------------------------------------ ABI, errors
def test_abi_exports_and_struct_sizes():
    for sym in ("mg_anymal_pre", "mg_anymal_post", "mg_anymal_reset_idx", "mg_anymal_params_sizeof",
                "mg_anymal_views_sizeof"):
        assert sym in _abi.EXPORTS, sym
    assert C.sizeof(_abi.AnymalViews) == 2 * C.sizeof(C.c_void_p)
    assert C.sizeof(_abi.AnymalParams) == 4 * (8 + 12 + 13 + 6 + 1 + 4 + 1 + 2 + 1)
    if os.path.exists(_abi.LIB_PATH):
        lib = _abi.lib()
        assert lib.mg_anymal_params_sizeof() == C.sizeof(_abi.AnymalParams)
        assert lib.mg_anymal_views_sizeof() == C.sizeof(_abi.AnymalViews)
        assert lib.mg_version() == 7


def _construct(cfg):
    """the constructor up to the point where it needs a device"""
    from migym.tasks import Anymal
    return Anymal(cfg=cfg, rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=-1, headless=True)


def test_error_paths(small_urdf):
    import migym
    from migym.tasks import isaacgym_task_map
    assert "Anymal" in isaacgym_task_map and "Anymal" in configs.TASKS
    cfg = R.task_cfg(4)
    cfg["task"]["randomize"] = True
    with pytest.raises(NotImplementedError, match="randomize"):
        _construct(cfg)
    cfg = R.task_cfg(4)
    cfg["env"]["asset"] = {"modelTable": "/nonexistent/anymal.json"}
    with pytest.raises(FileNotFoundError, match=r"tools/build_models\.py anymal_c"):
        _construct(cfg)
    cfg = R.task_cfg(4)   # a missing table is an error even where a URDF could be loaded instead
    cfg["env"]["asset"] = {"modelTable": "/nonexistent/anymal.json", "assetRoot": os.path.dirname(small_urdf),
                           "assetFileName": os.path.basename(small_urdf)}
    with pytest.raises(FileNotFoundError, match=r"/nonexistent/anymal\.json"):
        _construct(cfg)
    cfg = R.task_cfg(4)
    cfg["sim"]["use_gpu_pipeline"] = False
    with pytest.raises(NotImplementedError, match="host pipeline"):
        migym.make(seed=0, task="Anymal", num_envs=4, sim_device="cuda:0", rl_device="cuda:0", headless=True,
                   cfg={"task": cfg})
    bad = M.load_builtin("ant")
    with pytest.raises(ValueError, match="12-DOF"):
        taskdefs.anymal_spec(bad, R.task_cfg(4))


# ------------------------------------------------------------------------------------------------ the oracle alone
def test_oracle_rollout_from_the_reset_distribution():
    """64 envs from injected reset draws, 50 zero-action steps (targets = the default joint angles) under the fp64
    oracle: everything finite, no base or thigh net contact force above 1, at most 48 contact candidates at every
    step -- the discrete facts tests/test_gpu_anymal.py asserts of the GPU rollout; the robots end standing"""
    cfg = R.task_cfg(64)
    spec, mnp, sp, ap = R.task_model(cfg)
    p = R.params_from(ap)
    root, dof, _ = R.reset_state(p, 64, 11)
    h = R.AnymalHost(spec, root, dof, np.tile(p["default"], (64, 1)))
    most = 0
    for t in range(50):
        most = max(most, R.num_candidates(mnp, sp, h.root, h.dof).max())
        h.simulate(mnp, sp)
        for x in (h.root, h.dof, h.dof_force, h.ncf):
            assert np.isfinite(x).all(), f"step {t}"
        nrm = np.linalg.norm(h.ncf[:, [p["base"]] + p["knees"]], axis=-1)
        assert nrm.max() <= 1.0, f"step {t}: a base or thigh force of {nrm.max():.3g}"
    most = max(most, R.num_candidates(mnp, sp, h.root, h.dof).max())
    print(f"most contact candidates {most}, final base z {h.root[:, 2].min():.3f}..{h.root[:, 2].max():.3f}")
    assert most <= 48
    assert (h.root[:, 2] > 0.4).all() and (h.root[:, 2] < 0.62).all() and np.abs(h.dof_force).max() <= 80.0 + 1e-3
