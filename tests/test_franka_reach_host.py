"""CPU tests of the FrankaReachMA task layer (no GPU): the numpy restatement (tests/franka_reach_ref.py) against the
reference's own output (tests/golden/trace_franka_reach_ma.npz), the host-side constants, the model spec the task
builds, the ABI additions, the base poses and the constructor's error paths."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import franka_reach_ref as R
from migym import _abi, configs, model as M, taskdefs

CONFIGS = [(2, 2, 16), (3, 3, 8), (4, 2, 8), (1, 1, 8)]


def test_golden_covers_the_configurations():
    g = R.golden()
    assert [tuple(c) for c in g["configs"]] == CONFIGS and int(g["steps"]) == 6
    assert os.path.getsize(R.GOLDEN) < 1 << 20


@pytest.mark.parametrize("A,T,N", CONFIGS)
def test_restatement_reproduces_the_reference(A, T, N):
    g = R.golden()
    p = R.params_from(taskdefs.reach_params(R.golden_cfg(A, T, N), M.load_json(R.FRANKA_JSON)))
    st = R.golden_state0(g, A, T, N)
    saw_full = saw_part = saw_punish = saw_limit = False
    for t in range(int(g["steps"])):
        pre = f"A{A}T{T}_s{t}_"
        st["reset"][:], st["progress"][:] = g[pre + "reset_in"], g[pre + "progress_in"]
        st["q"][:], st["qd"][:] = g[pre + "q_in"], g[pre + "qd_in"]
        per_env = g[pre + "reset_in"].reshape(N, A).sum(1)
        saw_full |= bool((per_env == A).any())
        saw_part |= bool(((per_env > 0) & (per_env < A)).any())
        out = R.post_step(p, st, g[pre + "eef"], g[pre + "hand_force"], g[pre + "actions"], g[pre + "noise"])
        assert np.array_equal(out["obs"], g[pre + "obs"]), f"step {t}: obs"
        assert np.array_equal(st["reset"], g[pre + "reset"]) and np.array_equal(st["progress"], g[pre + "progress"])
        for k in R.STATE_KEYS:
            assert np.array_equal(st[k], g[pre + k]), f"step {t}: {k}"
        assert R.reward_close(out["rew"], g[pre + "rew"]).all(), f"step {t}: reward"
        saw_punish |= bool((np.linalg.norm(g[pre + "hand_force"], axis=-1) >= 0.1).any())
        saw_limit |= bool((g[pre + "progress"] >= int(g["max_episode_length"]) - 1).any())
        if A > 1:   # a partly done env is left alone, flags included
            e = 1
            assert g[pre + "reset_in"][e * A:(e + 1) * A].sum() == A - 1
            assert np.array_equal(g[pre + "reset"][e * A:(e + 1) * A][:A - 1], np.ones(A - 1, np.int64))
    assert saw_full and saw_punish and saw_limit and (saw_part or A == 1)


@pytest.mark.parametrize("A,T,N", CONFIGS)
def test_reach_params_match_the_reference_constants(A, T, N):
    g = R.golden()
    spec = M.load_json(R.FRANKA_JSON)
    rp = taskdefs.reach_params(R.golden_cfg(A, T, N), spec)
    tag = f"A{A}T{T}_"
    f32 = lambda x: np.float32(x)   # noqa: E731
    assert f32(rp.dof_noise_scale) == g[tag + "dof_noise_scale"]
    assert f32(rp.cube_xy_scale) == g[tag + "cube_xy_scale"]
    assert f32(rp.cube_z_base) == g[tag + "cube_z_base"] and f32(rp.cube_z_range) == f32(0.5)
    assert (rp.num_agents, rp.num_targets, rp.num_obs) == (A, T, 10 + 3 * T + 3 * (A - 1))
    assert rp.max_episode_length == int(g["max_episode_length"])
    assert np.array_equal(np.array(list(rp.default_dof_pos), np.float32), g["default_dof_pos"])
    assert np.array_equal(np.array(list(rp.dof_lower), np.float32), g["dof_lower"])
    assert np.array_equal(np.array(list(rp.dof_upper), np.float32), g["dof_upper"])
    assert list(rp.effort_limit) == [87, 87, 87, 87, 12, 12, 12]
    assert list(rp.kp) == [150.0] * 6 and list(rp.kp_null) == [10.0] * 7
    assert np.array_equal(np.array(list(rp.kd), np.float32), 2 * np.sqrt(np.full(6, 150, np.float32)))
    assert np.array_equal(np.array(list(rp.kd_null), np.float32), 2 * np.sqrt(np.full(7, 10, np.float32)))
    assert np.array_equal(np.array(list(rp.cmd_limit), np.float32), np.array([.1, .1, .1, .5, .5, .5], np.float32))
    assert spec.bodies[rp.jac_body].name == "panda_hand" == spec.bodies[rp.hand_body].name
    assert spec.bodies[rp.eef_body].name == "panda_grip_site"
    assert (rp.num_bodies, rp.num_dofs) == (16, 9)


def test_task_spec_drives_and_roundtrip():
    base = M.load_json(R.FRANKA_JSON)
    keep = copy.deepcopy(base)
    spec = taskdefs.reach_spec(base)
    assert base == keep, "the loaded table is not modified"
    assert spec.gravity_off == 1 and spec.fixed_base == 1
    assert (len(spec.nodes), spec.num_dofs, len(spec.geoms)) == (10, 9, 2)
    for j, n in enumerate(spec.nodes[1:]):
        assert n.stiffness == 0.0
        if j < 7:
            assert (n.damping, n.drive_kp) == (0.0, 0.0)
        else:
            assert (n.damping, n.drive_kp, n.effort_limit) == (100.0, 5000.0, 200.0)
    m = M.pack_model(spec)
    assert int(m["num_nodes"]) == 10 and int(m["gravity_off"]) == 1 and int(m["fixed_base"]) == 1
    assert list(m["drive_kp"][:10]) == [0] * 8 + [5000, 5000]
    assert list(m["damping"][:10]) == [0] * 8 + [100, 100]
    assert list(m["effort_limit"][8:10]) == [200, 200] and list(m["effort_limit"][1:8]) == [87] * 4 + [12] * 3
    assert np.allclose(m["lower"][1:10], R.golden()["dof_lower"]) and np.allclose(m["upper"][1:10],
                                                                                    R.golden()["dof_upper"])


def test_abi_exports_and_struct_sizes():
    for sym in ("mg_reach_pre", "mg_reach_post", "mg_reach_reset_idx", "mg_reach_params_sizeof",
                "mg_reach_views_sizeof"):
        assert sym in _abi.EXPORTS, sym
    assert C.sizeof(_abi.ReachViews) == 4 * C.sizeof(C.c_void_p)
    if os.path.exists(_abi.LIB_PATH):
        lib = _abi.lib()
        assert lib.mg_reach_params_sizeof() == C.sizeof(_abi.ReachParams)
        assert lib.mg_reach_views_sizeof() == C.sizeof(_abi.ReachViews)
        assert lib.mg_version() == 7


def test_circle_base_poses():
    g = R.golden()
    for A, T, _ in CONFIGS:
        pos, rot = taskdefs.franka_start_poses(A)
        assert np.array_equal(pos.numpy(), g[f"A{A}T{T}_base_pos"]) and np.array_equal(rot.numpy(),
                                                                                      g[f"A{A}T{T}_base_rot"])
    # the OSC golden's root rows are the A = 2 poses at the reference's start height
    osc = np.load(os.path.join(R.HERE, "golden", "osc_franka.npz"))["root_states"]
    pos, rot = taskdefs.franka_start_poses(2)
    z = np.float32(taskdefs.TASK_INFO["FrankaReachMA"][4])
    for k in range(2):
        assert np.array_equal(osc[k, 0:2], pos[k].numpy()) and osc[k, 2] == z
        assert np.array_equal(osc[k, 3:7], rot[k].numpy())
    for A in (7, 8):   # 360 // 7 = 51 gives eight angles: the first A are used
        assert taskdefs.franka_start_poses(A)[0].shape == (A, 2)


def _construct(cfg):
    """the constructor up to the point where it needs a device"""
    from migym.tasks import FrankaReachMA
    return FrankaReachMA(cfg=cfg, rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=-1, headless=True)


def test_error_paths():
    from migym.tasks import isaacgym_task_map
    assert "FrankaReachMA" in isaacgym_task_map and "FrankaReachMA" in configs.TASKS
    with pytest.raises(ValueError, match="joint_tor"):
        _construct(R.golden_cfg(2, 2, 4, controlType="joint_tor"))
    with pytest.raises(ValueError, match="numTargets"):
        _construct(R.golden_cfg(2, 3, 4))
    with pytest.raises(ValueError, match="numAgents"):
        _construct(R.golden_cfg(9, 1, 4))
    with pytest.raises(NotImplementedError):
        _construct(R.golden_cfg(2, 2, 4, frankaRotationNoise=0.1))
    cfg = R.golden_cfg(2, 2, 4)
    cfg["task"]["randomize"] = True
    with pytest.raises(NotImplementedError, match="randomize"):
        _construct(cfg)
    cfg = configs.task_config("FrankaReachMA", 4)   # the built-in config: no asset ships
    with pytest.raises(FileNotFoundError, match=r"tools/build_models\.py franka_panda"):
        _construct(cfg)
    cfg = R.golden_cfg(2, 2, 4)
    cfg["env"]["asset"] = {"modelTable": "/nonexistent/franka.json"}
    with pytest.raises(FileNotFoundError, match=r"tools/build_models\.py franka_panda"):
        _construct(cfg)


def test_host_pipeline_is_refused():
    import migym
    cfg = R.golden_cfg(2, 2, 4)
    cfg["sim"]["use_gpu_pipeline"] = False
    with pytest.raises(NotImplementedError, match="host pipeline"):
        migym.make(seed=0, task="FrankaReachMA", num_envs=4, sim_device="cuda:0", rl_device="cuda:0",
                   headless=True, cfg={"task": cfg})
