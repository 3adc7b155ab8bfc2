"""CPU tests of HumanoidAMP: the numpy restatement (tests/amp_ref.py) against every recorded trace of
the reference's own methods, migym.motion against MotionLib's tensors, taskdefs.amp_params against the reference's
constants, the model fixture, config and registration.  None needs a GPU.

Measured here (the restatement against the traces, |x - ref| / max(1, |ref|), largest over all traces): observations
after post_physics_step 7.7e-7, reset states 5.7e-7, reset observations and AMP history 7.2e-7, demo observations
7.2e-7; every integer and every velocity a reset writes exact.
"""
import ctypes as C
import os

import numpy as np
import pytest

import amp_ref as R
from migym import _abi, configs, taskdefs
from migym import model as M
from migym.motion import MotionTable, fetch_motion_files

CASES = [(N, name) for name in R.CONFIGS for N in R.SIZES]


def _state0(g, N, steps):
    return dict(progress=None, reset=np.zeros(N, np.int64), terminate=np.zeros(N, np.int64), amp=g["amp_0"].copy(),
                obs=np.zeros((N, 105), np.float32))


@pytest.mark.parametrize("N,name", CASES)
def test_restatement_replays_the_reference(N, name):
    """every step of every trace: pre, post, then reset_idx from the recorded uniforms; integers exact, floats by the
    1e-4 rule; the velocities a reset writes are unblended frame rows, so they are bit-equal and pin the frame index"""
    g = R.trace(N, name)
    _, _, _, ap = R.task_model(R.golden_cfg(N, name))
    p, tb = R.params_from(ap), R.table()
    st = _state0(g, N, p["steps"])
    worst = dict(obs=0.0, r_state=0.0, r_obs=0.0)
    for t in range(int(g["steps"])):
        k = f"s{t}_"
        st["progress"] = g[k + "progress_in"].copy()
        _, driven = R.pre_step(p, g[k + "actions"])
        assert np.array_equal(driven, g[k + "driven"]), f"step {t}: targets / efforts"
        amp_in = st["amp"].copy()
        R.post_step(p, st, g[k + "root_in"], g[k + "dof_in"], g[k + "rb_pos"], g[k + "ncf"])
        for key in ("progress", "reset", "terminate", "timeout"):
            assert np.array_equal(st[key], g[k + key]), f"step {t}: {key}"
        assert (st["rew"] == 1).all() and np.array_equal(g[k + "rew"], st["rew"])
        err, ok = R.close(st["obs"], g[k + "obs"])
        worst["obs"] = max(worst["obs"], err)
        assert ok, f"step {t}: obs off by {err:.3g}"
        # the chain continues from the reference's values
        st["obs"] = g[k + "obs"].copy()
        st["amp"] = np.concatenate([st["obs"][:, None], amp_in[:, :-1]], 1)
        st["root"], st["dof"] = g[k + "root_in"].copy(), g[k + "dof_in"].copy()
        ids = g[k + "ids"]
        before = {q: st[q].copy() for q in ("root", "dof", "obs", "amp", "progress")}
        R.reset_idx(p, tb, st, ids, g[k + "noise"], g[k + "rb_pos"])
        assert np.array_equal(st["dof"][ids][..., 1], g[k + "r_dof"][..., 1]), f"step {t}: frame index (dof velocities)"
        assert np.array_equal(st["root"][ids][:, 7:], g[k + "r_root"][:, 7:]), f"step {t}: frame index (root twist)"
        for got, want, w in ((st["root"][ids], g[k + "r_root"], "r_state"), (st["dof"][ids], g[k + "r_dof"], "r_state"),
                             (st["obs"][ids], g[k + "r_obs"], "r_obs"), (st["amp"][ids], g[k + "r_amp"], "r_obs")):
            err, ok = R.close(got, want)
            worst[w] = max(worst[w], err)
            assert ok, f"step {t}: reset {w} off by {err:.3g}"
        rest = np.setdiff1d(np.arange(N), ids)
        for q in before:
            assert np.array_equal(st[q][rest], before[q][rest]), f"step {t}: an unlisted env's {q} changed"
        assert (st["progress"][ids] == 0).all() and (st["reset"][ids] == 0).all() and (st["terminate"][ids] == 0).all()
        st["root"][ids], st["dof"][ids] = g[k + "r_root"], g[k + "r_dof"]
        st["obs"][ids], st["amp"][ids] = g[k + "r_obs"], g[k + "r_amp"]
    print(f"{name} N={N}: worst {worst}")


@pytest.mark.parametrize("name", ["random", "hybrid"])
@pytest.mark.parametrize("n", [5, 130])
def test_restatement_demo_observations(name, n):
    d = R.demo()
    _, _, _, ap = R.task_model(R.golden_cfg(4, name))
    p = R.params_from(ap)
    got = R.obs_demo(p, R.table(), d[f"{name}_n{n}_noise"])
    err, ok = R.close(got.reshape(n, -1), d[f"{name}_n{n}_out"])
    print(f"demo {name} n={n}: {err:.3g}")
    assert ok, err


def test_traces_hold_their_branches():
    """what the generator asserted, re-read from the files: hybrid resets take both paths, phases reach 0 and the
    clip's last frame, history times go negative, all three clips are drawn"""
    tb = R.table()
    for N in R.SIZES:
        g = R.trace(N, "hybrid")
        u = np.concatenate([g[f"s{t}_noise"] for t in range(6)])
        ref = u[:, 0] < np.float32(g["hybrid_prob"])
        assert ref.any() and (~ref).any()
        mids = R.pick_motion(tb, u[:, 1])
        assert set(mids.tolist()) == {0, 1, 2}
        t0 = u[:, 2].astype(np.float64) * tb.lengths[mids]
        dt = float(g["sim_dt"]) * int(g["control_freq_inv"])
        assert (t0 - 2 * dt < 0).any() and (u[:, 2] == 0).any() and (u[:, 2] > 0.9999).any()


@pytest.mark.parametrize("clip", R.CLIPS)
def test_motion_table_matches_motionlib(clip):
    """migym.motion against MotionLib's per-frame tensors: frame counts, lengths and dts exact; measured: every tensor
    bit-equal on this machine (the same fp32 expressions), asserted by the 1e-4 rule at 1e-6"""
    ml = R.motionlib()
    tb = MotionTable(os.path.join(R.GOLDEN, clip + ".npz"), [5, 8, 11, 14])
    m = tb.motions[0]
    assert tb.num_motions() == 1 and m.num_frames == int(ml[clip + "_num_frames"])
    assert tb.lengths[0] == float(ml[clip + "_length"]) and tb.dt[0] == float(ml[clip + "_dt"])
    assert tb.weights.tolist() == [1.0] and tb.cdf.tolist() == [1.0]
    for name, got in (("global_translation", m.global_translation), ("global_rotation", m.global_rotation),
                      ("local_rotation", m.local_rotation), ("root_velocity", m.root_velocity),
                      ("root_angular_velocity", m.root_angular_velocity), ("dof_vels", m.dof_vels)):
        err, ok = R.close(got, ml[f"{clip}_{name}"], 1e-6)
        assert got.shape == ml[f"{clip}_{name}"].shape and ok, f"{name}: {err:.3g}"
    assert np.array_equal(m.dof_vels[-1], m.dof_vels[-2]), "the last frame's DOF velocities repeat"
    # the packed layout
    f = tb.frames
    assert f.shape == (m.num_frames, _abi.MG_AMP_FRAME_FLOATS) and f.dtype == np.float32
    assert np.array_equal(f[:, 0:3], m.global_translation[:, 0]) and np.array_equal(f[:, 3:7], m.global_rotation[:, 0])
    assert np.array_equal(f[:, 13:73].reshape(-1, 15, 4), m.local_rotation)
    assert np.array_equal(f[:, 73:101], m.dof_vels.astype(np.float32))
    assert np.array_equal(f[:, 101:113].reshape(-1, 4, 3), m.global_translation[:, [5, 8, 11, 14]])


def test_motion_yaml_matches_motionlib():
    ml, tb = R.motionlib(), R.table()
    files, weights = fetch_motion_files(R.MOTIONS_YAML)
    assert [os.path.basename(f) for f in files] == [c + ".npz" for c in R.CLIPS] and weights == [0.5, 0.3, 0.2]
    assert np.array_equal(tb.lengths, ml["yaml_lengths"]) and np.array_equal(tb.weights, ml["yaml_weights"])
    assert np.array_equal(tb.dt, ml["yaml_dt"]) and np.array_equal(tb.num_frames, ml["yaml_num_frames"])
    assert tb.index.tolist() == [[0, 154], [154, int(tb.num_frames[1])], [154 + int(tb.num_frames[1]), 30]]
    assert tb.frames.shape[0] == int(tb.num_frames.sum()) and tb.time.shape == (3, 3) and tb.time.dtype == np.float64
    assert tb.cdf[-1] == 1.0 and (np.diff(tb.cdf) > 0).all()


def test_motion_loader_rejects_what_it_cannot_sample(tmp_path):
    with np.load(os.path.join(R.GOLDEN, "amp_humanoid_walk_flip.npz")) as z:
        c = {k: z[k] for k in z.files}
    one = dict(c)
    for k in ("rotation", "root_translation", "global_velocity", "global_angular_velocity"):
        one[k] = c[k][:1]
    np.savez(tmp_path / "one.npz", **one)
    with pytest.raises(ValueError, match="at least 2 frames"):
        MotionTable(str(tmp_path / "one.npz"), [5, 8, 11, 14])
    with pytest.raises(ValueError, match="expected .npy"):
        MotionTable(str(tmp_path / "clip.txt"), [5, 8, 11, 14])


def test_amp_params_match_the_reference():
    ml = R.motionlib()
    cfg = R.golden_cfg(8, "hybrid")
    spec, mnp, sp, ap = R.task_model(cfg)
    # _build_pd_action_offset_scale, run unmodified by the generator on this model's limits
    for got, want in ((ap.pd_action_offset, ml["pd_action_offset"]), (ap.pd_action_scale, ml["pd_action_scale"])):
        assert np.abs(np.array(list(got), np.float64) - want).max() <= 2.4e-7, "more than an fp32 ulp of pi apart"
    sizes = np.diff(taskdefs.AMP_DOF_OFFSETS)
    for j, o in enumerate(taskdefs.AMP_DOF_OFFSETS[:-1]):
        if sizes[j] == 3:
            assert list(ap.pd_action_offset)[o:o + 3] == [0.0] * 3
            assert list(ap.pd_action_scale)[o:o + 3] == [float(np.float32(np.pi))] * 3
    assert np.array_equal(np.array(list(ap.motor_effort), np.float32), ml["motor_efforts"])
    assert ap.dt == 2 * 0.0166 and ap.dt != float(np.float32(2 * 0.0166)), "dt is a Python double"
    assert list(ap.key_body) == [5, 8, 11, 14] and ap.contact_body_mask == (1 << 11) | (1 << 14) and ap.num_bodies == 15
    assert ap.max_episode_length == 12 and ap.termination_height == 0.5 and ap.enable_early_termination == 1
    assert ap.local_root_obs == 0 and ap.pd_control == 1 and ap.state_init == 3 and ap.num_amp_obs_steps == 3
    init = np.array(list(ap.initial_dof_pos), np.float32)
    names = spec.dof_names
    assert init[names.index("right_shoulder_x")] == np.float32(0.5 * np.pi)
    assert init[names.index("left_shoulder_x")] == np.float32(-0.5 * np.pi) and np.count_nonzero(init) == 2
    assert list(ap.initial_root) == [0, 0, np.float32(0.89), 0, 0, 0, 1] + [0] * 6
    for bad in (1, _abi.MG_AMP_MAX_OBS_STEPS + 1):
        cfg["env"]["numAMPObsSteps"] = bad
        with pytest.raises(ValueError, match="numAMPObsSteps"):
            taskdefs.amp_params(cfg, spec)
    cfg["env"]["numAMPObsSteps"] = 2
    cfg["env"]["stateInit"] = "Sideways"
    with pytest.raises(ValueError, match="stateInit"):
        taskdefs.amp_params(cfg, spec)


def test_amp_spec_drive_modes():
    raw = M.load_json(R.MODEL_TABLE)
    pd = taskdefs.amp_spec(raw, R.golden_cfg(8, "hybrid"))
    eff = taskdefs.amp_spec(raw, R.golden_cfg(8, "default"))
    for a, b, c in zip(raw.nodes[1:], pd.nodes[1:], eff.nodes[1:]):
        assert (b.drive_kp, b.stiffness, b.damping) == (a.stiffness, 0.0, a.damping) and a.stiffness > 0
        assert (c.drive_kp, c.stiffness, c.damping, c.effort_limit) == (0.0, a.stiffness, a.damping, a.effort_limit)
        assert b.effort_limit == a.effort_limit
    assert pd.angular_damping == 0.01 and pd.max_angular_velocity == 100.0 and raw.nodes[1].drive_kp == 0.0


def test_model_fixture_and_instance():
    """the fixture is what tools/build_models.py amp_humanoid writes; the dispatcher puts it on the 64-lane instance"""
    spec = M.load_json(R.MODEL_TABLE)
    assert (len(spec.nodes), len(spec.bodies), spec.num_dofs, len(spec.geoms), len(spec.pairs)) == (29, 15, 28, 18, 122)
    assert abs(spec.total_mass() - 48.89) < 0.01 and not spec.fixed_base and spec.self_collision
    assert [spec.body_index(n) for n in taskdefs.AMP_KEY_BODY_NAMES] == [5, 8, 11, 14]
    lib = _abi.lib()
    _, mnp, sp, _ = R.task_model(R.golden_cfg(8, "random"))
    t = C.c_int32()
    _abi.check(lib.mg_model_team_lanes(mnp.ctypes.data, 48, C.byref(t)), lib)
    assert t.value == 64 and sp.max_contacts == 48
    assert lib.mg_amp_params_sizeof() == C.sizeof(_abi.AmpParams) and lib.mg_version() == 7
    assert lib.mg_amp_views_sizeof() == C.sizeof(_abi.AmpViews)


def test_config_and_registration():
    import isaacgymenvs.tasks
    import migym.tasks
    from migym.tasks.humanoid_amp import HumanoidAMP
    assert migym.tasks.isaacgym_task_map["HumanoidAMP"] is HumanoidAMP is isaacgymenvs.tasks.HumanoidAMP
    cfg = configs.task_config("HumanoidAMP")
    env = cfg["env"]
    assert (env["numEnvs"], env["episodeLength"], env["controlFrequencyInv"]) == (4096, 300, 2)
    assert (env["stateInit"], env["hybridInitProb"], env["numAMPObsSteps"]) == ("Random", 0.5, 2)
    assert env["pdControl"] is True and env["localRootObs"] is False and env["terminationHeight"] == 0.5
    assert env["contactBodies"] == ["right_foot", "left_foot"] and env["motion_file"] == "amp_humanoid_run.npy"
    assert cfg["sim"]["dt"] == 0.0166 and cfg["sim"]["physx"]["num_position_iterations"] == 4
    assert taskdefs.TASK_INFO["HumanoidAMP"] == (None, None, 105, 28, 0.89, 48)
    assert taskdefs.render_settings("HumanoidAMP", cfg)["follow"] is True
    assert HumanoidAMP.supports_host_pipeline is False


def test_missing_assets_raise(tmp_path):
    from migym.tasks import humanoid_amp as H
    with pytest.raises(FileNotFoundError, match="build_models.py amp_humanoid"):
        H._load_model({"asset": {"modelTable": str(tmp_path / "nope.json")}})
    with pytest.raises(FileNotFoundError, match="motion file"):
        H._motion_path({"motion_file": "nope.npy", "asset": {"motionRoot": str(tmp_path)}})


def test_rlgames_env_info_carries_the_amp_space():
    from migym.utils.rlgames_utils import RLGPUEnv
    from migym import spaces

    class Env:
        action_space = observation_space = state_space = spaces.Box(np.zeros(2), np.ones(2))
        num_agents, num_states = 1, 0

    w = object.__new__(RLGPUEnv)
    w.env = Env()
    assert "amp_observation_space" not in w.get_env_info()
    Env.amp_observation_space = spaces.Box(-np.ones(210), np.ones(210))
    assert w.get_env_info()["amp_observation_space"] is Env.amp_observation_space
