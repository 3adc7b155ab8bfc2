"""CPU tests of the AnymalTerrain task layer (no GPU): the numpy restatement (tests/anymal_terrain_ref.py) against the
reference's own output (tests/golden/trace_anymal_terrain.npz), the terrain generator against the reference's Terrain
class (tests/golden/terrain_layout.npz) and against the definitions of its sub-terrain functions, the curriculum's one
deliberate deviation, the config, the ABI additions and the constructor's error paths."""
import ctypes as C
import re
import zlib

import numpy as np
import pytest

import anymal_terrain_ref as R
from migym import _abi, configs, taskdefs
from migym import terrain as T

SIZES = [6, 67]
BITWISE = ("progress", "reset", "timeout", "root", "dof", "terrain_levels", "env_origins", "feet_air_time",
           "last_actions", "last_dof_vel")


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("N", SIZES)
def test_restatement_reproduces_the_reference(N):
    """every recorded step from its recorded inputs: integer and copied outputs bit-equal, observations, reward,
    commands[:, 2], the episode sums and means by the 1e-4 rule; the reward clip falls on the same envs"""
    g = R.golden()
    ap, p, table, origins = R.golden_params(N)
    assert np.array_equal(np.array(list(ap.noise_scale_vec), np.float32), g["noise_scale_vec"])
    assert np.array_equal(p["points"], g["height_points"]) and p["max_episode_length"] == int(g["max_episode_length"])
    assert np.array_equal(np.append(p["rew"], p["rew_term"]), g["rew_scales"])
    pushed = 0
    for t in range(int(g["steps"])):
        pre = f"N{N}_s{t}_"
        st = R.golden_state(g, N, t)
        a, tq = R.pre_step(p, g[pre + "actions"], g[pre + "pre_dof"])
        assert np.array_equal(tq, g[pre + "torques_in"]), f"step {t}: the PD torques"
        push = bool(g[pre + "push_now"])
        pushed += push
        out = R.post_step(p, st, g[pre + "ncf"], g[pre + "actions"], g[pre + "noise"], push_now=push)
        for k in BITWISE:
            assert np.array_equal(st[k], g[pre + k]), f"step {t}: {k}"
        assert np.array_equal(st["commands"][:, [0, 1, 3]], g[pre + "commands"][:, [0, 1, 3]]), f"step {t}: commands"
        assert np.array_equal(out["measured_heights"], g[pre + "measured_heights"]), f"step {t}: heights"
        for name, got in (("commands", st["commands"]), ("obs", out["obs"]), ("rew", out["rew"]),
                          ("episode_sums", st["episode_sums"]), ("episode_out", st["episode_out"])):
            assert R.close(got, g[pre + name]).all(), f"step {t}: {name}"
        term = p["rew_term"] * ((g[pre + "reset"] != 0) & ~g[pre + "timeout_in"])
        assert np.array_equal((out["rew"] - term) == 0, g[pre + "clipped"]), f"step {t}: the clip at 0"
    assert pushed == 1


def test_the_trace_covers_its_branches():
    """what the generator asserts, read back from the file: resets by base, knee and time-out, none; levels up, down,
    unchanged and wrapped; roots outside the table; forced time-out flags that suppress a termination reward"""
    g = R.golden()
    for N in SIZES:
        up = down = stay = wrap = outside = suppressed = zeroed = False
        nx, ny = g[f"N{N}_height_field_raw"].shape
        for t in range(int(g["steps"])):
            pre = f"N{N}_s{t}_"
            rst = g[pre + "reset"] != 0
            a, b = g[pre + "terrain_levels_in"][rst].astype(int), g[pre + "terrain_levels"][rst].astype(int)
            up |= bool((b == a + 1).any())
            down |= bool((b == a - 1).any())
            stay |= bool((b == a).any())
            wrap |= bool(((a == int(g["env_rows"]) - 1) & (b == 0)).any())
            xy = g[pre + "root_in"][~rst, :2]
            outside |= bool(((xy < -float(g["border_size"])) | (xy > np.array([nx, ny]) * 0.1 - 1.0)).any())
            suppressed |= bool((rst & g[pre + "timeout_in"]).any())
            zeroed |= bool((g[pre + "commands"][rst] == 0).all(1).any())
            assert rst.any() and (~rst).any() and not g[pre + "timeout"].any()
        assert up and down and stay and wrap and outside and suppressed, N
    assert zeroed


def test_curriculum_decides_per_env():
    """two envs reset together; env 0 stands 0.3 m from its origin with a small command.  The reference's norm over
    both envs' commands (0.25 * 20 * |(0.1, 0, 1, 1)| = 7.1 m) would send it down a level, and so does its own (0.25 *
    20 * 0.1 = 0.5 m); at 0.6 m only the reference's norm would: the level stays"""
    cfg = R.task_cfg(2)
    spec, _, _, ap = R.task_model(cfg)
    ap.env_length, ap.env_rows, ap.env_cols, ap.custom_origins, ap.curriculum = 8.0, 10, 20, 1, 1
    p = R.params_from(ap, None, np.zeros((10, 20, 3), np.float32))
    st = dict(root=np.zeros((2, 13), np.float32), env_origins=np.zeros((2, 3), np.float32),
              commands=np.array([[0.1, 0, 0, 0], [1, 1, 0, 0]], np.float32), terrain_levels=np.array([3, 3], np.int32))
    st["root"][0, 0] = 0.3
    assert R.update_terrain_level(p, st, 0) == 2 and R.update_terrain_level(p, st, 0, frobenius_ids=[0, 1]) == 2
    st["root"][0, 0] = 0.6
    assert R.update_terrain_level(p, st, 0) == 3, "decided by the env's own commands"
    assert R.update_terrain_level(p, st, 0, frobenius_ids=[0, 1]) == 2, "the reference's norm would take it down"
    st["root"][1, 0] = 4.5
    assert R.update_terrain_level(p, st, 1) == 3, "past half a map, but within 0.25 * 20 * |(1, 1)|: up and down"
    st["commands"][1, :2] = 0.1
    assert R.update_terrain_level(p, st, 1) == 4
    st["terrain_levels"][1] = 9
    assert R.update_terrain_level(p, st, 1) == 0, "past the last level: the modulo wraps"
    st["terrain_levels"][0], st["root"][0, 0] = 0, 0.1
    assert R.update_terrain_level(p, st, 0) == 0, "below level 0: clipped"


# ------------------------------------------------------------------------------------------------ the terrain generator
@pytest.mark.parametrize("tag, curriculum, types, proportions", [
    ("cur_", True, 5, [0.1, 0.1, 0.35, 0.25, 0.2]), ("rnd_", False, 5, [0.1, 0.1, 0.35, 0.25, 0.2]),
    ("cur10_", True, 10, [0.1, 0.1, 0.3, 0.2, 0.2])])
def test_terrain_equals_the_reference_class(tag, curriculum, types, proportions):
    """migym.terrain.Terrain against the reference's Terrain class run on the same sub-terrain functions.  5 types
    enter four of the curriculum's brackets (j / 5 never falls in [0.1, 0.2)); 10 types with proportions summing to 0.9
    enter all six, the rough slope and the stepping stones included"""
    lay = np.load(R.LAYOUT)
    np.random.seed(int(lay[tag + "seed"]))
    cfg = dict(terrainType="trimesh", curriculum=curriculum, mapLength=8.0, mapWidth=8.0, numLevels=2,
               numTerrains=types, terrainProportions=proportions, slopeTreshold=0.5)
    t = T.Terrain(cfg, num_robots=10)
    assert (t.tot_rows, t.tot_cols) == (int(lay[tag + "tot_rows"]), int(lay[tag + "tot_cols"])) == (560, 80 * types + 400)
    assert t.height_field_raw.dtype == np.int16 and np.array_equal(t.height_field_raw, lay[tag + "field"])
    assert zlib.crc32(np.ascontiguousarray(t.height_field_raw).tobytes()) == int(lay[tag + "crc"])
    assert np.array_equal(t.env_origins, lay[tag + "env_origins"]) and t.env_origins.shape == (2, types, 3)
    assert (t.horizontal_scale, t.vertical_scale, t.border_size, t.env_length, t.env_rows) == (0.1, 0.005, 20, 8.0, 2)
    assert not hasattr(t, "vertices"), "no triangle mesh is built"
    if curriculum:
        # the harder level's maps.  5 types: smooth pit, stairs down (twice, alike), stairs up, obstacles; 10 types:
        # smooth pit, rough pit, stairs down (3 alike), stairs up (2 alike), obstacles (2, drawn apart), stepping stones
        cols = [t.height_field_raw[280:360, 200 + 80 * j:280 + 80 * j] for j in range(types)]
        assert all(c.any() for c in cols) and len({c.tobytes() for c in cols}) == (4 if types == 5 else 7)
        if types == 10:
            assert cols[9].min() == -2000 and len(np.unique(cols[1])) > 20, "stepping stones' pit; a rough slope"


def sub(width=80, length=80):
    return T.SubTerrain("terrain", width=width, length=length, vertical_scale=0.005, horizontal_scale=0.1)


@pytest.mark.parametrize("slope", [0.3, -0.2])
def test_pyramid_slope(slope):
    t = T.pyramid_sloped_terrain(sub(), slope=slope, platform_size=3.0)
    h = t.height_field_raw.astype(int) * (1 if slope > 0 else -1)
    assert t.height_field_raw.dtype == np.int16 and t.height_field_raw.shape == (80, 80)
    top = h[40 - 15, 40 - 15]
    assert top > 0 and h.max() == top and (h[26:55, 26:55] == top).all(), "a flat top at the platform corner's height"
    assert h.min() == 0 and (h[0] == 0).all() and (h[:, 0] == 0).all()
    assert (np.diff(h[:41], axis=0) >= 0).all() and (np.diff(h[40:], axis=0) <= 0).all(), "monotone toward the centre"
    assert (np.diff(h[:, :41], axis=1) >= 0).all() and (np.diff(h[:, 40:], axis=1) <= 0).all()
    peak = int(abs(slope) * (0.1 / 0.005) * 40)
    assert top == int(peak * (25 / 40) * (25 / 40))


@pytest.mark.parametrize("step_height", [0.1, -0.15])
def test_pyramid_stairs(step_height):
    t = T.pyramid_stairs_terrain(sub(), step_width=0.31, step_height=step_height, platform_size=3.0)
    h, sh = t.height_field_raw.astype(int), int(step_height / 0.005)
    assert t.height_field_raw.dtype == np.int16
    rings = 0
    for k in range(40 // 3 + 1):
        ring = np.concatenate([h[3 * k, 3 * k:80 - 3 * k], h[80 - 3 * k - 1, 3 * k:80 - 3 * k],
                               h[3 * k:80 - 3 * k, 3 * k], h[3 * k:80 - 3 * k, 80 - 3 * k - 1]])
        assert (ring == ring[0]).all(), f"ring {k} is not level"
        rings = max(rings, ring[0] // sh)
    assert h[0, 0] == 0 and h[3, 3] == sh and h[40, 40] == rings * sh and rings == 9
    side = 80 - 2 * 3 * rings
    assert side <= 30 < side + 6 and (h[40 - side // 2:40 + side // 2, 40 - side // 2:40 + side // 2] == rings * sh).all()


def test_discrete_obstacles():
    np.random.seed(3)
    t = T.discrete_obstacles_terrain(sub(), 0.15, 1.0, 2.0, 40, platform_size=3.0)
    H = int(0.15 / 0.005)
    assert t.height_field_raw.dtype == np.int16
    assert set(np.unique(t.height_field_raw)) <= {-H, -H // 2, 0, H // 2, H} and len(np.unique(t.height_field_raw)) > 2
    assert (t.height_field_raw[25:55, 25:55] == 0).all() and t.height_field_raw.any()


def test_random_uniform():
    np.random.seed(4)
    t = T.random_uniform_terrain(sub(), min_height=-0.1, max_height=0.1, step=0.025, downsampled_scale=0.2)
    h = t.height_field_raw
    assert h.dtype == np.int16 and h.min() >= -20 and h.max() <= 20 and len(np.unique(h)) > 10
    np.random.seed(4)
    base = T.pyramid_sloped_terrain(sub(), slope=0.2, platform_size=3.0).height_field_raw.copy()
    both = T.random_uniform_terrain(T.pyramid_sloped_terrain(sub(), slope=0.2, platform_size=3.0), -0.1, 0.1, 0.025, 0.2)
    assert np.array_equal(both.height_field_raw - base, h), "added to what the field holds"
    np.random.seed(5)
    flat = T.random_uniform_terrain(sub(), 0.05, 0.05, step=0.005)
    assert (flat.height_field_raw == 10).all(), "a single value interpolates to itself"


def test_stepping_stones():
    np.random.seed(6)
    t = T.stepping_stones_terrain(sub(), stone_size=0.5, stone_distance=0.2, max_height=0.05, platform_size=1.0,
                                  depth=-1.0)
    h = t.height_field_raw
    assert h.dtype == np.int16 and (h[35:45, 35:45] == 0).all()
    assert (h[5:7, :30] == -200).all() and (h[:30, 5:7] == -200).all(), "the gaps are at the pit's depth"
    assert (np.abs(h[0:5, 0:5]) <= 10).all() and (h[0:5, 0:5] == h[0, 0]).all(), "a stone is level"


# ------------------------------------------------------------------------------------------------ config, ABI, errors
def test_config_has_every_key_the_task_reads():
    cfg = configs.task_config("AnymalTerrain", 64)
    env = cfg["env"]
    assert cfg["name"] == "AnymalTerrain" and env["numEnvs"] == 64 and cfg["sim"]["dt"] == 0.005
    assert cfg["sim"]["substeps"] == 1 and "clipActions" not in env and "clipObservations" not in env
    for k in ("terrainType", "staticFriction", "dynamicFriction", "restitution", "curriculum", "maxInitMapLevel",
              "mapLength", "mapWidth", "numLevels", "numTerrains", "terrainProportions", "slopeTreshold"):
        assert k in env["terrain"], k
    for k in taskdefs.ANYMAL_TERRAIN_REWARD_KEYS + (
            "terminalReward", "allowKneeContacts", "linearVelocityScale", "angularVelocityScale", "dofPositionScale",
            "dofVelocityScale", "heightMeasurementScale", "addNoise", "noiseLevel", "dofPositionNoise",
            "dofVelocityNoise", "linearVelocityNoise", "angularVelocityNoise", "gravityNoise", "heightMeasurementNoise",
            "pushRobots", "pushInterval_s", "episodeLength_s", "frictionRange"):
        assert k in env["learn"], k
    assert env["control"] == {"stiffness": 80.0, "damping": 2.0, "actionScale": 0.5, "decimation": 4}
    assert env["urdfAsset"]["footName"] == "SHANK" and env["urdfAsset"]["kneeName"] == "THIGH"
    assert "AnymalTerrain" in taskdefs.TASK_INFO and "AnymalTerrain" in taskdefs.RENDER_DEFAULTS
    assert taskdefs.TASK_INFO["AnymalTerrain"][2:4] == (188, 12)


def test_params_follow_the_reference_constants():
    cfg = R.task_cfg(8)
    spec, mnp, sp, ap = R.task_model(cfg)
    f = np.float32
    dt = 4 * 0.005
    assert ap.max_episode_length == int(20 / dt + 0.5) == 1000 and f(ap.dt) == f(0.005)
    assert np.array_equal(np.array(list(ap.rew_scale), f),
                          np.array([x * dt for x in (1.0, -4.0, 0.5, -0.05, -0.0, -0.00002, -0.0005, -0.0, 1.0, -0.25,
                                                     -0.0, -0.01, -0.0)], f))
    assert (ap.Kp, ap.Kd, ap.action_scale, ap.torque_clip) == (80.0, 2.0, 0.5, 80.0)
    assert list(ap.knee_body) == [2, 5, 8, 11] and list(ap.foot_body) == [3, 6, 9, 12] and ap.base_body == 0
    assert list(ap.hip_dof) == [0, 3, 6, 9] and ap.allow_knee_contacts == 1 and ap.add_noise == 1
    assert np.isinf(ap.clip_actions) and np.isinf(ap.clip_obs)
    nv = np.array(list(ap.noise_scale_vec), f)
    assert nv[0] == f(0.1 * 1.0 * 2.0) and nv[3] == f(0.2 * 1.0 * 0.25) and nv[6] == f(0.05) and (nv[9:12] == 0).all()
    assert nv[12] == f(0.01) and nv[24] == f(1.5 * 1.0 * 0.05) and nv[36] == nv[175] == f(0.06 * 1.0 * 5.0)
    assert (nv[176:] == 0).all()
    pts = np.array(list(ap.height_points), f).reshape(140, 2)
    assert np.array_equal(pts[0], f([-0.8, -0.5])) and np.array_equal(pts[1], [f(0.1) * f(-8), f(0.1) * f(-4)])
    assert np.array_equal(pts[-1], f([0.8, 0.5])) and not (pts == 0).any()
    assert all(n.drive_kp == 0.0 and n.stiffness == 0.0 and n.effort_limit == 80.0 for n in spec.nodes[1:])
    assert spec.angular_damping == 0.0 and sp.substeps == 1 and sp.friction == 1.0


def test_abi_exports_and_struct_sizes():
    for name in ("mg_anymal_terrain_params_sizeof", "mg_anymal_terrain_views_sizeof", "mg_anymal_terrain_pre",
                 "mg_anymal_terrain_post", "mg_anymal_terrain_reset_idx"):
        assert name in _abi.EXPORTS, name
    assert (_abi.MG_ANYMAL_TERRAIN_OBS, _abi.MG_ANYMAL_TERRAIN_HEIGHT_POINTS, _abi.MG_ANYMAL_TERRAIN_NOISE_COLS) == \
        (188, 140, 219) and len(_abi.ANYMAL_TERRAIN_REWARDS) == 13
    lib = _abi.lib()
    assert lib.mg_version() == 7
    assert lib.mg_anymal_terrain_params_sizeof() == C.sizeof(_abi.AnymalTerrainParams)
    assert lib.mg_anymal_terrain_views_sizeof() == C.sizeof(_abi.AnymalTerrainViews)
    header = open(R.HERE + "/../include/migym.h").read()
    for name in _abi.EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), f"{name} is exported but not declared in migym.h"
    for name, value in (("MG_ANYMAL_TERRAIN_OBS", 188), ("MG_ANYMAL_TERRAIN_HEIGHT_POINTS", 140),
                        ("MG_ANYMAL_TERRAIN_NOISE_COLS", 219)):
        assert re.search(rf"#define {name} {value}\b", header)
    ap, v = _abi.AnymalTerrainParams(), _abi.AnymalTerrainViews()
    assert lib.mg_anymal_terrain_post(None, C.byref(ap), C.byref(v), C.byref(_abi.TaskBuffers()), None, None) != 0
    assert b"bad arguments" in lib.mg_last_error()


def test_constructor_error_paths():
    from migym.tasks.anymal_terrain import AnymalTerrain
    cfg = configs.task_config("AnymalTerrain", 4, overrides={"env.asset": {"modelTable": "/nonexistent/anymal.json"}})
    with pytest.raises(FileNotFoundError, match=r"AnymalTerrain: no ANYmal model found \(tried /nonexistent/anymal.json\)"
                                                r".*build_models.py anymal_minimal"):
        AnymalTerrain(cfg, "cpu", "cuda:0", -1, True)
    cfg = R.task_cfg(4, **{"terrain.terrainType": "none"})
    with pytest.raises(NameError, match="terrainType"):
        AnymalTerrain(cfg, "cpu", "cuda:0", -1, True)
    cfg = R.task_cfg(4)
    cfg["task"]["randomize"] = True
    with pytest.raises(NotImplementedError, match="task.randomize"):
        AnymalTerrain(cfg, "cpu", "cuda:0", -1, True)
