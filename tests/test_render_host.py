"""The fp64 reference ray caster (tests/render_ref.py) against analytic answers, the render ABI against its ctypes
mirror, and the condition the GPU tests rest on: at most 15 % of every image they compare is `ambiguous`.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import render_ref as RR
from migym import _abi, model as M, render as MR, taskdefs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I3 = np.eye(3)
GROUND_FAR = RR.prim(M.GT_PLANE, I3, [0, 0, -100.0], [0, 0, 0], MR.COL_GROUND)


def one_ray(prims, eye, d, hull=None):
    d = np.asarray(d, np.float64)
    ids, t, n, _ = RR.trace(prims, eye, (d / np.linalg.norm(d))[None, None], hull)
    return int(ids[0, 0]), float(t[0, 0]), n[0, 0]


# ------------------------------------------------------------------------------------------------ known answers
def test_unit_sphere_straight_ahead_at_distance_5_has_centre_depth_4():
    prims = [RR.prim(M.GT_SPHERE, I3, [5, 0, 1], [1, 0, 0], 0), GROUND_FAR]
    img = RR.render(prims, 9, 9, 60.0, (0, 0, 1), (5, 0, 1))
    assert img["ids"][4, 4] == 0 and img["depth"][4, 4] == pytest.approx(4.0, abs=1e-12)
    np.testing.assert_allclose(img["normals"][4, 4], [-1, 0, 0], atol=1e-12)
    sh = MR.AMBIENT + MR.DIFFUSE * max(0.0, -MR.LIGHT[0])
    assert tuple(img["rgb"][4, 4]) == tuple(int(math.floor(255 * c * sh + 0.5)) for c in MR.PALETTE[0])
    # a ray that passes the sphere at 1.5 radii misses it
    i, t, _ = one_ray(prims, (0, 0, 1), (5, 1.5, 0))
    assert i == -1 and np.isinf(t)                            # horizontal: not the ground either
    # the silhouette: the ray tangent to the sphere has sin(angle) = 1 / 5
    a = math.asin(0.2)
    assert one_ray(prims, (0, 0, 1), (math.cos(a - 1e-6), math.sin(a - 1e-6), 0))[0] == 0
    assert one_ray(prims, (0, 0, 1), (math.cos(a + 1e-6), math.sin(a + 1e-6), 0))[0] == -1


def test_box_face_depth_normal_and_rotation():
    box = RR.prim(M.GT_BOX, I3, [3, 0, 0], [0.5, 1.0, 0.25], 1)
    i, t, n = one_ray([box], (0, 0, 0), (1, 0, 0))
    assert i == 0 and t == pytest.approx(2.5, abs=1e-12) and tuple(n) == (-1, 0, 0)
    # from above, slanted: the top face z = 0.25 is hit where the ray crosses it
    eye, d = np.array([3.0, 0.0, 2.0]), np.array([0.1, 0.2, -1.0])
    i, t, n = one_ray([box], eye, d)
    assert t == pytest.approx(1.75 * np.linalg.norm(d), abs=1e-12) and tuple(n) == (0, 0, 1)
    # rotated 90 degrees about z the half extents swap: the face towards the eye is now 1.0 away from the centre
    Rz = M.qmat(M.quat_from_axis_angle([0, 0, 1], math.pi / 2))
    i, t, n = one_ray([RR.prim(M.GT_BOX, Rz, [3, 0, 0], [0.5, 1.0, 0.25], 1)], (0, 0, 0), (1, 0, 0))
    assert t == pytest.approx(2.0, abs=1e-12)
    np.testing.assert_allclose(n, [-1, 0, 0], atol=1e-12)
    # from inside, the exit face is the hit and the normal stays outward
    i, t, n = one_ray([box], (3, 0, 0), (0, 1, 0))
    assert t == pytest.approx(1.0, abs=1e-12) and tuple(n) == (0, 1, 0)


def test_capsule_side_against_its_cap():
    cap = RR.prim(M.GT_CAPSULE, I3, [0, 0, 0], [0.5, 1.0, 0], 2)    # radius 0.5, half length 1 along z
    # the side: a horizontal ray at z = 0.4 meets the cylinder at distance 5 - 0.5
    i, t, n = one_ray([cap], (5, 0, 0.4), (-1, 0, 0))
    assert t == pytest.approx(4.5, abs=1e-12)
    np.testing.assert_allclose(n, [1, 0, 0], atol=1e-12)
    # the cap: at z = 1.3 the ray meets the sphere about (0, 0, 1) at x = sqrt(0.25 - 0.09) = 0.4
    i, t, n = one_ray([cap], (5, 0, 1.3), (-1, 0, 0))
    assert t == pytest.approx(4.6, abs=1e-12)
    np.testing.assert_allclose(n, [0.8, 0, 0.6], atol=1e-12)
    # the seam z = 1 belongs to both and they agree there
    i, t, n = one_ray([cap], (5, 0, 1.0), (-1, 0, 0))
    assert t == pytest.approx(4.5, abs=1e-12)
    # down the axis: the top of the upper cap; past the caps: a miss
    i, t, n = one_ray([cap], (0, 0, 5), (0, 0, -1))
    assert t == pytest.approx(3.5, abs=1e-12)
    np.testing.assert_allclose(n, [0, 0, 1], atol=1e-12)
    assert one_ray([cap], (5, 0, 1.6), (-1, 0, 0))[0] == -1
    # the capped cylinder of the same size is flat on top: 4.0 down the axis, and missed at z = 1.3
    cyl = RR.prim(M.GT_CYLINDER, I3, [0, 0, 0], [0.5, 1.0, 0], 2)
    i, t, n = one_ray([cyl], (0.2, 0, 5), (0, 0, -1))
    assert t == pytest.approx(4.0, abs=1e-12) and tuple(n) == (0, 0, 1)
    assert one_ray([cyl], (5, 0, 1.3), (-1, 0, 0))[0] == -1
    assert one_ray([cyl], (5, 0, 0.4), (-1, 0, 0))[1] == pytest.approx(4.5, abs=1e-12)


def _rand_pose(rng):
    return M.qmat(M.quat_from_axis_angle(rng.normal(size=3), rng.uniform(-3, 3))), rng.uniform(-0.3, 0.3, 3)


def test_hull_of_a_boxs_six_planes_equals_the_box():
    rng = np.random.default_rng(3)
    h = np.array([0.3, 0.2, 0.4])
    planes = [[s if k == a else 0.0 for k in range(3)] + [h[a]] for a in range(3) for s in (1.0, -1.0)]
    Rw, p = _rand_pose(rng)
    box = [RR.prim(M.GT_BOX, Rw, p, h, 0), GROUND_FAR]
    hull = [RR.prim(M.GT_CONVEX, Rw, p, h, 0), GROUND_FAR]
    a = RR.render(box, 31, 23, 60.0, (1.2, -0.9, 0.8), (0, 0, 0))
    b = RR.render(hull, 31, 23, 60.0, (1.2, -0.9, 0.8), (0, 0, 0), planes)
    assert (a["ids"] == 0).sum() > 40
    assert (a["ids"] == b["ids"]).all() and (a["rgb"] == b["rgb"]).all()
    m = a["ids"] == 0
    np.testing.assert_allclose(a["depth"][m], b["depth"][m], rtol=0, atol=1e-12)
    np.testing.assert_allclose(a["normals"][m], b["normals"][m], atol=1e-12)


def test_ellipsoid_with_equal_semi_axes_equals_the_sphere():
    rng = np.random.default_rng(4)
    Rw, p = _rand_pose(rng)
    sph = [RR.prim(M.GT_SPHERE, Rw, p, [0.35, 0, 0], 3), GROUND_FAR]
    ell = [RR.prim(M.GT_ELLIPSOID, Rw, p, [0.35, 0.35, 0.35], 3), GROUND_FAR]
    a = RR.render(sph, 31, 23, 60.0, (1.2, -0.9, 0.8), (0, 0, 0))
    b = RR.render(ell, 31, 23, 60.0, (1.2, -0.9, 0.8), (0, 0, 0))
    assert (a["ids"] == 0).sum() > 40 and (a["ids"] == b["ids"]).all()
    m = a["ids"] == 0
    np.testing.assert_allclose(a["depth"][m], b["depth"][m], rtol=0, atol=1e-12)
    np.testing.assert_allclose(a["normals"][m], b["normals"][m], atol=1e-9)
    # a true ellipsoid along its axes: the hit is at the semi-axis
    e = RR.prim(M.GT_ELLIPSOID, I3, [0, 0, 0], [0.5, 0.2, 0.1], 3)
    assert one_ray([e], (3, 0, 0), (-1, 0, 0))[1] == pytest.approx(2.5, abs=1e-12)
    assert one_ray([e], (0, 0, 3), (0, 0, -1))[1] == pytest.approx(2.9, abs=1e-12)


def test_ground_checker_sky_and_ties():
    ground = RR.prim(M.GT_PLANE, I3, [0, 0, 0], [0, 0, 0], MR.COL_GROUND)
    img = RR.render([ground], 8, 8, 60.0, (0.5, 0.5, 2.0), (0.5001, 0.5, 0.0))
    sh = MR.AMBIENT + MR.DIFFUSE * MR.LIGHT[2]
    grey = [int(math.floor(255 * MR.PALETTE[MR.COL_GROUND + k][0] * sh + 0.5)) for k in (0, 1)]
    assert set(np.unique(img["rgb"])) == set(grey)           # both greys, shaded by the one normal
    i, t, n = one_ray([ground], (0.5, 0.5, 2), (0, 0, -1))
    assert i == 0 and t == pytest.approx(2.0) and tuple(n) == (0, 0, 1)
    # upwards: sky, +inf, id -1, the one sky colour
    up = RR.render([ground], 4, 4, 30.0, (0, 0, 1), (1, 0, 3))
    assert (up["ids"] == -1).all() and np.isinf(up["depth"]).all()
    assert (up["rgb"] == np.floor(255 * MR.PALETTE[MR.COL_SKY] + 0.5).astype(np.uint8)).all()
    # two identical spheres: the tie goes to the lower id
    s = [RR.prim(M.GT_SPHERE, I3, [4, 0, 0], [1, 0, 0], 0), RR.prim(M.GT_SPHERE, I3, [4, 0, 0], [1, 0, 0], 1)]
    assert one_ray(s, (0, 0, 0), (1, 0, 0))[0] == 0


def test_ambiguous_mask_marks_edges_grazing_hits_and_checker_borders():
    prims = [RR.prim(M.GT_SPHERE, I3, [5, 0, 1], [1, 0, 0], 0), RR.prim(M.GT_PLANE, I3, [0, 0, 0], [0, 0, 0], MR.COL_GROUND)]
    img = RR.render(prims, 41, 31, 60.0, (0, 0, 1), (5, 0, 1))
    amb, ids = img["ambiguous"], img["ids"]
    assert not amb[15, 20]                                   # the sphere's centre
    ndotd = np.abs(np.sum(img["normals"] * RR.rays(41, 31, 60.0, (0, 0, 1), (5, 0, 1)), -1))
    assert amb[(ids >= 0) & (ndotd < 0.1)].all() and ((ids >= 0) & (ndotd < 0.1)).any()
    assert 0 < amb.mean() < 0.5


# ------------------------------------------------------------------------------------------------ ABI
def test_render_exports_and_struct_size_match_the_mirror():
    lib = _abi.lib()
    for name in ("mg_render", "mg_render_args_sizeof", "mg_render_scratch_floats"):
        assert hasattr(lib, name) and name in _abi.EXPORTS
    assert lib.mg_render_args_sizeof() == C.sizeof(_abi.RenderArgs)
    assert lib.mg_version() == 7
    hdr = open(os.path.join(ROOT, "include", "migym.h")).read()
    fields = [f for f, _ in _abi.RenderArgs._fields_]
    body = hdr[hdr.index("typedef struct mg_render_args {"):hdr.index("} mg_render_args;")]
    decl = re.findall(r"\b(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert decl == fields, "the mirror's fields differ from the header's"
    # argument errors need no device: they are reported before anything is launched
    assert lib.mg_render(None, None, None) == -1 and b"mg_render" in lib.mg_last_error()
    assert lib.mg_render_scratch_floats(None, 1, 0) == 0


def test_render_defaults_cover_the_seven_tasks_and_take_overrides():
    for task in ("Cartpole", "Ant", "Humanoid", "ShadowHand", "MAAnt", "FrankaReachMA", "Anymal"):
        st = taskdefs.render_settings(task, {"env": {}})
        assert st["width"] > 0 and st["height"] > 0 and len(st["eye"]) == 3 and len(st["target"]) == 3
        f = np.subtract(st["target"], st["eye"])
        assert np.hypot(f[0], f[1]) > 1e-3, "the default view must not look along z"
    st = taskdefs.render_settings("Ant", {"env": {"render": {"width": 64, "height": 48, "follow": False}}})
    assert (st["width"], st["height"], st["follow"]) == (64, 48, False)
    with pytest.raises(ValueError):
        taskdefs.render_settings("Ant", {"env": {"render": {"widht": 64}}})


def test_primitive_count_matches_the_order_definition():
    ant, hand = M.load_builtin("ant"), taskdefs.hand_spec("egg")
    assert MR.num_primitives(ant, 4, 3) == 4 * len(ant.geoms) + 3 + 1
    assert MR.num_primitives(hand, 1, 0) == len(hand.geoms) + 2 + 1
    sc = RR.scene("boxes")
    prims = RR.scene_env_primitives(sc, 2)
    assert len(prims) == MR.num_primitives(sc["spec"], 1, 3)
    assert [p["type"] for p in prims[-4:]] == [M.GT_BOX] * 3 + [M.GT_PLANE]


# ------------------------------------------------------------------------------------------------ the GPU tests' scenes
@pytest.mark.parametrize("name", RR.SCENE_NAMES)
def test_scene_images_are_at_most_15_percent_ambiguous(name):
    """a condition of the GPU comparison, not a measurement: cameras and states are picked so that the reference alone
    meets it"""
    sc = RR.scene(name)
    assert sc["W"] % 16 and sc["H"] % 16 and (sc["W"] * sc["H"]) % 256
    for e, img in zip(RR.ENV_IDS, RR.scene_reference(name)):
        share = float(img["ambiguous"].mean())
        assert share <= 0.15, f"{name} env {e}: {share:.3f} of the image is ambiguous"
        # and the image is a picture of something: several primitives, the nearest of them not the ground alone
        clear = ~img["ambiguous"]
        assert len(np.unique(img["ids"][clear])) >= 3


def test_scenes_cover_every_primitive_type_and_high_nodes():
    seen = set()
    for name in RR.SCENE_NAMES:
        for img in RR.scene_reference(name):
            ids = img["ids"][~img["ambiguous"]]
            seen |= {img["prims"][i]["type"] for i in np.unique(ids[ids >= 0])}
    assert seen == {M.GT_PLANE, M.GT_SPHERE, M.GT_CAPSULE, M.GT_BOX, M.GT_CYLINDER, M.GT_ELLIPSOID, M.GT_CONVEX}
    for name in ("Humanoid", "ShadowHand-block"):
        spec = RR.scene(name)["spec"]
        high = {k for k, g in enumerate(spec.geoms) if g.node >= 16}
        assert high, name
        vis = set()
        for img in RR.scene_reference(name):
            vis |= set(np.unique(img["ids"][~img["ambiguous"]]).tolist())
        assert vis & high, f"{name}: no geom of a node >= 16 is visible"
