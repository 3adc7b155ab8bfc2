"""Heightfield terrain on the CPU (tests/heightfield_ref.py): the fp64 definitions hold what §15 says
of them, the frame argument holds, and the inputs of tests/test_gpu_heightfield.py are admitted by the reference alone.

  * facet(): a sampled plane is reproduced to 1e-12 inside the grid; the height is continuous across cell edges and
    the diagonal; a flat field has n = z; outside the grid the field is that of the nearest grid point.
  * frame(): R is orthonormal with determinant +1, R z = n, and R carries the flat frame's tangent basis onto n's
    (1e-12, random n with |n.x| < 0.5).
  * slope_case(): at most DISCARD_CAP of the drawn states are passed over by the oracle-decided conditions; the slope
    moves the oracle's own result out of the one-step tolerances (against its flat step under unrotated gravity) in at
    least 90 % of the kept states; the oracle's fp32 twin passes the rule the GPU test applies.
  * rough_case(), chain_case(), terrain_case(): the states stepped on rough ground, on the task's stairs and on a generated
    terrain meet their conditions on the oracle alone -- at most 5 % passed over, used rows on two or more facets in
    at least half of the states, steep rows along x and along y on the stairs in at least a tenth, the field moves the
    oracle's result in at least 90 % -- and the oracle's fp32 twin passes the rule the GPU tests apply.
  * the rough-ground contact sets and the scan points: at most 5 % of a set's contacts are ambiguous and at most 5 % of
    its envs can need an exemption; at most 2 % of the scan points sit in the rounding band.
  * the C ABI: the new symbols are exported, mg_heightfield_sizeof() is the ctypes mirror's, mg_version() is 7, and
    bad arguments fail with their messages (no device needed: the checks come first).
"""
import ctypes as C
import os

import numpy as np
import pytest

import contacts_ref as CR
import heightfield_ref as HF
import linkforce_ref as LF
from migym import _abi


# ------------------------------------------------------------------------------------------------ the facet function
def _plane(a, b, c, nx=9, ny=7, dx=0.5, x0=-1.0, y0=0.5):
    xs, ys = x0 + dx * np.arange(nx), y0 + dx * np.arange(ny)
    Xg, Yg = np.meshgrid(xs, ys, indexing="ij")
    f = HF.Field(np.zeros((nx, ny)), dx, x0, y0)
    f.H = a * Xg + b * Yg + c      # fp64 samples: the property is the facet function's, not the table's rounding
    return f


def test_facet_reproduces_a_sampled_plane():
    rng = np.random.default_rng(1)
    a, b, c = 0.3, -0.2, 0.7
    f = _plane(a, b, c)
    X, Y = rng.uniform(-1.0, 3.0, 4000), rng.uniform(0.5, 3.5, 4000)
    h, n, _ = HF.facet(f, X, Y)
    np.testing.assert_allclose(h, a * X + b * Y + c, atol=1e-12, rtol=0)
    nn = np.array([-a, -b, 1.0]) / np.sqrt(a * a + b * b + 1.0)
    np.testing.assert_allclose(n, np.broadcast_to(nn, n.shape), atol=1e-12, rtol=0)


def test_facet_height_is_continuous_across_edges_and_the_diagonal():
    rng = np.random.default_rng(2)
    f = HF.rough_field(seed=3)
    lo, hi = f.x0, f.x0 + (f.nx - 1) * f.dx
    eps = 1e-9
    # across vertical and horizontal cell edges
    k = rng.integers(1, f.nx - 1, 500)
    t = rng.uniform(lo, hi, 500)
    xe = f.x0 + k * f.dx
    for A, B in (((xe - eps, t), (xe + eps, t)), ((t, xe - eps), (t, xe + eps))):
        ha, hb = HF.facet(f, *A)[0], HF.facet(f, *B)[0]
        assert np.abs(ha - hb).max() < 1e-7      # slope <= 0.16 / 0.25 over 2e-9 m
    # across the diagonal of a cell: the two triangles agree on it
    i, j, s = rng.integers(0, f.nx - 1, 500), rng.integers(0, f.ny - 1, 500), rng.uniform(0.05, 0.95, 500)
    X, Y = f.x0 + (i + s) * f.dx, f.y0 + (j + s) * f.dx
    (hl, _), (hu, _), _ = HF.facet(f, X, Y, both=True)
    np.testing.assert_allclose(hl, hu, atol=1e-12, rtol=0)
    # and the two triangles of a random cell are different planes (the diagonal is a crease)
    (_, nl), (_, nu), _ = HF.facet(f, X, Y, both=True)
    assert np.linalg.norm(nl - nu, axis=-1).min() > 1e-4


def test_flat_field_has_vertical_normals():
    f = HF.Field(np.full((9, 9), 0.37), 0.5, -2.0, -2.0)
    rng = np.random.default_rng(4)
    h, n, _ = HF.facet(f, rng.uniform(-3, 3, 1000), rng.uniform(-3, 3, 1000))
    np.testing.assert_array_equal(n, np.broadcast_to([0.0, 0.0, 1.0], n.shape))
    np.testing.assert_allclose(h, float(np.float32(0.37)), atol=1e-15)


def test_outside_the_grid_the_nearest_grid_point_counts():
    f = HF.rough_field(seed=5)
    lo, hi = f.x0, f.x0 + (f.nx - 1) * f.dx
    rng = np.random.default_rng(6)
    X, Y = rng.uniform(lo - 3, hi + 3, 2000), rng.uniform(lo - 3, hi + 3, 2000)
    h, n, _ = HF.facet(f, X, Y)
    hc, nc, _ = HF.facet(f, np.clip(X, lo, hi), np.clip(Y, lo, hi))
    np.testing.assert_array_equal(h, hc)
    np.testing.assert_array_equal(n, nc)
    assert h.max() <= f.hmax + 1e-12 and ((X < lo) | (X > hi)).sum() > 100
    # far corners: the corner sample itself
    assert HF.facet(f, hi + 10, hi + 10)[0] == pytest.approx(float(f.H[-1, -1]), abs=1e-12)
    assert HF.facet(f, lo - 10, lo - 10)[0] == pytest.approx(float(f.H[0, 0]), abs=1e-12)


# ------------------------------------------------------------------------------------------------ the frame
def test_frame_is_a_rotation_onto_the_normal_and_its_tangent_basis():
    rng = np.random.default_rng(7)
    f1, f2 = HF.tangent_basis([0.0, 0.0, 1.0])
    np.testing.assert_allclose(f1, [0, -1, 0], atol=1e-15)
    np.testing.assert_allclose(f2, [1, 0, 0], atol=1e-15)
    for _ in range(500):
        n = HF.random_normal(rng)
        assert abs(n[0]) < 0.5
        R = HF.frame(n)
        np.testing.assert_allclose(R.T @ R, np.eye(3), atol=1e-12)
        assert np.linalg.det(R) == pytest.approx(1.0, abs=1e-12)
        np.testing.assert_allclose(R @ [0, 0, 1.0], n, atol=1e-12)
        t1, t2 = HF.tangent_basis(n)
        np.testing.assert_allclose(R @ f1, t1, atol=1e-12)
        np.testing.assert_allclose(R @ f2, t2, atol=1e-12)
        q = HF.rot_quat(R)
        from migym import model as M
        np.testing.assert_allclose(M.qmat(M.qnorm(q)), R, atol=1e-12)


def test_plane_field_samples_its_plane():
    rng = np.random.default_rng(8)
    n, p0 = HF.random_normal(rng), np.array([0.3, -0.4, 0.2])
    f = HF.plane_field(n, p0)
    assert f.H.shape == (33, 33) and f.dx == 0.5
    X, Y = rng.uniform(-8, 8, 1000), rng.uniform(-8, 8, 1000)
    h, nn, _ = HF.facet(f, X, Y)
    # the table is fp32: 2^-24 of the largest height on each of the three samples of a facet
    np.testing.assert_allclose(n[0] * (X - p0[0]) + n[1] * (Y - p0[1]) + n[2] * (h - p0[2]), 0, atol=2e-6)
    assert np.linalg.norm(nn - n, axis=-1).max() < 2e-6


# ------------------------------------------------------------------------------------------------ admission: slopes
SLOPES = [(m, tgs, "slope") for m in HF.SLOPE_MODELS for tgs in (False, True)] + \
    [(m, tgs, "facets") for m in ("Quadcopter", "Anymal") for tgs in (False, True)]


@pytest.mark.parametrize("model,tgs,kind", SLOPES)
def test_slope_states_are_admitted(model, tgs, kind):
    c = HF.slope_case(model, tgs, kind=kind)
    spec, mnp, sp0 = c["spec"], c["mnp"], LF.setup(model)[2]
    want = max(LF.BATCHES[model])
    tilt = np.degrees(np.arccos(c["n"][:, 2]))
    assert (np.abs(c["n"][:, 0]) < 0.5).all()
    if kind == "slope":
        assert HF.TILT[0] <= tilt[0] <= HF.TILT[1] and np.ptp(c["n"], axis=0).max() == 0
    else:
        assert len({tuple(np.round(n, 9)) for n in c["n"]}) == min(8, want) and tilt.min() > 1.0
        # every geom, with its bounding radius, projects into the actor's own triangle (the facet under its centre
        # and under the four points a radius away is one facet)
        f = c["fld"]
        for k in range(want):
            for _, _, _, _, bound, ctr in HF.candidates(spec, c["world"][k], c["dof"][k, :, 0]):
                for dx, dy in ((0, 0), (bound, 0), (-bound, 0), (0, bound), (0, -bound)):
                    np.testing.assert_allclose(HF.facet(f, ctr[0] + dx, ctr[1] + dy)[1], c["n"][k], atol=1e-12)
    assert len(c["idx"]) == want and c["cand"] <= sp0.max_contacts
    passed_over = c["scanned"] - want
    assert passed_over <= LF.DISCARD_CAP * c["scanned"], f"{model}: {passed_over} of {c['scanned']} drawn states passed over"
    mv = HF.moved(spec, c["ref"], c["base"], want)
    print(f"{model} {kind} tgs={tgs}: tilt {tilt.min():.1f} .. {tilt.max():.1f} deg, scanned {c['scanned']}, "
          f"moved {int(mv.sum())} / {want}")
    assert mv.sum() >= 0.9 * want, f"{model}: the slope moves the oracle in {int(mv.sum())} of {want}"
    # the actors sit inside the grid, and carried onto the plane and back the states are the flat ones to fp32 rounding
    assert np.abs(c["world"][:, 0:2]).max() < 7.5
    back = HF.to_flat(c, c["ref"].__class__(spec, c["world"], c["dof"]), want).root
    assert np.abs(back[:, 0:3] - c["root"][:, 0:3]).max() < 4e-6
    twin = LF.Host(spec, c["root"], c["dof"], c["act"], c["tgt"]).simulate_each(mnp, c["sps"], fp32=True)
    HF.compare_step(f"test_slope_states_are_admitted[{model}-{tgs}-{kind}]", spec, twin, c["ref"], want)


# ------------------------------------------------------------------------------------------------ admission: rough ground
@pytest.mark.parametrize("model,n", [("T16-free", 67), ("Anymal", 66)])
def test_rough_ground_sets_are_admitted(model, n):
    fld = HF.rough_field()
    spec, mnp, sp, root, dof, _, _ = HF.rough_states(model, n, fld, 61)
    lists = HF.contact_lists(spec, mnp, sp, fld, root, dof)
    reach, marked, ncon = CR.reference_reach(lists)
    half = 0.5 * (fld.nx - 1) * fld.dx
    outside = (np.abs(root[:, 0:2]) > half).any(1).sum()
    print(f"{model}: {ncon} contacts, ambiguous or ill {marked:.3f}, envs with an exemption available {reach:.3f}, "
          f"{outside} actors outside the grid")
    assert ncon >= n and outside >= 3
    assert marked <= 0.05 and reach <= 0.05
    # with H = 0 the definition gives the oracle's own plane list
    zero = HF.Field(np.zeros((9, 9)), 0.5, -2.0, -2.0)
    flat = HF.contact_lists(spec, mnp, sp, zero, root, dof)
    orc = CR.oracle_lists(mnp, CR.with_max_contacts(sp, 64), root, dof)
    for (r, m, _), (ro, mo, _) in zip(flat, orc):
        keep, keepo = (m & CR.BAND_OUT) == 0, (mo & CR.BAND_OUT) == 0
        assert [tuple(x[:4]) for x in r[keep]] == [tuple(x[:4]) for x in ro[keepo]]
        # (the oracle's kinematics run on the packed model's fp32 tables, this reference's on the spec: a few 1e-8 m,
        # far below contacts_ref's bounds of 5e-6)
        np.testing.assert_allclose(r[keep][:, 4:], ro[keepo][:, 4:], atol=2e-7, rtol=0)


# ------------------------------------------------------------------------------------------------ admission: stepped
ROUGH = [(m, tgs, "rough", org) for m in HF.ROUGH_MODELS for tgs in (False, True) for org in (False, True)] + \
    [(m, tgs, "stairs", org) for m in HF.STAIRS_MODELS for tgs in (False, True) for org in (False, True)]


def test_stairs_field_is_the_tasks_stairs():
    f = HF.stairs_field()
    assert f.H.shape == (65, 65) and f.dx == float(np.float32(0.1)) and f.H.max() > 1.0
    d = np.diff(f.H.astype(np.float64), axis=0)
    assert set(np.round(np.unique(d), 6)) == {-0.15, 0.0, 0.15}      # one-cell ramps of gradient 1.5: |n.x| = 0.83
    _, n, _ = HF.facet(f, -3.2 + 0.1 * np.array([2.3, 2.3]), np.array([0.02, 0.0]))
    assert np.abs(n[:, 0]).max() >= HF.STEEP


@pytest.mark.parametrize("model,tgs,kind,origins", ROUGH)
def test_rough_ground_steps_are_admitted(model, tgs, kind, origins):
    """the conditions of a rough_case, on the oracle alone.  Measured: DESIGN.md §15"""
    c = HF.rough_case(model, tgs, kind, origins)
    spec, mnp, sp = c["spec"], c["mnp"], c["sp"]
    want = max(LF.BATCHES[model])
    assert sp.substeps == 2 and len(c["idx"]) == want and c["cand"] <= sp.max_contacts
    assert (c["fld"].origins is not None) == origins
    if model == "T16-free":
        assert len(spec.pairs) > 0       # with its self-collision pairs
    passed_over = c["scanned"] - want
    multi, sx, sy = HF.row_stats(c)
    mv = HF.moved(spec, c["ref"], c["level"], want)
    print(f"{model} {kind} tgs={tgs} origins={origins}: scanned {c['scanned']}, passed over {passed_over} {c['why']}, "
          f"two or more facets {multi.mean():.2f}, steep along x {sx.mean():.2f}, along y {sy.mean():.2f}, "
          f"moved against the level step {mv.mean():.2f}")
    assert passed_over <= LF.DISCARD_CAP * c["scanned"], f"{passed_over} of {c['scanned']} drawn states passed over"
    assert multi.sum() >= 0.5 * want, "the case is only a slope case"
    if kind == "stairs":
        assert sx.sum() >= 0.1 * want and sy.sum() >= 0.1 * want
    assert mv.sum() >= 0.9 * want
    # inside the grid
    xy = c["root"][:, 0:2] + (c["fld"].origins[:, 0:2] if origins else 0)
    assert np.abs(xy).max() < 0.5 * (c["fld"].nx - 1) * c["fld"].dx
    twin = HF.field_step(c["fld"], LF.Host(spec, c["root"], c["dof"], c["act"], c["tgt"]), mnp, sp, fp32=True)
    HF.compare_step(f"test_rough_ground_steps_are_admitted[{model}-{tgs}-{kind}-{origins}]", spec, twin, c["ref"], want)


@pytest.mark.parametrize("model,tgs", [(m, tgs) for m in ("T16-free", "Anymal") for tgs in (False, True)])
def test_chained_launches_are_admitted(model, tgs):
    """four launches on the rough field, each from the last one's output, with the oracle's fp32 twin in the kernel's
    place: per launch at most 5 % of the states fail the admission, and the twin passes the one-step rule on the rest"""
    c = HF.rough_case(model, tgs)
    chain = HF.chain_case(model, tgs)
    assert len(chain) == 4
    for k, (inp, ref, ok) in enumerate(chain):
        n = inp.n
        print(f"{model} tgs={tgs} launch {k}: {int((~ok).sum())} of {n} states not admitted")
        assert (~ok).sum() <= LF.DISCARD_CAP * n
        twin = HF.field_step(c["fld"], LF.Host(c["spec"], inp.root, inp.dof, c["act"], c["tgt"]), c["mnp"], c["sp"], fp32=True)
        keep = np.flatnonzero(ok)
        HF.compare_step(f"test_chained_launches_are_admitted[{model}-{tgs}-{k}]", c["spec"], HF.take(twin, keep),
                        HF.take(ref, keep), len(keep))
        if k:
            assert np.abs(inp.root - chain[k - 1][0].root).max() > 1e-5     # the chain moves


@pytest.mark.parametrize("origins", [False, True], ids=["world", "origins"])
def test_terrain_physics_case_is_admitted(origins):
    """AnymalTerrain's physics on a generated terrain, the oracle's fp32 twin in the kernel's place: four launches, the
    efforts recomputed by the restatement's PD law before each, each compared with the fp64 oracle restarted from the
    same state -- the rule and the 5 % cap of the GPU test -- and the placement is what it says"""
    import types
    import anymal_terrain_ref as R
    c = HF.terrain_case(origins)
    n, fld = c["n"], c["fld"]
    assert fld.H.shape == (560, 800) and sorted(set(c["col"])) == sorted(HF.TERRAIN_COLS)
    xy = c["root"][:, 0:2] + (fld.origins[:, 0:2] if origins else 0)
    _, nrm, _ = HF.facet(fld, xy[:, 0], xy[:, 1])
    assert (np.abs(c["root"][:, 0:2]).max() < 4.0) == origins
    root, dof = c["root"], c["dof"]
    steep = 0
    for k in range(4):
        _, eff = R.pre_step(c["p"], c["actions"], dof)
        twin = HF.field_step(fld, LF.Host(c["spec"], root, dof, eff), c["mnp"], c["sp"], fp32=True)
        got = types.SimpleNamespace(root=twin.root, dof=twin.dof, ncf=twin.ncf)
        HF.terrain_compare(f"test_terrain_physics_case_is_admitted[{origins}-launch {k}]", c, got, root, dof, eff)
        rows = HF.field_rows(fld, LF.Host(c["spec"], root, dof, eff), c["mnp"], c["sp"])
        steep += sum(bool((np.abs(r[(r[:, 3] == -1) & (r[:, 11] > 1e-9)][:, 7:9]) >= HF.STEEP).any()) for r in rows)
        root, dof = twin.root, twin.dof
    print(f"origins={origins}: {steep} env-launches use a ground row with |n.x| or |n.y| >= {HF.STEEP}")
    assert steep >= 4


def test_scan_points_outside_the_rounding_band():
    fld = HF.rough_field()
    pts = HF.scan_points()
    assert pts.shape == (140, 2)
    rng = np.random.default_rng(71)
    root = HF.scan_roots(rng, 67, fld)
    for org in (None, HF.scan_origins(rng, 67)):
        f = HF.Field(fld.H, fld.dx, fld.x0, fld.y0, org)
        out, alts, band = HF.scan(f, root, pts)
        assert band.mean() <= 0.02, f"{band.mean():.4f} of the points in the band"
        assert out.shape == (67, 140) and np.unique(out).size > 50


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.fail("libmigym.so is not built (python __graft_entry__.py build)")
    return _abi.lib()


def test_heightfield_symbols_and_layout(lib):
    for name in ("mg_heightfield_sizeof", "mg_sim_set_heightfield", "mg_height_scan"):
        assert name in _abi.EXPORTS and hasattr(lib, name)
    assert lib.mg_heightfield_sizeof() == C.sizeof(_abi.Heightfield) == 40
    assert lib.mg_version() == 7


def test_heightfield_bad_arguments_fail_with_messages(lib):
    hf = _abi.Heightfield()
    assert lib.mg_sim_set_heightfield(None, C.byref(hf)) != 0 and b"mg_sim_set_heightfield" in lib.mg_last_error()
    assert lib.mg_height_scan(None, None, 0, None, None) != 0 and b"mg_height_scan" in lib.mg_last_error()
    # the field's own checks come before the sim's, so they show without a device
    dummy = (C.c_float * 4)()
    good = dict(heights=C.addressof(dummy), nx=2, ny=2, dx=0.5, x0=0.0, y0=0.0, hmax=0.0)
    for change, msg in ((dict(heights=None), b"heights is NULL"), (dict(nx=1), b"at least 2"), (dict(ny=0), b"at least 2"),
                        (dict(dx=0.0), b"dx must be finite and positive"), (dict(dx=-1.0), b"dx must be"),
                        (dict(dx=float("nan")), b"dx must be"), (dict(dx=float("inf")), b"dx must be")):
        hf = _abi.Heightfield(**{**good, **change})
        assert lib.mg_sim_set_heightfield(None, C.byref(hf)) != 0
        assert msg in lib.mg_last_error(), (change, lib.mg_last_error())
    hf = _abi.Heightfield(**good)
    assert lib.mg_sim_set_heightfield(None, C.byref(hf)) != 0 and b"sim is NULL" in lib.mg_last_error()
