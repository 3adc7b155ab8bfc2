"""Heightfield terrain on the CPU (tests/heightfield_ref.py): the fp64 definitions hold what §15 says
of them, the frame argument holds, and the inputs of tests/test_gpu_heightfield.py are admitted by the reference alone.

  * facet(): a sampled plane is reproduced to 1e-12 inside the grid; the height is continuous across cell edges and
    the diagonal; a flat field has n = z; outside the grid the field is that of the nearest grid point.
  * frame(): R is orthonormal with determinant +1, R z = n, and R carries the flat frame's tangent basis onto n's
    (1e-12, random n with |n.x| < 0.5).
  * slope_case(): at most DISCARD_CAP of the drawn states are passed over by the oracle-decided conditions; the slope
    moves the oracle's own result out of the one-step tolerances (against its flat step under unrotated gravity) in at
    least 90 % of the kept states; the oracle's fp32 twin passes the rule the GPU test applies.
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
