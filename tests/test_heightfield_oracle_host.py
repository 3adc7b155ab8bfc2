"""The oracle's heightfield (orc_set_heightfield) pinned on the CPU before it judges a kernel.  None of
these tests runs a kernel: the oracle does not get its credibility from agreeing with one.

  * zero field: orc_simulate_views is bit-equal with and without a field of zeros (n.z is exactly 1 in fp64, so
    (z - 0) 1 - r and e - r (0, 0, 1) are the plane's expressions), PGS and TGS, on linkforce_ref's pools.
  * contact lists: on heightfield_ref.rough_states, O.contacts_full on the field is heightfield_ref.ground_list -- the
    definition in numpy -- plus the oracle's pair contacts, in order, contact for contact to 1e-12 (the candidates'
    points are the oracle's own kinematics, heightfield_ref.oracle_candidates; against the spec's kinematics the
    lists agree to the 2e-7 the plane lists do).
  * the frame argument, turned round: on slope_case's planes the oracle stepped on the sampled field in world
    coordinates agrees with its flat step under R^T g carried back by R, within a tenth of the one-step tolerances.
  * a sphere on one facet tilted by 45 degrees, gradient along x (|n.x| = 0.707: tangent_basis' second branch) and
    along y (the first): it stays with mu > tan t and slides at |g| (sin t - mu cos t) with mu < tan t.
  * a capsule at rest across a V-shaped valley: its two end contacts lie on different facets, the net contact force
    carries the weight and its x components cancel.
"""
import copy
import math

import numpy as np
import pytest

import contacts_ref as CR
import heightfield_ref as HF
import linkforce_ref as LF
import parity_stats as PS
import pyoracle as O
import test_oracle_physics as OP
from migym import model as M


def sides(tgs):
    return "tgs" if tgs else "pgs"


# ------------------------------------------------------------------------------------------------ zero field
@pytest.mark.parametrize("tgs", [False, True], ids=["pgs", "tgs"])
@pytest.mark.parametrize("model", ["Cartpole", "Quadcopter", "T16-free", "Anymal", "AMP"])
def test_zero_field_is_bit_equal_to_the_plane(model, tgs):
    spec, mnp, sp0 = LF.setup(model)
    root, dof, act, tgt, _ = LF.pool(model)
    n = len(root)
    sp = LF.sp_at(sp0, None, 2, tgs)
    rng = np.random.default_rng(3)
    org = np.concatenate([rng.uniform(-1, 1, (n, 2)), np.zeros((n, 1))], 1)
    plane = LF.Host(spec, root, dof, act, tgt).simulate_each(mnp, [sp] * n)
    twin = LF.Host(spec, root, dof, act, tgt).simulate_each(mnp, [sp] * n, fp32=True)
    for fld in (HF.Field(np.zeros((9, 7)), 0.5, -2.0, -1.0), HF.Field(np.zeros((9, 7)), 0.5, -2.0, -1.0, org)):
        # (field_step binds actor e's origin row, env_base = e, for the one-row views it hands over)
        zero = HF.field_step(fld, LF.Host(spec, root, dof, act, tgt), mnp, sp)
        zero32 = HF.field_step(fld, LF.Host(spec, root, dof, act, tgt), mnp, sp, fp32=True)
        for name in ("root", "dof", "sensors", "dof_force", "ncf"):
            np.testing.assert_array_equal(getattr(zero, name), getattr(plane, name), err_msg=name)
            np.testing.assert_array_equal(getattr(zero32, name), getattr(twin, name), err_msg=name + " (fp32 twin)")
    assert np.abs(plane.dof - dof).max() > 0 or np.abs(plane.root - root).max() > 0
    # and the plane is back after the block
    again = LF.Host(spec, root, dof, act, tgt).simulate_each(mnp, [sp] * n)
    np.testing.assert_array_equal(again.root, plane.root)


# ------------------------------------------------------------------------------------------------ contact lists
@pytest.mark.parametrize("origins", [False, True], ids=["world", "origins"])
@pytest.mark.parametrize("model,n", [("T16-free", 67), ("Anymal", 66)])
def test_contact_lists_are_the_definition(model, n, origins):
    base = HF.rough_field()
    rng = np.random.default_rng(83)
    org = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-0.2, 0.2, (n, 1))], 1) if origins else None
    fld = HF.Field(base.H, base.dx, base.x0, base.y0, org)
    spec, mnp, sp, root, dof, _, _ = HF.rough_states(model, n, fld, 61)
    if origins:      # the feet near the ground under them, with the origin's height taken out
        root = np.array(root)
        root[:, 2] -= fld.origins[:, 2]
    half = 0.5 * (fld.nx - 1) * fld.dx
    assert ((np.abs(root[:, 0:2] + (0 if org is None else fld.origins[:, 0:2])) > half).any(1)).sum() >= 3
    roomy = CR.with_max_contacts(sp, 64)
    ground = tilted = pairs = optional = 0
    worst = worst_spec = 0.0
    for e in range(n):
        flat = O.contacts_full(mnp, roomy, root[e], dof[e], 64)                 # no field: the pair contacts
        # every candidate that can touch: those 0.1 m and more above the field's top are far from touching by the definition itself
        o = fld.origin(e)
        cands, rest = HF.oracle_candidates(spec, mnp, sp, root[e], dof[e], fld.hmax - o[2] + 0.1)
        for _, _, pt, r, _, _ in rest:
            h_, n_, _ = HF.facet(fld, pt[0] + o[0], pt[1] + o[1])
            assert (pt[2] - (h_ - o[2])) * n_[2] - r > sp.contact_offset + 0.01
        rows, marks = HF.ground_list(spec, sp, fld, e, root[e], dof[e, :, 0], delta=0.0, cands=cands)
        rspec, mspec = HF.ground_list(spec, sp, fld, e, root[e], dof[e, :, 0], delta=0.0)
        keep = (marks & CR.BAND_OUT) == 0
        optional += int((~keep).sum())
        want = np.concatenate([rows[keep], flat[flat[:, 3] >= 0]])
        with O.heightfield(fld, e):
            got = O.contacts_full(mnp, roomy, root[e], dof[e], 64)
            short = O.contacts(mnp, roomy, root[e], dof[e], 64)
            mk, mm, _ = O.contacts_marks(mnp, roomy, root[e], dof[e], 0.0, 64)
            ph = O.contacts_phases(mnp, roomy, root[e], dof[e], 0.0, 64)
        assert len(got) == len(want) < 64, f"actor {e}: {len(got)} contacts, the definition has {len(want)}"
        np.testing.assert_array_equal(got[:, :4], want[:, :4], err_msg=f"actor {e}: order")
        if len(got):
            worst = max(worst, float(np.abs(got[:, 4:] - want[:, 4:]).max()))
        np.testing.assert_allclose(got[:, 4:], want[:, 4:], atol=1e-12, rtol=0, err_msg=f"actor {e}")
        # the other hooks read the same field
        np.testing.assert_array_equal(mk, got)
        np.testing.assert_array_equal(short[:, 1:8], got[:, 4:11])
        ng = int(keep.sum())
        assert (ph[:ng] == O.PH_GROUND).all() and (ph[ng:] == O.PH_PAIR).all()
        # against the spec's kinematics: away from creases and the threshold, the same list to 2e-7
        if not mspec.any() and not marks.any() and len(rspec) == ng and ng:
            worst_spec = max(worst_spec, float(np.abs(got[:ng, 4:] - rspec[:, 4:]).max()))
        ground, pairs = ground + ng, pairs + len(want) - ng
        tilted += int((np.abs(got[:ng, 9]) < 0.999).sum())
    print(f"{model} origins={origins}: {ground} ground contacts ({tilted} tilted), {pairs} pair contacts, {optional} "
          f"optional rows; worst difference {worst:.3g}, against the spec's kinematics {worst_spec:.3g}")
    assert ground >= n and tilted >= n // 2
    assert worst_spec < 2e-7
    if model == "T16-free":
        assert pairs > 0, "no pair contact follows the ground contacts in any list"


# ------------------------------------------------------------------------------------------------ the frame, turned round
FRAME_CAP = 0.1       # of the one-step tolerances: nine tenths of the GPU test's tolerance stay the kernel's
SLOPES = [(m, tgs, "slope") for m in HF.SLOPE_MODELS for tgs in (False, True)] + \
    [(m, tgs, "facets") for m in ("Quadcopter", "Anymal") for tgs in (False, True)]


@pytest.mark.parametrize("model,tgs,kind", SLOPES)
def test_field_step_is_the_flat_step_in_the_rotated_frame(model, tgs, kind):
    """Measured: DESIGN.md §15"""
    c = HF.slope_case(model, tgs, kind=kind)
    spec, mnp = c["spec"], c["mnp"]
    n = len(c["idx"])
    with O.heightfield(c["fld"]):
        got = LF.Host(spec, c["world"], c["dof"], c["act"], c["tgt"]).simulate_each(mnp, [c["sp"]] * n)
    back = HF.to_flat(c, got, n)
    back.root = HF.quat_close(c["ref"].root[:n].astype(np.float64), back.root)
    worst = {}
    for name, x, y, atol, rtol in LF.outside(spec, back, c["ref"], n):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        worst[name] = float((np.abs(x - y) / (atol + rtol * np.abs(y))).max())
        PS.record(f"field step in the rotated frame[{model}-{sides(tgs)}-{kind}]", name, x, y, atol=atol, rtol=rtol)
    print(f"{model} {sides(tgs)} {kind}: err / tolerance " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= FRAME_CAP, worst


# ------------------------------------------------------------------------------------------------ one tilted facet
G = 9.81
TILT = math.radians(45.0)     # |n| component along the gradient sin 45 = 0.707 >= 0.57735
BIG_I = 1e4                   # kg m^2 on a 1 kg sphere of r = 0.5: it cannot roll (a_roll = g sin t / (1 + I / m r^2))


def ramp(axis, gx=1.0):
    """3 x 3 samples 4 m apart, heights gx * x (axis 0) or gx * y (axis 1): every facet is one plane.  The heights are
    whole numbers, exact in fp32"""
    xs = np.array([-4.0, 0.0, 4.0])
    H = gx * (xs[:, None] + 0 * xs[None, :]) if axis == 0 else gx * (0 * xs[:, None] + xs[None, :])
    return HF.Field(H, 4.0, -4.0, -4.0)


def sphere_on_ramp(axis, mu, u, fp32, steps, iters=64):
    """a 1 kg sphere of r = 0.5 touching the ramp (gap 0) over the world origin, moving down the slope at u; returns
    (root rows after each step (steps, 13), s the unit vector down the slope, n, sp)"""
    r = 0.5
    spec = OP.one_body_spec(M.GT_SPHERE, (r, 0, 0), 1.0, (BIG_I,) * 3)
    sp = OP._params(substeps=2, gravity=(0.0, 0.0, -G), friction=mu, pos_iters=iters)
    n = np.zeros(3)
    n[axis], n[2] = -math.sin(TILT), math.cos(TILT)
    s = np.zeros(3)
    s[axis], s[2] = -math.cos(TILT), -math.sin(TILT)
    root = OP._free_root(r * n, u * s)      # the plane passes through the origin: the centre is r along n
    out = []
    with O.heightfield(ramp(axis)):
        nd = O.contacts_full(M.pack_model(spec), sp, root[0], OP.NO_DOF[0], 8, fp32=fp32)
        assert len(nd) == 1 and abs(nd[0, 10]) < 1e-6 and np.abs(nd[0, 7:10] - n).max() < 1e-6
        for _ in range(steps):
            O.simulate(M.pack_model(spec), sp, root, OP.NO_DOF, fp32=fp32)
            out.append(root[0].astype(np.float64))
    return np.array(out), s, n, sp


@OP.BUILDS
@pytest.mark.parametrize("axis", [0, 1], ids=["along-x", "along-y"])
def test_sphere_slides_down_a_facet_at_the_coulomb_rate(axis, fp32):
    """mu = 0.5 < tan 45: the speed down the slope grows by |g| (sin t - mu cos t) dt per step, nothing across the
    slope and nothing along the normal; the tolerance is test_friction_bound_known_answers'"""
    tol = OP._tol(fp32, 1e-6, 2e-5)
    mu, u = 0.5, 1.0
    rows, s, n, sp = sphere_on_ramp(axis, mu, u, fp32, 1)
    v = rows[0, 7:10]
    a = G * (math.sin(TILT) - mu * math.cos(TILT))
    across = np.cross(n, s)
    print(f"axis {axis} fp32={fp32}: dv down the slope {v @ s - u:.9g}, expected {a * sp.dt:.9g}; across {v @ across:.3g}, "
          f"normal {v @ n:.3g}")
    assert abs((v @ s - u) - a * sp.dt) < tol
    assert abs(v @ across) < tol and abs(v @ n) < tol
    # without friction: |g| sin t
    rows, s, n, sp = sphere_on_ramp(axis, 0.0, u, fp32, 1)
    assert abs((rows[0, 7:10] @ s - u) - G * math.sin(TILT) * sp.dt) < tol


@OP.BUILDS
@pytest.mark.parametrize("axis", [0, 1], ids=["along-x", "along-y"])
def test_sphere_stays_on_a_facet_with_enough_friction(axis, fp32):
    """mu = 1.2 > tan 45: after 200 substeps the sphere has not moved; the bound on the velocities is
    test_dropped_ant_comes_to_rest_on_the_plane's 0.05 (m/s, rad/s), the drift along the facet that speed over the
    time (frictionless it would have slid 0.5 |g| sin t T^2 = 9.6 m)"""
    rows, s, n, sp = sphere_on_ramp(axis, 1.2, 0.0, fp32, 100)
    T = 100 * sp.dt
    x, v = rows[-1, 0:3] - 0.5 * n, rows[-1, 7:13]
    drift = np.linalg.norm(x - (x @ n) * n)
    print(f"axis {axis} fp32={fp32}: drift {drift:.3g} m, |v| {np.abs(v).max():.3g}, height over the facet {x @ n:.3g}")
    assert np.abs(v).max() < 0.05
    assert drift < 0.05 * T
    assert abs(x @ n) < 0.01     # neither sunk nor lifted: within the contact offset's scale


# ------------------------------------------------------------------------------------------------ a V-shaped valley
@OP.BUILDS
@pytest.mark.parametrize("tgs", [False, True], ids=["pgs", "tgs"])
@pytest.mark.parametrize("deg", [20.0, 40.0])
def test_capsule_rests_across_a_valley(deg, tgs, fp32):
    """heights |x| tan t, constant in y; a capsule along x, its ends at x = -+hl on the two sides.  At rest the two end
    contacts lie on different facets (normals (+-sin t, 0, cos t); at 40 degrees |n.x| = 0.64 takes tangent_basis'
    second branch), the net contact force is the weight along z and its x components cancel: within 15 % of m g, and
    the velocities within 0.05, the bounds of test_dropped_ant_comes_to_rest_on_the_plane"""
    t = math.radians(deg)
    r, hl, mass = 0.1, 0.5, 2.0
    spec = OP.one_body_spec(M.GT_CAPSULE, (r, hl, 0), mass, (0.2, 0.2, 0.2))
    spec.geoms[0].quat = [0.0, math.sqrt(0.5), 0.0, math.sqrt(0.5)]      # the capsule's axis (geom z) along world x
    mnp = M.pack_model(spec)
    sp = OP._params(substeps=2, gravity=(0.0, 0.0, -G), friction=1.2, pos_iters=32)
    if tgs:
        sp.solver_type = OP._abi_solver(True)
    fld = HF.Field(np.array([[4 * math.tan(t)] * 3, [0.0] * 3, [4 * math.tan(t)] * 3]), 4.0, -4.0, -4.0)
    h = LF.Host(spec, OP._free_root((0.0, 0.0, r / math.cos(t) + hl * math.tan(t))), OP.NO_DOF)
    with O.heightfield(fld):
        for _ in range(100):
            h.simulate_each(mnp, [sp], fp32=fp32)
        con = O.contacts_full(mnp, sp, h.root[0], OP.NO_DOF[0], 8, fp32=fp32)
    assert len(con) == 2
    nx = np.sort(con[:, 7])
    np.testing.assert_allclose(nx, [-math.sin(t), math.sin(t)], atol=1e-6)
    np.testing.assert_allclose(con[:, 9], math.cos(t), atol=1e-6)
    f = h.ncf[0].astype(np.float64).sum(0)
    print(f"{deg} deg {sides(tgs)} fp32={fp32}: net contact force {f}, weight {mass * G:.4g}, |v| {np.abs(h.root[0, 7:13]).max():.3g}")
    assert np.abs(h.root[0, 7:13]).max() < 0.05
    assert abs(f[2] - mass * G) < 0.15 * mass * G
    assert abs(f[0]) < 0.15 * mass * G and abs(f[1]) < 0.15 * mass * G
    # ... and far tighter than that, the forces are the ones that make the motion: over one more step of a single
    # substep h the net contact force is m (v' - v) / h - m g in every component (the linear momentum of one free
    # body; no other force acts on it).  Bound, relative to m g: the outputs are fp32, so the force is rounded at 6e-8
    # and the resting velocities at less; 1e-6 leaves a factor of ten, and the twin's own fp32 arithmetic (some hundred
    # operations on the way to the force) gets 1e-5
    sp1 = copy.copy(sp)
    sp1.dt, sp1.substeps = sp.dt / sp.substeps, 1
    v0 = h.root[0, 7:10].astype(np.float64)
    with O.heightfield(fld):
        h.simulate_each(mnp, [sp1], fp32=fp32)
    f1 = h.ncf[0].astype(np.float64).sum(0)
    want = mass * (h.root[0, 7:10].astype(np.float64) - v0) / sp1.dt + np.array([0.0, 0.0, mass * G])
    bal = np.abs(f1 - want).max()
    print(f"  momentum balance of the last substep: {bal:.3g} N")
    assert bal < (1e-5 if fp32 else 1e-6) * mass * G
    # at rest the two ends carry the same load: the balance of the forces along x and of the moments about y leaves
    # N1 = N2 (and equal friction) whatever the friction is, up to the residual acceleration (|v| < 0.05 over 100 steps)
    with O.heightfield(fld):
        rows = O.step_rows(mnp, sp1, HF._One(h, 0), 0)
    assert len(rows) == 2 and abs(rows[0, 11] - rows[1, 11]) < 1e-3 * rows[:, 11].max()
