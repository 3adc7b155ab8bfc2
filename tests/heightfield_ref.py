"""Heightfield terrain (mg_sim_set_heightfield, mg_height_scan): the definitions in fp64 numpy and the
state sets shared by tests/test_heightfield_host.py (the reference alone, on the CPU) and tests/test_gpu_heightfield.py.

  * facet(): the facet under a world point, as DESIGN.md §15 defines it (clamp, cell, the diagonal split, the normal).
  * frame(): the rotation R = [t2 | -t1 | n] of a unit normal n, built from the kernels' tangent basis.  A step on the
    plane through p0 with normal n under gravity g is the frozen oracle's flat step under gravity R^T g, tangent basis
    included, so the oracle verifies a planar slope by running in the frame R^T: slope_case() draws the states in the
    flat frame (linkforce_ref's pools: the quadcopter in flight, the T16-free tree off the ground, Anymal standing, the
    AMP humanoid on its feet), the kernel gets them carried onto the slope (position R x + p0, orientation q(R) q,
    velocities turned by R) over a field that samples the plane, and its outputs are carried back by R^T.  DOF state,
    DOF forces and sensors are body-frame and stay; net contact forces are env-frame vectors and turn with R.
  * ground_lists(): the ground contacts of a state on any field straight from the definition (candidates in
    collide()'s emission order: sphere centre, capsule ends, box corners), with contacts_ref's marks for the threshold
    band and for candidates next to a cell edge or diagonal; contacts between geoms come from the oracle's own list.
  * scan(): mg_height_scan's rule.
  * rough_case(), chain_case(), terrain_case(): states stepped on a field that is no plane -- the rough field, the
    task's stairs, a generated AnymalTerrain terrain -- against the oracle on the same field (pyoracle.set_heightfield;
    pinned on the CPU by tests/test_heightfield_oracle_host.py), admitted by the oracle alone.
"""
import copy

import numpy as np

import contacts_ref as CR
import dynamics_ref as DR
import linkforce_ref as LF
import parity_stats as PS
import pyoracle as O
import tree_physics_ref as TP
from migym import model as M

F = np.float32
_cache = {}
SLOPE_MODELS = ("Quadcopter", "T16-free", "Anymal", "AMP")
TILT = (5.0, 25.0)          # degrees
EDGE_EPS = 1e-5             # of a cell: a candidate this close to a cell edge or diagonal may take either facet
SCAN_BAND = 1e-4            # cells: a scan point this close to a cell boundary may take either neighbour


# ------------------------------------------------------------------------------------------------ the field
class Field:
    """H (nx, ny) fp32 at world (x0 + i dx, y0 + j dx); origins (n, 3) or None"""

    def __init__(self, H, dx, x0=0.0, y0=0.0, origins=None):
        self.H = np.ascontiguousarray(H, F)
        self.nx, self.ny = self.H.shape
        self.dx, self.x0, self.y0 = float(F(dx)), float(F(x0)), float(F(y0))
        self.origins = None if origins is None else np.ascontiguousarray(origins, F)
        self.hmax = float(self.H.max())

    def origin(self, e):
        return np.zeros(3) if self.origins is None else self.origins[e].astype(np.float64)


def facet(fld, X, Y, both=False):
    """(h, n, (i, j, fu, fv)) of the facet under world (X, Y), fp64, any shape.  both: (lower, upper) triangle results"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    H = fld.H.astype(np.float64)
    X = np.clip(X, fld.x0, fld.x0 + (fld.nx - 1) * fld.dx)
    Y = np.clip(Y, fld.y0, fld.y0 + (fld.ny - 1) * fld.dx)
    u, v = (X - fld.x0) / fld.dx, (Y - fld.y0) / fld.dx
    i = np.minimum(np.floor(u).astype(int), fld.nx - 2)
    j = np.minimum(np.floor(v).astype(int), fld.ny - 2)
    fu, fv = u - i, v - j
    h00, h10, h01, h11 = H[i, j], H[i + 1, j], H[i, j + 1], H[i + 1, j + 1]

    def tri(lower):
        if lower:    # fu >= fv
            h, gx, gy = h00 + (h10 - h00) * fu + (h11 - h10) * fv, (h10 - h00) / fld.dx, (h11 - h10) / fld.dx
        else:
            h, gx, gy = h00 + (h11 - h01) * fu + (h01 - h00) * fv, (h11 - h01) / fld.dx, (h01 - h00) / fld.dx
        n = np.stack([-gx, -gy, np.ones_like(gx)], -1) / np.sqrt(gx * gx + gy * gy + 1.0)[..., None]
        return h, n
    if both:
        return tri(True), tri(False), (i, j, fu, fv)
    (hl, nl), (hu, nu) = tri(True), tri(False)
    low = fu >= fv
    return np.where(low, hl, hu), np.where(low[..., None], nl, nu), (i, j, fu, fv)


# ------------------------------------------------------------------------------------------------ the frame
def tangent_basis(n):
    """tangent_basis_t (team_physics.hpp) in fp64"""
    n = np.asarray(n, np.float64)
    a = np.array([1.0, 0, 0]) if abs(n[0]) < 0.57735 else np.array([0, 1.0, 0])
    t = np.cross(a, n)
    t1 = t / np.linalg.norm(t)
    return t1, np.cross(n, t1)


def frame(n):
    """R = [t2 | -t1 | n] for |n.x| < 0.57735: a proper rotation with R z = n that carries the flat frame's tangent
    basis ((0, -1, 0), (1, 0, 0)) onto n's"""
    t1, t2 = tangent_basis(n)
    return np.stack([t2, -t1, np.asarray(n, np.float64)], 1)


def rot_quat(R):
    """xyzw quaternion of a rotation matrix (w > 0 here: tilts below 90 degrees)"""
    w = 0.5 * np.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 1e-300))
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def carry_root(R, p0, root):
    """root rows (n, 13) carried by x -> R x + p0 (fp64)"""
    root = np.asarray(root, np.float64)
    out = root.copy()
    q = rot_quat(R)
    out[:, 0:3] = root[:, 0:3] @ R.T + p0
    out[:, 3:7] = [M.qnorm(M.qmul(q, M.qnorm(r))) for r in root[:, 3:7]]
    out[:, 7:10], out[:, 10:13] = root[:, 7:10] @ R.T, root[:, 10:13] @ R.T
    return out


def random_normal(rng):
    while True:
        t, ph = np.radians(rng.uniform(*TILT)), rng.uniform(-np.pi, np.pi)
        n = np.array([np.sin(t) * np.cos(ph), np.sin(t) * np.sin(ph), np.cos(t)])
        if abs(n[0]) < 0.5:
            return n


def plane_field(n, p0, nx=33, dx=0.5):
    """the field that samples the plane through p0 with normal n on an nx x nx grid centred on the origin"""
    x0 = -0.5 * (nx - 1) * dx
    xs = x0 + dx * np.arange(nx)
    Xg, Yg = np.meshgrid(xs, xs, indexing="ij")
    return Field(p0[2] - (n[0] * (Xg - p0[0]) + n[1] * (Yg - p0[1])) / n[2], dx, x0, x0)


def gravity_sp(sp, g, substeps=None, tgs=False):
    sp = LF.sp_at(sp, None, substeps, tgs)
    for i in range(3):
        sp.gravity[i] = F(g[i])
    return sp


def facet_field(seed=47):
    """3 x 3 samples 8 m apart with random heights: eight triangles, eight distinct planes"""
    rng = np.random.default_rng(seed)
    return Field(rng.uniform(-1.0, 1.0, (3, 3)), 8.0, -8.0, -8.0)


def facet_plane(fld, k):
    """(n, p0) of triangle k of facet_field(): cell (k // 2) % 2, k // 4, lower / upper by k % 2; p0 its centroid"""
    i, j, low = (k // 2) % 2, k // 4, k % 2 == 0
    fu, fv = (2.0 / 3, 1.0 / 3) if low else (1.0 / 3, 2.0 / 3)
    X, Y = fld.x0 + (i + fu) * fld.dx, fld.y0 + (j + fv) * fld.dx
    h, n, _ = facet(fld, X, Y)
    return np.asarray(n), np.array([X, Y, float(h)])


def plane_setup(model):
    """LF.setup(model), the T16-free tree without its self-collision pairs.  The frame argument covers the ground
    contacts: their normal is R z and tangent_basis_t of it is R's image of the flat basis.  A contact between two
    geoms has any normal, and tangent_basis_t(R n) is not R tangent_basis_t(n) (the basis is built from the world's
    x or y axis), so the friction rows of such a contact are not the flat step's rows turned: the oracle itself is not
    invariant there.  13 % of the tree's admitted pool states carry such a contact before or after the step (none of
    the other three models' do), more than the 5 % that may be passed over, so the recipe drops the pairs instead."""
    spec, mnp, sp = LF.setup(model)
    if model == "T16-free":
        if ("plane setup", model) not in _cache:
            s2 = copy.deepcopy(spec)
            s2.pairs = []
            _cache["plane setup", model] = s2, M.pack_model(s2), sp
        return _cache["plane setup", model]
    return spec, mnp, sp


def nudged(host, rng):
    """the host with every position moved by +-SENS_EPS (an fp32 step's rounding; one draw of the signs), in place"""
    host.root[:, 0:3] += TP.SENS_EPS * rng.choice([-1.0, 1.0], (host.n, 3))
    host.dof[..., 0] += TP.SENS_EPS * rng.choice([-1.0, 1.0], host.dof[..., 0].shape)
    return host


def insensitive(nud, ref):
    """per state: the oracle's step from the nudged state stays within a quarter of the one-step tolerances of its step
    from the state itself (tree_physics_ref.states' criterion)"""
    return ~(PS.env_bad(nud.dof[..., 0], ref.dof[..., 0], 0.25 * 2e-4, 0) |
             PS.env_bad(nud.dof[..., 1], ref.dof[..., 1], 0.25 * 2e-3, 0.25 * 2e-3) |
             PS.env_bad(nud.root[:, 0:7], ref.root[:, 0:7], 0.25 * 2e-4, 0) |
             PS.env_bad(nud.root[:, 7:13], ref.root[:, 7:13], 0.25 * 2e-3, 0.25 * 2e-3))


def admit_on_field(spec, mnp, sp, fld, root, dof, act, tgt, rng):
    """(the fp64 oracle's Host after one step on the field, admitted per state, why, candidates, flags): the one
    admission rule of the stepped-field cases, the oracle's alone -- contact candidates within capacity before and
    after the step, no orc_step_flips flag (the field's bits 256 / 512 / 1024 included), finite, and insensitive()"""
    mk = lambda: LF.Host(spec, root, dof, act, tgt)    # noqa: E731
    ref = field_step(fld, mk(), mnp, sp)
    cand = np.maximum(field_candidates(fld, mnp, sp, root, dof), field_candidates(fld, mnp, sp, ref.root, ref.dof))
    flags = field_flags(fld, mk(), mnp, sp)
    ok = (cand <= sp.max_contacts) & (flags == 0) & np.isfinite(ref.root).all(1)
    why = {"capacity": int((cand > sp.max_contacts).sum()), "flags": int((flags != 0).sum())}
    ok &= insensitive(field_step(fld, nudged(mk(), rng), mnp, sp), ref)
    why["all"] = int((~ok).sum())
    return ref, ok, why, cand, flags


def slope_case(model, tgs, substeps=2, kind="slope"):
    """The admitted states of (model, solver) on planes, as LF.case.  kind "slope": one plane for the case, random tilt
    and direction, sampled by a 33 x 33 field; kind "facets": actor e on triangle e % 8 of facet_field(), its root over
    the triangle's centroid.  Keys: idx, scanned, the flat-frame inputs root / dof / act / tgt, n / p0 / R per actor,
    fld, world (the root rows on the planes), sp (the kernel's: gravity g), sps (the oracle's, per actor: gravity
    R^T g), ref (the fp64 oracle's Host in the flat frames under R^T g), base (the same under g), cand."""
    key = (kind, model, tgs, substeps)
    if key in _cache:
        return _cache[key]
    spec, mnp, sp0 = plane_setup(model)
    root, dof, act, tgt, _ = LF.pool(model)
    nn = len(root)
    rng = np.random.default_rng([41, SLOPE_MODELS.index(model), int(tgs)])
    if kind == "slope":
        nrm = random_normal(rng)
        p0 = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.5, 0.5)])
        fld = plane_field(nrm, p0)
        ns, p0s = np.tile(nrm, (nn, 1)), np.tile(p0, (nn, 1))
    else:
        fld = facet_field()
        ns, p0s = (np.array(x) for x in zip(*[facet_plane(fld, e % 8) for e in range(nn)]))
        root = np.array(root)
        root[:, 0:2] = 0.0       # the flat world does not change under a shift: every root over its triangle's centroid
    Rs = np.array([frame(n) for n in ns])
    sp = LF.sp_at(sp0, None, substeps, tgs)
    g = np.array([sp.gravity[i] for i in range(3)], np.float64)
    sps = [gravity_sp(sp0, Rs[e].T @ g, substeps, tgs) for e in range(nn)]
    ref = LF.Host(spec, root, dof, act, tgt).simulate_each(mnp, sps)
    base = LF.Host(spec, root, dof, act, tgt).simulate_each(mnp, [sp] * nn)
    cands = lambda r, d: np.array([len(O.contacts(mnp, sps[e], r[e], d[e], 96)) for e in range(nn)])    # noqa: E731
    before, after = cands(root, dof), cands(ref.root, ref.dof)
    pre = LF.Host(spec, root, dof, act, tgt)
    ok = (np.maximum(before, after) <= sp.max_contacts) & (pre.flags_each(mnp, sps) == 0) & np.isfinite(ref.root).all(1)
    r2 = np.random.default_rng([43, SLOPE_MODELS.index(model)])
    nud = nudged(LF.Host(spec, root, dof, act, tgt), r2).simulate_each(mnp, sps)
    ok &= insensitive(nud, ref)
    want = max(LF.BATCHES[model])
    idx = np.flatnonzero(ok)[:want]
    assert len(idx) == want, f"{model}: the pool admits only {len(idx)} of the {want} states"
    pick = lambda x: None if x is None else np.ascontiguousarray(x[idx])    # noqa: E731
    # no admitted state carries a contact between geoms (plane_setup)
    for e in idx:
        for r, d in ((root[e], dof[e]), (ref.root[e], ref.dof[e])):
            assert not (O.contacts_full(mnp, sps[e], r, d, 64)[:, 3] >= 0).any(), f"{model}: state {e} has a pair contact"
    out = dict(spec=spec, mnp=mnp, idx=idx, scanned=int(idx[-1]) + 1, root=pick(root), dof=pick(dof), act=pick(act), tgt=pick(tgt), n=ns[idx],
               p0=p0s[idx], R=Rs[idx], fld=fld, sp=sp, sps=[sps[e] for e in idx],
               cand=int(np.maximum(before, after)[idx].max()))
    out["world"] = np.concatenate([carry_root(out["R"][k], out["p0"][k], out["root"][k:k + 1])
                                   for k in range(want)]).astype(F)
    for k, src in (("ref", ref), ("base", base)):
        h = LF.Host(spec, out["root"], out["dof"], out["act"], out["tgt"])
        for name in ("root", "dof", "sensors", "dof_force", "ncf"):
            getattr(h, name)[:] = getattr(src, name)[idx]
        out[k] = h
    _cache[key] = out
    return out


def to_flat(c, got, n):
    """the kernel's outputs on the planes carried back into the oracle's flat frames (a copy; fp64 rows)"""
    import types
    root = np.concatenate([carry_root(c["R"][k].T, -c["R"][k].T @ c["p0"][k], got.root[k:k + 1]) for k in range(n)])
    ncf = np.einsum("kbi,kij->kbj", got.ncf[:n].astype(np.float64), c["R"][:n])
    return types.SimpleNamespace(root=root, dof=got.dof[:n], sensors=got.sensors[:n], dof_force=got.dof_force[:n], ncf=ncf)


def quat_close(a, b):
    """b with the sign of each quaternion row chosen nearest to a's (q and -q are one orientation)"""
    b = np.array(b, np.float64)
    s = np.sign(np.sum(a[:, 3:7] * b[:, 3:7], axis=1))
    b[:, 3:7] *= np.where(s == 0, 1.0, s)[:, None]
    return b


def compare_step(test, spec, got, ref, n):
    """the one-step rule (LF.outside) on n envs; returns per check the largest |err| / (atol + rtol |ref|)"""
    import types
    for x in (got.root, got.dof, got.dof_force, got.ncf):
        assert np.isfinite(np.asarray(x)).all(), f"{test}: not finite"
    refn = types.SimpleNamespace(root=quat_close(np.asarray(got.root, np.float64), ref.root[:n]), dof=ref.dof[:n],
                                 sensors=ref.sensors[:n], dof_force=ref.dof_force[:n], ncf=ref.ncf[:n])
    bad, worst = np.zeros(n, bool), {}
    for name, x, y, atol, rtol in LF.outside(spec, got, refn, n):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        eb = PS.env_bad(x, y, atol, rtol)
        ratio = float((np.abs(x - y) / (atol + rtol * np.abs(y))).max())
        print(f"{test} {name}: max err {np.abs(x - y).max():.3g} (atol {atol:.3g}, rtol {rtol:.3g}), "
              f"err / tolerance {ratio:.3g}, envs outside {int(eb.sum())} / {n}")
        PS.record(test, name, x, y, envs_outside=int(eb.sum()), atol=atol, rtol=rtol)
        worst[name] = ratio
        bad |= eb
    assert not bad.any(), f"{test}: envs {np.flatnonzero(bad)[:10].tolist()} leave the one-step tolerances"
    return worst


def moved(spec, a, b, n):
    bad = np.zeros(n, bool)
    for _, x, y, atol, rtol in LF.outside(spec, a, b, n):
        bad |= PS.env_bad(x[:n], y[:n], atol, rtol)
    return bad


# ------------------------------------------------------------------------------------------------ contact lists
def rough_field(seed=51, nx=17, dx=0.25, amp=0.08, origins=None):
    rng = np.random.default_rng(seed)
    x0 = -0.5 * (nx - 1) * dx
    return Field(rng.uniform(-amp, amp, (nx, nx)), dx, x0, x0, origins)


def candidates(spec, root13, q):
    """[(geom, node, e (3), r, bound)] of a state's ground candidates in collide()'s emission order (fp64)"""
    Rn, xn = DR.node_frames(spec, root13, q)
    out = []
    for gi, g in enumerate(spec.geoms):
        if not (g.filter & 1):
            continue
        Rg = Rn[g.node] @ M.qmat(M.qnorm(g.quat))
        c = xn[g.node] + Rn[g.node] @ np.asarray(g.pos, np.float64)
        s = [float(F(x)) for x in g.size]
        if g.gtype == M.GT_SPHERE:
            pts, r, bound = [c], s[0], s[0]
        elif g.gtype == M.GT_CAPSULE:
            ax = Rg[:, 2] * s[1]
            pts, r, bound = [c - ax, c + ax], s[0], s[0] + s[1]
        elif g.gtype == M.GT_BOX:
            pts = [c + Rg @ np.array([(1 if k & 1 else -1) * s[0], (1 if k & 2 else -1) * s[1], (1 if k & 4 else -1) * s[2]])
                   for k in range(8)]
            r, bound = 0.0, float(np.linalg.norm(s[:3]))
        elif g.gtype == M.GT_CONVEX:
            raise NotImplementedError("heightfield_ref: no hull geoms in these models")
        else:
            continue     # cylinders (the quadcopter's rotors): collide() has no ground candidates for them
        for e in pts:
            out.append((gi, g.node, e, r, bound, c))
    return out


def oracle_candidates(spec, mnp, sp, root13, dof2, zmax):
    """(cands, rest): candidates() with the points of the oracle's own kinematics (the packed model's fp32 tables;
    candidates() runs on the spec, a few 1e-8 m away).  The oracle's plane list -- no field set -- at contact offset
    zmax gives every candidate whose lowest point e.z - r is below zmax, in emission order, as p = e - r z (its list
    ends at 64 entries, fewer than the tree's box corners, hence the height); rest: candidates()'s other entries"""
    big = copy.copy(sp)
    big.contact_offset = zmax
    rows = O.contacts_full(mnp, big, root13, dof2, 64)
    rows = rows[rows[:, 2] == -1]
    assert len(rows) < 64        # (the pair contacts that follow may be cut: they are not read here)
    ref = candidates(spec, root13, dof2[:, 0])
    out, k = [], 0
    for row in rows:
        g = spec.geoms[int(row[1])]
        r = float(F(g.size[0])) if g.gtype in (M.GT_SPHERE, M.GT_CAPSULE) else 0.0
        e = row[4:7] + np.array([0.0, 0.0, r])
        while not (ref[k][0] == int(row[1]) and np.abs(ref[k][2] - e).max() < 1e-6):     # the same candidate: in order
            k += 1
        out.append((ref[k][0], ref[k][1], e, r, ref[k][4], ref[k][5], k))
        k += 1
    used = {c[6] for c in out}
    return [c[:6] for c in out], [c for i, c in enumerate(ref) if i not in used]


def ground_list(spec, sp, fld, env, root13, q, delta=CR.DELTA, cands=None):
    """(rows, marks) of one actor's ground contacts on the field by DESIGN.md §15, thresholds moved out by delta as
    orc_contacts_marks does: BAND_IN / BAND_OUT for a gap within delta of contact_offset; AMB for a candidate within
    EDGE_EPS cells of a cell edge or the diagonal whose other facet puts the gap on the other side of the threshold (or
    which is inside the band on either facet), ILL where it lies that close to a crease at all (its normal and point
    may be either facet's).  cands: the candidates, where they are not candidates()'s (oracle_candidates())"""
    off, o = float(sp.contact_offset), fld.origin(env)
    rows, marks = [], []
    for gi, node, e, r, bound, c in (candidates(spec, root13, q) if cands is None else cands):
        X, Y = e[0] + o[0], e[1] + o[1]
        h, n, (i, j, fu, fv) = facet(fld, X, Y)
        d = (e[2] - (h - o[2])) * n[2] - r
        # next to a crease: the diagonal, or a cell edge with another cell behind it (at the rim of the grid, where the
        # clamp puts every point outside, there is none)
        near = min(abs(fu - fv), fu if i > 0 else 1.0, fv if j > 0 else 1.0, 1.0 - fu if i < fld.nx - 2 else 1.0,
                   1.0 - fv if j < fld.ny - 2 else 1.0) < EDGE_EPS
        mark = 0
        ds = [d]
        if near:     # the facets of the neighbouring cells / the other triangle at points nudged across the crease
            for ddx, ddy in ((2, 0), (-2, 0), (0, 2), (0, -2), (2, -2), (-2, 2)):
                h2, n2, _ = facet(fld, X + ddx * EDGE_EPS * fld.dx, Y + ddy * EDGE_EPS * fld.dx)
                ds.append((e[2] - (h2 - o[2])) * n2[2] - r)
            mark |= CR.ILL
            if (min(ds) < off - delta) != (max(ds) < off - delta) or (min(ds) < off + delta) != (max(ds) < off + delta):
                mark |= CR.AMB
        if not (d < off + delta):
            if not (mark & CR.AMB and min(ds) < off + delta):
                continue
            mark |= CR.BAND_OUT
        elif not (d < off - delta):
            mark |= CR.BAND_IN
        if mark & CR.AMB:
            mark |= CR.BAND_IN if not (mark & CR.BAND_OUT) else 0
        p = e - r * n
        rows.append([node, gi, -1, -1, *p, *n, d])
        marks.append(mark)
    return np.array(rows, np.float64).reshape(-1, 11), np.array(marks, np.int32)


def contact_lists(spec, mnp, sp, fld, root, dof):
    """per actor (rows, marks, False) on the field: the ground contacts of ground_list(), then the contacts between
    geoms from the oracle's own list (they do not see the ground; taken with room for every candidate)"""
    roomy = CR.with_max_contacts(sp, 64)
    out = []
    for e in range(len(root)):
        rows, marks = ground_list(spec, sp, fld, e, root[e], dof[e, :, 0])
        r, m, _ = O.contacts_marks(mnp, roomy, root[e], dof[e], CR.DELTA, 64)
        pair = r[:, 3] >= 0
        out.append((np.concatenate([rows, r[pair]]), np.concatenate([marks, m[pair]]), False))
    return out


def cut_lists(lists, cap):
    """the first cap entries of each list at the thresholds themselves (with its band entries kept optional)"""
    out = []
    for rows, marks, lost in lists:
        real = np.cumsum((marks & CR.BAND_OUT) == 0)
        keep = real <= cap
        out.append((rows[keep], marks[keep], lost))
    return out


def rough_states(model, n, fld, seed):
    """n states of the model dropped at random xy over (and past) the field, feet near the ground under them"""
    spec, mnp, sp = LF.setup(model)
    root, dof, act, tgt, _ = LF.pool(model)
    rng = np.random.default_rng(seed)
    root, dof = np.array(root[:n], F), np.array(dof[:n], F)
    half = 0.5 * (fld.nx - 1) * fld.dx
    root[:, 0:2] = rng.uniform(-1.15 * half, 1.15 * half, (n, 2))
    # past one side of the grid, not past a corner: there both coordinates are clamped, every candidate sits on the
    # corner cell's diagonal, and all of them would carry the crease mark (3 of 67 actors: 5.2 % of the tree's contacts)
    corner = (np.abs(root[:, 0]) > half) & (np.abs(root[:, 1]) > half)
    root[corner, 1] *= 0.7
    if model == "T16-free":
        root[:, 2] -= 0.5    # back down: linkforce_ref raised the tree off the ground
    root[:, 2] += rng.uniform(-0.05, 0.05, n)
    return spec, mnp, sp, root, dof, (None if act is None else act[:n]), (None if tgt is None else tgt[:n])


# ------------------------------------------------------------------------------------------------ the height scan
def scan_points():
    """the reference's measured points (anymal_terrain.py init_height_points): 14 x 10 on a 0.1 m grid"""
    y = 0.1 * np.array([-5, -4, -3, -2, -1, 1, 2, 3, 4, 5], np.float64)
    x = 0.1 * np.array([-8, -7, -6, -5, -4, -3, -2, 2, 3, 4, 5, 6, 7, 8], np.float64)
    gx, gy = np.meshgrid(x, y, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], -1).astype(F)


def scan(fld, root, points):
    """(out (n, P) fp32, alt, band): mg_height_scan's rule in fp64 on the fp32 inputs; band marks points whose cell
    coordinate is within SCAN_BAND of an integer, alt their value in the neighbouring cell(s) (a list of arrays)"""
    root, pts = np.asarray(root, np.float64), np.asarray(points, np.float64)
    n = len(root)
    q = np.stack([root[:, 5], root[:, 6]], -1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    z, w = q[:, 0:1], q[:, 1:2]
    c, s = w * w - z * z, 2.0 * w * z
    org = np.zeros((n, 3)) if fld.origins is None else fld.origins.astype(np.float64)
    X = c * pts[None, :, 0] - s * pts[None, :, 1] + root[:, 0:1] + org[:, 0:1]
    Y = s * pts[None, :, 0] + c * pts[None, :, 1] + root[:, 1:2] + org[:, 1:2]
    u, v = (X - fld.x0) / fld.dx, (Y - fld.y0) / fld.dx
    H = fld.H

    def at(u, v):
        i = np.clip(np.trunc(u).astype(int), 0, fld.nx - 2)
        j = np.clip(np.trunc(v).astype(int), 0, fld.ny - 2)
        return (np.minimum(H[i, j], H[i + 1, j + 1]) - org[:, 2:3].astype(F)).astype(F)
    band = (np.abs(u - np.round(u)) < SCAN_BAND) | (np.abs(v - np.round(v)) < SCAN_BAND)
    alts = [at(u + a, v + b) for a in (-2 * SCAN_BAND, 2 * SCAN_BAND) for b in (-2 * SCAN_BAND, 0, 2 * SCAN_BAND)] + \
           [at(u, v - 2 * SCAN_BAND), at(u, v + 2 * SCAN_BAND)]
    return at(u, v), alts, band


def scan_roots(rng, n, fld):
    """random position over and past the field, random yaw and tilt"""
    half = 0.5 * (fld.nx - 1) * fld.dx
    root = np.zeros((n, 13), F)
    root[:, 0:2], root[:, 2] = rng.uniform(-1.1 * half, 1.1 * half, (n, 2)), rng.uniform(0.3, 0.8, n)
    yaw = rng.uniform(-np.pi, np.pi, n)
    q = np.stack([rng.normal(0, 0.2, n), rng.normal(0, 0.2, n), np.sin(yaw / 2), np.cos(yaw / 2)], -1)
    root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return root


def scan_origins(rng, n):
    return np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-0.2, 0.2, (n, 1))], 1).astype(F)


# ------------------------------------------------------------------------------------------------ rough ground, stepped
ROUGH_MODELS = ("T16-free", "Anymal", "AMP")
# The T16-free tree is smaller than a tread of the stairs (0.3 m): dropped anywhere, most of its states stand on one
# level, and pressed in until half of them use two facets more than 5 % of the pool exceed its 24 contacts on the
# risers.  place_straddling() puts it where it straddles a riser instead.
STAIRS_MODELS = ("T16-free", "Anymal")
STEEP = 0.57735             # tangent_basis_t's branch: |n.x| at or above it takes the y axis
# place()'s quantile of the feet's lifts (0: every foot pressed in or touching), and how far (m) the state is lowered
# after that.  Chosen so that the cases meet test_heightfield_host's conditions on the oracle alone
PRESS = {("T16-free", "rough"): 0.25, ("T16-free", "stairs"): 0.0, ("Anymal", "rough"): 0.0, ("Anymal", "stairs"): 0.0, ("AMP", "rough"): 0.5}
SINK = {("T16-free", "rough"): 0.03, ("T16-free", "stairs"): 0.0, ("Anymal", "rough"): 0.0, ("Anymal", "stairs"): 0.0, ("AMP", "rough"): 0.0}
SLIP = 1e-2                 # m/s: a contact point this fast along its facet has friction rows that matter


def stairs_field(origins=None):
    """migym.terrain.pyramid_stairs_terrain at AnymalTerrain's scales (horizontal 0.1 m, vertical 0.005 m, steps of
    0.15 m every 0.31 m: three cells of tread, and between two treads one cell that climbs 0.15 m, gradient 1.5), on a
    65 x 65 grid centred on the origin"""
    from migym import terrain as TR
    t = TR.pyramid_stairs_terrain(TR.SubTerrain(width=65, length=65, vertical_scale=0.005, horizontal_scale=0.1), 0.31, 0.15)
    return Field(t.height_field_raw.astype(np.float64) * 0.005, 0.1, -3.2, -3.2, origins)


def step_field(kind, origins=None):
    return rough_field(origins=origins) if kind == "rough" else stairs_field(origins)


def on_field(fld, fn, n):
    """[fn(e) for e < n] with the oracle's ground set to the field and actor e's origin row bound (env_base = e: the
    calls below hand the oracle one-row views, whose env index is 0)"""
    try:
        out = []
        for e in range(n):
            if e == 0 or fld.origins is not None:
                O.set_heightfield(fld, e if fld.origins is not None else 0)
            out.append(fn(e))
        return out
    finally:
        O.set_heightfield(None)


def field_step(fld, host, mnp, sp, fp32=False):
    """one simulate of every actor of an LF.Host on the field (the oracle, or its fp32 twin), in place"""
    import ctypes as C
    lib = O.lib_f32() if fp32 else O.lib()

    def one(e):
        v = host.views(e, e + 1)
        lib.orc_simulate_views(mnp.ctypes.data, C.byref(sp), 1, C.byref(v), 1)
    on_field(fld, one, host.n)
    return host


def field_flags(fld, host, mnp, sp):
    import ctypes as C

    def one(e):
        v = host.views(e, e + 1)
        return O.lib().orc_step_flips(mnp.ctypes.data, C.byref(sp), C.byref(v), 0, PS.STEP_DELTA, PS.STEP_DF)
    return np.array(on_field(fld, one, host.n), np.int32)


def field_candidates(fld, mnp, sp, root, dof):
    return np.array(on_field(fld, lambda e: len(O.contacts(mnp, sp, root[e], dof[e], 96)), len(root)))


class _One:
    """one actor of a host, as the hooks that take a host and an env index want it"""

    def __init__(self, host, e):
        self.v = host.views(e, e + 1)

    def views(self):
        return self.v


def field_rows(fld, host, mnp, sp):
    """per actor O.step_rows on the field"""
    return on_field(fld, lambda e: O.step_rows(mnp, sp, _One(host, e), 0), host.n)


def place_one(spec, fld, e, row, q, xy, q_lift, sink, off=None):
    """actor e's root row put at world xy over the field (place()'s rule); with off, also the planes (normal and
    offset, rounded) of the ground candidates that then touch by the definition (gap below off)"""
    row = np.array(row, F)
    o = fld.origin(e)
    row[0:2] = xy - o[0:2]
    cs = candidates(spec, row, q)
    gaps = np.array([c[2][2] - c[3] for c in cs])
    low = gaps.min()
    at = [facet(fld, c[2][0] + o[0], c[2][1] + o[1])[:2] for c in cs]
    lift = [(low + c[3]) / nrm[2] + (h - o[2]) - c[2][2] for c, g, (h, nrm) in zip(cs, gaps, at) if g < low + 0.05]
    dz = np.quantile(lift, q_lift) - sink
    row[2] += dz
    if off is None:
        return row, None
    dz = float(row[2]) - (float(row[2]) - dz)       # (what the fp32 row took)
    touch = [tuple(np.round(np.append(nrm, nrm[2] * float(h - o[2])), 6)) for c, (h, nrm) in zip(cs, at)
             if (c[2][2] + dz - (h - o[2])) * nrm[2] - c[3] < off]
    return row, touch


def place(spec, fld, root, dof, rng, span, q=0.5, sink=0.0, xy=None):
    """pool states put over the field: random xy within +-span of the grid's centre (world coordinates; the origin, if
    any, is taken out), and raised so that the share q of the ground candidates that touch the plane in the pool state
    have at most the gap over their facets that the lowest of them has over the plane (the others hang above theirs):
    feet near the ground under them, some pressed in and some free"""
    root = np.array(root, F)
    n = len(root)
    xy = rng.uniform(-span, span, (n, 2)) if xy is None else xy
    for e in range(n):
        root[e] = place_one(spec, fld, e, root[e], dof[e, :, 0], xy[e], q, sink)[0]
    return root


STRADDLE_TRIES, STRADDLE_MOST, STRADDLE_STEEP = 64, 14, 3


def place_straddling(spec, fld, root, dof, rng, span, q, sink, off):
    """place() for a body smaller than a tread of the stairs: per actor the first of STRADDLE_TRIES random xy at which,
    by the definition alone (no step is run), the candidates that touch lie on two or more planes, STRADDLE_STEEP or
    more of them on a facet steep along x or y, and are at most STRADDLE_MOST (room under the contact capacity for the
    step to add some)"""
    root = np.array(root, F)
    for e in range(len(root)):
        for xy in rng.uniform(-span, span, (STRADDLE_TRIES, 2)):
            row, touch = place_one(spec, fld, e, root[e], dof[e, :, 0], xy, q, sink, off)
            if len(set(touch)) >= 2 and len(touch) <= STRADDLE_MOST and \
                    sum(max(abs(t[0]), abs(t[1])) >= STEEP for t in touch) >= STRADDLE_STEEP:
                break
        root[e] = row
    return root


def rough_case(model, tgs, kind="rough", origins=False, substeps=2):
    """The admitted states of (model, solver) on a field that is no plane, as slope_case: kind "rough" (rough_field())
    or "stairs" (stairs_field()); origins: per-actor env origins (random xy, oz +-0.2).  T16-free keeps its
    self-collision pairs.  Admission is the oracle's alone: candidates within capacity before and after the step, no
    orc_step_flips flag (the field's bits 256 / 512 / 1024 included), not sensitive to the SENS_EPS nudge, finite.
    Keys: spec, mnp, sp, fld, idx, scanned, root / dof / act / tgt, ref (the fp64 oracle's Host after the step), level
    (the same over the plane at the height under each root), rows (O.step_rows per state), cand."""
    key = ("rough case", kind, model, tgs, origins, substeps)
    if key in _cache:
        return _cache[key]
    spec, mnp, sp0 = LF.setup(model)
    root, dof, act, tgt, _ = LF.pool(model)
    nn = len(root)
    rng = np.random.default_rng([53, ROUGH_MODELS.index(model), int(kind == "stairs"), int(origins)])
    org = np.concatenate([rng.uniform(-0.5, 0.5, (nn, 2)), rng.uniform(-0.2, 0.2, (nn, 1))], 1) if origins else None
    fld = step_field(kind, org)
    root = np.array(root, F)
    if model == "T16-free":
        root[:, 2] -= 0.5     # back down: linkforce_ref raised the tree off the ground
    half = 0.5 * (fld.nx - 1) * fld.dx
    if (model, kind) == ("T16-free", "stairs"):
        root = place_straddling(spec, fld, root, dof, rng, 0.8 * half, PRESS[model, kind], SINK[model, kind],
                                float(sp0.contact_offset))
    else:
        root = place(spec, fld, root, dof, rng, 0.8 * half, PRESS[model, kind], SINK[model, kind])
    sp = LF.sp_at(sp0, None, substeps, tgs)
    ref, ok, why, cand, flags = admit_on_field(spec, mnp, sp, fld, root, dof, act, tgt,
                                               np.random.default_rng([59, ROUGH_MODELS.index(model)]))
    want = max(LF.BATCHES[model])
    idx = np.flatnonzero(ok)[:want]
    assert len(idx) == want, f"{model} {kind}: the pool admits only {len(idx)} of the {want} states ({why})"
    pick = lambda x: None if x is None else np.ascontiguousarray(x[idx])    # noqa: E731
    out = dict(spec=spec, mnp=mnp, sp=sp, idx=idx, scanned=int(idx[-1]) + 1, root=pick(root), dof=pick(dof), act=pick(act),
               tgt=pick(tgt), cand=int(cand[idx].max()), flags=flags, why=why)
    out["fld"] = Field(fld.H, fld.dx, fld.x0, fld.y0, None if org is None else org[idx])
    h = LF.Host(spec, out["root"], out["dof"], out["act"], out["tgt"])
    for name in ("root", "dof", "sensors", "dof_force", "ncf"):
        getattr(h, name)[:] = getattr(ref, name)[idx]
    out["ref"] = h
    # the plane at the height under each root: the oracle's flat step of the state lowered by that height
    hz = np.array([float(facet(out["fld"], *(out["root"][k, 0:2] + out["fld"].origin(k)[0:2]))[0]) - out["fld"].origin(k)[2]
                   for k in range(want)])
    low = np.array(out["root"])
    low[:, 2] -= hz.astype(F)
    lev = LF.Host(spec, low, out["dof"], out["act"], out["tgt"]).simulate_each(mnp, [sp] * want)
    lev.root[:, 2] += hz.astype(F)
    out["level"] = lev
    out["rows"] = field_rows(out["fld"], LF.Host(spec, out["root"], out["dof"], out["act"], out["tgt"]), mnp, sp)
    _cache[key] = out
    return out


def row_stats(c):
    """(multi, steep_x, steep_y) per admitted state of a rough_case: ground rows the solve uses (a normal impulse above
    1e-9 at some visit) lie on two or more facets in one substep; one of them has |n.x| >= STEEP / |n.y| >= STEEP and a
    contact point moving along its facet faster than SLIP"""
    multi, sx, sy = [], [], []
    for rows in c["rows"]:
        used = rows[(rows[:, 3] == -1) & (rows[:, 11] > 1e-9)]
        # a facet is its plane: the normal and the offset n . (p - d n) (two treads of the stairs share a normal only)
        plane = lambda r: tuple(np.round(np.append(r[7:10], r[7:10] @ r[4:7] - r[10]), 6))    # noqa: E731
        multi.append(any(len({plane(r) for r in used[used[:, 0] == st]}) >= 2 for st in np.unique(used[:, 0])))
        fast = used[used[:, 12] > SLIP]
        sx.append(bool((np.abs(fast[:, 7]) >= STEEP).any()))
        sy.append(bool((np.abs(fast[:, 8]) >= STEEP).any()))
    return np.array(multi), np.array(sx), np.array(sy)


def chain_case(model, tgs, launches=4, fp32=True):
    """rough_case(model, tgs)'s states stepped `launches` times by the oracle's fp32 twin (in the kernel's place: launch k
    starts from launch k - 1's output), the fp64 oracle restarted from the same state each time.  Per launch: (input
    Host, ref Host, admitted (bool per state): the admission of rough_case on that launch's inputs)."""
    key = ("chain", model, tgs, launches, fp32)
    if key in _cache:
        return _cache[key]
    c = rough_case(model, tgs)
    out, cur = [], LF.Host(c["spec"], c["root"], c["dof"], c["act"], c["tgt"])
    for _ in range(launches):
        inp, ref, ok = chain_admit(c, cur.root, cur.dof)
        out.append((inp, ref, ok))
        cur = field_step(c["fld"], LF.Host(c["spec"], cur.root, cur.dof, c["act"], c["tgt"]), c["mnp"], c["sp"], fp32=fp32)
    _cache[key] = out
    return out


def chain_admit(c, root, dof):
    """(input Host, the fp64 oracle's Host after one step from it, admitted per state) on rough_case c's field"""
    ref, ok, _, _, _ = admit_on_field(c["spec"], c["mnp"], c["sp"], c["fld"], root, dof, c["act"], c["tgt"],
                                      np.random.default_rng(67))
    return LF.Host(c["spec"], root, dof, c["act"], c["tgt"]), ref, ok


def take(h, keep):
    """the rows `keep` of a step's outputs (a Host or a namespace), as a namespace"""
    import types
    return types.SimpleNamespace(**{k: np.asarray(getattr(h, k))[keep] for k in ("root", "dof", "sensors", "dof_force", "ncf")})


# ------------------------------------------------------------------------------------------------ AnymalTerrain's physics
TERRAIN_COLS = (0, 2, 3)     # of the generated terrain's five columns: pyramid slope, stairs, discrete obstacles


def terrain_case(origins):
    """AnymalTerrain's effort-mode model at the task's sim parameters on a terrain generated by migym.terrain.Terrain (2
    levels x 5 columns of 8 m maps, seeded, curriculum: a slope, two stairs columns, obstacles, stepping stones), the
    standing states of anymal_ref on the harder level's slope, stairs and obstacle maps, off the central platform.
    origins: per-actor env origins, each map's own origin (the task itself runs in world coordinates).  Keys: spec, mnp,
    sp, p (the restatement's params), fld, root, dof, actions, n."""
    key = ("terrain case", origins)
    if key in _cache:
        return _cache[key]
    import anymal_ref as AR
    import anymal_terrain_ref as R
    from migym import terrain as TR
    _, _, _, root, dof, _, _ = AR.physics_states("standing")
    n = len(root)
    spec, mnp, sp, ap = R.task_model(R.task_cfg(n))
    state = np.random.get_state()
    np.random.seed(7)       # the terrain's draws
    t = TR.Terrain(dict(terrainType="trimesh", mapLength=8.0, mapWidth=8.0, numLevels=2, numTerrains=5, curriculum=True,
                        terrainProportions=[0.1, 0.1, 0.35, 0.25, 0.2]), n)
    np.random.set_state(state)
    table = (t.height_field_raw.astype(F) * F(t.vertical_scale)).astype(F)
    rng = np.random.default_rng(73)
    col = np.array(TERRAIN_COLS)[np.arange(n) % len(TERRAIN_COLS)]
    off = rng.uniform(1.7, 3.5, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))       # off the 3 m platform, inside the 8 m map
    org = t.env_origins[1, col].astype(F)
    xy = org[:, 0:2].astype(np.float64) + off
    fld = Field(table, t.horizontal_scale, -t.border_size, -t.border_size, org if origins else None)
    root = place(spec, fld, np.array(root, F), dof, rng, 0.0, 0.0, 0.0, xy)
    actions = np.random.default_rng(41).uniform(-1, 1, (n, 12)).astype(F)
    out = dict(spec=spec, mnp=mnp, sp=sp, p=R.params_from(ap), fld=fld, root=root, dof=np.array(dof, F), actions=actions, n=n,
               col=col)
    _cache[key] = out
    return out


TERRAIN_CHECKS = (("root pose", "root", slice(0, 7), 2e-4, 0), ("dof pos", "dof", 0, 2e-4, 0),
                  ("root twist", "root", slice(7, 13), 2e-3, 2e-3), ("dof vel", "dof", 1, 2e-3, 2e-3))


def terrain_compare(test, c, got, root, dof, eff):
    """one launch's outputs (root, dof, ncf) against the fp64 oracle stepped on the field from (root, dof) with the
    efforts eff, by test_one_decimation_step_matches_the_oracle's rule: the one-step tolerances, net contact forces to
    1 % of the batch's largest, a disagreeing env only where orc_step_flips flags its step, the flags reaching at most
    5 % of the envs.  Returns (the oracle's Host, flags, worst err / tolerance per check)."""
    n = len(root)
    mk = lambda: LF.Host(c["spec"], root, dof, eff)    # noqa: E731
    ref = field_step(c["fld"], mk(), c["mnp"], c["sp"])
    flags = field_flags(c["fld"], mk(), c["mnp"], c["sp"])
    for x in (got.root, got.dof, got.ncf):
        assert np.isfinite(x).all(), f"{test}: not finite"
    assert np.abs(got.dof[..., 0] - dof[..., 0]).max() > 1e-4, "the step moved nothing"
    pick = lambda h, name, sl: (h.root[:, sl] if name == "root" else h.dof[..., sl])    # noqa: E731
    checks = [(nm, pick(got, a, sl), pick(ref, a, sl), atol, rtol) for nm, a, sl, atol, rtol in TERRAIN_CHECKS]
    root_ref = quat_close(np.asarray(got.root, np.float64), ref.root)
    checks[0] = ("root pose", got.root[:, 0:7], root_ref[:, 0:7], 2e-4, 0)
    checks.append(("net contact forces", got.ncf, ref.ncf, 1e-2 * max(1.0, float(np.abs(ref.ncf).max())), 0))
    bad, worst = np.zeros(n, bool), {}
    for name, a, b, atol, rtol in checks:
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        eb = PS.env_bad(a, b, atol, rtol)
        ratio = (np.abs(a - b) / (atol + rtol * np.abs(b))).reshape(n, -1).max(1)
        worst[name] = float(ratio[flags == 0].max())
        print(f"{test} {name}: max err {np.abs(a - b).max():.3g} (atol {atol:.3g}), err / tolerance on unflagged envs "
              f"{worst[name]:.3g}, envs outside {int(eb.sum())} / {n}")
        PS.record(test, name, a, b, envs_outside=int(eb.sum()), atol=atol, rtol=rtol)
        bad |= eb
    print(f"{test}: {int((flags != 0).sum())} of {n} envs flagged")
    PS.assert_steps_explained(test, bad[None], flags[None], sens=None, reach_cap=PS.REACH_CAP, allow_unexplained=0.0)
    return ref, flags, worst
