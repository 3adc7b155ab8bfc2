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
    nud = LF.Host(spec, root, dof, act, tgt)
    nud.root[:, 0:3] += TP.SENS_EPS * r2.choice([-1.0, 1.0], (nn, 3))
    nud.dof[..., 0] += TP.SENS_EPS * r2.choice([-1.0, 1.0], (nn, spec.num_dofs))
    nud.simulate_each(mnp, sps)
    ok &= ~(PS.env_bad(nud.dof[..., 0], ref.dof[..., 0], 0.25 * 2e-4, 0) |
            PS.env_bad(nud.dof[..., 1], ref.dof[..., 1], 0.25 * 2e-3, 0.25 * 2e-3) |
            PS.env_bad(nud.root[:, 0:7], ref.root[:, 0:7], 0.25 * 2e-4, 0) |
            PS.env_bad(nud.root[:, 7:13], ref.root[:, 7:13], 0.25 * 2e-3, 0.25 * 2e-3))
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


def ground_list(spec, sp, fld, env, root13, q, delta=CR.DELTA):
    """(rows, marks) of one actor's ground contacts on the field by DESIGN.md §15, thresholds moved out by delta as
    orc_contacts_marks does: BAND_IN / BAND_OUT for a gap within delta of contact_offset; AMB for a candidate within
    EDGE_EPS cells of a cell edge or the diagonal whose other facet puts the gap on the other side of the threshold (or
    which is inside the band on either facet), ILL where it lies that close to a crease at all (its normal and point
    may be either facet's)"""
    off, o = float(sp.contact_offset), fld.origin(env)
    rows, marks = [], []
    for gi, node, e, r, bound, c in candidates(spec, root13, q):
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
