"""An fp64 numpy ray caster written from the definitions in include/migym.h (mg_render): the reference the GPU
renderer is held to (tests/test_gpu_render.py), with known-answer tests of its own (tests/test_render_host.py).

Nothing here is shared with the kernels but the colour table and the constants migym/render.py restates.  Node frames
come from dynamics_ref.node_frames.  ``render`` also returns the ``ambiguous`` mask: the pixels at which an fp32 and an
fp64 ray caster may legitimately disagree (an edge, a near tie, a grazing hit, a checker border), which the GPU tests
leave out; test_render_host.py asserts that the mask covers at most 15 % of every image the GPU tests use.
"""
import functools
import math

import numpy as np

import dynamics_ref as R
from migym import model as M, taskdefs
from migym.render import (AMBIENT, COL_BOX, COL_GOAL, COL_GROUND, COL_OBJECT, COL_SKY, DIFFUSE, LIGHT, PALETTE,
                          T_MIN)

AMBIGUOUS_CAP = 0.15     # the largest ambiguous share an image of the GPU tests may have
JITTER = 0.02            # pixels
TIE = 1e-3               # nearest and second-nearest t closer than this: ambiguous
GRAZING = 0.1            # |n . d| below this: ambiguous
BORDER = 1e-3            # a ground hit this close (m) to a checker border: ambiguous


# ------------------------------------------------------------------------------------------------ primitives
def prim(gtype, Rw, p, size, colour):
    return {"type": int(gtype), "R": np.asarray(Rw, np.float64), "p": np.asarray(p, np.float64),
            "size": np.asarray(size, np.float64), "colour": int(colour)}


def env_primitives(spec, roots, qs, obj_rows=None, boxes=None):
    """the primitives of one env in id order: the geoms of each actor (roots (A, 13), qs (A, nD)), the free object
    and the goal (obj_rows (2, 13), models with spec.obj), the extra boxes (K, 10), the ground plane"""
    out = []
    for root, q in zip(np.asarray(roots, np.float64), np.asarray(qs, np.float64)):
        Rn, xn = R.node_frames(spec, root, q)
        for g in spec.geoms:
            out.append(prim(g.gtype, Rn[g.node] @ M.qmat(M.qnorm(g.quat)), xn[g.node] + Rn[g.node] @ np.asarray(g.pos),
                            g.size, g.body % 8))
    if spec.obj:
        for row, col in zip(np.asarray(obj_rows, np.float64), (COL_OBJECT, COL_GOAL)):
            out.append(prim(spec.obj["type"], M.qmat(M.qnorm(row[3:7])), row[0:3], spec.obj["size"], col))
    if boxes is not None:
        for b in np.asarray(boxes, np.float64):
            out.append(prim(M.GT_BOX, M.qmat(M.qnorm(b[3:7])), b[0:3], b[7:10], COL_BOX))
    out.append(prim(M.GT_PLANE, np.eye(3), np.zeros(3), np.zeros(3), COL_GROUND))
    return out


# ------------------------------------------------------------------------------------------------ intersections
def _near(t0, t1):
    return np.where(t0 > T_MIN, t0, np.where(t1 > T_MIN, t1, np.inf))


def _sphere_roots(o, d, r):
    """roots of |o + t d| = r (o (3,) or (..., 3), d (..., 3)); NaN where the ray misses"""
    a = np.sum(d * d, -1)
    b = np.sum(o * d, -1) / a
    c = (np.sum(o * o, -1) - r * r) / a
    h = np.sqrt(b * b - c)
    return -b - h, -b + h


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _pick(t, n, tc, nc, ok):
    """take candidate (tc, nc) where it is valid and nearer"""
    take = ok & (tc > T_MIN) & (tc < t)
    return np.where(take, tc, t), np.where(take[..., None], nc, n)


def hit(p, o, d, hull_planes=None):
    """(t, n): the nearest hit beyond T_MIN of primitive p on the rays o + t d in p's own frame (+inf: none) and the
    outward normal there, local"""
    ty, sz = p["type"], p["size"]
    shape = d.shape[:-1]
    t = np.full(shape, np.inf)
    n = np.zeros(shape + (3,))
    n[..., 2] = 1.0
    o = np.broadcast_to(o, d.shape)
    if ty == M.GT_SPHERE:
        t0, t1 = _sphere_roots(o, d, sz[0])
        t = np.where(np.isnan(t0), np.inf, _near(t0, t1))
        n = (o + d * np.where(np.isfinite(t), t, 0.0)[..., None]) / sz[0]
    elif ty == M.GT_ELLIPSOID:
        os_, ds = o / sz, d / sz
        t0, t1 = _sphere_roots(os_, ds, 1.0)
        t = np.where(np.isnan(t0), np.inf, _near(t0, t1))
        pt = os_ + ds * np.where(np.isfinite(t), t, 0.0)[..., None]
        n = _unit(pt / sz + 1e-300)
    elif ty in (M.GT_CAPSULE, M.GT_CYLINDER):
        r, h = sz[0], sz[1]
        o2, d2 = o.copy(), d.copy()
        o2[..., 2] = 0.0
        d2[..., 2] = 0.0
        t0, t1 = _sphere_roots(o2, d2, r)
        for tc in (t0, t1):
            pc = o + d * np.nan_to_num(tc)[..., None]
            nc = np.stack([pc[..., 0] / r, pc[..., 1] / r, np.zeros(shape)], -1)
            t, n = _pick(t, n, tc, nc, ~np.isnan(tc) & (np.abs(pc[..., 2]) <= h))
        for sg in (1.0, -1.0):
            if ty == M.GT_CAPSULE:
                oc = o - np.array([0.0, 0.0, sg * h])
                t0, t1 = _sphere_roots(oc, d, r)
                for tc in (t0, t1):
                    pc = oc + d * np.nan_to_num(tc)[..., None]
                    t, n = _pick(t, n, tc, pc / r, ~np.isnan(tc) & (pc[..., 2] * sg >= 0.0))
            else:
                tc = (sg * h - o[..., 2]) / d[..., 2]
                pc = o + d * np.nan_to_num(tc, posinf=0.0, neginf=0.0)[..., None]
                nc = np.broadcast_to(np.array([0.0, 0.0, sg]), d.shape)
                t, n = _pick(t, n, tc, nc, np.isfinite(tc) & (pc[..., 0] ** 2 + pc[..., 1] ** 2 <= r * r))
    elif ty == M.GT_BOX:
        ta, tb = (-sz - o) / d, (sz - o) / d
        lo, hi = np.fmin(ta, tb), np.fmax(ta, tb)
        tn, tf = lo.max(-1), hi.min(-1)
        an, af = lo.argmax(-1), hi.argmin(-1)
        ok = tn <= tf
        t = np.where(ok, _near(tn, tf), np.inf)
        entry = tn > T_MIN
        ax = np.where(entry, an, af)
        dax = np.take_along_axis(d, ax[..., None], -1)[..., 0]
        sg = np.where((dax > 0) == entry, -1.0, 1.0)
        n = np.zeros(shape + (3,))
        np.put_along_axis(n, ax[..., None], sg[..., None], -1)
    elif ty == M.GT_CONVEX:
        pl = np.asarray(hull_planes, np.float64)
        den = d @ pl[:, :3].T                               # (..., planes)
        dist = pl[:, 3] - o @ pl[:, :3].T
        tk = dist / np.where(den == 0.0, 1.0, den)
        tn_all = np.where(den < 0, tk, -np.inf)
        tf_all = np.where(den > 0, tk, np.inf)
        tn, tf = tn_all.max(-1), tf_all.min(-1)
        outside = np.any((den == 0) & (dist < 0), -1)
        ok = ~outside & (tn <= tf)
        t = np.where(ok, _near(tn, tf), np.inf)
        which = np.where(tn > T_MIN, tn_all.argmax(-1), tf_all.argmin(-1))
        n = pl[which, :3]
    elif ty == M.GT_PLANE:
        tp = -o[..., 2] / d[..., 2]
        t = np.where(tp > T_MIN, tp, np.inf)
    else:
        raise ValueError(f"unknown primitive type {ty}")
    return t, n


# ------------------------------------------------------------------------------------------------ camera
def camera(eye, target):
    f = _unit(np.asarray(target, np.float64) - np.asarray(eye, np.float64))
    r = _unit(np.cross(f, [0.0, 0.0, 1.0]))
    return f, r, np.cross(r, f)


def rays(W, H, fov_deg, eye, target, dx=0.0, dy=0.0):
    """unit ray directions (H, W, 3) through the pixel centres shifted by (dx, dy) pixels"""
    f, r, u = camera(eye, target)
    th = math.tan(math.radians(fov_deg) / 2)
    j, i = np.meshgrid(np.arange(W) + 0.5 + dx, np.arange(H) + 0.5 + dy)
    x = (2 * j / W - 1) * th * W / H
    y = (1 - 2 * i / H) * th
    return _unit(f + x[..., None] * r + y[..., None] * u)


def trace(prims, eye, d, hull_planes=None):
    """ids (-1 sky), t (+inf sky), world normals, the second-nearest t (another primitive's)"""
    eye = np.asarray(eye, np.float64)
    ts, ns = [], []
    with np.errstate(all="ignore"):
        for p in prims:
            t, nl = hit(p, (eye - p["p"]) @ p["R"], d @ p["R"], hull_planes)
            ts.append(t)
            ns.append(nl @ p["R"].T)
    ts, ns = np.stack(ts), np.stack(ns)
    ids = ts.argmin(0)                                     # the first of equal minima: the lower id
    t = np.take_along_axis(ts, ids[None], 0)[0]
    n = np.take_along_axis(ns, ids[None, ..., None], 0)[0]
    rest = ts.copy()
    np.put_along_axis(rest, ids[None], np.inf, 0)
    second = rest.min(0)
    ids = np.where(np.isfinite(t), ids, -1)
    return ids, t, n, second


def shade(prims, ids, t, n, eye, d):
    col = np.array([p["colour"] for p in prims] + [COL_SKY])[ids]      # ids -1 -> the sky entry
    hp = np.asarray(eye) + d * np.where(np.isfinite(t), t, 0.0)[..., None]
    chk = (np.floor(hp[..., 0]).astype(np.int64) + np.floor(hp[..., 1]).astype(np.int64)) & 1
    col = np.where(col == COL_GROUND, col + chk, col)
    sh = AMBIENT + DIFFUSE * np.maximum(0.0, n @ LIGHT)
    c = PALETTE[col] * np.where(ids >= 0, sh, 1.0)[..., None]
    return np.clip(np.floor(255.0 * c + 0.5), 0, 255).astype(np.uint8), hp


def render(prims, W, H, fov_deg, eye, target, hull_planes=None):
    """{"ids", "depth", "normals", "rgb", "ambiguous"} of one image"""
    d = rays(W, H, fov_deg, eye, target)
    ids, t, n, second = trace(prims, eye, d, hull_planes)
    rgb, hp = shade(prims, ids, t, n, eye, d)
    amb = np.zeros(ids.shape, bool)
    for dx, dy in ((JITTER, JITTER), (JITTER, -JITTER), (-JITTER, JITTER), (-JITTER, -JITTER)):
        amb |= trace(prims, eye, rays(W, H, fov_deg, eye, target, dx, dy), hull_planes)[0] != ids
    hitm = ids >= 0
    amb |= hitm & (second - np.where(hitm, t, 0.0) < TIE)
    amb |= hitm & (np.abs(np.sum(n * d, -1)) < GRAZING)
    ground = hitm & (ids == len(prims) - 1)
    fr = np.abs(hp[..., :2] - np.round(hp[..., :2])).min(-1)
    amb |= ground & (fr < BORDER)
    return {"ids": ids.astype(np.int32), "depth": t, "normals": n, "rgb": rgb, "ambiguous": amb}


# ------------------------------------------------------------------------------------------------ the GPU tests' scenes
N_ENVS = 5
ENV_IDS = (4, 0, 2)
W, H = 37, 21            # neither side a multiple of the trace tile


def _limits(spec):
    lo, hi = taskdefs.dof_limits(spec)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    free = ~(hi > lo)                      # an unlimited DOF
    return np.where(free, -1.0, lo), np.where(free, 1.0, hi)


def _tilt(rng, n, ang):
    """n unit quaternions: a rotation of up to `ang` about a random axis"""
    out = []
    for _ in range(n):
        out.append(M.quat_from_axis_angle(rng.normal(size=3), rng.uniform(-ang, ang)))
    return np.array(out)


def _scene(name, spec, A, z, spread, eye, target, follow, seed, tilt=0.4, obj=None, boxes=None, size=(W, H),
           agent_spacing=0.0):
    """N_ENVS envs of A actors: joint positions uniform within the limits, distinct root poses (base height z, xy
    within +-spread, a random tilt), everything fp32 as the device sees it"""
    rng = np.random.default_rng(seed)
    n = N_ENVS * A
    lo, hi = _limits(spec)
    q = (lo + (hi - lo) * rng.uniform(0.05, 0.95, (n, spec.num_dofs))).astype(np.float32)
    rows = 3 if spec.obj else A
    root = np.zeros((N_ENVS * rows, 13), np.float32)
    root[:, 6] = 1.0
    offs = taskdefs.agent_offsets(A, agent_spacing)
    for e in range(N_ENVS):
        for a in range(A):
            r = root[e * rows + a]
            r[0:3] = np.array([rng.uniform(-spread, spread), rng.uniform(-spread, spread), z + rng.uniform(-0.05, 0.05)])
            r[0:3] += np.asarray(offs[a])
            r[3:7] = _tilt(rng, 1, tilt)[0]
        if spec.obj:
            base = root[e * rows, 0:3]
            for k, off in enumerate(obj):
                r = root[e * rows + 1 + k]
                r[0:3] = base + np.asarray(off) + rng.uniform(-0.02, 0.02, 3)
                r[3:7] = _tilt(rng, 1, 3.0)[0]
    bx = None
    if boxes:
        bx = np.zeros((N_ENVS, boxes, 10), np.float32)
        for e in range(N_ENVS):
            for k in range(boxes):
                bx[e, k, 0:3] = root[e * rows, 0:3] + rng.uniform(-0.6, 0.6, 3) * np.array([1, 1, 0.3])
                bx[e, k, 3:7] = _tilt(rng, 1, 3.0)[0]
                bx[e, k, 7:10] = rng.uniform(0.05, 0.2, 3)
    return {"name": name, "spec": spec, "A": A, "rows": rows, "root": root, "q": q, "boxes": bx, "eye": eye,
            "target": target, "follow": follow, "fov_deg": 60.0, "W": size[0], "H": size[1]}


def _render_tree():
    """the synthetic tree of the dynamics tests (free base, 20 nodes, sphere / capsule / box geoms) with a cylinder and
    an ellipsoid geom put on two of its nodes"""
    spec = R.random_tree(20, 7, free_base=True, num_geoms=12)
    spec.geoms[3].gtype, spec.geoms[3].size = M.GT_CYLINDER, [0.05, 0.09, 0.0]
    spec.geoms[7].gtype, spec.geoms[7].size = M.GT_ELLIPSOID, [0.09, 0.05, 0.07]
    return spec


SCENE_NAMES = ("Cartpole", "Ant", "Humanoid", "ShadowHand-block", "ShadowHand-egg", "ShadowHand-pen", "MAAnt", "tree",
               "boxes")


@functools.lru_cache(maxsize=None)
def scene(name):
    """the scene `name` of the GPU tests, built once and shared (read-only)"""
    if name == "Cartpole":
        return _scene(name, M.load_builtin("cartpole"), 1, 2.0, 0.5, (3.0, 0.4, 3.0), (0, 0, -0.3), True, 11, tilt=0.0)
    if name == "Ant":
        return _scene(name, M.load_builtin("ant"), 1, 0.6, 1.0, (0.9, -0.8, 0.9), (0, 0, -0.15), True, 12)
    if name == "Humanoid":
        return _scene(name, M.load_builtin("humanoid"), 1, 1.3, 1.0, (1.4, -1.2, 0.6), (0, 0, -0.3), True, 13)
    if name.startswith("ShadowHand-"):
        kind = name.split("-")[1]
        return _scene(name, taskdefs.hand_spec(kind), 1, 0.5, 0.3, (0.2, -0.5, 0.33), (0.0, -0.32, 0.06), True,
                      14 + len(kind), tilt=0.15, obj=((0.0, -0.39, 0.1), (-0.2, -0.33, 0.14)))
    if name == "MAAnt":
        return _scene(name, M.load_builtin("ant"), 4, 0.6, 0.2, (2.0, -1.8, 2.2), (0, 0, 0.2), False, 15,
                      agent_spacing=1.4)
    if name == "tree":
        return _scene(name, _render_tree(), 1, 0.7, 0.5, (0.55, -0.5, 0.45), (0, 0, 0), True, 16)
    if name == "boxes":
        return _scene(name, M.load_builtin("ant"), 1, 0.6, 1.0, (1.3, -1.1, 1.2), (0, 0, -0.1), True, 17, boxes=3)
    raise KeyError(name)


def scene_env_primitives(sc, e):
    A, rows, nd = sc["A"], sc["rows"], sc["spec"].num_dofs
    roots = sc["root"][e * rows:e * rows + A]
    qs = sc["q"][e * A:(e + 1) * A].reshape(A, nd)
    obj = sc["root"][e * rows + 1:e * rows + 3] if sc["spec"].obj else None
    return env_primitives(sc["spec"], roots, qs, obj, None if sc["boxes"] is None else sc["boxes"][e])


def scene_camera(sc, e):
    anchor = sc["root"][e * sc["rows"], 0:3].astype(np.float64) if sc["follow"] else np.zeros(3)
    return anchor + np.asarray(sc["eye"], np.float64), anchor + np.asarray(sc["target"], np.float64)


@functools.lru_cache(maxsize=None)
def scene_reference(name):
    """[render(...) of env e for e in ENV_IDS] and the primitives, computed once, shared and never written to"""
    sc = scene(name)
    hull = sc["spec"].hull["planes"] if sc["spec"].hull else None
    out = []
    for e in ENV_IDS:
        prims = scene_env_primitives(sc, e)
        eye, target = scene_camera(sc, e)
        img = render(prims, sc["W"], sc["H"], sc["fov_deg"], eye, target, hull)
        img["prims"] = prims
        for v in img.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(img)
    return out
