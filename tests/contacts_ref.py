"""Contact lists of the step kernels' collide() against the fp64 oracle's, contact by contact.

mg_debug_contacts reads the first substep's contact list of the real collide path; the oracle lists its own
(orc_contacts_marks: rows (nodeA, geomA, nodeB, geomB, p[3], n[3], gap) plus per-contact marks).  `compare` is the
rule both tests/test_contacts_host.py (the oracle's fp32 twin, CPU) and tests/test_gpu_contacts.py (the kernels) apply:

  id list   the sequence of (nodeA, geomA, nodeB, geomB) equals the oracle's, in order and length.  Two exceptions:
            a contact whose oracle gap is within DELTA of its threshold (it may be on either side of it: the oracle
            lists its candidates with the thresholds moved out by DELTA and marks them), and a geom-object pair the
            oracle marks ambiguous (its rows leave both lists, but only if the lists do not match with them in).
  values    on matched contacts: gap; the point's error split into its part along the oracle's normal and the
            tangential rest; the normal as |n x n_ref|.  Normals and tangential parts of contacts marked ill or
            ambiguous are not compared; their gaps and the normal part of their points are.
  caps      envs with an id-list exemption: at most 5 % of a set; marked contacts: at most 5 % of a set's contacts
            (10 % on the hull-exact sets).  Both are properties of the reference alone.

BOUNDS: 4 x the largest error of the oracle's fp32 twin through this same rule, per object type and quantity, on the
contacts without marks (tests/test_contacts_host.py measures it again and asserts the twin stays within a quarter of
each bound).  The table is DESIGN.md §6.
"""
import copy

import numpy as np

import parity_stats as PS
import pyoracle as O
from migym import model as M

DELTA = PS.STEP_DELTA  # m: the contact-threshold band, the step tests' own (orc_contacts_marks moves the thresholds by it)
REACH_CAP = 0.05      # envs with an id-list exemption, of a set
MARK_CAP = 0.05       # marked contacts, of a set's contacts
MARK_CAP_HULL = 0.10  # ... on the hull-exact sets (the step tests grant them 0.10)
AMB, ILL, BAND_IN, BAND_OUT, EDGE = 1, 2, 4, 8, 16
QUANT = ("gap", "point_n", "point_t", "normal")

# 4 x the fp32 twin's largest error: kind -> (gap m, point along the normal m, tangential m,
# |n x n_ref|)
TWIN_MAX = {   # the twin's largest error over the kind's sets, rounded up to two digits
    "none": (1.3e-6, 1.3e-6, 1.7e-6, 9.0e-6),     # trees, Ant, Humanoid
    "block": (1.2e-7, 8.6e-8, 3.3e-7, 5.3e-5),    # hand with the cube, curled fingers
    "egg": (3.6e-6, 1.8e-6, 3.2e-6, 3.4e-3),
    "pen": (1.7e-7, 7.1e-8, 2.2e-5, 2.3e-4),
}
BOUNDS = {k: tuple(4.0 * x for x in v) for k, v in TWIN_MAX.items()}


# ------------------------------------------------------------------------------------------------ the lists
def oracle_lists(mnp, sp, root, dof, cap=64):
    """per env: (rows, marks, pair_lost) of orc_contacts_marks at DELTA; root (n, 13 * rows), dof (n, nd, 2)"""
    return [O.contacts_marks(mnp, sp, np.asarray(root[i]).ravel(), dof[i], DELTA, cap) for i in range(len(root))]


def twin_lists(mnp, sp, root, dof, cap=64):
    """per env: the fp32 twin's orc_contacts_full rows"""
    return [O.contacts_full(mnp, sp, np.asarray(root[i]).ravel(), dof[i], cap, fp32=True) for i in range(len(root))]


def plain_lists(mnp, sp, root, dof, cap=64):
    """per env: the fp64 oracle's orc_contacts_full rows (its list at the thresholds themselves)"""
    return [O.contacts_full(mnp, sp, np.asarray(root[i]).ravel(), dof[i], cap) for i in range(len(root))]


def _ids(r):
    return tuple(int(x) for x in r[:4])


def _align(got, ref, optional, prefix):
    """the cheapest alignment of every got row with a ref row of the same ids, in order, skipping only optional ref
    rows (and, with prefix, any ref rows behind the last match): [(i_got, j_ref)] or None.  Cost: the point distance,
    which settles which of several rows with the same ids an optional one is."""
    ng, nr = len(got), len(ref)
    INF = float("inf")
    cost = np.full((ng + 1, nr + 1), INF)
    back = np.zeros((ng + 1, nr + 1), np.int8)
    cost[0, 0] = 0.0
    for j in range(1, nr + 1):
        if optional[j - 1] and cost[0, j - 1] < INF:
            cost[0, j], back[0, j] = cost[0, j - 1], 1
    for i in range(1, ng + 1):
        for j in range(1, nr + 1):
            best, how = INF, 0
            if cost[i - 1, j - 1] < INF and _ids(got[i - 1]) == _ids(ref[j - 1]):
                best, how = cost[i - 1, j - 1] + float(np.linalg.norm(got[i - 1][4:7] - ref[j - 1][4:7])), 2
            if optional[j - 1] and cost[i, j - 1] < best:
                best, how = cost[i, j - 1], 1
            cost[i, j], back[i, j] = best, how
    ends = range(nr + 1) if prefix else [nr]
    j = min(ends, key=lambda e: cost[ng, e])
    if not cost[ng, j] < INF:
        return None
    i, out = ng, []
    while i > 0 or j > 0:
        if back[i, j] == 2:
            out.append((i - 1, j - 1))
            i, j = i - 1, j - 1
        elif back[i, j] == 1:
            j -= 1
        else:
            return None
    return out[::-1]


def match_env(got, ref, marks, lost, max_contacts=None):
    """(pairs, exempted, why): the alignment of one env's lists ([(i_got, j_ref)], or None if the id lists differ
    beyond the two exceptions), and whether an exception was needed"""
    got, ref = np.asarray(got, np.float64).reshape(-1, 11), np.asarray(ref, np.float64).reshape(-1, 11)
    prefix = max_contacts is not None and len(got) >= max_contacts
    if max_contacts is not None and len(got) > max_contacts:
        return None, False, f"{len(got)} contacts with max_contacts {max_contacts}"
    band = (marks & (BAND_IN | BAND_OUT)) != 0
    # 1. as they are: the oracle's list at the thresholds themselves (without the rows at or above them)
    real = np.flatnonzero((marks & BAND_OUT) == 0)
    al = _align(got, ref[real], np.zeros(len(real), bool), prefix)
    if al is not None:
        return [(a, int(real[b])) for a, b in al], False, ""
    # 2. the threshold band on either side
    al = _align(got, ref, band, prefix)
    if al is not None:
        return al, True, "band"
    # 3. without the ambiguous pairs' rows (and, when an ambiguous decision left a pair empty in the oracle, without
    # the kernel's rows of geom-object pairs the oracle's list does not hold)
    amb_pairs = {(int(r[1]), int(r[3])) for r, m in zip(ref, marks) if m & AMB}
    ref_pairs = {(int(r[1]), int(r[3])) for r in ref}
    drop_g = np.array([(int(r[1]), int(r[3])) in amb_pairs or
                       (lost and int(r[3]) == -2 and (int(r[1]), int(r[3])) not in ref_pairs) for r in got], bool)
    keep_r = np.array([(int(r[1]), int(r[3])) not in amb_pairs for r in ref], bool)
    if (amb_pairs or lost) and (drop_g.any() or not keep_r.all()):
        gi, rj = np.flatnonzero(~drop_g), np.flatnonzero(keep_r)
        al = _align(got[gi], ref[rj], band[rj], prefix or max_contacts is not None)
        if al is not None:
            return [(int(gi[a]), int(rj[b])) for a, b in al], True, "ambiguous pair"
    return None, False, f"ids {[_ids(r) for r in got]} against {[(_ids(r), int(m)) for r, m in zip(ref, marks)]}"


def errors(g, r):
    """(gap, point along the normal, tangential point, normal) errors of a matched contact"""
    e = g[4:7] - r[4:7]
    en = float(np.dot(e, r[7:10]))
    return (abs(float(g[10] - r[10])), abs(en), float(np.linalg.norm(e - en * r[7:10])),
            float(np.linalg.norm(np.cross(g[7:10], r[7:10]))))


def reference_reach(lists):
    """(fraction of envs with an id-list exemption available, fraction of contacts with a mark) of a set's oracle
    lists: what the caps bound, from the reference alone.  Contacts: those at the thresholds themselves."""
    envs = sum(1 for _, m, lost in lists if lost or (m & (AMB | BAND_IN | BAND_OUT)).any())
    real = [m[(m & BAND_OUT) == 0] for _, m, _ in lists]
    ncon = sum(len(m) for m in real)
    marked = sum(int(((m & (AMB | ILL)) != 0).sum()) for m in real)
    return envs / max(len(lists), 1), marked / max(ncon, 1), ncon


def compare(test, got, lists, kind, max_contacts=None, reach_cap=REACH_CAP, mark_cap=MARK_CAP, bounds=None,
            record=True):
    """got: per env an (k, 11) array; lists: oracle_lists of the same states; kind: none / block / egg / pen.
    Asserts the caps, the id lists and the bounds; returns the statistics (also recorded for MIGYM_PARITY_REPORT)."""
    bounds = BOUNDS[kind] if bounds is None else bounds
    n = len(lists)
    assert len(got) == n
    reach, mfrac, ncon = reference_reach(lists)
    assert reach <= reach_cap, f"{test}: the oracle's band / ambiguity marks reach {reach:.3f} of the envs"
    assert mfrac <= mark_cap, f"{test}: {mfrac:.3f} of the oracle's contacts carry a mark"
    used, unexplained, worst = 0, [], np.zeros(4)
    errs = {q: [] for q in QUANT}
    matched = 0
    for e in range(n):
        ref, marks, lost = lists[e]
        g = np.asarray(got[e], np.float64).reshape(-1, 11)
        al, ex, why = match_env(g, ref, marks, lost, max_contacts)
        if al is None:
            unexplained.append((e, why))
            continue
        used += ex
        for i, j in al:
            er = errors(g[i], ref[j])
            loose = (marks[j] & (AMB | ILL)) != 0
            matched += 1
            for q, (name, x, b) in enumerate(zip(QUANT, er, bounds)):
                if loose and name in ("point_t", "normal"):
                    continue
                errs[name].append(x)
                if x > b:
                    unexplained.append((e, f"contact {i} {_ids(g[i])}: {name} off by {x:.3g} (bound {b:.3g})"))
                worst[q] = max(worst[q], x)
    st = dict(envs=n, contacts=ncon, matched=matched, exempt_envs_used=used, reach=reach, marked=mfrac,
              unexplained=len({e for e, _ in unexplained}), **{f"max_{q}": float(worst[i]) for i, q in enumerate(QUANT)})
    if record:
        for q in QUANT:
            a = np.asarray(errs[q], np.float64)
            PS.record(test, f"contact {q}", a, np.zeros_like(a), **st)
    assert used <= reach_cap * n, f"{test}: {used} envs needed an id-list exemption"
    assert not unexplained, f"{test}: {len(unexplained)} findings, first: {unexplained[:4]}"
    return st


# ------------------------------------------------------------------------------------------------ the state sets
_cache = {}
HAND_SETS = ("palm-block", "palm-egg", "palm-pen", "forearm-block", "forearm-egg", "forearm-pen", "hull-block",
             "hull-pen", "fingers")


def hand_set(name, n=256):
    """(spec, sp, mnp, root (n, 39), dof, host env) of a hand state set: the builders and seeds of tests/test_gpu_hand.py
    (palm: test_hand_physics_step_matches_oracle; forearm: ..._near_forearm_...; hull: ..._hull_exact_...; fingers:
    test_hand_finger_pairs_match_oracle)"""
    if ("hand", name, n) in _cache:
        return _cache["hand", name, n]
    import test_gpu_hand as H
    where, kind = name.split("-") if "-" in name else (name, "block")
    if where == "hull":
        spec, sp, tp, h = H.hull_exact_states(kind, n, np.random.default_rng(13))
    elif where == "ground":
        # the object lying on the ground plane below the hand, tilted by ~0.01 rad, its centre within 1 mm of resting
        # height: several of its lower corners within the contact offset (only the list-cut tests use this set)
        spec, sp, tp = H.setup(kind=kind)
        rng = np.random.default_rng(19)
        h = H.hand_states(spec, tp, n, rng, H.PALM_DZ[kind])
        yaw, tilt = rng.uniform(-np.pi, np.pi, n), rng.normal(0, 0.005, (n, 2))
        q = np.stack([tilt[:, 0], tilt[:, 1], np.sin(yaw / 2), np.cos(yaw / 2)], -1)
        h.root[:, 1, 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
        h.root[:, 1, 2] = float(M.pack_model(spec)["obj_size"][2]) + rng.uniform(-1e-3, 1e-3, n)
    else:
        spec, sp, tp = H.setup(kind=kind)
        rng = np.random.default_rng({"palm": 5, "forearm": 11, "fingers": 17}[where])
        if where == "fingers":
            h = H.hand_states(spec, tp, n, rng)
            lo = np.array([x.lower for x in spec.nodes[1:]])
            hi = np.array([x.upper for x in spec.nodes[1:]])
            h.dof[:, :, 0] = lo + (hi - lo) * rng.uniform(0.6, 0.95, (n, spec.num_dofs))
            h.root[:, 1, 0:3] = (5.0, 5.0, 3.0)
        else:
            h = H.hand_states(spec, tp, n, rng, H.PALM_DZ[kind], pen=kind == "pen")
        if where == "forearm":
            top = H.forearm_top(spec, h)
            ob = h.root[:, 1]
            reach = {"block": 0.025, "egg": 0.03, "pen": 0.008}[kind]
            ob[:, 0:3] = top + np.c_[rng.normal(0, 0.02, (n, 2)), reach * rng.uniform(0.6, 1.4, n)]
            ob[:, 7:13] = rng.normal(0, 0.1, (n, 6))
            h.dof[:, :, 0] = 0.0
    mnp = M.pack_model(spec)
    out = (spec, sp, mnp, h.root.reshape(n, -1).copy(), h.dof.copy(), h)
    _cache["hand", name, n] = out
    return out


def kind_of(name):
    return {"block": "block", "egg": "egg", "pen": "pen"}.get(name.split("-")[-1], "block" if name == "fingers" else "none")


def hand_reach(name):
    """what a hand set's states reach, found with the oracle (envs): hull = the forearm hull touches the object;
    seg_mtd = the egg overlaps a sphere's / capsule's core (gap below minus the radius); mpr = the egg more than 1 mm
    (CVX_MARGIN) into a box; edge = a box_box_edge contact; pairs = a contact of an explicit MJCF pair"""
    spec, sp, mnp, root, dof, _ = hand_set(name)
    lists = cached_lists(("hand", name), mnp, sp, root, dof)
    hull = spec.hull["geom"] if getattr(spec, "hull", None) else -1
    out = dict(hull=0, seg_mtd=0, mpr=0, edge=0, pairs=0)
    for rows, marks, _ in lists:
        real = (marks & BAND_OUT) == 0
        obj = real & (rows[:, 3] == -2)
        gt = np.array([spec.geoms[int(g)].gtype if g >= 0 else -1 for g in rows[:, 1]], int)
        rad = np.array([spec.geoms[int(g)].size[0] if g >= 0 else 0.0 for g in rows[:, 1]])
        out["hull"] += bool((obj & (rows[:, 1] == hull)).any())
        out["seg_mtd"] += bool((obj & np.isin(gt, (M.GT_SPHERE, M.GT_CAPSULE)) & (rows[:, 10] < -rad)).any())
        out["mpr"] += bool((obj & (gt == M.GT_BOX) & (rows[:, 10] < -1e-3)).any())
        out["edge"] += bool((real & ((marks & EDGE) != 0)).any())
        out["pairs"] += bool((real & (rows[:, 3] >= 0)).any())
    return out


def tree_set(case, kind):
    """(spec, sp, mnp, root, dof, act) of a tree_physics_ref case's states"""
    import tree_physics_ref as TP
    spec, sp = TP.spec_of(case), TP.sim_params(case)
    root, dof, act, _ = TP.states(case, kind)
    return spec, sp, M.pack_model(spec), root, dof, act


# ------------------------------------------------------------------------------------------------ a cut in every phase
# (phase, state set, max_contacts k): the capacity cut between the oracle's entries k - 1 and k falls inside that part
# of collide() -- both entries emitted by it, the ground phases' by the same geom -- in at least CUT_ENVS envs of the
# set, so that each pass's own `slot < cap` guard decides a contact.  Sets: hand:<hand_set>, tree:<case>:<kind>,
# task:<task>:<envs>.  k = 24 / 48 on the overflow trees is the instance's MC (slot k is the first one past the
# per-team arrays).  "compact": any cut, the task model on the compact layout.  hand:ground-block is a set of its
# own (hand_set): the cube lying on the ground plane, which no other set reaches.
CUT_ENVS = 8
CUTS = (
    ("capsule ends, one pass", "tree:T16-fixed-round:overflow", 2),
    ("capsule ends, one pass", "tree:T16-fixed-round:overflow", 24),
    ("box corners", "tree:T16-fixed:overflow", 21),
    ("object on the ground", "hand:ground-block", 2),
    ("self pairs", "tree:T32-free:overflow", 48),
    ("self pairs", "hand:fingers", 1),
    ("hull vertices", "hand:forearm-block", 1),
    ("hull faces", "hand:forearm-block", 2),
    ("exact hull", "hand:hull-pen", 1),
    ("exact hull", "hand:forearm-pen", 4),
    ("egg staged", "hand:palm-egg", 2),
    ("geom-object map", "hand:palm-block", 2),
    ("geom-object map", "hand:palm-pen", 3),
    ("compact", "task:Ant:256", 2),
    ("compact", "task:Humanoid:128", 4),
)
_PHASES = {"object on the ground": O.PH_OBJ_GROUND, "capsule ends, one pass": O.PH_GROUND, "box corners": O.PH_GROUND,
           "self pairs": O.PH_PAIR,
           "hull vertices": O.PH_HULL_VERT, "hull faces": O.PH_HULL_FACE, "exact hull": O.PH_HULL_EXACT,
           "egg staged": O.PH_GEOM_OBJ, "geom-object map": O.PH_GEOM_OBJ}


def cut_id(cut):
    return f"{cut[0]}-{cut[1]}-{cut[2]}".replace(" ", "_").replace(",", "")


def cut_set(where):
    """(spec, sp, mnp, root, dof, extra, kind, lists key) of a CUTS set; extra: the hand's host env, or the actuation"""
    what, name, *rest = where.split(":")
    if what == "hand":
        spec, sp, mnp, root, dof, h = hand_set(name)
        return spec, sp, mnp, root, dof, h, kind_of(name), ("hand", name)
    if what == "tree":
        import tree_physics_ref as TP
        spec, sp, mnp, root, dof, act = tree_set(TP.CASES[name], rest[0])
        return spec, sp, mnp, root, dof, act, "none", ("tree", name, rest[0])
    spec, sp, tp, mnp, root, dof, act = task_set(name, int(rest[0]))
    return spec, sp, mnp, root, dof, act, "none", ("task", name, int(rest[0]))


def cut_envs(cut):
    """the envs of the set in which the cut at k falls inside the phase, decided from the fp64 oracle's list at the
    thresholds themselves (by the emitting part and the geom of entries k - 1 and k)"""
    phase, where, k = cut
    spec, sp, mnp, root, dof, _, _, key = cut_set(where)
    lists = cached_lists(key, mnp, sp, root, dof)
    ground_round = not any(g.gtype in (M.GT_BOX, M.GT_CONVEX) for g in spec.geoms)
    hits = []
    for e, (rows, marks, _) in enumerate(lists):
        real = (marks & BAND_OUT) == 0
        if real.sum() <= k:
            continue
        if phase == "compact":
            hits.append(e)
            continue
        ph = O.contacts_phases(mnp, sp, np.asarray(root[e]).ravel(), dof[e], DELTA, 64)[real]
        a, b = rows[real][k - 1], rows[real][k]
        ok = ph[k - 1] == ph[k] == _PHASES[phase]
        if ok and ph[k] == O.PH_GROUND:
            gt = spec.geoms[int(b[1])].gtype
            want = gt == M.GT_CAPSULE and ground_round if phase.startswith("capsule") else gt == M.GT_BOX
            ok = a[1] == b[1] and want
        if ok and ph[k] == O.PH_GEOM_OBJ:
            ok = (int(mnp["obj_type"]) == M.GT_ELLIPSOID) == (phase == "egg staged")
        if ok:
            hits.append(e)
    return hits


TASK_ROLLOUT = {"Ant": 40, "Humanoid": 25}   # control steps from the reset pose to feet on the ground


def task_set(task, n):
    """(spec, sp, tp, mnp, root, dof, act) of a locomotion task after a short oracle rollout under random actions:
    the bodies have come down on their feet"""
    if ("task", task, n) in _cache:
        return _cache["task", task, n]
    from test_gpu_parity import setup
    spec, sp, tp = setup(task)
    mnp = M.pack_model(spec)
    h = O.HostEnv(tp, spec, n)
    rng = np.random.default_rng(23)
    for t in range(TASK_ROLLOUT[task]):
        h.actions[:] = rng.uniform(-1.0, 1.0, (n, tp.num_actions)).astype(np.float32)
        h.env_step(mnp, sp, tp, seed=7, step=t, threads=8)
    out = (spec, sp, tp, mnp, h.root.copy(), h.dof.copy(), h.act_eff.copy())
    _cache["task", task, n] = out
    return out


def cached_lists(key, mnp, sp, root, dof):
    if ("lists", key) not in _cache:
        _cache["lists", key] = oracle_lists(mnp, sp, root, dof)
    return _cache["lists", key]


def with_max_contacts(sp, k):
    s = copy.copy(sp)
    s.max_contacts = k
    return s
