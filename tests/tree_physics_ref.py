"""Step-ready synthetic articulations for the three step-kernel instances no task model selects (csrc/dispatch.hpp:
(16, 16, 24, 24, 32), (32, 32, 48, 48, 192) and (64, 40, 48, 48, 192)), with their states, the fp64 oracle's step and
the comparison, shared by tests/test_gpu_tree_physics.py (the GPU against the oracle) and
tests/test_tree_physics_host.py (the oracle's fp32 twin against it, through the same rule).

A case is a dynamics_ref.random_tree with gravity, joint damping / stiffness / frictionloss, ground geoms, self pairs
and sensors, and three kinds of states of CASE_ACTORS actors:

  * dropped: a random base pose with the lowest geom point U(-3, 3) cm from the plane, q in U(-1.05, 1.05) (limits
    are +-1, the limit margin 0.1: a third of the joints carry a limit row), qd ~ N(0, 1), the base twist ~ N(0, 0.5)
    when the base is free, effort actuation in U(-2, 2);
  * settled: the dropped states rolled SETTLE_STEPS steps by the fp64 oracle, so that contacts rest;
  * overflow (OVERFLOW_CASES): drawn like dropped, then every actor sunk a centimetre at a time, SINK_STEPS at most,
    until the fp64 oracle counts more contact candidates than max_contacts.  max_contacts is the instance's MC (24 or
    48), so collide() cuts the list at the last slot of the per-team arrays and the step runs on a full list.

On the 16- and 32-lane cases every fourth dropped actor is lowered further, until it has more contact candidates than
the team has lanes (dropped_pool); the settled states roll from the pool without that.

States are drawn into a pool and taken in pool order under conditions on the INPUTS, all decided by the fp64
oracle alone: the contact candidates of the state and of the oracle's state after the step stay at or below
max_contacts (overflow turns this round: more than max_contacts and fewer than ORACLE_MAXC = 64 before the step, the
most the oracle can count), no self pair overlaps by more than
PAIR_DEPTH (3 cm, as deep as the lowest geom may stand in the ground: a 40-link chain thrown apart at the
depenetration speed is a stress state, where the oracle's own fp32 build leaves the tolerances), the oracle's step
is not sensitive to SENS_EPS on the positions, and the first SMALL_N actors' steps pass no discontinuity (orc_step_flips == 0): the batches of 1 and 6 actors are prefixes of the 66, and a single
flagged env of 6 would already be 17 % of them, past the 5 % the exemption rule may reach.

Past capacity two more things hold.  The overflow states are also chosen so that the cut matters: at most half of
them may be states where the oracle's step with room for every candidate (max_contacts = 64) stays within the
tolerances of its step at capacity; past that such a state is passed over in pool order (it changes the selection of
T16-free alone, whose free base rests on 24 redundant ground contacts: 17 of its first 66 usable states feel the
cut).  truncation_moves() recomputes that, and tests/test_tree_physics_host.py asserts at least half.  And the
dropped states of LOWERED run once more with max_contacts = 8 (states(..., cap=8): the same states, the oracle's step
recomputed at that capacity), the p->max_contacts < MC branch.

Every case stands at the Ant's sim parameters.  sim_params, states and compare take point=<a name of
simparams_ref.POINTS> to move them (tests/test_gpu_simparams.py, tests/test_simparams_host.py): the states are chosen
again at the point by the same rule, and point=None is the Ant's parameters and the states of before, bit for bit.

The fixed bases and the sink depth.  A fixed-base tree cannot rise out of the ground, so a sunk one is a stress state
(contact forces 1e6-1e12 N, most hinge rates at the 64 rad/s cap).  The fp32 twin on the whole pools (264 actors per
case, no filter): no env leaves the tolerances on T16-fixed and T32-fixed at any depth up to 60 cm; 2 of 144
past-capacity actors do on T16-fixed-round (39 and 40 cm), 4 of 114 on T64-fixed (28-48 cm), 20 of 134 on
T64-fixed-chain (from 24 cm), each 1.1-18 x the velocity tolerance and none flagged.  They do not gather at the deep
end, and a bound that excludes them leaves too few states: the pool yields 66 usable states only from 42 cm
(T16-fixed-round), 60 cm (T32-fixed), 50 cm (T64-fixed) and 42 cm (T64-fixed-chain) on.  So SINK_STEPS_FIXED stays at
the 60 cm of SINK_STEPS; T64-fixed and T64-fixed-chain are left out of OVERFLOW_CASES (the twin leaves the rule in 4
and 6 of their 66 states); and T16-fixed-round draws its overflow pool from overflow_seed = state_seed + 1000, the
first of state_seed + 1000 k at which the twin stays within the rule (at state_seed itself actor 2 is 1.96 x outside
the velocity tolerance, unflagged).
"""
import dataclasses

import numpy as np

import dynamics_ref as D
import parity_stats as PS
import pyoracle as O
import simparams_ref as SR
from migym import _abi, configs, model as M, taskdefs

CASE_ACTORS = 66      # 16 full waves of four 16-lane teams and a half-filled one; 33 waves of two; 66 of one
SMALL_N = 6           # a partial wave at 4 and at 2 actors per wave
ACTOR_COUNTS = (1, SMALL_N, CASE_ACTORS)
SETTLE_STEPS = 10
POOL = 4 * CASE_ACTORS


@dataclasses.dataclass(frozen=True)
class Case:
    lanes: int             # the team size of the instance the case must run on
    tree: dict             # random_tree arguments
    max_contacts: int
    state_seed: int
    # what puts the case past the next smaller instance (asserted on the spec): each a (count name, more than)
    past: tuple
    reaches: tuple         # the paths its inputs must reach (asserted on the host): see reach_report
    overflow_seed: int = None   # the overflow pool's seed where state_seed's draw leaves the twin's rule

    def name(self):
        return (f"T{self.lanes}-{'free' if self.tree.get('free_base') else 'fixed'}"
                f"{'-chain' if self.tree.get('chain') else ''}{'' if self.tree.get('boxes', True) else '-round'}")


def _tree(num_nodes, seed, **kw):
    return dict(num_nodes=num_nodes, seed=seed, physics=True, num_sensors=M.MAX_SENSORS, **kw)


# The smallest shapes that reach each path no task model runs.  Tree seeds: the first (from 1) whose tree has a hinge
# below a slide and a slide below a hinge (random_tree asserts both).  "geoms>T": a second round of the lane-per-geom
# loops; "cand>T": more contact candidates than team lanes.
CASES = {c.name(): c for c in (
    Case(16, _tree(12, 1, num_geoms=20, num_pairs=8), 24, 101, (("nodes", 9), ("geoms", 16), ("pairs", 0)),
         ("box", "cand>T", "pair", "limit", "geoms>T")),
    # spheres and capsules alone take the one-pass ground loop (team_physics.hpp collide, ground_round): its second round
    Case(16, _tree(12, 1, num_geoms=20, num_pairs=8, boxes=False), 24, 108, (("nodes", 9), ("geoms", 16), ("pairs", 0)),
         ("cand>T", "pair", "limit", "geoms>T"), overflow_seed=1108),
    Case(16, _tree(10, 1, num_geoms=18, num_pairs=8, free_base=True), 24, 102, (("nodes", 9), ("geoms", 16)),
         ("box", "cand>T", "pair", "limit", "geoms>T")),
    Case(32, _tree(30, 1, num_geoms=40, num_pairs=170), 48, 103, (("nodes", 24), ("geoms", 24), ("pairs", 160)),
         ("box", "cand>T", "pair", "limit", "geoms>T")),
    Case(32, _tree(26, 1, num_geoms=36, num_pairs=100, free_base=True), 48, 104, (("nodes", 24), ("geoms", 24)),
         ("box", "cand>T", "pair", "limit", "geoms>T")),
    Case(64, _tree(40, 3, num_geoms=44, num_pairs=100), 48, 105, (("nodes", 32),), ("box", "pair", "limit")),
    Case(64, _tree(40, 4, num_geoms=44, num_pairs=100, chain=True), 48, 106, (("nodes", 32),),
         ("box", "pair", "limit")),
    Case(64, _tree(34, 1, num_geoms=40, num_pairs=100, free_base=True), 48, 107, (("lanes", 32), ("nodes", 32)),
         ("box", "pair", "limit")),
)}
KINDS = ("dropped", "settled")
# past capacity (module docstring): the cases whose pool yields CASE_ACTORS usable overflow states, and the lowered
# capacity the dropped states of two of them also run at (the p->max_contacts < MC branch of collide())
OVERFLOW_CASES = ("T16-fixed", "T16-fixed-round", "T16-free", "T32-fixed", "T32-free", "T64-free")
LOWERED = (("T16-fixed", 8), ("T32-free", 8))
SINK_STEPS = 60          # an actor sinks a centimetre at a time, at most this far (as dropped_pool)
SINK_STEPS_FIXED = 60    # ... and a fixed-base tree at most this far: no tighter bound helps (module docstring)
ORACLE_MAXC = 64         # the oracle's own list ends here: it cannot count a state with this many candidates
_cache = {}


def spec_of(case):
    if ("spec", case.name()) not in _cache:
        _cache["spec", case.name()] = D.random_tree(**case.tree)
    return _cache["spec", case.name()]


def counts(spec):
    return dict(nodes=len(spec.nodes), geoms=len(spec.geoms), pairs=len(spec.pairs),
                lanes=max((0 if spec.fixed_base else 6) + spec.num_dofs, len(spec.sensors)))


def sim_params(case, tgs=False, cap=None, point=None):
    """cap: a lowered max_contacts (None: the case's, which equals its instance's MC); point: a name of
    simparams_ref.POINTS, the fields it sets replacing the Ant's (None: the Ant's own)"""
    sp = taskdefs.sim_params(configs.task_config("Ant", 16), case.max_contacts if cap is None else cap)
    if tgs:
        sp.solver_type = _abi.MG_SOLVER_TGS
    return SR.apply(sp, point, case.name())


class TreeHost:
    """The views orc_step_flips and orc_simulate_views read of a model without a task: root states, DOF states, effort
    actuation, sensors, DOF forces and the net contact force tensor (pyoracle.HostEnv without its task buffers)."""

    def __init__(self, spec, root, dof, act):
        self.n = len(root)
        self.root, self.dof, self.act_eff = (np.array(a, np.float32) for a in (root, dof, act))
        self.sensors = np.zeros((self.n, max(len(spec.sensors), 1) * 6), np.float32)
        self.dof_force = np.zeros((self.n, spec.num_dofs), np.float32)
        self.ncf = np.zeros((self.n, len(spec.bodies), 3), np.float32)

    def views(self):
        v = _abi.StateViews()
        v.root_states, v.dof_state, v.dof_actuation = O.p(self.root), O.p(self.dof), O.p(self.act_eff)
        v.sensors, v.dof_force, v.net_contact_forces = O.p(self.sensors), O.p(self.dof_force), O.p(self.ncf)
        return v

    def simulate(self, mnp, sp, fp32=False):
        v = self.views()
        (O.lib_f32() if fp32 else O.lib()).orc_simulate_views(mnp.ctypes.data, O.C.byref(sp), self.n, O.C.byref(v), 8)
        return self


# ------------------------------------------------------------------------------------------------ states
def lowest_point(spec, root13, q):
    """z of the lowest point of any geom (spheres, capsule end spheres, box corners)"""
    R, x = D.node_frames(spec, root13, q)
    z = np.inf
    for g in spec.geoms:
        Rg = R[g.node] @ M.qmat(M.qnorm(g.quat))
        c = x[g.node] + R[g.node] @ np.asarray(g.pos)
        if g.gtype == M.GT_SPHERE:
            z = min(z, c[2] - g.size[0])
        elif g.gtype == M.GT_CAPSULE:
            z = min(z, c[2] - abs(Rg[2, 2]) * g.size[1] - g.size[0])
        else:
            z = min(z, c[2] - np.abs(Rg[2]) @ np.asarray(g.size))
    return z


def dropped_pool(spec, mnp, sp, lanes, n, seed, sink=True):
    rng = np.random.default_rng(seed)
    nd = spec.num_dofs
    root = np.zeros((n, 13), np.float32)
    root[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    qt = rng.normal(size=(n, 4))
    root[:, 3:7] = qt / np.linalg.norm(qt, axis=1, keepdims=True)
    dof = np.zeros((n, nd, 2), np.float32)
    dof[..., 0] = rng.uniform(-1.05, 1.05, (n, nd))
    dof[..., 1] = rng.normal(0, 1, (n, nd))
    twist = rng.normal(0, 0.5, (n, 6))
    if not spec.fixed_base:
        root[:, 7:13] = twist
    gap = rng.uniform(-0.03, 0.03, n)
    for a in range(n):
        root[a, 2] = gap[a] - lowest_point(spec, root[a], dof[a, :, 0])
    # every fourth actor sinks on, a centimetre at a time, until it has more contact candidates than the team has
    # lanes (a geom below the plane stays a candidate however deep) or another centimetre would take it past capacity
    # (the 64-lane team has more lanes than contacts: nothing to reach there; and not before settling: a fixed-base
    # tree stays buried, ten steps on its contact forces are ~1e6 N and their fp32 rounding alone leaves the tolerances)
    for a in range(3, n, 4) if sink and lanes < sp.max_contacts else ():
        for _ in range(60):
            if len(O.contacts(mnp, sp, root[a], dof[a], 64)) > lanes:
                break
            root[a, 2] -= 0.01
            if len(O.contacts(mnp, sp, root[a], dof[a], 64)) > sp.max_contacts:
                root[a, 2] += 0.01
                break
    act = rng.uniform(-2, 2, (n, nd)).astype(np.float32)
    return root, dof, act


def overflow_pool(spec, mnp, sp, n, seed):
    """the dropped pool (no actor lowered for "cand>T"), then every actor sunk a centimetre at a time until the fp64
    oracle counts more than max_contacts candidates, SINK_STEPS cm at most (SINK_STEPS_FIXED for a fixed base, which
    cannot rise out of the ground: see the comment in dropped_pool); an actor that never gets there stays in the
    pool and fails the capacity condition of states()"""
    root, dof, act = dropped_pool(spec, mnp, sp, 0, n, seed, sink=False)
    for a in range(n):
        for _ in range(SINK_STEPS_FIXED if spec.fixed_base else SINK_STEPS):
            if len(O.contacts(mnp, sp, root[a], dof[a], ORACLE_MAXC)) > sp.max_contacts:
                break
            root[a, 2] -= 0.01
    return root, dof, act


SENS_EPS = 1e-6      # parity_stats.simulate_sensitive's perturbation
PAIR_DEPTH = 0.03    # a self pair may overlap as far as the lowest geom may stand in the ground


def num_candidates(mnp, sp, root, dof):
    """per actor: the contact candidates (-1: a self pair overlaps by more than PAIR_DEPTH)"""
    out = np.zeros(len(root), int)
    for a in range(len(root)):
        c = O.contacts(mnp, sp, root[a], dof[a], 64)
        out[a] = -1 if (c[c[:, 8] >= 0, 7] < -PAIR_DEPTH).any() else len(c)
    return out


def states(case, kind, tgs=False, cap=None, point=None):
    """(root, dof, act, host64): CASE_ACTORS actors' states before the step, read-only, and the fp64 oracle's TreeHost
    after one simulate from them; computed once per (case, kind, solver, capacity, point).  cap: the states chosen at
    the case's own capacity, with the oracle's step recomputed at max_contacts = cap.  point: the sim parameters moved
    to a point of simparams_ref.POINTS; the states are chosen again there by the same rule (candidates, flags and
    sensitivity all depend on the parameters), from the pool of state_seed + 1000 k where the admission rule took
    the k-th next seed"""
    key = ("states", case.name(), kind, tgs, cap, point)
    if key in _cache:
        return _cache[key]
    spec, sp = spec_of(case), sim_params(case, tgs, point=point)
    mnp = M.pack_model(spec)
    if cap is not None:
        root, dof, act, _ = states(case, kind, tgs, point=point)
        _cache[key] = root, dof, act, TreeHost(spec, root, dof, act).simulate(mnp, sim_params(case, tgs, cap, point))
        return _cache[key]
    shift = 1000 * SR.seed_shift(point, case.name()) if point is not None else 0
    if kind == "overflow":
        root, dof, act = overflow_pool(spec, mnp, sp, POOL, (case.overflow_seed or case.state_seed) + shift)
    else:
        root, dof, act = dropped_pool(spec, mnp, sp, case.lanes, POOL, case.state_seed + shift, sink=kind == "dropped")
    if kind == "settled":
        h = TreeHost(spec, root, dof, act)
        for _ in range(SETTLE_STEPS):
            h.simulate(mnp, sp)
        root, dof = h.root, h.dof
        ok = np.isfinite(root).all(axis=1) & np.isfinite(dof).all(axis=(1, 2))
        root, dof, act = root[ok], dof[ok], act[ok]
    after = TreeHost(spec, root, dof, act).simulate(mnp, sp)
    before = num_candidates(mnp, sp, root, dof)
    if kind == "overflow":   # the capacity condition turned round: past it, and countable by the oracle
        fits = (before > case.max_contacts) & (before < ORACLE_MAXC)
    else:
        fits = (before >= 0) & (before <= case.max_contacts) & \
            (np.abs(num_candidates(mnp, sp, after.root, after.dof)) <= case.max_contacts)
    # ... and the oracle's own step is not sensitive there: with every position moved by +-SENS_EPS (an fp32 step's
    # rounding; one draw of the signs), its result stays within a quarter of the tolerances
    n = len(root)
    rng = np.random.default_rng([case.state_seed, 2])
    moved = TreeHost(spec, root, dof, act)
    moved.root[:, 0:3] += SENS_EPS * rng.choice([-1.0, 1.0], (n, 3))
    moved.dof[..., 0] += SENS_EPS * rng.choice([-1.0, 1.0], (n, spec.num_dofs))
    moved.simulate(mnp, sp)
    fits &= ~(PS.env_bad(moved.dof[..., 0], after.dof[..., 0], 0.25 * 2e-4, 0) |
              PS.env_bad(moved.dof[..., 1], after.dof[..., 1], 0.25 * 2e-3, 0.25 * 2e-3) |
              PS.env_bad(moved.root[:, 0:7], after.root[:, 0:7], 0.25 * 2e-4, 0) |
              PS.env_bad(moved.root[:, 7:13], after.root[:, 7:13], 0.25 * 2e-3, 0.25 * 2e-3))
    _cache[("pool", case.name(), kind, tgs) + (() if point is None else (point,))] = (n, int(fits.sum()))
    flags = O.step_flips(mnp, sp, TreeHost(spec, root, dof, act), PS.STEP_DELTA, PS.STEP_DF)
    # overflow: at most half of the states may be ones where the cut does not matter to the oracle itself (its step
    # with room for every candidate stays within the tolerances of its step at capacity): past that, such a state is
    # passed over, so that a kernel that ignored the cut could not pass
    inert = np.zeros(n, bool)
    if kind == "overflow":
        roomy = TreeHost(spec, root, dof, act).simulate(mnp, sim_params(case, tgs, ORACLE_MAXC, point))
        inert[:] = True
        for _, a, b, atol, rtol in outside(roomy, after, n):
            inert &= ~PS.env_bad(a, b, atol, rtol)
    keep = []
    for a in np.flatnonzero(fits):
        if inert[a] and inert[keep].sum() >= CASE_ACTORS // 2:
            continue
        if len(keep) >= SMALL_N or flags[a] == 0:
            keep.append(a)
        if len(keep) == CASE_ACTORS:
            break
    assert len(keep) == CASE_ACTORS, f"{case.name()}/{kind}: the pool holds only {len(keep)} usable states"
    root, dof, act = (np.ascontiguousarray(x[keep]) for x in (root, dof, act))
    for x in (root, dof, act):
        x.setflags(write=False)
    _cache[key] = root, dof, act, TreeHost(spec, root, dof, act).simulate(mnp, sp)
    return _cache[key]


def pgs_step_of_tgs_states(case, kind):
    """the fp64 oracle's PGS step from the states of the TGS case (states(case, kind, tgs=True)): where a TGS result
    must NOT end"""
    spec = spec_of(case)
    root, dof, act, _ = states(case, kind, True)
    return TreeHost(spec, root, dof, act).simulate(M.pack_model(spec), sim_params(case))


# ------------------------------------------------------------------------------------------------ what the inputs reach
def reach_report(case, kind, tgs=False):
    """which of the paths the case is there for its CASE_ACTORS states reach, by the fp64 oracle's contact list:
    box: a box corner at or below the plane; cand>T: more candidates than team lanes; pair: a self-pair contact;
    limit: a joint within the limit margin; geoms>T: a geom of index >= T in contact; most: the largest count"""
    spec, sp = spec_of(case), sim_params(case, tgs)
    mnp = M.pack_model(spec)
    root, dof, act, _ = states(case, kind, tgs)
    out = dict.fromkeys(("box", "cand>T", "pair", "limit", "geoms>T"), False)
    most = 0
    for a in range(len(root)):
        c = O.contacts_full(mnp, sp, root[a], dof[a], 64)
        most = max(most, len(c))
        ground = c[c[:, 2] < 0]
        out["box"] |= any(spec.geoms[int(g)].gtype == M.GT_BOX and d <= 0 for g, d in zip(ground[:, 1], ground[:, 10]))
        out["cand>T"] |= len(c) > case.lanes
        out["pair"] |= bool((c[:, 2] >= 0).any())
        out["geoms>T"] |= bool((c[:, 1] >= case.lanes).any())
    out["limit"] = bool((np.abs(dof[..., 0]) > 1.0 - sp.limit_margin).any())
    out["most"] = most
    return out


# ------------------------------------------------------------------------------------------------ the comparison
def outside(got, ref, n):
    """[(name, got, ref, atol, rtol)] of the one-step tolerances, the references cut to the first n envs"""
    f_h, s_h, c_h = ref.dof_force[:n], ref.sensors[:n], ref.ncf[:n]
    return [("root pose", got.root[:, 0:7], ref.root[:n, 0:7], 2e-4, 0),
            ("dof pos", got.dof[..., 0], ref.dof[:n, :, 0], 2e-4, 0),
            ("root twist", got.root[:, 7:13], ref.root[:n, 7:13], 2e-3, 2e-3),
            ("dof vel", got.dof[..., 1], ref.dof[:n, :, 1], 2e-3, 2e-3),
            ("dof force", got.dof_force, f_h, 1e-2 * max(1.0, np.abs(f_h).max()), 0),
            ("sensors", got.sensors, s_h, 1e-2 * max(1.0, np.abs(s_h).max()), 0),
            ("net contact forces", got.ncf, c_h, 1e-2 * max(1.0, np.abs(c_h).max()), 0)]


def truncation_moves(case, kind, tgs=False, cap=None):
    """per env: the fp64 oracle's step with room for every candidate (max_contacts = ORACLE_MAXC) leaves the one-step
    tolerances of its step at the capacity under test -- the cut changes the result there, so an implementation that
    ignored it would be caught"""
    spec = spec_of(case)
    root, dof, act, ref = states(case, kind, tgs, cap)
    roomy = TreeHost(spec, root, dof, act).simulate(M.pack_model(spec), sim_params(case, tgs, ORACLE_MAXC))
    bad = np.zeros(len(root), bool)
    for _, a, b, atol, rtol in outside(roomy, ref, len(root)):
        bad |= PS.env_bad(a, b, atol, rtol)
    return bad


def candidates_before(case, kind, tgs=False):
    """per env: the fp64 oracle's count of contact candidates before the step (at most ORACLE_MAXC)"""
    spec = spec_of(case)
    root, dof, act, _ = states(case, kind, tgs)
    return np.abs(num_candidates(M.pack_model(spec), sim_params(case, tgs), root, dof))


def compare(test, case, kind, n, got, tgs=False, reach_cap=PS.REACH_CAP, cap=None, point=None):
    """`got`: a TreeHost-like result (root, dof, sensors, dof_force, ncf) of one simulate of the case's first n states
    by the implementation under test.  Every env within the one-step tolerances of the fp64 oracle (positions 2e-4,
    velocities 2e-3 + 2e-3 |v|, DOF forces / sensors / net contact forces 1 % of the batch's largest), unless
    orc_step_flips puts its step at a discontinuity (parity_stats.assert_steps_explained: reach at most 5 %, no
    sensitivity fallback, nothing unexplained); finite; and the states moved.  Returns the exemption record."""
    spec, sp = spec_of(case), sim_params(case, tgs, cap, point)
    root, dof, act, ref = states(case, kind, tgs, cap, point)
    for x in (got.root, got.dof, got.sensors, got.dof_force, got.ncf):
        assert np.isfinite(x).all()
    assert np.abs(got.dof[..., 0] - dof[:n, :, 0]).max() > 1e-3, "the step moved nothing"
    if spec.fixed_base:
        np.testing.assert_array_equal(got.root, root[:n])   # a fixed root is left as it was
    else:
        assert np.abs(got.root[:, 0:3] - root[:n, 0:3]).max() > 1e-3
    bad = np.zeros(n, bool)
    for name, a, b, atol, rtol in outside(got, ref, n):
        eb = PS.env_bad(a, b, atol, rtol)
        PS.record(test, name, a, b, envs_outside=int(eb.sum()), atol=atol, rtol=rtol)
        bad |= eb
    pre = TreeHost(spec, root[:n], dof[:n], act[:n])
    flags = PS.step_flags(M.pack_model(spec), sp, pre)
    return PS.assert_steps_explained(test, bad[None], flags[None], sens=None, reach_cap=reach_cap,
                                     allow_unexplained=0.0)


TGS_CASES = ("T16-fixed", "T32-free", "T64-fixed")   # one per instance with solver_type TGS


def assert_case_inputs(case):
    """On the host: the spec's counts put the case past the next smaller instance; every actor's contact candidates
    are within capacity; and the states reach the paths the case is there for (reach_report), in both kinds of
    states -- but for "cand>T", which only the dropped states reach (dropped_pool lowers some of them for it)."""
    spec, sp = spec_of(case), sim_params(case)
    cnt = counts(spec)
    for what, more_than in case.past:
        assert cnt[what] > more_than, f"{case.name()}: {what} = {cnt[what]} fits a smaller instance (<= {more_than})"
    assert cnt["lanes"] <= case.lanes and cnt["nodes"] <= M.MAX_NODES
    mnp = M.pack_model(spec)
    for kind in KINDS:
        root, dof, act, ref = states(case, kind)
        for r, d in ((root, dof), (ref.root, ref.dof)):
            nc = np.abs(num_candidates(mnp, sp, r, d))
            assert nc.max() <= case.max_contacts, f"{case.name()}/{kind}: {nc.max()} candidates"
        rep = reach_report(case, kind)
        missing = [k for k in case.reaches if not rep[k] and (k != "cand>T" or kind == "dropped")]
        assert not missing, f"{case.name()}/{kind}: the states do not reach {missing} ({rep})"
