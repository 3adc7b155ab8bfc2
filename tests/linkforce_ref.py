"""Link forces (mg_sim_set_link_forces): the models, states and references shared by
tests/test_linkforce_host.py (the reference alone admits the inputs, on the CPU) and tests/test_gpu_linkforce.py.

The frozen oracle applies no force to a link, so nothing here asks it to.  Two facts about a force at a body's centre
of mass need only what it already has:

  * Gravity equivalence.  Forces F_b = m_b a on every body, in the env frame, are the physics of gravity g + a, and the
    oracle takes gravity in mg_sim_params.  This pins the whole step -- contacts, PD drives, limits, several substeps.
    MODES: "env" (MG_ENV_SPACE, 2 substeps) and "local" (MG_LOCAL_SPACE at 1 substep with f_b = R_b(q0)^T m_b a: the
    body frame of the launch's start is the frame of its only substep).  Every actor has an `a` of its own, so the
    oracle runs actor by actor.  A state is admitted by the oracle alone: its contact candidates within capacity before
    and after the step at g + a, no orc_step_flips flag at g or at g + a, and the oracle's step not sensitive to its
    positions (tree_physics_ref.states' criterion); at most DISCARD_CAP of the states drawn may be passed over (the
    recipe changes otherwise, not the cap: Anymal's drives hold the standing pose for that reason, see pool()).
  * Momentum identity, one link at a time.  On a free-base model without contacts, over one substep h, on a passive
    copy (every node's drive_kp, damping, stiffness, armature, frictionloss and limited 0, angular_damping 0, and no
    cap on the links' angular velocities, which clips after the solve): run once
    with a force F on body b and once without from the same (q0, v0); linear and angular momentum about the world
    origin, evaluated at the OLD pose q0 with each run's NEW velocities, differ by h F and h c_b x F exactly, c_b the
    loaded body's COM at q0 (the velocity update is M(q0) dv = h (bias + J^T F), and momentum is linear in v at a fixed
    pose).  The oracle shows it through the gravity equivalence (all bodies loaded with m_b a: h M a and
    h (sum m_b c_b) x a), and its fp32 twin's residual on the same states, x TWIN_FACTOR, bounds the kernel's.  The
    residuals are relative to the impulse h |F| (angular: times the arm |c|), and the one-link loads have |F| = M |a|,
    the twin's total, so the cancellation in the difference of two momenta is the same in both.

Models: Cartpole (8 lanes, fixed base), the quadcopter as its task configures it and the T16-free tree of
tree_physics_ref raised off the ground (16 lanes), Anymal standing on its feet (32 lanes), the AMP humanoid on its
feet (64 lanes).  The tree's bodies sit at random poses on their nodes and carry no mass of their own, so its copy
here gives every body its node's mass and puts the body's COM on the node's: the one model whose body frames differ
from its node frames.
"""
import copy
import ctypes as C

import numpy as np

import parity_stats as PS
import pyoracle as O
import tree_physics_ref as TP
from migym import _abi, configs, model as M, taskdefs

F = np.float32
ENV, LOCAL = _abi.MG_ENV_SPACE, _abi.MG_LOCAL_SPACE
MODES = {"env": (ENV, 2), "local": (LOCAL, 1)}       # name -> (rb_force_space, substeps)
LANES = {"Cartpole": 8, "Quadcopter": 16, "T16-free": 16, "Anymal": 32, "AMP": 64}
# the smallest batches that cross each instance's wave edge (64 / lanes actors per wave)
BATCHES = {"Cartpole": (9, 67), "Quadcopter": (6, 67), "T16-free": (6, 67), "Anymal": (6, 66), "AMP": (3,)}
POOL = {"Cartpole": 70, "Quadcopter": 70, "T16-free": 70, "Anymal": 69, "AMP": 8}
DISCARD_CAP = 0.05
ACC = 3.0                # every component of an actor's a is U(-ACC, ACC) m/s^2
TWIN_FACTOR = 4.0        # the project's bound on a kernel's error in units of the fp32 twin's own
_cache = {}


class Host:
    """host views of n actors for orc_simulate_views / orc_step_flips: every tensor gym.simulate reads or writes"""

    def __init__(self, spec, root, dof, act=None, tgt=None):
        self.n = n = len(root)
        nd, nb = spec.num_dofs, len(spec.bodies)
        self.root, self.dof = np.array(root, F), np.array(dof, F)
        self.act_eff = np.zeros((n, nd), F) if act is None else np.array(act, F)
        self.tgt = None if tgt is None else np.array(tgt, F)
        self.sensors = np.zeros((n, max(len(spec.sensors), 1) * 6), F)
        self.dof_force, self.ncf = np.zeros((n, nd), F), np.zeros((n, nb, 3), F)

    def views(self, lo=0, hi=None):
        v = _abi.StateViews()
        s = slice(lo, hi)
        v.root_states, v.dof_state, v.dof_actuation = O.p(self.root[s]), O.p(self.dof[s]), O.p(self.act_eff[s])
        v.sensors, v.dof_force, v.net_contact_forces = O.p(self.sensors[s]), O.p(self.dof_force[s]), O.p(self.ncf[s])
        v.dof_targets = None if self.tgt is None else O.p(self.tgt[s])
        return v

    def simulate_each(self, mnp, sps, fp32=False):
        """one simulate of every actor at its own sim parameters"""
        lib = O.lib_f32() if fp32 else O.lib()
        for e in range(self.n):
            v = self.views(e, e + 1)
            lib.orc_simulate_views(mnp.ctypes.data, C.byref(sps[e]), 1, C.byref(v), 1)
        return self

    def flags_each(self, mnp, sps):
        v = self.views()
        return np.array([O.lib().orc_step_flips(mnp.ctypes.data, C.byref(sps[e]), C.byref(v), e, PS.STEP_DELTA, PS.STEP_DF)
                         for e in range(self.n)], np.int32)


def sp_at(sp, a=None, substeps=None, tgs=False):
    """a copy of sp with gravity g + a (as the fp32 the struct holds), the substeps and the solver"""
    sp = copy.copy(sp)
    if a is not None:
        for i in range(3):
            sp.gravity[i] = F(sp.gravity[i]) + F(a[i])
    if substeps is not None:
        sp.substeps = substeps
    if tgs:
        sp.solver_type = _abi.MG_SOLVER_TGS
    return sp


def masses(spec):
    return np.array([b.mass for b in spec.bodies], np.float64)


def body_rotations(mnp, root13, dof2, nb):
    """(nb, 3, 3): R_body of every body at a state, by the oracle's orc_rigid_body_states"""
    rb = O.rigid_body_states(mnp, root13, dof2, nb).astype(np.float64)
    return np.array([M.qmat(M.qnorm(q)) for q in rb[:, 3:7]])


def forces(spec, mnp, root, dof, a, space):
    """(n, nB, 3) fp32: m_b a_e on every body of actor e, in the env frame or in the body's own at the state"""
    m = masses(spec)
    f = m[None, :, None] * np.asarray(a, np.float64)[:, None, :]
    if space == LOCAL:
        for e in range(len(root)):
            R = body_rotations(mnp, root[e], dof[e], len(m))
            f[e] = np.einsum("bji,bj->bi", R, f[e])
    return f.astype(F)


# ------------------------------------------------------------------------------------------------ the models
def tree_with_coms(spec):
    """a copy of a tree_physics_ref tree whose bodies carry their nodes' masses with their COMs on the nodes' COMs
    (the tree's bodies are massless frames at random poses on their nodes)"""
    spec = copy.deepcopy(spec)
    for b in spec.bodies:
        n = spec.nodes[b.node]
        b.mass = n.mass
        b.com = (M.qmat(M.qnorm(b.quat)).T @ (np.asarray(n.com) - np.asarray(b.pos))).tolist()
    return spec


def quad_sim_params():
    """the reference's cfg/task/Quadcopter.yaml where it differs from the Ant's: dt 0.01, 16 contacts"""
    cfg = configs.task_config("Ant", 16)
    cfg["sim"]["dt"] = 0.01
    return taskdefs.sim_params(cfg, taskdefs.QUADCOPTER_MAX_CONTACTS)


def setup(model):
    """(spec, packed model, sim params at the model's own values)"""
    if ("setup", model) in _cache:
        return _cache["setup", model]
    if model == "Cartpole":
        import simparams_ref as SR
        spec, _, sp, _ = SR.task_setup("Cartpole")
    elif model == "Quadcopter":
        spec, sp = taskdefs.quadcopter_spec(), quad_sim_params()
    elif model == "T16-free":
        case = TP.CASES[model]
        spec, sp = tree_with_coms(TP.spec_of(case)), TP.sim_params(case)
    elif model == "Anymal":
        import anymal_ref as AR
        spec, _, sp, _ = AR.task_model(AR.task_cfg(POOL[model]))
    else:
        import amp_ref as AM
        spec, _, sp, _ = AM.task_model(AM.physics_cfg(POOL[model]))
    assert abs(masses(spec).sum() - spec.total_mass()) < 1e-9 * spec.total_mass() or spec.fixed_base
    _cache["setup", model] = spec, M.pack_model(spec), sp
    return _cache["setup", model]


def pool(model):
    """(root, dof, act, tgt, a): POOL[model] drawn states before the step, their inputs, and each actor's a"""
    if ("pool", model) in _cache:
        return _cache["pool", model]
    spec, mnp, sp = setup(model)
    n, nd = POOL[model], spec.num_dofs
    rng = np.random.default_rng([17, sorted(LANES).index(model)])
    act, tgt = np.zeros((n, nd), F), None
    if model == "Cartpole":
        import simparams_ref as SR
        tp = SR.task_setup("Cartpole")[3]
        root, dof = SR.random_states(spec, tp, n, rng, (2.0, 2.0))
        root[:, :] = 0
        root[:, 2], root[:, 6] = 2.0, 1.0
        act = rng.uniform(-50, 50, (n, nd)).astype(F)
    elif model == "Quadcopter":
        root = np.zeros((n, 13), F)
        root[:, 0:2], root[:, 2] = rng.uniform(-1.5, 1.5, (n, 2)), rng.uniform(0.8, 2.5, n)
        q = np.concatenate([rng.normal(0, 0.15, (n, 3)), np.ones((n, 1))], 1)
        root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
        root[:, 7:13] = rng.normal(0, 0.5, (n, 6))
        dof = np.zeros((n, nd, 2), F)
        dof[..., 0], dof[..., 1] = rng.uniform(-0.45, 0.45, (n, nd)), rng.normal(0, 0.5, (n, nd))
        # PD targets near the positions: at stiffness 1000 on 2e-5 kg m^2 a drive closes its error within a substep,
        # and an error of 0.03 rad already makes 6 rad/s of the 4 pi the hinge rates are capped at
        tgt = (dof[..., 0] + rng.uniform(-0.03, 0.03, (n, nd))).astype(F)
    elif model == "T16-free":
        case = TP.CASES[model]
        root, dof, act = TP.dropped_pool(spec, mnp, sp, case.lanes, n, 1717, sink=False)
        root[:, 2] += 0.5     # off the ground: the contacts are the standing models' part
    elif model == "Anymal":
        import anymal_ref as AR
        ap = AR.task_model(AR.task_cfg(n))[3]
        p = AR.params_from(ap)
        root, dof, _ = AR.reset_state(p, n, int(rng.integers(1 << 30)))
        h = AR.AnymalHost(spec, root, dof, np.tile(p["default"], (n, 1)))
        for _ in range(AR.STANDING_STEPS):
            h.simulate(mnp, sp)
        root, dof = h.root.copy(), h.dof.copy()
        # the drives hold the standing pose (a zero action).  With targets drawn over the whole action range, as
        # anymal_ref.physics_states draws them, the TGS step is sensitive (tree_physics_ref's criterion, in case()) in
        # 10 of these 69 states and the fp32 twin leaves the tolerances in one: past the 5 % that may be passed over
        tgt = np.tile(p["default"], (n, 1)).astype(F)
    else:
        import amp_ref as AM
        _, _, _, r, d, t, _, _ = AM.physics_states("clip")
        root, dof, tgt = r[:n].copy(), d[:n].copy(), t[:n].copy()
    a = rng.uniform(-ACC, ACC, (n, 3)).astype(F)
    out = tuple(None if x is None else np.ascontiguousarray(x, F) for x in (root, dof, act, tgt, a))
    for x in out:
        if x is not None:
            x.setflags(write=False)
    _cache["pool", model] = out
    return out


def num_candidates(mnp, sp, root, dof):
    return np.array([len(O.contacts(mnp, sp, root[e], dof[e], 96)) for e in range(len(root))])


def case(model, mode, tgs):
    """The admitted states of (model, mode, solver), in pool order, as a dict: idx (their pool indices), scanned (how
    far into the pool the largest batch reaches), root / dof / act / tgt / a, f (the force tensor of the mode), sps
    (each actor's sim params at g + a), sp (at g), ref (the fp64 oracle's Host after the step at g + a), base (the
    same at g), cand (the most contact candidates, before or after)."""
    key = ("case", model, mode, tgs)
    if key in _cache:
        return _cache[key]
    spec, mnp, sp0 = setup(model)
    root, dof, act, tgt, a = pool(model)
    space, sub = MODES[mode]
    n = len(root)
    sp = sp_at(sp0, None, sub, tgs)
    sps = [sp_at(sp0, a[e], sub, tgs) for e in range(n)]
    ref = Host(spec, root, dof, act, tgt).simulate_each(mnp, sps)
    base = Host(spec, root, dof, act, tgt).simulate_each(mnp, [sp] * n)
    before, after = num_candidates(mnp, sp, root, dof), num_candidates(mnp, sp, ref.root, ref.dof)
    pre = Host(spec, root, dof, act, tgt)
    ok = (np.maximum(before, after) <= sp.max_contacts) & (pre.flags_each(mnp, [sp] * n) == 0) & \
        (pre.flags_each(mnp, sps) == 0) & np.isfinite(ref.root).all(1)
    # ... and, as tree_physics_ref.states asks, the oracle's own step is not sensitive there: with every position
    # moved by +-SENS_EPS (an fp32 step's rounding; one draw of the signs) its result stays within a quarter of the
    # tolerances
    rng = np.random.default_rng([29, sorted(LANES).index(model)])
    nudged = Host(spec, root, dof, act, tgt)
    nudged.root[:, 0:3] += TP.SENS_EPS * rng.choice([-1.0, 1.0], (n, 3))
    nudged.dof[..., 0] += TP.SENS_EPS * rng.choice([-1.0, 1.0], (n, spec.num_dofs))
    nudged.simulate_each(mnp, sps)
    ok &= ~(PS.env_bad(nudged.dof[..., 0], ref.dof[..., 0], 0.25 * 2e-4, 0) |
            PS.env_bad(nudged.dof[..., 1], ref.dof[..., 1], 0.25 * 2e-3, 0.25 * 2e-3) |
            PS.env_bad(nudged.root[:, 0:7], ref.root[:, 0:7], 0.25 * 2e-4, 0) |
            PS.env_bad(nudged.root[:, 7:13], ref.root[:, 7:13], 0.25 * 2e-3, 0.25 * 2e-3))
    want = max(BATCHES[model])
    idx = np.flatnonzero(ok)[:want]
    assert len(idx) == want, f"{model}/{mode}: the pool admits only {len(idx)} of the {want} states"
    pick = lambda x: None if x is None else np.ascontiguousarray(x[idx])
    out = dict(idx=idx, scanned=int(idx[-1]) + 1, root=pick(root), dof=pick(dof), act=pick(act), tgt=pick(tgt),
               a=pick(a), sps=[sps[e] for e in idx], sp=sp, cand=int(np.maximum(before, after)[idx].max()))
    out["f"] = forces(spec, mnp, out["root"], out["dof"], out["a"], space)
    for k in ("ref", "base"):
        h, src = Host(spec, out["root"], out["dof"], out["act"], out["tgt"]), ref if k == "ref" else base
        for name in ("root", "dof", "sensors", "dof_force", "ncf"):
            getattr(h, name)[:] = getattr(src, name)[idx]
        out[k] = h
    _cache[key] = out
    return out


def outside(spec, got, ref, n):
    """tree_physics_ref.outside: the one-step tolerances (sensors where the model has any)"""
    out = TP.outside(got, ref, n)
    return out if spec.sensors else [c for c in out if c[0] != "sensors"]


def moved(model, mode, tgs):
    """per admitted state: the oracle's result at g + a leaves the one-step tolerances of its result at g"""
    c = case(model, mode, tgs)
    n = len(c["idx"])
    bad = np.zeros(n, bool)
    for _, x, y, atol, rtol in outside(setup(model)[0], c["ref"], c["base"], n):
        bad |= PS.env_bad(x, y, atol, rtol)
    return bad


def compare(test, model, mode, tgs, n, got):
    """`got` (root, dof, sensors, dof_force, ncf of the first n admitted states after one simulate under gravity g
    with the case's force tensor) against the fp64 oracle at g + a by the one-step rule of tree_physics_ref.compare.
    The states carry no orc_step_flips flag, so no env is exempt.  Returns the largest error of each check."""
    spec = setup(model)[0]
    c = case(model, mode, tgs)
    for x in (got.root, got.dof, got.dof_force, got.ncf):
        assert np.isfinite(x).all()
    assert np.abs(got.dof[..., 0] - c["dof"][:n, :, 0]).max() > 1e-4, "the step moved nothing"
    worst, bad = {}, np.zeros(n, bool)
    for name, x, y, atol, rtol in outside(spec, got, c["ref"], n):
        eb = PS.env_bad(x, y, atol, rtol)
        err = float(np.abs(x.astype(np.float64) - y).max())
        print(f"{test} {name}: max err {err:.3g} (atol {atol:.3g}, rtol {rtol:.3g}), envs outside {int(eb.sum())} / {n}")
        PS.record(test, name, x, y, envs_outside=int(eb.sum()), atol=atol, rtol=rtol)
        worst[name] = err
        bad |= eb
    assert not bad.any(), f"{test}: envs {np.flatnonzero(bad)[:10].tolist()} leave the one-step tolerances"
    return worst


# ------------------------------------------------------------------------------------------------ momentum identity
MOMENTUM_MODELS = ("Quadcopter", "Anymal", "AMP")
MOMENTUM_ACC = 5.0       # |a| of the twin's runs; a one-link load is M |a| along x, y or z


def passive(spec):
    """the passive copy: no drive, damping, stiffness, armature, dry friction or limit on any node, no link damping,
    and no cap on the links' angular velocities (mg_model.link_max_ang_vel 0: the cap clips hinge rates after the
    solve, and a one-link load of M |a| on the humanoid's thigh takes a hip past its 100 rad/s)"""
    spec = copy.deepcopy(spec)
    for n in spec.nodes:
        n.drive_kp = n.damping = n.stiffness = n.armature = n.frictionloss = 0.0
        n.limited = 0
    spec.angular_damping = 0.0
    spec.max_angular_velocity = 0.0
    return spec


def momentum_setup(model):
    """(passive spec, packed, sim params at one substep, root, dof, body, direction): 3 nB contact-free states at
    z = 3 m with random poses and velocities; actor e loads body e % nB along axis (e // nB) % 3"""
    if ("mom", model) in _cache:
        return _cache["mom", model]
    spec0, _, sp0 = setup(model)
    spec = passive(spec0)
    nb, nd = len(spec.bodies), spec.num_dofs
    n = 3 * nb
    rng = np.random.default_rng([23, MOMENTUM_MODELS.index(model)])
    sp = sp_at(sp0, None, 1)
    mnp = M.pack_model(spec)
    draws = 8 * n     # a random pose of the humanoid often touches itself: the first n draws without a candidate
    root = np.zeros((draws, 13), F)
    root[:, 0:2], root[:, 2] = rng.uniform(-1, 1, (draws, 2)), 3.0
    q = rng.normal(size=(draws, 4))
    root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    root[:, 7:13] = rng.normal(0, 0.5, (draws, 6))
    lo, hi = (np.array(x) for x in taskdefs.dof_limits(spec0))
    dof = np.zeros((draws, nd, 2), F)
    dof[..., 0] = lo + (hi - lo) * rng.uniform(0.1, 0.9, (draws, nd))
    dof[..., 1] = rng.normal(0, 1.0, (draws, nd))
    free = np.flatnonzero(num_candidates(mnp, sp, root, dof) == 0)[:n]
    assert len(free) == n, f"{model}: only {len(free)} of {draws} draws are contact-free"
    root, dof = np.ascontiguousarray(root[free]), np.ascontiguousarray(dof[free])
    body, axis = np.arange(n) % nb, (np.arange(n) // nb) % 3
    assert abs(sum(spec.nodes[k].mass for k in {b.node for b in spec.bodies}) - spec.total_mass()) < 1e-9
    for x in (root, dof):
        x.setflags(write=False)
    _cache["mom", model] = spec, mnp, sp, root, dof, body, axis
    return _cache["mom", model]


def momentum(spec, mnp, root0, dof0, root1, dof1):
    """(P, L, c): per actor, linear momentum and angular momentum about the world origin at the pose of (root0, dof0)
    with the velocities of (root1, dof1), and every body's COM there (n, nB, 3).  Body poses and COM velocities come
    from orc_rigid_body_states; the root row's linear velocity is the root body's COM velocity at the new pose, so it
    is rebuilt for pose 0: v_c1 - w1 x (R1 com0 + p1 - p0) + w1 x (R0 com0).  The p1 - p0 term undoes the last thing
    the integrator does: it carries the root twist, a spatial velocity about the root origin, to the origin's new
    place (Team::integrate(): vn = vo + w x dp; the oracle likewise).  Without it the identity is off by h |w|."""
    n, nb = len(root0), len(spec.bodies)
    m = masses(spec)
    com0 = np.asarray(spec.bodies[0].com, np.float64)
    P, L, cs = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, nb, 3))
    for e in range(n):
        r0, r1 = root0[e].astype(np.float64), root1[e].astype(np.float64)
        R0, R1 = M.qmat(M.qnorm(r0[3:7])), M.qmat(M.qnorm(r1[3:7]))
        w1 = r1[10:13]
        v = r1[7:10] - np.cross(w1, R1 @ com0 + (r1[0:3] - r0[0:3])) + np.cross(w1, R0 @ com0)
        row = np.concatenate([r0[0:7], v, w1])
        d = np.stack([dof0[e, :, 0], dof1[e, :, 1]], -1)
        rb = O.rigid_body_states(mnp, row, d, nb).astype(np.float64)
        seen = set()
        for b in range(nb):
            body = spec.bodies[b]
            Rb = M.qmat(M.qnorm(rb[b, 3:7]))
            cs[e, b] = rb[b, 0:3] + Rb @ np.asarray(body.com)
            if body.node in seen:     # bodies welded onto one node (the AMP humanoid's hands): the node counts once
                continue
            seen.add(body.node)
            nd_ = spec.nodes[body.node]
            i = nd_.inertia
            In = np.array([[i[0], i[3], i[4]], [i[3], i[1], i[5]], [i[4], i[5], i[2]]])
            Rn = Rb @ M.qmat(M.qnorm(body.quat)).T
            w = rb[b, 10:13]
            c = rb[b, 0:3] - Rn @ np.asarray(body.pos) + Rn @ np.asarray(nd_.com)       # the node's COM
            vc = rb[b, 7:10] + np.cross(w, c - cs[e, b])
            P[e] += nd_.mass * vc
            L[e] += nd_.mass * np.cross(c, vc) + Rn @ In @ Rn.T @ w
    return P, L, cs


def momentum_residuals(dP, dL, Fw, c, h):
    """per actor: |dP - h F| / (h |F|) and |dL - h c x F| / (h |F| max(|c|, 1))"""
    imp = h * np.linalg.norm(Fw, axis=1)
    lin = np.linalg.norm(dP - h * Fw, axis=1) / imp
    ang = np.linalg.norm(dL - h * np.cross(c, Fw), axis=1) / (imp * np.maximum(np.linalg.norm(c, axis=1), 1.0))
    return lin, ang


def one_link_loads(model):
    """(n, nB, 3) fp32 env-frame force tensor of momentum_setup's actors, and each actor's force (n, 3)"""
    spec, _, _, root, _, body, axis = momentum_setup(model)
    n, nb = len(root), len(spec.bodies)
    Fw = np.zeros((n, 3))
    Fw[np.arange(n), axis] = spec.total_mass() * MOMENTUM_ACC
    f = np.zeros((n, nb, 3), F)
    f[np.arange(n), body] = Fw
    return f, f[np.arange(n), body].astype(np.float64)


def oracle_momentum_residuals(model, fp32):
    """(lin, ang) per actor of the oracle (fp64, or its fp32 twin) on momentum_setup's states: every body loaded with
    m_b a through gravity g + a, a = MOMENTUM_ACC along the actor's axis; the identity then reads h M a and
    h (sum m_b c_b) x a"""
    key = ("mom oracle", model, fp32)
    if key in _cache:
        return _cache[key]
    spec, mnp, sp, root, dof, _, axis = momentum_setup(model)
    n = len(root)
    a = np.zeros((n, 3), F)
    a[np.arange(n), axis] = MOMENTUM_ACC
    with_f = Host(spec, root, dof).simulate_each(mnp, [sp_at(sp, a[e]) for e in range(n)], fp32)
    without = Host(spec, root, dof).simulate_each(mnp, [sp] * n, fp32)
    P1, L1, cs = momentum(spec, mnp, root, dof, with_f.root, with_f.dof)
    P0, L0, _ = momentum(spec, mnp, root, dof, without.root, without.dof)
    m = masses(spec)
    Mtot = m.sum()
    # what the struct holds: fp32(g + a) - fp32(g)
    da = np.array([[F(F(sp.gravity[i]) + a[e, i]) - F(sp.gravity[i]) for i in range(3)] for e in range(n)], np.float64)
    ctot = np.einsum("b,ebi->ei", m, cs) / Mtot
    _cache[key] = momentum_residuals(P1 - P0, L1 - L0, Mtot * da, ctot, sp.dt / sp.substeps)
    return _cache[key]
