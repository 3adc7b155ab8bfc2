"""References of the dynamics tensors and the operational-space controller (shared by tests/test_gpu_dynamics.py,
tests/test_dynamics_host.py and tests/golden/make_osc_golden.py): the fp64 oracle's mass matrix and body-origin
Jacobian of a fixed-base model table; synthetic trees (random_tree) with an independent fp64 formula for both; an fp64
numpy statement of the controller (osc_reference); an fp32 emulation of the kernel's pivots (osc_pivot_ratios); and the
test cases the CPU and GPU tests share."""
import copy
import os

import numpy as np

import pyoracle as O
from migym import _abi, model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRANKA_JSON = os.path.join(GOLDEN, "franka_panda.json")
OSC_NPZ = os.path.join(GOLDEN, "osc_franka.npz")


def oracle_model(spec):
    """the packed model with joint damping and stiffness zeroed: orc_mass_matrix adds their implicit terms
    (h b + h^2 k) to the diagonal, which the mass-matrix tensor does not carry"""
    s = copy.deepcopy(spec)
    for nd in s.nodes:
        nd.damping, nd.stiffness = 0.0, 0.0
    return M.pack_model(s)


def oracle_sim_params():
    sp = _abi.SimParams()
    sp.dt, sp.substeps = 1.0 / 60.0, 2
    return sp


def oracle_mass_matrix(mnp, root13, q):
    q = np.asarray(q, np.float32)
    dof = np.stack([q, np.zeros_like(q)], 1)
    return O.mass_matrix(mnp, oracle_sim_params(), np.asarray(root13, np.float32), dof)


def oracle_jacobian(spec, mnp, root13, q):
    """(nB, 6, nD) Jacobian of every body ORIGIN, [linear; angular], world frame: column j is the body's velocity
    under qd = e_j (orc_rigid_body_states reports the COM's: v_o = v_com - w x R body_com)"""
    nd, nb = spec.num_dofs, len(spec.bodies)
    J = np.zeros((nb, 6, nd))
    root13 = np.asarray(root13, np.float32)
    com = np.array([b.com for b in spec.bodies], np.float64)
    lever = None   # R_body com, world frame: the pose does not depend on qd, so the first column's serves them all
    for j in range(nd):
        dof = np.zeros((nd, 2), np.float32)
        dof[:, 0] = q
        dof[j, 1] = 1.0
        rb = O.rigid_body_states(mnp, root13, dof, nb).astype(np.float64)
        if lever is None:
            lever = np.stack([M.qmat(rb[b, 3:7]) @ com[b] if com[b].any() else np.zeros(3) for b in range(nb)])
        w = rb[:, 10:13]
        J[:, 0:3, j] = rb[:, 7:10] - np.cross(w, lever)
        J[:, 3:6, j] = w
    return J


OSC_EDGES_NPZ = os.path.join(GOLDEN, "osc_franka_edges.npz")


# ------------------------------------------------------------------------------------------------ synthetic trees
def random_tree(num_nodes, seed, chain=False, extra_bodies=0, chain_prefix=0, physics=False, free_base=False,
                num_geoms=0, num_pairs=0, num_sensors=0, boxes=True):
    """A synthetic fixed-base articulation that reaches what the Franka chain and Cartpole cannot: branching, more
    than 16 / 32 nodes, slides in the interior, body origins off the joint anchor, several bodies on one node.

    Node 0 is the fixed root; node i >= 1 hangs on a parent drawn from [max(0, i - 6), i) (i - 1 when ``chain``, or
    when i <= ``chain_prefix``: the first chain_prefix DOFs then form a serial arm), is a slide with probability 0.3
    and a hinge otherwise, and has a random unit axis, a random rest rotation, an anchor in U(-0.15, 0.15)^3, a COM in
    U(-0.05, 0.05)^3, a random SPD inertia about the COM (0.01 A A^T + 0.005 I), a mass in U(0.2, 2) and an armature
    in U(0, 0.05); limits are +-1.  One body per node at a random origin in U(-0.1, 0.1)^3 of the node frame, plus
    ``extra_bodies`` more on random nodes (the fixed-joint case: a non-identity body_node map).  No geoms, pairs,
    actuators or sensors; gravity off.

    The keyword options after ``chain_prefix`` make the tree step-ready (tests/tree_physics_ref.py); they draw from a
    generator of their own, so the tree above is the same with and without them.  ``physics``: gravity on, joint
    damping in U(0.05, 0.5), stiffness in U(0, 5), frictionloss in U(0.05, 0.3) on every fourth DOF.  ``free_base``:
    node 0 is a free joint (its mass and inertia are the ones drawn above).  ``num_geoms`` geoms cycling sphere,
    capsule, box over the nodes in a random order (distinct nodes until every node has one), a centre in
    U(-0.03, 0.03)^3 of the node frame and a rotation of up to 0.3 rad about a random axis, colliding with the ground
    only (``boxes`` False: spheres and capsules alone, the kernel's one-pass ground path).  ``num_pairs`` self-collision pairs of sphere / capsule geoms whose nodes are neither equal nor parent and
    child: those whose bounding spheres are apart at the zero pose, the nearest first (random poses then put some in
    contact, few of them deep), then the ones that overlap there, the shallowest first.  ``num_sensors`` force sensors on leaf bodies (as many as the
    tree has leaves, at most)."""
    rng = np.random.default_rng(seed)

    def unit(k):
        v = rng.normal(size=k)
        return v / np.linalg.norm(v)

    nodes, bodies = [], []
    for i in range(num_nodes):
        if i == 0:
            parent, jt = -1, M.JT_FIXED
        else:
            parent = i - 1 if (chain or i <= chain_prefix) else int(rng.integers(max(0, i - 6), i))
            jt = M.JT_SLIDE if rng.random() < 0.3 else M.JT_HINGE
        axis, r0, t = unit(3), unit(4), rng.uniform(-0.15, 0.15, 3)
        com, A = rng.uniform(-0.05, 0.05, 3), rng.normal(size=(3, 3))
        I = 0.01 * A @ A.T + 0.005 * np.eye(3)
        mass, arm = rng.uniform(0.2, 2.0), rng.uniform(0.0, 0.05)
        if i == 0:   # the root's frame is the base pose itself
            t, r0 = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])
        nodes.append(M.Node(name=f"j{i}", parent=parent, jtype=jt, t=t.tolist(), r0=r0.tolist(), axis=axis.tolist(),
                            body=i, mass=float(mass), com=com.tolist(),
                            inertia=[I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]], armature=float(arm),
                            lower=-1.0, upper=1.0, limited=1))
        bodies.append(M.Body(name=f"b{i}", node=i, pos=rng.uniform(-0.1, 0.1, 3).tolist(), quat=unit(4).tolist(),
                             parent_body=parent))
    for e in range(extra_bodies):
        nd = int(rng.integers(1, num_nodes))
        bodies.append(M.Body(name=f"x{e}", node=nd, pos=rng.uniform(-0.1, 0.1, 3).tolist(), quat=unit(4).tolist(),
                             parent_body=nd))
    jt = [n.jtype for n in nodes]
    par = [n.parent for n in nodes]
    assert any(jt[i] == M.JT_HINGE and jt[par[i]] == M.JT_SLIDE for i in range(1, num_nodes)), "no hinge below a slide"
    assert any(jt[i] == M.JT_SLIDE and jt[par[i]] == M.JT_HINGE for i in range(1, num_nodes)), "no slide below a hinge"
    spec = M.ModelSpec(name=f"tree{num_nodes}_{seed}", fixed_base=1, nodes=nodes, bodies=bodies, geoms=[], pairs=[],
                       actuators=[], dof_names=[n.name for n in nodes[1:]], gravity_off=1)
    if physics or free_base or num_geoms or num_pairs or num_sensors:
        _step_ready(spec, np.random.default_rng([seed, 1]), physics, free_base, num_geoms, num_pairs, num_sensors,
                    boxes)
    return spec


def _step_ready(spec, rng, physics, free_base, num_geoms, num_pairs, num_sensors, boxes):
    """random_tree's step options, in place"""
    nn = len(spec.nodes)
    if physics:
        spec.gravity_off = 0
        for i, nd in enumerate(spec.nodes[1:]):
            nd.damping, nd.stiffness = float(rng.uniform(0.05, 0.5)), float(rng.uniform(0.0, 5.0))
            if i % 4 == 2:
                nd.frictionloss = float(rng.uniform(0.05, 0.3))
    if free_base:
        spec.fixed_base, spec.nodes[0].jtype = 0, M.JT_FREE
    order = np.concatenate([rng.permutation(nn) for _ in range(-(-max(num_geoms, 1) // nn))])
    for g in range(num_geoms):
        gt = (M.GT_SPHERE, M.GT_CAPSULE, M.GT_BOX)[g % (3 if boxes else 2)]
        size = {M.GT_SPHERE: [rng.uniform(0.03, 0.06), 0.0, 0.0],
                M.GT_CAPSULE: [rng.uniform(0.02, 0.04), rng.uniform(0.04, 0.1), 0.0],
                M.GT_BOX: rng.uniform(0.03, 0.08, 3).tolist()}[gt]
        ax = rng.normal(size=3)
        quat = M.quat_from_axis_angle(ax, rng.uniform(-0.3, 0.3))
        nd = int(order[g])
        spec.geoms.append(M.Geom(name=f"g{g}", gtype=gt, node=nd, body=nd, size=[float(v) for v in size],
                                 pos=rng.uniform(-0.03, 0.03, 3).tolist(), quat=quat.tolist(),
                                 filter=M.COLLIDE_GROUND))
    if num_pairs:
        root = np.array([0, 0, 0, 0, 0, 0, 1.0] + [0.0] * 6)
        R, x = node_frames(spec, root, np.zeros(spec.num_dofs))
        ctr = [x[g.node] + R[g.node] @ np.asarray(g.pos) for g in spec.geoms]
        cand = []
        for i, gi in enumerate(spec.geoms):
            for j in range(i + 1, len(spec.geoms)):
                gj = spec.geoms[j]
                if M.GT_BOX in (gi.gtype, gj.gtype) or gi.node == gj.node:
                    continue
                if spec.nodes[gi.node].parent == gj.node or spec.nodes[gj.node].parent == gi.node:
                    continue
                reach = gi.size[0] + gi.size[1] + gj.size[0] + gj.size[1]   # the two bounding spheres
                gap = float(np.linalg.norm(ctr[i] - ctr[j])) - reach
                cand.append((gap if gap >= 0 else 1e3 - gap, i, j))
        assert len(cand) >= num_pairs, f"only {len(cand)} candidate pairs"
        spec.pairs = [[i, j] for _, i, j in sorted(cand)[:num_pairs]]
    if num_sensors:
        parents = {n.parent for n in spec.nodes}
        spec.sensors = [i for i in range(1, nn) if i not in parents][:num_sensors]


def node_frames(spec, root13, q):
    """(R, x): world rotation and origin of every node frame, plain fp64 numpy; FK as include/migym.h states it: a
    hinge has R = R_p R0 exp([axis] q), x = x_p + R_p t; a slide R = R_p R0, x = x_p + R_p t + (R_p R0 axis) q"""
    root13, q = np.asarray(root13, np.float64), np.asarray(q, np.float64)
    nn = len(spec.nodes)
    R, x = [None] * nn, [None] * nn
    R[0], x[0] = M.qmat(M.qnorm(root13[3:7])), root13[0:3].copy()
    for i in range(1, nn):
        n, p = spec.nodes[i], spec.nodes[i].parent
        Rp0 = R[p] @ M.qmat(M.qnorm(n.r0))
        ax = np.asarray(n.axis, np.float64)
        if n.jtype == M.JT_HINGE:
            K = _skew(ax)
            R[i] = Rp0 @ (np.eye(3) + np.sin(q[i - 1]) * K + (1.0 - np.cos(q[i - 1])) * K @ K)
            x[i] = x[p] + R[p] @ np.asarray(n.t)
        else:
            R[i] = Rp0
            x[i] = x[p] + R[p] @ np.asarray(n.t) + (Rp0 @ ax) * q[i - 1]
    return R, x


def ancestors(spec, node):
    """the nodes on ``node``'s chain, itself included, the root excluded"""
    out = []
    while node > 0:
        out.append(node)
        node = spec.nodes[node].parent
    return out


def random_states(spec, n, seed, qmax=1.0):
    """n actors: root (n, 13) fp32 with a random base position and unit quaternion, q (n, nD) fp32 in U(-qmax, qmax)"""
    rng = np.random.default_rng(seed)
    root = np.zeros((n, 13), np.float32)
    root[:, 0:3] = rng.uniform(-1, 1, (n, 3))
    qt = rng.normal(size=(n, 4))
    root[:, 3:7] = qt / np.linalg.norm(qt, axis=1, keepdims=True)
    q = rng.uniform(-qmax, qmax, (n, spec.num_dofs)).astype(np.float32)
    return root, q


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def independent_mass_matrix_and_jacobian(spec, root13, q):
    """(M (nD, nD), J (nB, 6, nD) [linear; angular] of every body origin) in plain fp64 numpy, from the definition
    M = diag(armature) + sum over links of m Jv^T Jv + Jw^T (R I R^T) Jw with Jv at the link's COM -- no composite
    inertias, no spatial vectors, nothing shared with the oracle's CRBA.  FK as include/migym.h states it: a hinge has
    R = R_p R0 exp([axis] q), x = x_p + R_p t; a slide R = R_p R0, x = x_p + R_p t + (R_p R0 axis) q."""
    root13 = np.asarray(root13, np.float64)
    q = np.asarray(q, np.float64)
    nn, nd, nb = len(spec.nodes), spec.num_dofs, len(spec.bodies)
    R, x, a = [None] * nn, [None] * nn, [None] * nn
    R[0], x[0] = M.qmat(M.qnorm(root13[3:7])), root13[0:3].copy()
    for i in range(1, nn):
        n, p = spec.nodes[i], spec.nodes[i].parent
        Rp0 = R[p] @ M.qmat(M.qnorm(n.r0))
        ax = np.asarray(n.axis, np.float64)
        a[i] = Rp0 @ ax
        if n.jtype == M.JT_HINGE:
            K = _skew(ax)
            R[i] = Rp0 @ (np.eye(3) + np.sin(q[i - 1]) * K + (1.0 - np.cos(q[i - 1])) * K @ K)
            x[i] = x[p] + R[p] @ np.asarray(n.t)
        else:
            assert n.jtype == M.JT_SLIDE
            R[i] = Rp0
            x[i] = x[p] + R[p] @ np.asarray(n.t) + a[i] * q[i - 1]

    def point_jacobian(node, c):
        Jv, Jw = np.zeros((3, nd)), np.zeros((3, nd))
        for k in ancestors(spec, node):
            if spec.nodes[k].jtype == M.JT_HINGE:
                Jv[:, k - 1], Jw[:, k - 1] = np.cross(a[k], c - x[k]), a[k]
            else:
                Jv[:, k - 1] = a[k]
        return Jv, Jw

    Mq = np.diag([n.armature for n in spec.nodes[1:]]).astype(np.float64)
    for l in range(1, nn):
        n = spec.nodes[l]
        Jv, Jw = point_jacobian(l, x[l] + R[l] @ np.asarray(n.com))
        i6 = n.inertia
        I = np.array([[i6[0], i6[3], i6[4]], [i6[3], i6[1], i6[5]], [i6[4], i6[5], i6[2]]])
        Mq += n.mass * Jv.T @ Jv + Jw.T @ (R[l] @ I @ R[l].T) @ Jw
    J = np.zeros((nb, 6, nd))
    for b, body in enumerate(spec.bodies):
        J[b, 0:3], J[b, 3:6] = point_jacobian(body.node, x[body.node] + R[body.node] @ np.asarray(body.pos))
    return Mq, J


def off_chain_mask(spec):
    """(nB, nD) bool: DOF d is not on body b's chain (its Jacobian column is structurally zero)"""
    m = np.ones((len(spec.bodies), spec.num_dofs), bool)
    for b, body in enumerate(spec.bodies):
        for k in ancestors(spec, body.node):
            m[b, k - 1] = False
    return m


# ------------------------------------------------------------------------------------------------ OSC
def osc_reference(Mm, J, q, qd, dpose, eef_vel, kp, kd, kp_null, kd_null, default, limit=None, dtype=np.float64):
    """include/migym.h's mg_osc_torques formula as the maths reads, batched numpy with explicit inverses:
    A = J M^-1 J^T, u = J^T A^-1 (kp dpose - kd eef_vel) + (I - J^T A^-1 J M^-1) M u_null,
    u_null = kd_null (-qd) + kp_null (((default - q + pi) mod 2 pi) - pi), clamped to +-limit (None: no clamp).
    Mm (n, k, k), J (n, 6, k), q, qd (n, k), dpose, eef_vel (n, 6); gains per axis / per DOF or scalars.
    dtype float64: returns u.  dtype float32: every array and scalar in fp32; returns (u32, ref_err) with
    ref_err = max |u32 - u64| over the unclamped torques, u64 from the same inputs in double."""
    def run(dt):
        c = lambda v: np.asarray(v, dt)   # noqa: E731
        Mx, Jx, pi = c(Mm), c(J), dt(np.pi)
        k = Mx.shape[-1]
        Jt = np.swapaxes(Jx, 1, 2)
        Minv = np.linalg.inv(Mx)
        Ainv = np.linalg.inv(Jx @ Minv @ Jt)
        w = c(kp) * c(dpose) - c(kd) * c(eef_vel)
        u = Jt @ Ainv @ w[..., None]
        un = c(kd_null) * -c(qd) + c(kp_null) * (np.mod(c(default) - c(q) + pi, dt(2) * pi) - pi)
        u = u + (np.eye(k, dtype=dt) - Jt @ Ainv @ Jx @ Minv) @ (Mx @ un[..., None])
        assert u.dtype == dt
        return u[..., 0]

    def clamp(u):
        return u if limit is None else np.clip(u, -np.asarray(limit, u.dtype), np.asarray(limit, u.dtype))

    u64 = run(np.float64)
    if dtype == np.float64:
        return clamp(u64)
    u32 = run(np.float32)
    return clamp(u32), float(np.abs(u32.astype(np.float64) - u64).max())


def wrap_margin(default, q):
    """distance of (default - q + pi) mod 2 pi from 0 and from 2 pi: where fp32 and fp64 could wrap differently"""
    y = np.mod(np.asarray(default, np.float64) - np.asarray(q, np.float64) + np.pi, 2 * np.pi)
    return np.minimum(y, 2 * np.pi - y)


def osc_pivot_ratios(Mm, J, dtype=np.float64):
    """The pivot ratios s_j / X_jj of the two Cholesky factorisations of csrc/dynamics_tensors.hpp's osc_solve, in
    its order of operations (M = L L^T, Y = L^-1 J^T, A = Y^T Y = G G^T; one multiply and one add per step, no FMA),
    on one actor's M (k, k) and J (6, k) padded to 7 DOFs as the kernel pads them.  Returns (rM (7), rA (6)); a pivot
    <= 0 is carried on as the kernel carries it (sqrt(max(s, 1e-30)))."""
    f = dtype
    k = Mm.shape[0]
    N = 7
    Mp, Jp = np.eye(N, dtype=f), np.zeros((6, N), f)
    Mp[:k, :k], Jp[:, :k] = np.asarray(Mm, f), np.asarray(J, f)

    def chol(X, n):
        L, di, r = np.zeros((n, n), f), np.zeros(n, f), np.zeros(n)
        for j in range(n):
            s = X[j, j]
            for c in range(j):
                s = f(s - f(L[j, c] * L[j, c]))
            with np.errstate(divide="ignore", invalid="ignore"):
                r[j] = float(s) / float(X[j, j]) if X[j, j] != 0 else (0.0 if s == 0 else np.sign(s) * np.inf)
            di[j] = f(1.0) / f(np.sqrt(max(s, f(1e-30))))
            for i in range(j + 1, n):
                t = X[i, j]
                for c in range(j):
                    t = f(t - f(L[i, c] * L[j, c]))
                L[i, j] = f(t * di[j])
        return L, di, r

    with np.errstate(over="ignore", invalid="ignore"):
        L, di, rM = chol(Mp, N)
        Y = np.zeros((N, 6), f)
        for c in range(6):
            for i in range(N):
                s = Jp[c, i]
                for j in range(i):
                    s = f(s - f(L[i, j] * Y[j, c]))
                Y[i, c] = f(s * di[i])
        A = np.zeros((6, 6), f)
        for a in range(6):
            for b in range(a + 1):
                s = f(0)
                for j in range(N):
                    s = f(s + f(Y[j, a] * Y[j, b]))
                A[a, b] = A[b, a] = s
        _, _, rA = chol(A, 6)
    return rM, rA


# ------------------------------------------------------------------------------------------------ shared test cases
# the smallest trees that reach each edge of the kernels' node loops (one lane owns nodes tl, tl + 16, tl + 32)
TREES = {
    "branched17": dict(num_nodes=17, seed=1),                     # one node in the second round
    "branched33x": dict(num_nodes=33, seed=2, extra_bodies=7),    # third round, mask bits >= 32, MG_MAX_BODIES bodies
    "branched40": dict(num_nodes=40, seed=3),                     # MG_MAX_NODES
    "chain40": dict(num_nodes=40, seed=4, chain=True),            # the deepest ancestor walk
}
TREE_ACTORS = 66   # 16 full waves of four teams and a half-filled one
# the serial-arm variant for the controller: nodes 1..6 are a chain, body 6 (on node 6) carries the Jacobian.  Tree
# and pose seeds were picked on the CPU from the fp64 figures alone (tests/test_dynamics_host.py asserts them): of the
# seeds whose 66 poses all have cond(J M^-1 J^T) <= 5e4 on the six arm DOFs and leading-block pivot ratios >= 1e-2 at
# arm_dofs 3 and 5, the one closest to the condition limit (4.06e4).
ARM_TREE = dict(num_nodes=17, seed=12, chain_prefix=6)
ARM_POSE_SEED, ARM_BODY, ARM_SPREAD = 4, 6, 0.1
BASES = [((-0.45, 0.0, 1.125), (0.0, 0.0, 0.0, 1.0)),
         ((0.45, 0.1, 1.0), (0.18257419, -0.36514837, 0.73029674, 0.54772256))]   # yawed and tilted

_cache = {}


def _frozen(*xs):
    for x in xs:
        x.setflags(write=False)
    return xs


def tree(name):
    if ("tree", name) not in _cache:
        _cache["tree", name] = random_tree(**(ARM_TREE if name == "arm17" else TREES[name]))
    return _cache["tree", name]


def oracle_tensors(spec, root, q):
    """(Mo (n, nD, nD), Jo (n, nB, 6, nD)) of the oracle for n actors"""
    mnp = oracle_model(spec)
    Mo = np.stack([oracle_mass_matrix(mnp, root[a], q[a]) for a in range(len(q))])
    Jo = np.stack([oracle_jacobian(spec, mnp, root[a], q[a]) for a in range(len(q))])
    return Mo, Jo


def tree_case(name, n):
    """the first n of the tree's TREE_ACTORS actors (alternating base poses, a different q in U(-1, 1) per actor) and
    the oracle's tensors for them: computed once per (tree, n), shared, read-only"""
    if ("case", name, n) not in _cache:
        spec = tree(name)
        root, q = random_states(spec, TREE_ACTORS, 7000 + len(spec.nodes))
        for a in range(TREE_ACTORS):
            if a % 3:   # two fixed base poses and, every third actor, the random one
                root[a, 0:3], root[a, 3:7] = BASES[a % 2]
        root, q = root[:n].copy(), q[:n].copy()
        _cache["case", name, n] = _frozen(root, q, *oracle_tensors(spec, root, q))
    return _cache["case", name, n]


def arm_case(n=TREE_ACTORS):
    """the controller's actors on the serial-arm tree: q within ARM_SPREAD of one pose, the two base poses
    alternating; (root, q, qd, dpose, eef_vel, Mo, Jo) with Jo the oracle's Jacobian of body ARM_BODY"""
    if ("arm", n) not in _cache:
        spec = tree("arm17")
        rng = np.random.default_rng(ARM_POSE_SEED)
        q0 = rng.uniform(-1, 1, spec.num_dofs)
        q = (q0 + rng.uniform(-ARM_SPREAD, ARM_SPREAD, (TREE_ACTORS, spec.num_dofs))).astype(np.float32)
        root = np.zeros((TREE_ACTORS, 13), np.float32)
        for a in range(TREE_ACTORS):
            root[a, 0:3], root[a, 3:7] = BASES[a % 2]
        qd = rng.uniform(-1, 1, (TREE_ACTORS, spec.num_dofs)).astype(np.float32)
        dpose = (rng.uniform(-1, 1, (TREE_ACTORS, 6)) * [0.1, 0.1, 0.1, 0.5, 0.5, 0.5]).astype(np.float32)
        root, q, qd, dpose = root[:n].copy(), q[:n].copy(), qd[:n].copy(), dpose[:n].copy()
        Mo, Jo = oracle_tensors(spec, root, q)
        Jo = np.ascontiguousarray(Jo[:, ARM_BODY])
        eef_vel = np.einsum("nij,nj->ni", Jo, qd.astype(np.float64)).astype(np.float32)
        _cache["arm", n] = _frozen(root, q, qd, dpose, eef_vel, Mo, Jo)
    return _cache["arm", n]


# gains of the arm-tree controller tests: distinct per axis / per DOF, kd != 2 sqrt(kp)
ARM_GAINS = dict(kp=[150.0, 90.0, 210.0, 60.0, 120.0, 30.0], kd=[11.0, 23.0, 17.0, 5.0, 29.0, 7.0],
                 kp_null=[10.0, 4.0, 16.0, 7.0, 13.0, 5.5, 19.0], kd_null=[3.0, 5.5, 2.0, 7.5, 1.5, 6.0, 4.5],
                 default_dof_pos=[0.3, -0.2, 0.5, -0.4, 0.1, 0.6, -0.1])
