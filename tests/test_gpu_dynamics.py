"""GPU tests of the dynamics tensors and the fused operational-space controller (include/migym.h: mg_dynamics_bind,
mg_dynamics_refresh, mg_osc_torques).

The references are the fp64 oracle (tests/dynamics_ref.py: its CRBA mass matrix and, column by column, its rigid-body
velocities under qd = e_j) and the reference's own ``_compute_osc_torques`` (tests/golden/osc_franka.npz, written by
tests/golden/make_osc_golden.py).  Actor counts are the smallest that cross the team layout's edges (one 16-lane
team per actor, four per wave): 6 = a partial wave, 66 = 16 full waves and a half-filled one; the OSC golden's 64 is
16 full waves (and one full wave of the injected path's lane-per-actor kernel).

The OSC tests print max |u_gpu - u_ref64| / ref_err (ref_err = 1.13e-3 N m) before they assert; the figures measured
on the MI355X are in their docstrings and in DESIGN.md §10.

The synthetic trees (tests/dynamics_ref.py: random_tree, TREES) reach what the Franka chain and Cartpole cannot: a
second and third round of the lane-per-node loops (17, 33, 40 nodes), branching (ancestor masks with holes, bits >= 32,
exact zeros off the chain), slides in the interior, body origins off the anchor, 40 bodies, and a 30 KB per-block LDS
carve-up in which a stride error between teams corrupts the neighbouring actor.  tests/test_dynamics_host.py holds
the oracle to an independent fp64 formula on the same trees first.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dynamics_ref as R
import migym
from dr_trace import defaults, layout
from migym import _abi, configs, model as M, taskdefs
from migym.dynamics import DynamicsTensors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HAND, GRIP = "panda_hand", "panda_grip_site"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


@functools.lru_cache(maxsize=None)
def franka():
    return M.load_json(R.FRANKA_JSON)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(R.OSC_NPZ))


@functools.lru_cache(maxsize=None)
def edges():
    return dict(np.load(R.OSC_EDGES_NPZ))


class Sim:
    """a sim handle on a model table with its state tensors on the device (no task layer)"""

    def __init__(self, lib, spec, root, q, qd=None, props=None):
        self.lib, self.spec, self.n = lib, spec, root.shape[0]
        nd = spec.num_dofs
        dof = np.stack([q, np.zeros_like(q) if qd is None else qd], -1).astype(np.float32)
        self.root = torch.from_numpy(np.array(root, np.float32)).to(DEV)   # (a copy: the shared cases are read-only)
        self.dof = torch.from_numpy(dof.reshape(self.n * nd, 2)).to(DEV)
        self.act = torch.zeros(self.n * nd, device=DEV)
        self.props = None if props is None else torch.from_numpy(np.ascontiguousarray(props, np.float32)).to(DEV)
        v = _abi.StateViews()
        v.root_states, v.dof_state, v.dof_actuation = self.root.data_ptr(), self.dof.data_ptr(), self.act.data_ptr()
        if props is not None:
            v.env_props, v.env_props_stride = self.props.data_ptr(), props.shape[1]
        self.views = v
        sp = taskdefs.sim_params(configs.task_config("Cartpole", 4), 8)
        self.mnp = M.pack_model(spec)
        self.sim = C.c_void_p()
        _abi.check(lib.mg_sim_create(self.mnp.ctypes.data, C.byref(sp), self.n, 0, C.byref(self.sim)), lib)
        _abi.check(lib.mg_sim_bind(self.sim, C.byref(v)), lib)
        self.dyn = DynamicsTensors(lib, self.sim, spec, self.n, DEV)

    def tensors(self):
        """(J, M) refreshed from the bound state, as numpy"""
        J, Mm = self.dyn.acquire_jacobian(), self.dyn.acquire_mass_matrix()
        self.dyn.refresh()
        torch.cuda.synchronize()
        return J.cpu().numpy(), Mm.cpu().numpy()

    def close(self):
        if self.sim is not None:
            self.lib.mg_sim_destroy(self.sim)
            self.sim = None


@functools.lru_cache(maxsize=None)
def franka_case(n):
    """n Franka actors (two per env on differently rotated bases, random joint positions within the limits) and
    the oracle's mass matrices and Jacobians for them -- computed once, shared by the tests, never written to"""
    spec = franka()
    rng = np.random.default_rng(1000 + n)
    lo = np.array([x.lower for x in spec.nodes[1:]])
    hi = np.array([x.upper for x in spec.nodes[1:]])
    q = (lo + (hi - lo) * rng.uniform(0.02, 0.98, (n, spec.num_dofs))).astype(np.float32)
    root = np.zeros((n, 13), np.float32)
    bases = [((-0.45, 0.0, 1.125), (0.0, 0.0, 0.0, 1.0)),                  # franka_reach_MA.py:912-918, agent 0
             ((0.45, 0.1, 1.0), (0.18257419, -0.36514837, 0.73029674, 0.54772256))]   # yawed and tilted
    for a in range(n):
        root[a, 0:3], root[a, 3:7] = bases[a % 2]
    mnp = R.oracle_model(spec)
    Mo = np.stack([R.oracle_mass_matrix(mnp, root[a], q[a]) for a in range(n)])
    Jo = np.stack([R.oracle_jacobian(spec, mnp, root[a], q[a]) for a in range(n)])
    for x in (q, root, Mo, Jo):
        x.setflags(write=False)
    return root, q, Mo, Jo


def check_tensors(J, Mm, Jo, Mo):
    """the project's 1e-4 relative rule: M within 1e-4 max diag(M), J within 1e-4 max(1, |J|), per actor"""
    n, nd = Mm.shape[0], Mm.shape[1]
    assert J.shape == (n, Jo.shape[1] - 1, 6, nd) and np.isfinite(J).all() and np.isfinite(Mm).all()
    for a in range(n):
        tol = 1e-4 * np.diag(Mo[a]).max()
        err = np.abs(Mm[a] - Mo[a]).max()
        assert err <= tol, f"actor {a}: |M - M_oracle| = {err:.3g} > {tol:.3g}"
        ej = np.abs(J[a] - Jo[a, 1:]) / np.maximum(1.0, np.abs(Jo[a, 1:]))
        assert ej.max() <= 1e-4, f"actor {a}: Jacobian off by {ej.max():.3g} (1e-4 allowed)"


def test_cartpole_tensors_through_vectask(lib):
    """slide + hinge, the shipped asset, the gym-named VecTask calls"""
    n = 5
    env = migym.make(seed=0, task="Cartpole", num_envs=n, sim_device=DEV, rl_device=DEV, headless=True)
    spec = env.model_spec
    rng = np.random.default_rng(5)
    q = np.stack([rng.uniform(-2, 2, n), rng.uniform(-3.1, 3.1, n)], 1).astype(np.float32)
    env.dof_state.view(n, 2, 2)[..., 0] = torch.from_numpy(q).to(DEV)
    J, Mm = env.acquire_jacobian_tensor(), env.acquire_mass_matrix_tensor()
    assert J.shape == (n, len(spec.bodies) - 1, 6, 2) and Mm.shape == (n, 2, 2)
    env.refresh_jacobian_tensors()
    env.refresh_mass_matrix_tensors()   # served by the launch above
    torch.cuda.synchronize()
    root = env.root_states.cpu().numpy()
    mnp = R.oracle_model(spec)
    Mo = np.stack([R.oracle_mass_matrix(mnp, root[a], q[a]) for a in range(n)])
    Jo = np.stack([R.oracle_jacobian(spec, mnp, root[a], q[a]) for a in range(n)])
    assert np.abs(Mo).max() > 0 and np.abs(Jo).max() > 0
    check_tensors(J.cpu().numpy(), Mm.cpu().numpy(), Jo, Mo)
    # a state change through the task ends the pairing: both calls see the new state
    env.step(torch.zeros((n, 1), device=DEV))
    env.refresh_mass_matrix_tensors()
    env.refresh_jacobian_tensors()
    torch.cuda.synchronize()
    q2 = env.dof_pos.cpu().numpy()
    root2 = env.root_states.cpu().numpy()
    Mo2 = np.stack([R.oracle_mass_matrix(mnp, root2[a], q2[a]) for a in range(n)])
    Jo2 = np.stack([R.oracle_jacobian(spec, mnp, root2[a], q2[a]) for a in range(n)])
    check_tensors(J.cpu().numpy(), Mm.cpu().numpy(), Jo2, Mo2)
    env.close()


@pytest.mark.parametrize("n", [6, 66])
def test_franka_tensors_match_oracle(lib, n):
    spec = franka()
    root, q, Mo, Jo = franka_case(n)
    s = Sim(lib, spec, root, q)
    J, Mm = s.tensors()
    s.close()
    check_tensors(J, Mm, Jo, Mo)
    assert np.array_equal(Mm, Mm.transpose(0, 2, 1)), "M must equal its transpose bit for bit"
    # bodies joined by fixed joints move as one: the grip site's rows are the hand's plus the lever arm
    hb, gb = spec.body_index(HAND), spec.body_index(GRIP)
    assert spec.bodies[hb].node == spec.bodies[gb].node
    Jh, Jg = J[:, hb - 1].astype(np.float64), J[:, gb - 1].astype(np.float64)
    assert np.array_equal(Jh[:, 3:6], Jg[:, 3:6])
    mnp = R.oracle_model(spec)
    for a in range(n):
        # lever = o_grip - o_hand, from the oracle's body positions
        rb = R.O.rigid_body_states(mnp, root[a], np.stack([q[a], 0 * q[a]], 1), len(spec.bodies))
        lever = rb[gb, 0:3].astype(np.float64) - rb[hb, 0:3]
        assert np.linalg.norm(lever) > 0.05
        want = Jh[a, 0:3] + np.cross(Jh[a, 3:6].T, lever).T
        assert np.abs(Jg[a, 0:3] - want).max() <= 1e-5


def test_env_props_masses_reach_the_tensors(lib):
    """domain randomization: the tensors describe the actor that is simulated"""
    spec, n, k = franka(), 6, 2
    root, q, _, _ = franka_case(n)
    s0 = Sim(lib, spec, root, q)
    J0, M0 = s0.tensors()
    s0.close()
    props = np.tile(defaults(spec), (n, 1))
    assert props.shape[1] == layout(spec)[0]
    W = _abi.MG_EP_NODE_WIDTH
    props[k, 0:W * len(spec.nodes):W] *= 2.0
    s1 = Sim(lib, spec, root, q, props=props)
    J1, M1 = s1.tensors()
    s1.close()
    arm = np.diag([x.armature for x in spec.nodes[1:]])
    want = 2.0 * (M0[k].astype(np.float64) - arm) + arm
    assert np.abs(M1[k] - want).max() <= 1e-5 * np.abs(want).max()
    keep = [a for a in range(n) if a != k]
    assert np.array_equal(M1[keep], M0[keep]) and np.array_equal(J1, J0)


def osc_sim(lib, n):
    g = golden()
    return Sim(lib, franka(), g["root_states"][:n], g["q"][:n], g["qd"][:n]), g


def osc_kwargs(g, clamp):
    return dict(jac_body=int(g["jac_body"]), arm_dofs=7, kp=float(g["kp"]), kp_null=float(g["kp_null"]),
                default_dof_pos=g["default_dof_pos"][:7].tolist(),
                effort_limit=g["effort_limit"][:7].tolist() if clamp else None)


def report(name, u, ref, ref_err, bound):
    ratio = np.abs(u.astype(np.float64) - ref).max() / ref_err
    print(f"{name}: max |u_gpu - u_ref64| / ref_err = {ratio:.3f} (bound {bound})")
    assert np.isfinite(u).all()
    assert ratio <= bound, f"{name}: {ratio:.3f} x ref_err exceeds {bound} x"


@pytest.mark.parametrize("n", [6, 64])
@pytest.mark.parametrize("clamp", [False, True])
def test_osc_injected_matches_reference(lib, n, clamp):
    """the linear algebra alone, on the golden's own J and M: within 4 x ref_err of the reference's fp64 run (the
    bound two fp32 algorithms on the same fp32 inputs are held to; the Cholesky path here works in double).
    Measured: 0.005 x ref_err at 64 actors, unclamped and clamped (0.002 x on the first 6); 0.30 x (0.02 x) before
    the solve moved to double."""
    s, g = osc_sim(lib, n)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x[:n])).to(DEV)   # noqa: E731
    u = s.dyn.osc_torques(dev(g["dpose"]), dev(g["eef_vel"]), jac_in=dev(g["j_eef"]), mm_in=dev(g["mm"]),
                          **osc_kwargs(g, clamp))
    torch.cuda.synchronize()
    s.close()
    report(f"osc injected n={n} clamp={clamp}", u.cpu().numpy(), g["u_ref64" if clamp else "u_ref64_free"][:n],
           float(g["ref_err"]), 4.0)


@pytest.mark.parametrize("n", [6, 64])
def test_osc_end_to_end_matches_reference(lib, n):
    """J and M built in the kernel from q and the base poses, eef_vel read in place from a rigid_body_states-shaped
    tensor: within 8 x ref_err (fp32 FK / CRBA rounding on top of the input rounding the reference shares).
    Measured: 0.11 x ref_err at 64 actors, unclamped and on the clamped columns :6 (0.08 x on the first 6); 1.06 x at
    64 actors before the solve moved to double."""
    s, g = osc_sim(lib, n)
    spec = s.spec
    nb, nd, grip = len(spec.bodies), spec.num_dofs, spec.body_index(GRIP)
    rbs = torch.zeros((n, nb, 13), device=DEV)
    rbs[:, grip, 7:13] = torch.from_numpy(g["eef_vel"][:n]).to(DEV)
    eef = rbs[:, grip, 7:13]
    assert eef.stride() == (13 * nb, 1)
    dpose = torch.from_numpy(g["dpose"][:n]).to(DEV)
    u = s.dyn.osc_torques(dpose, eef, **osc_kwargs(g, False))
    # clamped, fused into the actuation tensor: the reference writes columns :6 only (franka_reach_MA.py:817)
    s.act.fill_(7.0)
    out = s.dyn.osc_torques(dpose, eef, out=s.act, out_stride=nd, out_cols=6, **osc_kwargs(g, True))
    torch.cuda.synchronize()
    assert out.data_ptr() == s.act.data_ptr()
    act = s.act.view(n, nd).cpu().numpy()
    s.close()
    report(f"osc end-to-end n={n}", u.cpu().numpy(), g["u_ref64_free"][:n], float(g["ref_err"]), 8.0)
    assert (act[:, 6:] == 7.0).all(), "columns 6, 7, 8 of the actuation tensor must stay untouched"
    report(f"osc end-to-end n={n} clamped, actuation[:, :6]", act[:, :6], g["u_ref64"][:n, :6],
           float(g["ref_err"]), 8.0)


def test_stream_async_and_free_base_rejected(lib):
    """both calls run on the caller's stream; a free-base model is an argument error, never a launch"""
    n = 6
    s, g = osc_sim(lib, n)
    dpose = torch.from_numpy(g["dpose"][:n]).to(DEV)
    eef = torch.from_numpy(g["eef_vel"][:n]).to(DEV)
    J, Mm = s.dyn.acquire_jacobian(), s.dyn.acquire_mass_matrix()
    u0 = s.dyn.osc_torques(dpose, eef, **osc_kwargs(g, True)).clone()
    s.dyn.refresh()
    torch.cuda.synchronize()
    J0, M0 = J.clone(), Mm.clone()
    assert J0.abs().max() > 0 and M0.abs().max() > 0 and u0.abs().max() > 0
    J.zero_()
    Mm.zero_()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        u1 = torch.zeros((n, 7), device=DEV)
        s.dyn.osc_torques(dpose, eef, out=u1, stream=side.cuda_stream, **osc_kwargs(g, True))
        s.dyn.refresh(stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(u1, u0) and torch.equal(J, J0) and torch.equal(Mm, M0)
    s.close()
    env = migym.make(seed=0, task="Ant", num_envs=4, sim_device=DEV, rl_device=DEV, headless=True)
    assert lib.mg_dynamics_refresh(env.sim, None) == -1
    msg = lib.mg_last_error().decode()
    assert "fixed-base" in msg
    a = _abi.OscArgs()
    assert lib.mg_osc_torques(env.sim, C.byref(a), None) == -1 and "fixed-base" in lib.mg_last_error().decode()
    v = _abi.DynamicsViews()
    assert lib.mg_dynamics_bind(env.sim, C.byref(v)) == -1
    with pytest.raises(NotImplementedError, match="fixed-base"):
        env.acquire_jacobian_tensor()
    with pytest.raises(NotImplementedError, match="fixed-base"):
        env.compute_osc_torques(torch.zeros((4, 6), device=DEV), torch.zeros((4, 6), device=DEV), jac_body=1)
    env.close()
    # a hand-task sim (fixed base, but three root rows per env) is refused too
    env = migym.make(seed=0, task="ShadowHand", num_envs=4, sim_device=DEV, rl_device=DEV, headless=True)
    assert lib.mg_dynamics_refresh(env.sim, None) == -1 and "free object" in lib.mg_last_error().decode()
    env.close()


# ------------------------------------------------------------------------------------------------ synthetic trees
def related_dofs(spec):
    """(nD, nD) bool: DOFs r and c lie on one chain (M[r][c] is structurally non-zero)"""
    nd = spec.num_dofs
    rel = np.zeros((nd, nd), bool)
    for c in range(nd):
        for k in R.ancestors(spec, c + 1):
            rel[k - 1, c] = rel[c, k - 1] = True
    return rel


@pytest.mark.parametrize("n", [1, 6, 66])
@pytest.mark.parametrize("name", list(R.TREES))
def test_tree_tensors_match_oracle(lib, name, n):
    """J and M on the branched / 40-node trees against the oracle (the 1e-4 rule), a different q and alternating base
    poses per actor so that a team reading its neighbour's LDS slice fails; exact zeros off the chain; M == M^T bit
    for bit; bodies sharing a node differ by the lever arm only"""
    spec = R.tree(name)
    root, q, Mo, Jo = (x[:n] for x in R.tree_case(name, R.TREE_ACTORS))
    s = Sim(lib, spec, root, q)
    J, Mm = s.tensors()
    s.close()
    check_tensors(J, Mm, Jo, Mo)
    assert np.array_equal(Mm, Mm.transpose(0, 2, 1)), "M must equal its transpose bit for bit"
    off = R.off_chain_mask(spec)[1:]
    assert (J.transpose(0, 1, 3, 2)[:, off] == 0.0).all(), "Jacobian entries of DOFs off the chain are exact zeros"
    assert (J.transpose(0, 1, 3, 2)[:, ~off] != 0.0).any(axis=-1).all(), "every on-chain column is non-zero"
    assert (Mm[:, ~related_dofs(spec)] == 0.0).all(), "M entries of DOFs on different branches are exact zeros"
    # several bodies on one node (fixed joints): identical angular rows, linear rows apart by the lever arm
    by_node = {}
    for b, body in enumerate(spec.bodies):
        by_node.setdefault(body.node, []).append(b)
    pairs = [(v[0], b) for k, v in by_node.items() if k > 0 for b in v[1:]]
    assert bool(pairs) == (len(spec.bodies) > len(spec.nodes))
    mnp = R.oracle_model(spec)
    for a in range(min(n, 6)):
        rb = R.O.rigid_body_states(mnp, root[a], np.stack([q[a], 0 * q[a]], 1), len(spec.bodies)).astype(np.float64)
        for b0, b1 in pairs:
            J0, J1 = J[a, b0 - 1].astype(np.float64), J[a, b1 - 1].astype(np.float64)
            assert np.array_equal(J0[3:6], J1[3:6])
            lever = rb[b1, 0:3] - rb[b0, 0:3]
            assert np.linalg.norm(lever) > 1e-3
            assert np.abs(J1[0:3] - (J0[0:3] + np.cross(J0[3:6].T, lever).T)).max() <= 1e-5


def test_one_tensor_bound(lib):
    """only J or only M acquired: the same values, bit for bit, as with both; nothing bound is MG_EINVAL"""
    name, n = "branched33x", 6
    spec = R.tree(name)
    root, q, Mo, Jo = (x[:n] for x in R.tree_case(name, R.TREE_ACTORS))
    s = Sim(lib, spec, root, q)
    assert lib.mg_dynamics_refresh(s.sim, None) == -1 and "no tensor bound" in lib.mg_last_error().decode()
    J, Mm = s.tensors()
    s.close()
    sj, sm = Sim(lib, spec, root, q), Sim(lib, spec, root, q)
    Jt, Mt = sj.dyn.acquire_jacobian(), sm.dyn.acquire_mass_matrix()
    sj.dyn.refresh()
    sm.dyn.refresh()
    torch.cuda.synchronize()
    assert sj.dyn.mass_matrix is None and sm.dyn.jacobian is None
    assert np.array_equal(Jt.cpu().numpy(), J) and np.array_equal(Mt.cpu().numpy(), Mm)
    sj.close()
    sm.close()
    check_tensors(J, Mm, Jo, Mo)


def test_env_props_on_second_round_nodes(lib):
    """domain randomization on the 33-node tree: one actor's nodes >= 16 (the second and third round of the
    per-actor [mass, armature] staging) get twice the mass and a new armature; its tensors match the oracle on a model
    changed the same way (mass and COM inertia x 2), every other actor is bit-equal to the run without env_props"""
    name, n, k = "branched33x", 6, 2
    spec = R.tree(name)
    root, q, Mo, Jo = (x[:n] for x in R.tree_case(name, R.TREE_ACTORS))
    s0 = Sim(lib, spec, root, q)
    J0, M0 = s0.tensors()
    s0.close()
    props = np.tile(defaults(spec), (n, 1))
    assert props.shape[1] == layout(spec)[0]
    W = _abi.MG_EP_NODE_WIDTH
    spec2 = copy.deepcopy(spec)
    for i in range(16, len(spec.nodes)):
        nd = spec2.nodes[i]
        nd.mass, nd.inertia, nd.armature = 2.0 * nd.mass, [2.0 * v for v in nd.inertia], 0.06 + 0.002 * i
        props[k, W * i], props[k, W * i + 1] = nd.mass, nd.armature
    s1 = Sim(lib, spec, root, q, props=props)
    J1, M1 = s1.tensors()
    s1.close()
    M2, J2 = R.oracle_tensors(spec2, root[k:k + 1], q[k:k + 1])
    check_tensors(J1[k:k + 1], M1[k:k + 1], J2, M2)
    assert np.abs(M2[0] - Mo[k]).max() > 1e-2 * np.diag(Mo[k]).max(), "the change is far above the tolerance"
    keep = [a for a in range(n) if a != k]
    assert np.array_equal(M1[keep], M0[keep]) and np.array_equal(J1, J0)


# ------------------------------------------------------------------------------------------------ OSC edges
def edge_kwargs(g, na=7, **kw):
    return dict(jac_body=int(g["jac_body"]), arm_dofs=na, kp=g["kp"].tolist(), kd=g["kd"].tolist(),
                kp_null=g["kp_null"][:na].tolist(), kd_null=g["kd_null"][:na].tolist(),
                default_dof_pos=g["default_dof_pos"][:na].tolist(), **kw)


@pytest.mark.parametrize("n", [6, 64])
def test_osc_edge_gains_injected(lib, n):
    """per-axis kp and kd (kd != 2 sqrt(kp)), per-DOF null-space gains and a wrap that fires in both directions, on
    the edges golden's J and M: within 4 x its ref_err (9.58e-4 N m) of the reference's fp64 run.
    Measured: 0.007 x ref_err at 64 actors (0.002 x on the first 6)."""
    g = edges()
    s = Sim(lib, franka(), g["root_states"][:n], g["q"][:n], g["qd"][:n])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x[:n])).to(DEV)   # noqa: E731
    u = s.dyn.osc_torques(dev(g["dpose"]), dev(g["eef_vel"]), jac_in=dev(g["j_eef"]), mm_in=dev(g["mm"]),
                          **edge_kwargs(g))
    torch.cuda.synchronize()
    s.close()
    report(f"osc edges injected n={n}", u.cpu().numpy(), g["u_ref64_free"][:n], float(g["ref_err"]), 4.0)


@pytest.mark.parametrize("n", [6, 64])
def test_osc_edge_gains_end_to_end(lib, n):
    """the same through the in-kernel J and M (q carries whole turns: the same pose): within 8 x ref_err.
    Measured: 0.07 x ref_err at 64 actors (0.07 x on the first 6)."""
    g = edges()
    s = Sim(lib, franka(), g["root_states"][:n], g["q"][:n], g["qd"][:n])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x[:n])).to(DEV)   # noqa: E731
    u = s.dyn.osc_torques(dev(g["dpose"]), dev(g["eef_vel"]), **edge_kwargs(g))
    torch.cuda.synchronize()
    s.close()
    report(f"osc edges end-to-end n={n}", u.cpu().numpy(), g["u_ref64_free"][:n], float(g["ref_err"]), 8.0)


def test_osc_injected_plumbing(lib):
    """the lane-per-actor kernel past its first block (n = 70: a second block of 6 lanes), writing 5 columns into the
    actuation tensor (out_stride = nD) and reading eef_vel in place from a rigid-body-state tensor: the written
    columns match the reference within 4 x ref_err, every other element keeps its sentinel.
    Measured: 0.007 x ref_err."""
    g, n, cols = edges(), 70, 5
    idx = np.arange(n) % 64
    spec = franka()
    nb, nd, grip = len(spec.bodies), spec.num_dofs, spec.body_index(GRIP)
    s = Sim(lib, spec, g["root_states"][idx], g["q"][idx], g["qd"][idx])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x[idx])).to(DEV)   # noqa: E731
    rbs = torch.full((n, nb, 13), 1e6, device=DEV)
    rbs[:, grip, 7:13] = dev(g["eef_vel"])
    eef = rbs[:, grip, 7:13]
    assert eef.stride() == (13 * nb, 1)
    s.act.fill_(7.0)
    out = s.dyn.osc_torques(dev(g["dpose"]), eef, jac_in=dev(g["j_eef"]), mm_in=dev(g["mm"]), out=s.act,
                            out_stride=nd, out_cols=cols, **edge_kwargs(g))
    torch.cuda.synchronize()
    assert out.data_ptr() == s.act.data_ptr()
    act = s.act.view(n, nd).cpu().numpy()
    s.close()
    assert (act[:, cols:] == 7.0).all(), "columns past out_cols must stay untouched"
    report("osc injected plumbing n=70, actuation[:, :5]", act[:, :cols], g["u_ref64_free"][idx, :cols],
           float(g["ref_err"]), 4.0)


def arm_reference(na=6):
    """the fp64 numpy controller on the oracle's fp32-rounded M[:na, :na] and J[:, :na] of the serial-arm tree, and
    the case's own ref_err = max |u32 - u64|"""
    root, q, qd, dpose, eef, Mo, Jo = R.arm_case()
    G = R.ARM_GAINS
    M32, J32 = Mo[:, :na, :na].astype(np.float32), Jo[:, :, :na].astype(np.float32)
    args = (M32, J32, q[:, :na], qd[:, :na], dpose, eef, G["kp"], G["kd"], G["kp_null"][:na], G["kd_null"][:na],
            G["default_dof_pos"][:na])
    u64 = R.osc_reference(*args)
    _, ref_err = R.osc_reference(*args, dtype=np.float32)
    return M32, J32, u64, ref_err


def arm_kwargs(na, **kw):
    G = R.ARM_GAINS
    return dict(jac_body=R.ARM_BODY, arm_dofs=na, kp=G["kp"], kd=G["kd"], kp_null=G["kp_null"][:na],
                kd_null=G["kd_null"][:na], default_dof_pos=G["default_dof_pos"][:na], **kw)


@pytest.mark.parametrize("path", ["injected", "end_to_end"])
def test_osc_six_arm_dofs_on_the_tree(lib, path):
    """arm_dofs = 6 (M padded with the identity, J with zeros) on the 17-node serial-arm tree, 66 actors, against the
    fp64 numpy controller on the oracle's M[:6, :6] and J[:, :6]: 4 x (injected) / 8 x (end to end) the case's own
    ref_err; column 6 of the 7-wide out keeps its sentinel (out_cols = 6).
    Measured (ref_err 2.62e-2 N m on torques up to 661 N m, cond(J M^-1 J^T) up to 4.06e4): injected 0.002 x ref_err,
    end to end 0.06 x.  This case is why osc_solve works in double: in fp32 the injected path measured 6.24 x (bound
    4 x), all of it on the worst-conditioned actor (0.16 N m of 614; numpy's fp32 LU inverses err by 0.022 there), with
    no single stage at fault (DESIGN.md s. 10); end to end it measured 2.15 x."""
    root, q, qd, dpose, eef, Mo, Jo = R.arm_case()
    n = len(q)
    M32, J32, u64, ref_err = arm_reference(6)
    assert max(np.linalg.cond(Jo[a][:, :6] @ np.linalg.solve(Mo[a][:6, :6], Jo[a][:, :6].T)) for a in range(n)) <= 5e4
    s = Sim(lib, R.tree("arm17"), root, q, qd)
    dev = lambda x: torch.from_numpy(np.array(x)).to(DEV)   # noqa: E731  (a copy: the shared cases are read-only)
    out = torch.full((n, 7), 7.0, device=DEV)
    inj = dict(jac_in=dev(J32), mm_in=dev(M32)) if path == "injected" else {}
    s.dyn.osc_torques(dev(dpose), dev(eef), out=out, out_stride=7, out_cols=6, **inj, **arm_kwargs(6))
    torch.cuda.synchronize()
    s.close()
    u = out.cpu().numpy()
    assert (u[:, 6] == 7.0).all(), "column 6 must stay untouched"
    assert np.abs(u64).max() > 1.0
    print(f"arm tree ref_err = {ref_err:.3g}, |u| max = {np.abs(u64).max():.3g}")
    report(f"osc arm_dofs=6 {path}", u[:, :6], u64, ref_err, 4.0 if path == "injected" else 8.0)


def test_osc_under_env_props_end_to_end(lib):
    """the fused controller reads the actor that is simulated: with one actor's masses doubled through env_props its
    torques match the fp64 numpy controller on the oracle's M of the doubled model (8 x ref_err); the other actors
    are bit-equal to the launch without env_props.
    Measured: 0.01 x ref_err (ref_err 1.00e-3 N m)."""
    g, n, k = golden(), 64, 21
    spec = franka()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x[:n])).to(DEV)   # noqa: E731
    kw = osc_kwargs(g, False)
    s0 = Sim(lib, spec, g["root_states"][:n], g["q"][:n], g["qd"][:n])
    u0 = s0.dyn.osc_torques(dev(g["dpose"]), dev(g["eef_vel"]), **kw).cpu().numpy()
    s0.close()
    props = np.tile(defaults(spec), (n, 1))
    W = _abi.MG_EP_NODE_WIDTH
    props[k, 0:W * len(spec.nodes):W] *= 2.0
    s1 = Sim(lib, spec, g["root_states"][:n], g["q"][:n], g["qd"][:n], props=props)
    u1 = s1.dyn.osc_torques(dev(g["dpose"]), dev(g["eef_vel"]), **kw).cpu().numpy()
    s1.close()
    spec2 = copy.deepcopy(spec)
    for nd in spec2.nodes:
        nd.mass, nd.inertia = 2.0 * nd.mass, [2.0 * v for v in nd.inertia]
    mm = g["mm"].copy()
    mm[k] = R.oracle_mass_matrix(R.oracle_model(spec2), g["root_states"][k], g["q"][k])[:7, :7].astype(np.float32)
    assert np.abs(mm[k] - g["mm"][k]).max() > 0.1 * np.abs(g["mm"][k]).max()
    kp, kpn = np.full(6, float(g["kp"])), np.full(7, float(g["kp_null"]))
    args = (mm, g["j_eef"], g["q"][:, :7], g["qd"][:, :7], g["dpose"], g["eef_vel"], kp, 2 * np.sqrt(kp), kpn,
            2 * np.sqrt(kpn), g["default_dof_pos"][:7])
    u64 = R.osc_reference(*args)
    _, ref_err = R.osc_reference(*args, dtype=np.float32)
    assert np.abs(u64[k] - g["u_ref64_free"][k]).max() > 100 * ref_err, "doubling the masses moves the torques"
    print(f"ref_err of the doubled-mass case = {ref_err:.3g}")
    report(f"osc under env_props, actor {k}", u1[k:k + 1], u64[k:k + 1], ref_err, 8.0)
    keep = [a for a in range(n) if a != k]
    assert np.array_equal(u1[keep], u0[keep])


# ------------------------------------------------------------------------------------------------ failure contract
@pytest.mark.parametrize("clamp", [False, True])
def test_osc_failure_contract_injected(lib, clamp):
    """include/migym.h: an actor whose factorisation fails gets exactly 0 in every written column, never NaN, and no
    other actor is affected -- a J with a zero row, a J with two equal rows, a negative diagonal entry of M, a NaN in
    M, M = 0, on lanes spread over the wave"""
    g, n = golden(), 64
    J, Mm = g["j_eef"].copy(), g["mm"].copy()
    bad = [3, 17, 30, 45, 63]
    J[3, 2] = 0.0
    J[17, 4] = J[17, 1]
    Mm[30, 3, 3] = -Mm[30, 3, 3]
    Mm[45, 5, 2] = np.nan
    Mm[63] = 0.0
    s = Sim(lib, franka(), g["root_states"][:n], g["q"][:n], g["qd"][:n])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x[:n])).to(DEV)   # noqa: E731
    kw = osc_kwargs(g, clamp)
    u0 = s.dyn.osc_torques(dev(g["dpose"]), dev(g["eef_vel"]), jac_in=dev(g["j_eef"]), mm_in=dev(g["mm"]), **kw)
    u0 = u0.cpu().numpy()
    out = torch.full((n, 7), 7.0, device=DEV)
    s.dyn.osc_torques(dev(g["dpose"]), dev(g["eef_vel"]), jac_in=dev(J), mm_in=dev(Mm), out=out, **kw)
    torch.cuda.synchronize()
    s.close()
    u1 = out.cpu().numpy()
    assert np.abs(u0[bad]).min(axis=1).max() > 0
    for a in bad:
        assert (u1[a] == 0.0).all(), f"actor {a}: a failed factorisation must write zeros, got {u1[a]}"
    keep = [a for a in range(n) if a not in bad]
    assert np.array_equal(u1[keep], u0[keep]), "a failure must not leak across lanes"


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("na", [3, 5])
def test_osc_failure_contract_end_to_end(lib, na, clamp):
    """arm_dofs < 6 makes A = J M^-1 J^T structurally singular (rank arm_dofs) while its leading block is well
    conditioned (tests/test_dynamics_host.py): every one of the 66 actors gets zeros, with and without an effort
    limit.  An absolute pivot test (s > 0) lets the fp32 rounding of an exact zero through: that kernel returned
    torques for 1 of 66 actors at arm_dofs = 3 and 39 of 66 at arm_dofs = 5 here (up to 3.7e3 N m, +-effort_limit
    when clamped)."""
    root, q, qd, dpose, eef, Mo, Jo = R.arm_case()
    n = len(q)
    s = Sim(lib, R.tree("arm17"), root, q, qd)
    dev = lambda x: torch.from_numpy(np.array(x)).to(DEV)   # noqa: E731  (a copy: the shared cases are read-only)
    out = torch.full((n, na), 7.0, device=DEV)
    s.dyn.osc_torques(dev(dpose), dev(eef), out=out, **arm_kwargs(na, effort_limit=[50.0] * na if clamp else None))
    torch.cuda.synchronize()
    s.close()
    u = out.cpu().numpy()
    wrong = np.flatnonzero(~(u == 0.0).all(axis=1))
    print(f"arm_dofs={na} clamp={clamp}: {len(wrong)} of {n} actors not zero"
          + (f", |u| max {np.nanmax(np.abs(u[wrong])):.3g}" if len(wrong) else ""))
    assert len(wrong) == 0, f"{len(wrong)} of {n} singular actors got torques, e.g. actor {wrong[0]}: {u[wrong[0]]}"
