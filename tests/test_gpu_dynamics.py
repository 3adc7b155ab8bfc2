"""GPU tests of the dynamics tensors and the fused operational-space controller (include/migym.h: mg_dynamics_bind,
mg_dynamics_refresh, mg_osc_torques).

The references are the fp64 oracle (tests/dynamics_ref.py: its CRBA mass matrix and, column by column, its rigid-body
velocities under qd = e_j) and the reference's own ``_compute_osc_torques`` (tests/golden/osc_franka.npz, written by
tests/golden/make_osc_golden.py).  Actor counts are the smallest that cross the team layout's edges (one 16-lane
team per actor, four per wave): 6 = a partial wave, 66 = 16 full waves and a half-filled one; the OSC golden's 64 is
16 full waves (and one full wave of the injected path's lane-per-actor kernel).

The OSC tests print max |u_gpu - u_ref64| / ref_err (ref_err = 1.13e-3 N m) before they assert; the figures measured
on the MI355X are in their docstrings and in DESIGN.md §10.
"""
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
    Cholesky path here and the reference's LU inverses are two fp32 algorithms on the same fp32 inputs).
    Measured: 0.30 x ref_err at 64 actors, unclamped and clamped (0.02 x on the first 6)."""
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
    Measured: 1.06 x ref_err at 64 actors, unclamped and on the clamped columns :6 (0.08 x on the first 6)."""
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
