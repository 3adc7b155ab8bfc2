"""Link forces in mg_sim_simulate (mg_sim_set_link_forces, k_simulate_xf) on the GPU.

The oracle applies no force to a link, so each test rests on something it does have (tests/linkforce_ref.py; the
inputs are admitted on the CPU by tests/test_linkforce_host.py):

  * Gravity equivalence: the kernel under gravity g with F_b = m_b a on every body, a different a per actor, against
    the fp64 oracle run actor by actor at g + a, by the one-step rule of tree_physics_ref.compare (positions 2e-4,
    velocities 2e-3 + 2e-3 |v|, DOF forces / sensors / net contact forces 1 % of the batch's largest; no state carries
    a flag, so none is exempt).  PGS and TGS; MG_ENV_SPACE at 2 substeps and MG_LOCAL_SPACE at 1 substep with
    f = R_b(q0)^T m_b a; the smallest batches across each instance's wave edge.
  * Momentum identity, one loaded link per actor, every body and three directions in turn, on passive copies: the
    bound is 4 x the fp32 twin's own residual on the same states (the project's twin factor), computed here.
  * The body frame is followed substep by substep: MG_LOCAL_SPACE at 2 substeps on spinning actors.
  * The switch: off, a bound tensor changes no bit; on, an all-zero tensor gives the plain kernel's result; the
    refused combinations fail and leave the state as it was.
  * The dispatcher: a batch whose plain dispatch is the compact layout runs the classic variant; a model with more
    bodies than its instance has nodes is refused; the (32, 24, 32, 24, 160) variant, which none of linkforce_ref's
    models selects, is held to the oracle on the built-in Humanoid.
  * Through make(): an Anymal pushed with m_b a tracks an Anymal made with gravity g + a; Ant raises.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import linkforce_ref as LF
import parity_stats as PS
import pyoracle as O
from migym import _abi, model as M, taskdefs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MG_OK = 0


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


def T(a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV).contiguous()   # a copy: the states are read-only


class Sim:
    """an mg_sim of n actors; run() binds fresh device copies of a state and simulates once"""

    def __init__(self, lib, spec, mnp, sp, n):
        self.lib, self.spec, self.mnp, self.n, self.h = lib, spec, mnp, n, C.c_void_p()
        _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(self.h)), lib)

    def lanes(self):
        t, lay = C.c_int32(), C.c_int32()
        _abi.check(self.lib.mg_sim_kernel_layout(self.h, C.byref(t), C.byref(lay)), self.lib)
        return t.value

    def bind(self, root, dof, act=None, tgt=None, f=None, space=LF.ENV, env_props=None):
        """device copies of the first n rows, bound; returns the dict of tensors"""
        n, spec = self.n, self.spec
        nd, nb, ns = spec.num_dofs, len(spec.bodies), max(len(spec.sensors), 1)
        d = {"root": T(root[:n]), "dof": T(dof[:n]),
             "act_eff": T(act[:n]) if act is not None else torch.zeros((n, nd), device=DEV),
             "tgt": T(tgt[:n]) if tgt is not None else None,
             "sensors": torch.zeros((n, ns * 6), device=DEV), "dof_force": torch.zeros((n, nd), device=DEV),
             "ncf": torch.full((n, nb, 3), float("nan"), device=DEV),     # every row must be written
             "f": T(f[:n]) if f is not None else None, "env_props": env_props}
        v = _abi.StateViews()
        v.root_states, v.dof_state, v.dof_actuation = d["root"].data_ptr(), d["dof"].data_ptr(), d["act_eff"].data_ptr()
        v.sensors, v.dof_force, v.net_contact_forces = d["sensors"].data_ptr(), d["dof_force"].data_ptr(), d["ncf"].data_ptr()
        v.dof_targets = _abi.ptr(d["tgt"])
        v.rb_forces, v.rb_force_space = _abi.ptr(d["f"]), int(space)
        if env_props is not None:
            v.env_props, v.env_props_stride = env_props.data_ptr(), env_props.shape[1]
        _abi.check(self.lib.mg_sim_bind(self.h, C.byref(v)), self.lib)
        return d

    def link(self, on):
        _abi.check(self.lib.mg_sim_set_link_forces(self.h, int(on)), self.lib)

    def simulate(self):
        return self.lib.mg_sim_simulate(self.h, torch.cuda.current_stream().cuda_stream)

    def run(self, root, dof, act=None, tgt=None, f=None, space=LF.ENV, link=True):
        d = self.bind(root, dof, act, tgt, f, space)
        self.link(link)
        _abi.check(self.simulate(), self.lib)
        torch.cuda.synchronize()
        return result(d)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.mg_sim_destroy(self.h)


FIELDS = ("root", "dof", "sensors", "dof_force", "ncf")


def result(d):
    import types
    return types.SimpleNamespace(**{k: d[k].cpu().numpy() for k in FIELDS})


def same_bits(a, b, what):
    for k in FIELDS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{k}: {what}")


# ------------------------------------------------------------------------------------------------ gravity equivalence
GRAVITY_CASES = [(m, mode, tgs, n) for m in LF.LANES for mode in LF.MODES for tgs in (False, True)
                 for n in LF.BATCHES[m]]


@pytest.mark.parametrize("model,mode,tgs,n", GRAVITY_CASES)
def test_link_forces_equal_gravity(lib, model, mode, tgs, n):
    spec, mnp, _ = LF.setup(model)
    c = LF.case(model, mode, tgs)
    space, sub = LF.MODES[mode]
    assert c["sp"].substeps == sub and (c["sp"].solver_type == _abi.MG_SOLVER_TGS) == tgs
    with Sim(lib, spec, mnp, c["sp"], n) as sim:
        assert sim.lanes() == LF.LANES[model], f"{model}: ran on {sim.lanes()} lanes"
        got = sim.run(c["root"], c["dof"], c["act"], c["tgt"], c["f"], space)
        again = sim.run(c["root"], c["dof"], c["act"], c["tgt"], c["f"], space)
    same_bits(got, again, "the second run differs")
    LF.compare(f"test_link_forces_equal_gravity[{model}-{mode}-{'tgs' if tgs else 'pgs'}-{n}]", model, mode, tgs, n, got)


# ------------------------------------------------------------------------------------------------ momentum identity
def _gpu_step(lib, spec, mnp, sp, root, dof, f, space=LF.ENV):
    with Sim(lib, spec, mnp, sp, len(root)) as sim:
        return sim.run(root, dof, None, None, f, space)


@pytest.mark.parametrize("model", LF.MOMENTUM_MODELS)
def test_momentum_identity_one_link_at_a_time(lib, model):
    """h F and h c_b x F, to 4 x the fp32 twin's residual on the same states.  Measured (MI355X): see DESIGN.md §14"""
    spec, mnp, sp, root, dof, body, axis = LF.momentum_setup(model)
    f, Fw = LF.one_link_loads(model)
    n = len(root)
    on = _gpu_step(lib, spec, mnp, sp, root, dof, f)
    off = _gpu_step(lib, spec, mnp, sp, root, dof, np.zeros_like(f))
    P1, L1, cs = LF.momentum(spec, mnp, root, dof, on.root, on.dof)
    P0, L0, _ = LF.momentum(spec, mnp, root, dof, off.root, off.dof)
    h = sp.dt / sp.substeps
    lin, ang = LF.momentum_residuals(P1 - P0, L1 - L0, Fw, cs[np.arange(n), body], h)
    tlin, tang = LF.oracle_momentum_residuals(model, True)
    print(f"momentum[{model}]: kernel linear {lin.max():.3g} angular {ang.max():.3g}; fp32 twin linear {tlin.max():.3g} "
          f"angular {tang.max():.3g}; bound x{LF.TWIN_FACTOR:g}")
    PS._REPORT.setdefault(f"test_momentum_identity_one_link_at_a_time[{model}]", {})["residuals"] = {
        "kernel_linear": float(lin.max()), "kernel_angular": float(ang.max()), "twin_linear": float(tlin.max()),
        "twin_angular": float(tang.max())}
    assert np.linalg.norm(P1 - P0, axis=1).min() > 0.5 * h * np.linalg.norm(Fw, axis=1).min(), "a load moved nothing"
    assert lin.max() <= LF.TWIN_FACTOR * tlin.max(), f"linear {lin.max():.3g} > 4 x {tlin.max():.3g}"
    assert ang.max() <= LF.TWIN_FACTOR * tang.max(), f"angular {ang.max():.3g} > 4 x {tang.max():.3g}"


# ------------------------------------------------------------------------------------------------ the frame, per substep
def test_local_frame_is_followed_per_substep(lib):
    """MG_LOCAL_SPACE at 2 substeps on the passive quadcopter spinning at 10 rad/s, one loaded body per actor (every
    body, three body-frame directions): the linear momentum changes by h (R_b(q0) + R_b(q1)) f, q1 from a one-substep
    run.  The change is taken substep by substep, each time as the difference of two runs from one state, where the
    identity is exact (linkforce_ref: the velocity-product terms depend on the state alone and cancel):
      substep 1: one-substep launches from (q0, v0) with and without the force: h R_b(q0) f;
      substep 2: the two-substep launch with the force against a one-substep launch WITHOUT it from the state the
                 forced one-substep launch left, (q1, v1), both momenta at q1: h R_b(q1) f if the kernel turned the
                 force with the body, h R_b(q0) f if it froze the frame at the launch's start.
    (The state between the substeps of the two-substep launch never leaves the registers; the one-substep launch's
    output is that state to fp32 rounding.)  A frozen frame misses the sum by |w| h / 2 = 2.5 % where the chassis is
    loaded and by more on a rotor, which the load itself turns; the median miss is asserted to be over 1 %.  The bound
    is 1e-3 of the impulse 2 h |f|, far above the fp32 rounding of the momenta (|P| is about the impulse here, so about
    1e-6, as in the momentum test)."""
    spec = LF.passive(M.quadcopter_model())
    mnp, sp = M.pack_model(spec), LF.sp_at(LF.quad_sim_params(), None, 2)
    nb = len(spec.bodies)
    n = 3 * nb
    rng = np.random.default_rng(31)
    root = np.zeros((n, 13), np.float32)
    root[:, 2] = 3.0
    q = rng.normal(size=(n, 4))
    root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    w = rng.normal(size=(n, 3))
    root[:, 7:10], root[:, 10:13] = rng.normal(0, 0.3, (n, 3)), 10.0 * w / np.linalg.norm(w, axis=1, keepdims=True)
    dof = np.zeros((n, spec.num_dofs, 2), np.float32)
    dof[..., 0], dof[..., 1] = rng.uniform(-0.4, 0.4, (n, spec.num_dofs)), rng.normal(0, 1.0, (n, spec.num_dofs))
    body, axis = np.arange(n) % nb, (np.arange(n) // nb) % 3
    mag = 20.0 * spec.total_mass()
    f = np.zeros((n, nb, 3), np.float32)
    f[np.arange(n), body, axis] = mag
    h = sp.dt / 2
    sp1 = LF.sp_at(sp, None, 1)
    sp1.dt = np.float32(h)
    assert np.float32(sp1.dt / sp1.substeps) == np.float32(sp.dt / sp.substeps)

    zero = np.zeros_like(f)
    step = lambda p, r, d, ff: _gpu_step(lib, spec, mnp, p, r, d, ff, LF.LOCAL)   # noqa: E731
    one, one0, two = step(sp1, root, dof, f), step(sp1, root, dof, zero), step(sp, root, dof, f)
    free = step(sp1, one.root, one.dof, zero)
    P = lambda r0, d0, b: LF.momentum(spec, mnp, r0, d0, b.root, b.dof)[0]   # noqa: E731
    dP = (P(root, dof, one) - P(root, dof, one0)) + (P(one.root, one.dof, two) - P(one.root, one.dof, free))
    R0 = np.array([LF.body_rotations(mnp, root[e], dof[e], nb)[body[e]] for e in range(n)])
    R1 = np.array([LF.body_rotations(mnp, one.root[e], one.dof[e], nb)[body[e]] for e in range(n)])
    fl = f[np.arange(n), body].astype(np.float64)
    followed = h * np.einsum("eij,ej->ei", R0 + R1, fl)
    frozen = 2 * h * np.einsum("eij,ej->ei", R0, fl)
    imp = 2 * h * mag
    err, miss = np.linalg.norm(dP - followed, axis=1) / imp, np.linalg.norm(dP - frozen, axis=1) / imp
    print(f"local frame per substep: worst error {err.max():.3g} of the impulse; a frozen frame misses by "
          f"{miss.min():.3g} .. {miss.max():.3g} (median {np.median(miss):.3g})")
    assert np.median(miss) > 1e-2, "the states do not tell a followed frame from a frozen one"
    assert err.max() <= 1e-3


# ------------------------------------------------------------------------------------------------ the switch
def _anymal6():
    spec, mnp, _ = LF.setup("Anymal")
    return spec, mnp, LF.case("Anymal", "env", False)


def test_off_ignores_a_bound_tensor(lib):
    """link forces off (the default, and after set(0)): a non-zero tensor on the articulation rows changes no bit"""
    spec, mnp, c = _anymal6()
    n = 6
    with Sim(lib, spec, mnp, c["sp"], n) as sim:
        d = sim.bind(c["root"], c["dof"], c["act"], c["tgt"])          # no tensor, never switched on
        _abi.check(sim.simulate(), lib)
        plain = result(d)
        bound = sim.run(c["root"], c["dof"], c["act"], c["tgt"], c["f"], LF.ENV, link=False)
        on = sim.run(c["root"], c["dof"], c["act"], c["tgt"], c["f"], LF.ENV, link=True)
        back = sim.run(c["root"], c["dof"], c["act"], c["tgt"], c["f"], LF.ENV, link=False)
    same_bits(bound, plain, "off, a bound tensor changed the result")
    same_bits(back, plain, "switched off again, the result differs from the plain one")
    assert not np.array_equal(on.root, plain.root), "on, the forces changed nothing"


@pytest.mark.parametrize("tgs", (False, True))
def test_on_with_zero_forces_is_the_plain_kernel(lib, tgs):
    """on with an all-zero tensor: the plain instance's result by the one-step rule (the variant is code of its own,
    so its bits are not promised)"""
    spec, mnp, _ = LF.setup("Anymal")
    c = LF.case("Anymal", "env", tgs)
    n = 66
    with Sim(lib, spec, mnp, c["sp"], n) as sim:
        plain = sim.run(c["root"], c["dof"], c["act"], c["tgt"], None, LF.ENV, link=False)
        zero = sim.run(c["root"], c["dof"], c["act"], c["tgt"], np.zeros_like(c["f"]), LF.ENV, link=True)
    print("zero forces bit-equal to the plain kernel:", all(np.array_equal(getattr(zero, k), getattr(plain, k))
                                                            for k in FIELDS))
    for name, x, y, atol, rtol in LF.outside(spec, zero, plain, n):
        assert not PS.env_bad(x, y, atol, rtol).any(), name


def test_refused_combinations_leave_the_state_alone(lib, monkeypatch):
    """on: no tensor, env_props bound, a model with a free object, the compact layout pinned -- mg_sim_simulate fails
    with a message and writes nothing; mg_env_step fails while link forces are on"""
    spec, mnp, c = _anymal6()
    n = 6

    def refused(sim, d, what):
        before = {k: d[k].clone() for k in ("root", "dof", "dof_force")}
        assert sim.simulate() != MG_OK, f"{what}: not refused"
        assert lib.mg_last_error(), what
        torch.cuda.synchronize()
        for k, x in before.items():
            assert torch.equal(d[k], x), f"{what}: {k} was written"

    with Sim(lib, spec, mnp, c["sp"], n) as sim:
        sim.link(True)
        refused(sim, sim.bind(c["root"], c["dof"], c["act"], c["tgt"]), "no rb_forces tensor")
        stride = lib.mg_env_props_layout(mnp.ctypes.data, None)
        row = np.zeros(stride, np.float32)
        _abi.check(lib.mg_env_props_defaults(mnp.ctypes.data, row.ctypes.data), lib)
        props = T(np.tile(row, (n, 1)))
        d = sim.bind(c["root"], c["dof"], c["act"], c["tgt"], c["f"], LF.ENV, env_props=props)
        refused(sim, d, "env_props bound")
        sim.link(False)
        _abi.check(sim.simulate(), lib)     # the same views simulate once the switch is off
    # a model with a free object (the ShadowHand block)
    import simparams_ref as SR
    import test_gpu_hand as GH
    hspec, hmnp, hsp, _ = SR.hand_setup()
    h0 = SR.hand_states("substeps1")[0]
    with Sim(lib, hspec, hmnp, hsp, h0.n) as sim:
        e = GH.DevHandEnv(h0)
        _abi.check(lib.mg_sim_bind(sim.h, C.byref(e.views())), lib)
        sim.link(True)
        refused(sim, {"root": e.root, "dof": e.dof, "dof_force": e.dof_force}, "a model with a free object")
    # the compact layout pinned
    aspec, amnp, asp, _ = SR.task_setup("Ant")
    root, dof, act, _, _ = SR.task_states("Ant", "substeps1")
    monkeypatch.setenv("MIGYM_LAYOUT", "compact")
    with Sim(lib, aspec, amnp, asp, 16) as sim:
        d = sim.bind(root, dof, act, None, np.zeros((16, len(aspec.bodies), 3), np.float32))
        sim.link(True)
        refused(sim, d, "MIGYM_LAYOUT=compact")
    monkeypatch.delenv("MIGYM_LAYOUT")
    # the fused step
    import isaacgymenvs
    env = isaacgymenvs.make(seed=0, task="Ant", num_envs=16, sim_device=DEV, rl_device=DEV, headless=True)
    env.step(env.zero_actions())
    _abi.check(lib.mg_sim_set_link_forces(env.sim, 1), lib)
    before = env.root_states.clone()
    with pytest.raises(_abi.MigymError, match="link forces"):
        env.step(env.zero_actions())
    torch.cuda.synchronize()
    assert torch.equal(env.root_states, before)
    _abi.check(lib.mg_sim_set_link_forces(env.sim, 0), lib)
    env.step(env.zero_actions())
    env.close()


# ------------------------------------------------------------------------------------------------ through make()
def test_anymal_pushed_tracks_anymal_under_tilted_gravity():
    """Anymal with apply_rigid_body_force_tensors(m_b a, None, ENV_SPACE) against a second Anymal made with gravity
    g + a: 3 steps of the same actions from the same injected reset draws, each step's state within the one-step
    tolerances"""
    import anymal_ref as AR
    import isaacgymenvs
    import migym
    N, a = 6, np.array([1.5, -1.0, 2.0], np.float32)
    cfg_a, cfg_b = AR.task_cfg(N), AR.task_cfg(N)
    cfg_b["sim"]["gravity"] = [float(np.float32(g) + x) for g, x in zip(cfg_b["sim"].get("gravity", [0, 0, -9.81]), a)]
    mk = lambda cfg: isaacgymenvs.make(seed=0, task="Anymal", num_envs=N, sim_device=DEV, rl_device=DEV, headless=True,
                                       cfg={"task": cfg})
    pushed, tilted = mk(cfg_a), mk(cfg_b)
    p = AR.params_from(pushed.anymal_params)
    _, _, noise = AR.reset_state(p, N, 11)
    m = LF.masses(pushed.model_spec)
    f = T(np.tile((m[:, None] * a[None].astype(np.float64)).astype(np.float32), (N, 1, 1)))
    assert f.shape == (N, pushed.num_bodies, 3)
    with pytest.raises(NotImplementedError, match="torques"):
        pushed.apply_rigid_body_force_tensors(f, f, migym.ENV_SPACE)
    pushed.apply_rigid_body_force_tensors(f, None, migym.ENV_SPACE)
    assert pushed.rb_forces.data_ptr() == f.data_ptr(), "the tensor is bound, not copied"
    rng = np.random.default_rng(5)
    for env in (pushed, tilted):
        env.set_reset_noise(T(noise))
    moved = 0.0
    for t in range(3):
        act = T(rng.uniform(-1, 1, (N, 12)))
        for env in (pushed, tilted):
            env.step(act)
        torch.cuda.synchronize()
        ra, rb = pushed.root_states.cpu().numpy(), tilted.root_states.cpu().numpy()
        da, db = (e.dof_state.view(N, 12, 2).cpu().numpy() for e in (pushed, tilted))
        for name, x, y, atol, rtol in (("root pose", ra[:, 0:7], rb[:, 0:7], 2e-4, 0), ("dof pos", da[..., 0], db[..., 0], 2e-4, 0),
                                       ("root twist", ra[:, 7:13], rb[:, 7:13], 2e-3, 2e-3),
                                       ("dof vel", da[..., 1], db[..., 1], 2e-3, 2e-3)):
            print(f"step {t} {name}: max diff {np.abs(x - y).max():.3g}")
            assert not PS.env_bad(x, y, atol, rtol).any(), f"step {t}: {name}"
        moved = max(moved, float(np.abs(rb[:, 7:9]).max()))
    assert moved > 3 * 2e-3, "the tilt moved nothing sideways"
    f.zero_()                     # the sim reads the caller's tensor at every simulate: zeros stop the push
    pushed.close()
    tilted.close()


def test_fused_tasks_raise():
    import isaacgymenvs
    import migym
    env = isaacgymenvs.make(seed=0, task="Ant", num_envs=16, sim_device=DEV, rl_device=DEV, headless=True)
    f = torch.zeros((16, env.num_bodies, 3), device=DEV)
    with pytest.raises(NotImplementedError, match="fused step"):
        env.apply_rigid_body_force_tensors(f, None, migym.LOCAL_SPACE)
    env.close()


# ------------------------------------------------------------------------------------------------ the dispatcher
def test_classic_layout_is_taken_at_a_batch_the_compact_layout_serves(lib):
    """8,200 quadcopters are 2,050 waves of the 16-lane instance, past the 2,048 from which the dispatcher picks the
    compact layout: with link forces on the launch still takes the classic variant, and its first 67 actors come out
    bit for bit as in a batch of 67 (the actors are independent)"""
    model, n = "Quadcopter", 8200
    spec, mnp, _ = LF.setup(model)
    c = LF.case(model, "env", False)
    rep = lambda x: None if x is None else np.tile(x, (n // len(x) + 1,) + (1,) * (x.ndim - 1))[:n]   # noqa: E731
    with Sim(lib, spec, mnp, c["sp"], n) as sim:
        t, lay = C.c_int32(), C.c_int32()
        _abi.check(lib.mg_sim_kernel_layout(sim.h, C.byref(t), C.byref(lay)), lib)
        assert (t.value, lay.value) == (16, 1), "the plain dispatch of this batch is the compact layout"
        big = sim.run(rep(c["root"]), rep(c["dof"]), rep(c["act"]), rep(c["tgt"]), rep(c["f"]), LF.ENV)
    with Sim(lib, spec, mnp, c["sp"], 67) as sim:
        small = sim.run(c["root"], c["dof"], c["act"], c["tgt"], c["f"], LF.ENV)
    for k in FIELDS:
        np.testing.assert_array_equal(getattr(big, k)[:67], getattr(small, k), err_msg=k)
        np.testing.assert_array_equal(getattr(big, k)[67:134], getattr(small, k), err_msg=k + " (second copy)")
    LF.compare("test_classic_layout_is_taken_at_a_batch_the_compact_layout_serves", model, "env", False, 67,
               types_ns(big, 67))


def types_ns(r, n):
    import types
    return types.SimpleNamespace(**{k: getattr(r, k)[:n] for k in FIELDS})


def test_more_bodies_than_nodes_of_the_instance_is_refused(lib):
    """a tree of 8 nodes with 20 bodies (12 welded on) runs on the (16, 9, 16, 16, 0) instance, whose link-force
    variant has one LDS row and one lane per body for 9: refused with a message, nothing written; off, it simulates"""
    import dynamics_ref as D
    spec = D.random_tree(num_nodes=8, seed=1, extra_bodies=12, physics=True)
    assert len(spec.bodies) == 20
    mnp, n = M.pack_model(spec), 6
    sp = LF.sp_at(LF.quad_sim_params())
    rng = np.random.default_rng(0)
    root = np.zeros((n, 13), np.float32)
    root[:, 2], root[:, 6] = 2.0, 1.0
    dof = rng.uniform(-0.5, 0.5, (n, spec.num_dofs, 2)).astype(np.float32)
    with Sim(lib, spec, mnp, sp, n) as sim:
        assert sim.lanes() == 16
        d = sim.bind(root, dof, None, None, np.ones((n, 20, 3), np.float32))
        sim.link(True)
        before = d["dof"].clone()
        assert sim.simulate() != MG_OK and b"more bodies" in lib.mg_last_error()
        torch.cuda.synchronize()
        assert torch.equal(d["dof"], before)
        sim.link(False)
        _abi.check(sim.simulate(), lib)
        torch.cuda.synchronize()
        assert not torch.equal(d["dof"], before)


@pytest.mark.parametrize("tgs", (False, True))
def test_humanoid_instance_equals_gravity(lib, tgs):
    """the (32, 24, 32, 24, 160) variant, which none of linkforce_ref's models selects (its block is the widest: eight
    waves and 161,152 bytes of LDS): the built-in Humanoid in the air, 6 actors (two per wave), m_b a on every body
    against the fp64 oracle at g + a by the one-step rule; the states carry no orc_step_flips flag (asserted)"""
    import simparams_ref as SR
    spec, mnp, sp0, tp = SR.task_setup("Humanoid")
    n, nd = 6, spec.num_dofs
    rng = np.random.default_rng(41)
    root, dof = SR.random_states(spec, tp, n, rng, (2.0, 2.5))
    lo, hi = np.array(tp.dof_lower[:nd]), np.array(tp.dof_upper[:nd])
    dof[..., 0] = lo + (hi - lo) * rng.uniform(0.3, 0.7, (n, nd))
    act = rng.uniform(-50, 50, (n, nd)).astype(np.float32)
    a = rng.uniform(-LF.ACC, LF.ACC, (n, 3)).astype(np.float32)
    sp = LF.sp_at(sp0, None, 2, tgs)
    sps = [LF.sp_at(sp0, a[e], 2, tgs) for e in range(n)]
    pre = LF.Host(spec, root, dof, act)
    assert not pre.flags_each(mnp, sps).any() and not pre.flags_each(mnp, [sp] * n).any()
    assert LF.num_candidates(mnp, sp, root, dof).max() == 0
    ref = LF.Host(spec, root, dof, act).simulate_each(mnp, sps)
    base = LF.Host(spec, root, dof, act).simulate_each(mnp, [sp] * n)
    f = LF.forces(spec, mnp, root, dof, a, LF.ENV)
    with Sim(lib, spec, mnp, sp, n) as sim:
        assert sim.lanes() == 32
        got = sim.run(root, dof, act, None, f, LF.ENV)
    moved = np.zeros(n, bool)
    for name, x, y, atol, rtol in LF.outside(spec, got, ref, n):
        assert not PS.env_bad(x, y, atol, rtol).any(), name
    for name, x, y, atol, rtol in LF.outside(spec, base, ref, n):
        moved |= PS.env_bad(x, y, atol, rtol)
    assert moved.all(), "the forces matter in every state"
