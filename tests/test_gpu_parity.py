"""GPU parity: the HIP path (through the C ABI) vs the golden fixtures and vs the
CPU oracle.  Needs an MI355X: run with ``pytest -m gpu``.

Tolerances (stated per north_star, obs/reward parity <= 1e-4 relative):
  * jit obs/reward kernels vs the reference's own outputs: rtol 1e-4, atol 1e-4
    (fp32 with the reference's op order; transcendentals differ by ulps);
    potentials bit-exact (same fp32 sequence); resets exact.
  * physics (one control step from identical states, fp32 GPU vs fp64 oracle):
    positions/angles atol 2e-4, velocities atol 2e-3 + 2e-3 |v| (see
    DESIGN.md §Parity for the derivation), sensors atol 1e-2 |F|max.
  * RNG: the device counter RNG equals the oracle's bit for bit.
"""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import parity_stats as PS
import pyoracle as O
from migym import _abi, configs, model as M, taskdefs
from simparams_ref import random_states   # the physics tests' random states (shared with the CPU tests)

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"


def load(name):
    return dict(np.load(os.path.join(G, name)))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def P(t):
    return None if t is None else t.data_ptr()


def setup(task, n_contacts=None):
    cfg = configs.task_config(task, 16)
    spec = M.load_builtin(taskdefs.TASK_INFO[task][1])
    sp = taskdefs.sim_params(cfg, n_contacts or taskdefs.TASK_INFO[task][5])
    tp = taskdefs.task_params(task, cfg, spec)
    return spec, sp, tp


def stream():
    return torch.cuda.current_stream().cuda_stream


# -------------------------------------------------------------------------------------- jit kernels
@pytest.mark.parametrize("task", ["Ant", "Humanoid"])
def test_observation_kernel_matches_reference(lib, task):
    d = load(f"jit_{task.lower()}.npz")
    spec, sp, tp = setup(task)
    n = d["root"].shape[0]
    nd = tp.num_actions
    root = T(d["root"])
    dof = T(np.stack([d["dof_pos"], d["dof_vel"]], -1))
    dforce = T(d.get("dof_force", np.zeros((n, nd))))
    sens = T(d["sensors"])
    act = T(d["actions"])
    pot = T(d["potentials_in"])
    prev = torch.zeros(n, device=DEV)
    up = torch.zeros((n, 3), device=DEV)
    hd = torch.zeros((n, 3), device=DEV)
    obs = torch.zeros((n, tp.num_obs), device=DEV)
    _abi.check(lib.mg_compute_observations(C.byref(tp), n, P(root), P(dof), P(dforce), P(sens), P(act), P(pot),
                                           P(prev), P(up), P(hd), P(obs), stream()), lib)
    torch.cuda.synchronize()
    np.testing.assert_allclose(obs.cpu().numpy(), d["obs"], rtol=1e-4, atol=1e-4)
    np.testing.assert_array_equal(pot.cpu().numpy(), d["potentials"])
    np.testing.assert_array_equal(prev.cpu().numpy(), d["prev_potentials"])
    np.testing.assert_allclose(up.cpu().numpy(), d["up_vec"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(hd.cpu().numpy(), d["heading_vec"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("task", ["Ant", "Humanoid", "Cartpole"])
def test_reward_kernel_matches_reference(lib, task):
    d = load(f"jit_{task.lower()}.npz")
    spec, sp, tp = setup(task)
    obs = T(d["obs"])
    n = obs.shape[0]
    act = T(d["actions"]) if "actions" in d else torch.zeros((n, 1), device=DEV)
    pot = T(d["potentials"]) if "potentials" in d else torch.zeros(n, device=DEV)
    prev = T(d["prev_potentials"]) if "prev_potentials" in d else torch.zeros(n, device=DEV)
    prog = T(d["progress"], torch.int64)
    reset = T(d["reset_buf"], torch.int64)
    rew = torch.zeros(n, device=DEV)
    _abi.check(lib.mg_compute_reward(C.byref(tp), n, P(obs), P(act), P(pot), P(prev), P(prog), P(reset), P(rew),
                                     stream()), lib)
    torch.cuda.synchronize()
    np.testing.assert_allclose(rew.cpu().numpy(), d["rew"], rtol=1e-4, atol=1e-4)
    np.testing.assert_array_equal(reset.cpu().numpy(), d["reset"])


class DevEnv:
    """Device buffers mirroring pyoracle.HostEnv (so both paths see identical inputs)."""

    def __init__(self, h: O.HostEnv):
        self.h = h
        self.root = T(h.root)
        self.dof = T(h.dof)
        self.act_eff = T(h.act_eff)
        self.sensors = T(h.sensors)
        self.dof_force = T(h.dof_force)
        self.actions = T(h.actions)
        self.actions_out = T(h.actions_out)
        self.obs = T(h.obs)
        self.obs_clamped = T(h.obs_clamped)
        self.rew = T(h.rew)
        self.reset = T(h.reset, torch.int64)
        self.progress = T(h.progress, torch.int64)
        self.timeout = torch.zeros(h.n, dtype=torch.bool, device=DEV)
        self.potentials = T(h.potentials)
        self.prev_potentials = T(h.prev_potentials)
        self.up = T(h.up)
        self.heading = T(h.heading)
        self.noise = None
        self.env_props = None if h.env_props is None else T(h.env_props)   # domain-randomized rows, as the oracle's

    def views(self):
        v = _abi.StateViews()
        v.root_states, v.dof_state, v.dof_actuation = P(self.root), P(self.dof), P(self.act_eff)
        v.sensors, v.dof_force, v.rigid_body_states = P(self.sensors), P(self.dof_force), None
        if self.env_props is not None:
            v.env_props, v.env_props_stride = P(self.env_props), self.env_props.shape[1]
        return v

    def buffers(self, seed=0, step=0):
        b = _abi.TaskBuffers()
        b.actions, b.actions_out, b.obs, b.obs_clamped = P(self.actions), P(self.actions_out), P(self.obs), \
            P(self.obs_clamped)
        b.rew, b.reset, b.progress, b.timeout = P(self.rew), P(self.reset), P(self.progress), P(self.timeout)
        b.potentials, b.prev_potentials = P(self.potentials), P(self.prev_potentials)
        b.up_vec, b.heading_vec = P(self.up), P(self.heading)
        b.noise = P(self.noise)
        b.seed, b.step_counter, b.env_offset = seed, step, 0
        return b


@pytest.mark.parametrize("task", ["Ant", "Humanoid"])
def test_post_physics_replays_reference_trace(lib, task):
    d = load(f"trace_{task.lower()}.npz")
    spec, sp, tp = setup(task)
    tp.max_episode_length = int(d["episode_length"])
    Tn, N = d["actions"].shape[:2]
    h = O.HostEnv(tp, spec, N)
    e = DevEnv(h)
    for t in range(Tn):
        e.actions.copy_(T(d["actions"][t]))
        e.root.copy_(T(d["phys_root"][t]))
        e.dof.copy_(T(d["phys_dof"][t]))
        e.sensors.copy_(T(d["phys_sensors"][t]))
        e.dof_force.copy_(T(d["phys_dof_force"][t]))
        e.noise = T(d["noise"][t])
        v, b = e.views(), e.buffers()
        _abi.check(lib.mg_post_physics(None, C.byref(tp), C.byref(v), C.byref(b), N, stream()), lib)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(e.root.cpu().numpy(), d["root_after"][t])
        np.testing.assert_allclose(e.dof.cpu().numpy(), d["dof_after"][t], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(e.obs_clamped.cpu().numpy(), d["obs"][t], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(e.rew.cpu().numpy(), d["rew"][t], rtol=1e-4, atol=1e-4)
        np.testing.assert_array_equal(e.reset.cpu().numpy(), d["reset"][t])
        np.testing.assert_array_equal(e.progress.cpu().numpy(), d["progress"][t])
        np.testing.assert_array_equal(e.timeout.cpu().numpy().astype(np.int64), d["timeouts"][t])
        np.testing.assert_array_equal(e.potentials.cpu().numpy(), d["potentials"][t])


def test_cartpole_post_physics_replays_reference_trace(lib):
    d = load("trace_cartpole.npz")
    spec, sp, tp = setup("Cartpole")
    Tn, N = d["actions"].shape[:2]
    h = O.HostEnv(tp, spec, N)
    e = DevEnv(h)
    for t in range(Tn):
        e.actions.copy_(T(d["actions"][t]))
        e.dof.copy_(T(d["phys_dof"][t]))
        e.noise = T(d["noise"][t])
        v, b = e.views(), e.buffers()
        _abi.check(lib.mg_post_physics(None, C.byref(tp), C.byref(v), C.byref(b), N, stream()), lib)
        torch.cuda.synchronize()
        np.testing.assert_allclose(e.dof.cpu().numpy(), d["dof_after"][t], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(e.obs_clamped.cpu().numpy(), d["obs"][t], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(e.rew.cpu().numpy(), d["rew"][t], rtol=1e-4, atol=1e-4)
        np.testing.assert_array_equal(e.reset.cpu().numpy(), d["reset"][t])
        np.testing.assert_array_equal(e.progress.cpu().numpy(), d["progress"][t])


def test_device_rng_equals_oracle_rng(lib):
    spec, sp, tp = setup("Ant")
    n = 1000
    h = O.HostEnv(tp, spec, n)
    h.reset[:] = 1
    e = DevEnv(h)
    v, b = e.views(), e.buffers(seed=1234, step=77)
    _abi.check(lib.mg_post_physics(None, C.byref(tp), C.byref(v), C.byref(b), n, stream()), lib)
    h.post_physics(tp, seed=1234, step=77)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(e.dof.cpu().numpy(), h.dof)


# -------------------------------------------------------------------------------------- physics
def _gpu_simulate(lib, mnp, sp, root, dof, act, ns):
    """one mg_sim_simulate of the states on the device: (root, dof, sensors, dof force) after it"""
    n = len(root)
    r_d, d_d, a_d = T(root), T(dof), T(act)
    s_d, f_d = torch.zeros((n, ns * 6), device=DEV), torch.zeros((n, dof.shape[1]), device=DEV)
    h = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(h)), lib)
    v = _abi.StateViews()
    v.root_states, v.dof_state, v.dof_actuation, v.sensors, v.dof_force = P(r_d), P(d_d), P(a_d), P(s_d), P(f_d)
    _abi.check(lib.mg_sim_bind(h, C.byref(v)), lib)
    _abi.check(lib.mg_sim_simulate(h, stream()), lib)
    torch.cuda.synchronize()
    lib.mg_sim_destroy(h)
    return r_d.cpu().numpy(), d_d.cpu().numpy(), s_d.cpu().numpy(), f_d.cpu().numpy()


@pytest.mark.parametrize("task,n,z,fast", [("Ant", 512, (0.25, 0.7), 0), ("Humanoid", 256, (0.6, 1.4), 0),
                                           ("Cartpole", 256, (2.0, 2.0), 0), ("Ant", 256, (4.0, 5.0), 1),
                                           ("Humanoid", 256, (4.0, 5.0), 1), ("Cartpole", 256, (2.0, 2.0), 1),
                                           ("Humanoid", 4096, (4.0, 5.0), 1)])
def test_physics_step_matches_oracle(lib, task, n, z, fast):
    """one gym.simulate from random states; fast = 1: joint rates ~N(0, 40) and root spins ~N(0, 40) in the
    air, so that the link angular-velocity cap (max_angular_velocity) and the link damping act in most envs"""
    spec, sp, tp = setup(task)
    rng = np.random.default_rng(7 + fast)
    root, dof = random_states(spec, tp, n, rng, z)
    if task == "Cartpole":
        root[:, :] = 0
        root[:, 2] = 2.0
        root[:, 6] = 1.0
    if fast:
        dof[:, :, 1] *= 40.0
        root[:, 10:13] *= 80.0
    act = (rng.uniform(-1, 1, (n, spec.num_dofs)) * (15.0 if task == "Ant" else 50.0)).astype(np.float32)
    ns = max(len(spec.sensors), 1)
    sens_h = np.zeros((n, ns * 6), np.float32)
    dfor_h = np.zeros((n, spec.num_dofs), np.float32)
    mnp = M.pack_model(spec)
    r_h, d_h = root.copy(), dof.copy()
    O.simulate(mnp, sp, r_h, d_h, act, sens_h, dfor_h, threads=8)
    rg, dg, sg, fg = _gpu_simulate(lib, mnp, sp, root, dof, act, ns)
    test = f"test_physics_step_matches_oracle[{task}{'-fast' if fast else ''}{f'-{n}' if n > 512 else ''}]"
    if fast:   # the cap acted: some link ends at |w| = W (root spin or a joint rate above it)
        W = float(mnp["link_max_ang_vel"])
        assert (np.abs(d_h[..., 1]).max() > 0.5 * W) and (np.abs(dof[..., 1]).max() > W)
    checks = (("root pose", rg[:, 0:7], r_h[:, 0:7], 2e-4, 0), ("dof pos", dg[..., 0], d_h[..., 0], 2e-4, 0),
              ("root twist", rg[:, 7:13], r_h[:, 7:13], 2e-3, 2e-3), ("dof vel", dg[..., 1], d_h[..., 1], 2e-3, 2e-3))
    for name, a, b, _, _ in checks:
        PS.record(test, name, a, b)
    if fast:   # every env within tolerance unless its step clipped a rate to an ill-conditioned cap interval end
        pre = O.HostEnv(tp, spec, n)
        pre.root[:], pre.dof[:], pre.act_eff[:] = root, dof, act
        bad = PS.spin_bad(rg, dg, r_h, d_h, root, dof, sp.dt)
        # every env spins its root above the cap, so each hinge below a clamped link has |w_p| = W and an interval
        # of half-width |a . w_p|: bit 64 reaches ~3% (Ant) / ~8% (Humanoid) of these stress states, hence 12%
        # and the oracle-sensitivity fallback where the dynamics are stiff (tests/test_step_flags.py)
        # No oracle-sensitivity fallback here (round 4 perturbed each env by the kernel's own first-substep drift, the
        # quantity under test).  These states are a stress case -- every root spins above the 100 rad/s cap, so fp32
        # rounding of the |w|^2 h Coriolis and cap terms reaches every velocity -- and some env-steps may disagree
        # without a flag.  How many is set by the fp32 twin (the oracle's own fp32 build, an implementation independent
        # of the kernel) on the same states, not by the kernel's own count: the GPU may leave at most 4 x
        # the twin's unflagged disagreements unexplained (the factor of the column rule, assert_north_star_rtol).
        # Measured round 5: twin 1 of 4,096 Humanoid env-steps (tests/test_step_flags.py, same seed), GPU 3; Ant and
        # the 256-env cases 0 and 0.
        flags = PS.step_flags(mnp, sp, pre)
        r32, d32 = root.copy(), dof.copy()
        O.simulate(mnp, sp, r32, d32, act, np.zeros_like(sens_h), np.zeros_like(dfor_h), threads=8, fp32=True)
        twin_unexplained = int((PS.spin_bad(r32, d32, r_h, d_h, root, dof, sp.dt) & (flags == 0)).sum())
        PS.record(test, "fp32 twin: unflagged disagreeing env-steps", np.array([twin_unexplained]), np.array([0]))
        PS.assert_steps_explained(test, bad[None], flags[None], sens=None, reach_cap=0.12,
                                  allow_unexplained=4.0 * twin_unexplained / n)
        return
    np.testing.assert_allclose(rg[:, 0:7], r_h[:, 0:7], atol=2e-4)
    np.testing.assert_allclose(dg[..., 0], d_h[..., 0], atol=2e-4)
    np.testing.assert_allclose(rg[:, 7:13], r_h[:, 7:13], atol=2e-3, rtol=2e-3)
    np.testing.assert_allclose(dg[..., 1], d_h[..., 1], atol=2e-3, rtol=2e-3)
    if len(spec.sensors):
        scale = max(1.0, np.abs(sens_h).max())
        PS.record(test, "sensors", sg, sens_h, scale=scale)
        np.testing.assert_allclose(sg, sens_h, atol=1e-2 * scale)
    PS.record(test, "dof force", fg, dfor_h)
    np.testing.assert_allclose(fg, dfor_h, atol=1e-2 * max(1.0, np.abs(dfor_h).max()))


def test_free_link_damping_and_cap_on_device(lib):
    """k_simulate on one free rigid link (spherical inertia, gravity off): w decays by 1 / (1 + h c) per substep
    (gym AssetOptions.angular_damping), and a spin past max_angular_velocity ends at W"""
    node = M.Node(name="link", parent=-1, jtype=M.JT_FREE, t=[0, 0, 0], r0=[0, 0, 0, 1], axis=[0, 0, 1], body=0,
                  mass=1.0, inertia=[0.02, 0.02, 0.02, 0.0, 0.0, 0.0])
    body = M.Body(name="link", node=0, pos=[0, 0, 0], quat=[0, 0, 0, 1], parent_body=-1, mass=1.0)
    spec = M.ModelSpec(name="link", fixed_base=0, nodes=[node], bodies=[body], geoms=[], pairs=[], actuators=[],
                       dof_names=[], angular_damping=0.5, max_angular_velocity=10.0)
    mnp = M.pack_model(spec)
    sp = taskdefs.sim_params(configs.task_config("Ant", 1), 1)
    for i in range(3):
        sp.gravity[i] = 0.0
    sp.dt, sp.substeps = sp.dt / sp.substeps, 1   # the clamp ends the substep: |w| = W exactly
    n = 64
    root = np.zeros((n, 13), np.float32)
    root[:, 2] = 1.0
    root[:, 6] = 1.0
    root[:, 7:10] = (0.3, -0.2, 0.1)
    rng = np.random.default_rng(0)
    root[:, 10:13] = rng.normal(0, 1.0, (n, 3)) * np.where(np.arange(n) < n // 2, 2.0, 30.0)[:, None]
    r_d, d_d = T(root), torch.zeros((n, 1, 2), device=DEV)  # no DOFs (a non-empty buffer to bind)
    h = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(h)), lib)
    v = _abi.StateViews()
    v.root_states, v.dof_state = P(r_d), P(d_d)
    _abi.check(lib.mg_sim_bind(h, C.byref(v)), lib)
    _abi.check(lib.mg_sim_simulate(h, stream()), lib)
    torch.cuda.synchronize()
    lib.mg_sim_destroy(h)
    rg = r_d.cpu().numpy()
    hh = sp.dt / sp.substeps
    # exact decay while below the cap (first half: |w| <= ~8 < W)
    w0 = root[:, 10:13].astype(np.float64)
    slow = np.linalg.norm(w0, axis=1) < 10.0
    want = w0 / (1.0 + hh * 0.5) ** sp.substeps
    np.testing.assert_allclose(rg[slow, 10:13], want[slow], rtol=2e-6, atol=1e-7)
    wn = np.linalg.norm(rg[:, 10:13].astype(np.float64), axis=1)
    assert np.all(wn <= 10.0 * (1 + 1e-6)) and np.all(np.abs(wn[~slow] - 10.0) < 1e-5 * 10.0), wn
    # the linear velocity is not asserted constant: the semi-implicit step carries the Coriolis term of the pre-cap
    # spin (|w| h up to ~1 rad here), which turns v; the clamp itself adds nothing (COM at the origin), and the
    # oracle, which runs the same integrator, agrees on every env
    r_h = root.copy()
    O.simulate(mnp, sp, r_h, np.zeros((n, 0, 2), np.float32))
    np.testing.assert_allclose(rg, r_h, atol=1e-6, rtol=1e-6)


def test_frictionloss_on_device(lib):
    """the dry joint friction law (MJCF frictionloss, -f tanh(qd / v_s) linearly implicit) in k_simulate: one hinge
    link spun at rates across v_s (0 .. 2 rad/s, both signs) under torques below and above f, 20 steps on the
    device against the oracle (tests/test_oracle_physics.py pins the law itself)"""
    from test_oracle_physics import hinge_link_spec
    f = 0.01
    mnp = M.pack_model(hinge_link_spec(f))
    sp = taskdefs.sim_params(configs.task_config("Ant", 1), 1)
    for i in range(3):
        sp.gravity[i] = 0.0
    sp.limit_margin = -1.0
    n = 64
    rng = np.random.default_rng(3)
    root = np.zeros((n, 13), np.float32)
    root[:, 6] = 1.0
    dof = np.zeros((n, 1, 2), np.float32)
    dof[:, 0, 1] = np.concatenate([rng.uniform(-0.03, 0.03, n // 2), rng.uniform(-2.0, 2.0, n // 2)])
    act = (rng.uniform(-2.0, 2.0, (n, 1)) * f).astype(np.float32)
    r_d, d_d, a_d = T(root), T(dof), T(act)
    h = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(h)), lib)
    v = _abi.StateViews()
    v.root_states, v.dof_state, v.dof_actuation = P(r_d), P(d_d), P(a_d)
    _abi.check(lib.mg_sim_bind(h, C.byref(v)), lib)
    r_h, d_h = root.copy(), dof.copy()
    for _ in range(20):
        _abi.check(lib.mg_sim_simulate(h, stream()), lib)
        O.simulate(mnp, sp, r_h, d_h, act)
    torch.cuda.synchronize()
    lib.mg_sim_destroy(h)
    dg = d_d.cpu().numpy()
    np.testing.assert_allclose(dg[..., 1], d_h[..., 1], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(dg[..., 0], d_h[..., 0], rtol=1e-4, atol=1e-6)
    # the friction acted: the rates moved from where a frictionless hinge would take them
    free = dof[:, 0, 1] + act[:, 0] / 0.02 * 20 * sp.dt
    assert np.abs(d_h[:, 0, 1] - free).max() > 0.05


def _teacher_forced(lib, test, spec, sp, tp, h, steps, actions, seed, mutate=None, threads=8):
    """mg_env_step vs orc_env_step step by step, each step started on both sides from the oracle's state (the GPU
    buffers are reloaded from it), so one step's fp32-vs-fp64 difference cannot grow into a chaotic divergence
    over the following steps.  Per step: progress exact; every env's obs within 2e-3 + 2e-3 |x|, reward within
    5e-3 + 5e-3 |r| and the same reset, unless orc_step_flips puts that env's step at a discontinuity (or the
    oracle is itself sensitive there); the exemptions' reach is capped (parity_stats.assert_steps_explained).
    Returns the per-column-group statistics against north_star's 1e-4 relative over the unflagged env-steps
    (parity_stats.column_stats; recorded in the parity report)."""
    n = h.n
    mnp = M.pack_model(spec)
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    bad = np.zeros((steps, n), bool)
    flags = np.zeros((steps, n), np.int32)
    pres, outs, rews = [], [], []
    try:
        for t in range(steps):
            h.actions[:] = actions[t]
            if mutate is not None:
                mutate(t, h)
            e = DevEnv(h)
            _abi.check(lib.mg_sim_bind(sim, C.byref(e.views())), lib)
            flags[t] = PS.step_flags(mnp, sp, PS.loco_physics_input(h, mnp, sp, tp, seed, t, threads=threads))
            pres.append(copy.deepcopy(h))
            h.env_step(mnp, sp, tp, seed=seed, step=t, threads=threads)
            _abi.check(lib.mg_env_step(sim, C.byref(tp), C.byref(e.buffers(seed=seed, step=t)), stream()), lib)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(e.progress.cpu().numpy(), h.progress)
            og, rg = e.obs.cpu().numpy(), e.rew.cpu().numpy()
            bad[t] = (PS.env_bad(og, h.obs, 2e-3, 2e-3) | PS.env_bad(rg[:, None], h.rew[:, None], 5e-3, 5e-3)
                      | (e.reset.cpu().numpy() != h.reset))
            outs.append((og, h.obs.copy()))
            rews.append((rg, h.rew.copy()))
            PS.record(test, f"obs step {t}", og, h.obs, envs_outside=int(bad[t].sum()))
    finally:
        lib.mg_sim_destroy(sim)
    sens = lambda t, i: PS.oracle_sensitive_step(mnp, sp, tp, pres[t], actions[t], i, outs[t][0][i], outs[t][1][i],
                                                 seed=seed, step=t, hand=False)
    # (a multi-agent env cannot be replayed one actor alone: no sensitivity fallback there)
    PS.assert_steps_explained(test, bad, flags, sens if tp.num_agents <= 1 else None)
    keep = (flags == 0).ravel()
    og = np.concatenate([o[0] for o in outs])
    oh = np.concatenate([o[1] for o in outs])
    groups = dict(PS.OBS_GROUPS.get(tp.num_obs, {"obs": list(range(tp.num_obs))}))
    cols = PS.column_stats(test, "columns vs 1e-4 rel (unflagged env-steps)", og, oh, keep, groups)
    rh = np.concatenate([r[1] for r in rews])[:, None]
    rw = PS.column_stats(test, "reward vs 1e-4 rel (unflagged env-steps)", np.concatenate([r[0] for r in rews])[:, None],
                         rh, keep, {"reward": [0]})
    cols.update(rw)
    # the fp32 twin: the same teacher-forced steps through the oracle's own fp32 build (liboracle_f32, an fp32
    # implementation independent of the kernel), against the same fp64 results -- how far fp32 rounding alone moves
    # each column group
    o32, r32 = [], []
    for t in range(steps):
        g = copy.deepcopy(pres[t])
        g.env_step(mnp, sp, tp, seed=seed, step=t, threads=threads, fp32=True)
        o32.append(g.obs.copy())
        r32.append(g.rew.copy())
    twin = PS.column_stats(test, "fp32 twin: columns vs 1e-4 rel (unflagged env-steps)", np.concatenate(o32), oh, keep,
                           groups)
    twin.update(PS.column_stats(test, "fp32 twin: reward vs 1e-4 rel (unflagged env-steps)",
                                np.concatenate(r32)[:, None], rh, keep, {"reward": [0]}))
    # the reward's progress term is a difference of two potentials -|to_target| / dt, |potential| ~ 6e4 in fp32: its
    # resolution is that magnitude's fp32 spacing (2^-8), whichever side of a rounding boundary a state lands on
    pot_ulp = float(np.spacing(np.float32(max(np.abs(p.potentials).max() for p in pres) if tp.num_obs >= 60 else 0.0)))
    return cols, twin, pot_ulp


def assert_north_star_rtol(res, twin_factor=4.0, frac_margin=0.005):
    """north_star: obs / reward parity within 1e-4 relative.  Per column group g over the unflagged env-steps (the
    teacher-forced fp32 GPU step against the fp64 oracle from the same state): |gpu - oracle| <= 1e-4 |oracle| + a_g,
    a_g = max(1e-4 S_g, 4 x the fp32 twin's need, the reward's potential spacing), S_g the group's magnitude in the
    batch (max |oracle|).  The floor 1e-4 S_g is the 1e-4 relative taken on the group's scale: a solve mixes a group's
    magnitudes, and an entry that ends near 0 keeps the rounding of the O(S_g) terms that cancelled.  Where fp32
    rounding itself needs more -- the oracle's own fp32 build from the same states needs a larger atol (the stiff
    contact / limit impulses behind the Humanoid's foot force-torques and DOF velocities) -- the GPU may need up to
    twin_factor times that (different operation order, FMA contraction, 1-ulp hardware reciprocals).  The reward
    adds the fp32 spacing of its potentials (DESIGN.md §6 lists the groups where 1e-4 S_g does not hold and why).
    Per element, the fraction of a group's entries within 1e-4 |x| (no floor) must be at least the twin's minus
    frac_margin (0.5 %)."""
    cols, twin, pot_ulp = res
    bad = {}
    for g, v in cols.items():
        a = max(1e-4 * v["scale"], twin_factor * twin[g]["atol_needed"], pot_ulp if g == "reward" else 0.0)
        if v["atol_needed"] > a:
            bad[g] = dict(v, allowed=a)
        # and element by element: the fraction of the group's entries within 1e-4 |x| alone, with no
        # floor, at least the fp32 twin's own fraction minus 0.5 % (measured round 6: Ant DOF velocities 88.9 % vs
        # 89.1 %; the fused PGS velocity update had left them 0.8 % below, team_physics.hpp substep() visit)
        if v["frac_within_rtol"] < twin[g]["frac_within_rtol"] - frac_margin:
            bad[g + " (fraction within 1e-4 |x|)"] = {"gpu": v["frac_within_rtol"], "twin": twin[g]["frac_within_rtol"]}
    assert not bad, f"column groups outside 1e-4 |x| + a_g: {bad}"


@pytest.mark.parametrize("task,n", [("Ant", 256), ("Humanoid", 128), ("Cartpole", 256)])
def test_fused_env_step_matches_oracle(lib, task, n):
    """mg_env_step (the bench path) vs orc_env_step over 4 teacher-forced control steps, device RNG resets."""
    spec, sp, tp = setup(task)
    h = O.HostEnv(tp, spec, n)
    rng = np.random.default_rng(3)
    acts = [rng.uniform(-1.2, 1.2, (n, tp.num_actions)).astype(np.float32) for _ in range(4)]
    cols = _teacher_forced(lib, f"test_fused_env_step_matches_oracle[{task}]", spec, sp, tp, h, 4, acts, seed=5)
    assert_north_star_rtol(cols)


def kernel_layout(lib, spec, sp, n):
    """(team lanes, compact) of the step-kernel instance mg_sim_create picks for n envs (mg_sim_kernel_layout)"""
    mnp = M.pack_model(spec)
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    t, lay = C.c_int32(), C.c_int32()
    try:
        _abi.check(lib.mg_sim_kernel_layout(sim, C.byref(t), C.byref(lay)), lib)
    finally:
        lib.mg_sim_destroy(sim)
    return t.value, lay.value


@pytest.mark.parametrize("layout", ["classic", "compact"])
@pytest.mark.parametrize("task,n", [("Ant", 256), ("Humanoid", 128)])
def test_pinned_layout_matches_oracle(lib, task, n, layout, monkeypatch):
    """MIGYM_LAYOUT: the locomotion models' two team layouts -- classic (8 waves per CU; the default
    up to 2,048 waves) and compact (12 waves per CU; the default above) -- each pinned at a small batch and put
    through test_fused_env_step_matches_oracle's teacher-forced check; mg_sim_kernel_layout shows which ran."""
    monkeypatch.setenv("MIGYM_LAYOUT", layout)
    spec, sp, tp = setup(task)
    assert kernel_layout(lib, spec, sp, n)[1] == (layout == "compact")
    h = O.HostEnv(tp, spec, n)
    rng = np.random.default_rng(3)
    acts = [rng.uniform(-1.2, 1.2, (n, tp.num_actions)).astype(np.float32) for _ in range(4)]
    cols = _teacher_forced(lib, f"test_pinned_layout_matches_oracle[{task}-{layout}]", spec, sp, tp, h, 4, acts,
                           seed=5)
    assert_north_star_rtol(cols)


def test_layout_env_rejects_unknown_values(lib, monkeypatch):
    """MIGYM_LAYOUT accepts auto / compact / classic only: anything else fails mg_sim_create with MG_EINVAL"""
    monkeypatch.setenv("MIGYM_LAYOUT", "fast")
    spec, sp, tp = setup("Ant")
    mnp = M.pack_model(spec)
    sim = C.c_void_p()
    rc = lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), 64, 0, C.byref(sim))
    assert rc != 0 and b"MIGYM_LAYOUT" in lib.mg_last_error()


@pytest.mark.parametrize("task,n,compact", [("Ant", 8192, 0), ("Ant", 8196, 1), ("Humanoid", 4096, 0),
                                            ("Humanoid", 4098, 1), ("MAAnt", 2048, 0), ("Cartpole", 65536, 0)])
def test_auto_layout_threshold(lib, task, n, compact, monkeypatch):
    """the default layout choice: compact once the batch has more than 2,048 waves (dispatch.hpp kCompactMinWaves;
    Ant / MA-Ant 4 actors per wave, Humanoid 2), never for a model without a compact instance (Cartpole)"""
    monkeypatch.delenv("MIGYM_LAYOUT", raising=False)
    spec, sp, tp = ma_setup(4) if task == "MAAnt" else setup(task)
    assert kernel_layout(lib, spec, sp, n * (4 if task == "MAAnt" else 1)) == ({"Cartpole": 8, "Humanoid": 32}.get(
        task, 16), compact)


@pytest.mark.parametrize("task,n", [("Ant", 16384), ("Humanoid", 32768), ("Ant", 65536)])
def test_fused_parity_at_baseline_size(lib, task, n):
    """BASELINE.json configs[1] (Ant, 16,384 envs), configs[2] (Humanoid, 32,768 envs: the work-ordered K = 1
    path) and the headline configuration (Ant, 65,536 envs: the compact 12-wave kernel on the sorted
    path, the second and third teacher-forced launches run in the sort's permutation) against the oracle at full
    size: the oracle first rolls every env 12 steps on from the
    all-reset start (random actions; falls, resets and contacts spread over the batch), then 3 fused steps are
    teacher-forced as in test_fused_env_step_matches_oracle.  The per-column-group errors against north_star's
    1e-4 relative are recorded (MIGYM_PARITY_REPORT)."""
    spec, sp, tp = setup(task)
    h = O.HostEnv(tp, spec, n)
    mnp = M.pack_model(spec)
    rng = np.random.default_rng(31)
    for t in range(12):
        h.actions[:] = rng.uniform(-1, 1, (n, tp.num_actions)).astype(np.float32)
        h.env_step(mnp, sp, tp, seed=7, step=100 + t, threads=16)
    acts = [rng.uniform(-1.2, 1.2, (n, tp.num_actions)).astype(np.float32) for _ in range(3)]
    cols = _teacher_forced(lib, f"test_fused_parity_at_baseline_size[{task}-{n}]", spec, sp, tp, h, 3, acts, seed=7,
                           threads=16)
    assert_north_star_rtol(cols)


@pytest.mark.parametrize("task,n", [("Ant", 256), ("Humanoid", 128)])
def test_error_budget_over_horizon(lib, task, n):
    """GPU (fp32) vs oracle (fp64) from identical states over 30 fused control steps with random actions and
    device-RNG resets: the per-horizon error budget of DESIGN.md §6.  Errors start at fp32 rounding and grow
    where a contact / limit decision flips between the two; the bounds below are the stated budget."""
    spec, sp, tp = setup(task)
    h = O.HostEnv(tp, spec, n)
    e = DevEnv(h)
    mnp = M.pack_model(spec)
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    _abi.check(lib.mg_sim_bind(sim, C.byref(e.views())), lib)
    rng = np.random.default_rng(21)
    # p99 of the |root position| error (m) at each horizon (measured: Ant 0 / 6e-8 / 4e-7 / 2.5e-4,
    # Humanoid 0 / 1.4e-7 / 5e-6 / 2.8e-5)
    budget = {1: 1e-6, 3: 1e-5, 10: 1e-4, 30: 2e-3}
    test = f"test_error_budget_over_horizon[{task}]"
    for t in range(30):
        a = rng.uniform(-1, 1, (n, tp.num_actions)).astype(np.float32)
        h.actions[:] = a
        e.actions.copy_(T(a))
        h.env_step(mnp, sp, tp, seed=13, step=t, threads=8)
        _abi.check(lib.mg_env_step(sim, C.byref(tp), C.byref(e.buffers(seed=13, step=t)), stream()), lib)
        if t + 1 in budget:
            torch.cuda.synchronize()
            rp = e.root.cpu().numpy().reshape(n, 13)
            st = PS.record(test, f"root pos, {t + 1} steps", rp[:, 0:3], h.root.reshape(n, 13)[:, 0:3])
            PS.record(test, f"dof pos, {t + 1} steps", e.dof.cpu().numpy().reshape(n, -1, 2)[..., 0],
                      h.dof.reshape(n, -1, 2)[..., 0])
            assert st["p99"] <= budget[t + 1], (t + 1, st)
    lib.mg_sim_destroy(sim)


def test_set_indexed_scatters_rows(lib):
    spec, sp, tp = setup("Ant")
    n = 100
    mnp = M.pack_model(spec)
    root = torch.zeros((n, 13), device=DEV)
    dof = torch.zeros((n * 8, 2), device=DEV)
    src = torch.randn((n, 13), device=DEV)
    idx = torch.tensor([3, 7, 50, 99], dtype=torch.int32, device=DEV)
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    v = _abi.StateViews()
    v.root_states, v.dof_state, v.sensors = P(root), P(dof), P(torch.zeros((n * 4, 6), device=DEV))
    _abi.check(lib.mg_sim_bind(sim, C.byref(v)), lib)
    _abi.check(lib.mg_set_indexed(sim, _abi.MG_SET_ROOT_STATE, P(src), P(idx), 4, stream()), lib)
    torch.cuda.synchronize()
    lib.mg_sim_destroy(sim)
    exp = torch.zeros_like(root)
    exp[idx.long()] = src[idx.long()]
    assert torch.equal(root, exp)


# -------------------------------------------------------------------------------------- full size
@pytest.mark.parametrize("task,n", [("Ant", 65536), ("Humanoid", 32768)])
def test_full_size_rollout_is_sane(task, n):
    import migym
    env = migym.make(seed=0, task=task, num_envs=n, sim_device=DEV, rl_device=DEV, headless=True)
    g = torch.Generator(device=DEV).manual_seed(0)
    resets = 0
    for _ in range(20):
        a = torch.rand((n, env.num_actions), device=DEV, generator=g) * 2 - 1
        obs_dict, rew, reset, extras = env.step(a)
        obs = obs_dict["obs"]
        resets += int(reset.sum())
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
    assert torch.isfinite(env.root_states).all()
    # every env left the initial all-reset state; torsos are above ground
    assert int(env.progress_buf.min()) >= 0 and float(env.root_states[:, 2].min()) > 0.0
    assert extras["time_outs"].dtype == torch.bool
    env.close()


# -------------------------------------------------------------------------------------- multi-agent
def ma_setup(A=4):
    cfg = configs.task_config("MAAnt", 16)
    cfg["env"]["numAgents"] = A
    spec = M.load_builtin("ant")
    return spec, taskdefs.sim_params(cfg, 16, A), taskdefs.task_params("MAAnt", cfg, spec)


@pytest.mark.parametrize("layout", ["auto", "compact"])
@pytest.mark.parametrize("A", [2, 4])
def test_multi_agent_env_step_matches_oracle(lib, A, layout, monkeypatch):
    """MAAnt fused step (AND-filter resets via wave ballot, others-block via shuffles) vs the oracle, teacher-forced
    step by step (as test_fused_env_step_matches_oracle); `compact` pins the 12-wave team layout."""
    monkeypatch.setenv("MIGYM_LAYOUT", layout)
    spec, sp, tp = ma_setup(A)
    n = A * 96
    h = O.HostEnv(tp, spec, n)
    rng = np.random.default_rng(11)
    acts = [rng.uniform(-1, 1, (n, tp.num_actions)).astype(np.float32) for _ in range(4)]
    masks = {2: (rng.random(n) < 0.6).astype(np.int64)}   # a mix of fully-done and partially-done envs

    def mutate(t, hh):
        if t in masks:
            hh.reset[:] = masks[t]
    assert tp.num_obs == 60 + 3 * (A - 1)
    _teacher_forced(lib, f"test_multi_agent_env_step_matches_oracle[{A}-{layout}]", spec, sp, tp, h, 4, acts, seed=9,
                    mutate=mutate)


def test_multi_agent_parity_at_baseline_shard(lib):
    """BASELINE.json configs[3] (MA-Ant, 65,536 envs x 4 agents over 8 GPUs) at its per-GPU shard, 8,192 envs x 4
    agents: a 12-step oracle pre-roll, then 3 teacher-forced fused steps; every obs column group (the other agents'
    relative torso positions included) and the reward against north_star's 1e-4 relative"""
    spec, sp, tp = ma_setup(4)
    n = 4 * 8192
    h = O.HostEnv(tp, spec, n)
    mnp = M.pack_model(spec)
    rng = np.random.default_rng(41)
    for t in range(12):
        h.actions[:] = rng.uniform(-1, 1, (n, tp.num_actions)).astype(np.float32)
        h.env_step(mnp, sp, tp, seed=13, step=300 + t, threads=16)
    acts = [rng.uniform(-1.2, 1.2, (n, tp.num_actions)).astype(np.float32) for _ in range(3)]
    res = _teacher_forced(lib, "test_multi_agent_parity_at_baseline_shard[8192x4]", spec, sp, tp, h, 3, acts, seed=13,
                          threads=16)
    assert_north_star_rtol(res)


def test_multi_agent_rejects_agents_spanning_waves(lib):
    """Ant teams are 16 lanes (4 actors per wave): 8 agents per env cannot share one wave."""
    spec, sp, tp = ma_setup(8)
    n = 8 * 8
    h = O.HostEnv(tp, spec, n)
    e = DevEnv(h)
    mnp = M.pack_model(spec)
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    _abi.check(lib.mg_sim_bind(sim, C.byref(e.views())), lib)
    rc = lib.mg_env_step(sim, C.byref(tp), C.byref(e.buffers()), stream())
    lib.mg_sim_destroy(sim)
    assert rc == -1 and b"num_agents" in lib.mg_last_error()


def test_multi_agent_make_full_size():
    import migym
    n = 4096
    env = migym.make(seed=0, task="MAAnt", num_envs=n, sim_device=DEV, rl_device=DEV, headless=True)
    assert env.num_agents == 4 and env.num_obs == 69
    from migym.utils.rlgames_utils import RLGPUEnv
    assert RLGPUEnv(env).get_env_info()["agents"] == 4
    a = torch.rand((n * 4, 8), device=DEV) * 2 - 1
    for _ in range(5):
        obs, rew, reset, extras = env.step(a)
    torch.cuda.synchronize()
    assert obs["obs"].shape == (n * 4, 69) and rew.shape == (n * 4,)
    assert torch.isfinite(obs["obs"]).all()
    env.close()


@pytest.mark.parametrize("task,n,z", [("Ant", 512, (0.25, 0.7)), ("Humanoid", 256, (0.6, 1.4))])
def test_net_contact_forces_match_oracle(lib, task, n, z):
    """gym's net contact force tensor (acquire / refresh_net_contact_force_tensor, franka_reach_MA.py:506, 563;
    mg_state_views.net_contact_forces): after one gym.simulate from random states, every body's world-frame net
    contact force equals the oracle's (orc_simulate_views' net_contact_forces) within 1 % of the batch's largest, like
    the sensors.  (The hand's rows -- the object and the goal
    included -- are checked in test_gpu_hand.py's physics tests.)"""
    spec, sp, tp = setup(task)
    rng = np.random.default_rng(11)
    root, dof = random_states(spec, tp, n, rng, z)
    act = (rng.uniform(-1, 1, (n, spec.num_dofs)) * (15.0 if task == "Ant" else 50.0)).astype(np.float32)
    nb = len(spec.bodies)
    mnp = M.pack_model(spec)
    h = O.HostEnv(tp, spec, n)
    h.root[:], h.dof[:], h.act_eff[:] = root, dof, act
    h.ncf = np.zeros((n, nb, 3), np.float32)
    h.simulate(mnp, sp, threads=8)
    r_d, d_d, a_d = T(root), T(dof), T(act)
    s_d = torch.zeros((n, max(len(spec.sensors), 1) * 6), device=DEV)
    c_d = torch.full((n * nb, 3), float("nan"), device=DEV)   # every row must be written
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    v = _abi.StateViews()
    v.root_states, v.dof_state, v.dof_actuation, v.sensors = P(r_d), P(d_d), P(a_d), P(s_d)
    v.net_contact_forces = P(c_d)
    _abi.check(lib.mg_sim_bind(sim, C.byref(v)), lib)
    _abi.check(lib.mg_sim_simulate(sim, stream()), lib)
    torch.cuda.synchronize()
    lib.mg_sim_destroy(sim)
    g = c_d.cpu().numpy().reshape(n, nb, 3)
    assert np.isfinite(g).all()
    scale = max(1.0, float(np.abs(h.ncf).max()))
    assert float(np.abs(h.ncf).max()) > 1.0, "no contact force at all: the states would check nothing"
    PS.record(f"test_net_contact_forces_match_oracle[{task}]", "net contact forces", g, h.ncf, scale=scale)
    np.testing.assert_allclose(g, h.ncf, atol=1e-2 * scale)
