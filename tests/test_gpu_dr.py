"""Domain randomization on the GPU, through the C ABI.

* mg_dr_apply / mg_dr_noise replay the reference's recorded draws (tests/golden/trace_ant_dr.npz, the
  same replay as tests/test_dr.py's oracle check): property values within 1e-6 relative, noise lambdas
  through the reference's actuation and observations (fp32 op order), randomize_buf exact.
* the physics kernels with an env_props table (the domain-randomized instances) vs the oracle applying
  the same rows to its fp64 model, for Ant and ShadowHand, from identical random states — the bars of
  tests/test_gpu_parity.py / test_gpu_hand.py.
* the same on the capacities those two do not reach (Cartpole's 8 lanes, the Humanoid's 32 in both layouts and
  under TGS, the three tree capacities), sensors and DOF forces included; the fused mg_env_step with env_props bound
  (k_env_step<DR>, k_hand_step<DR>) teacher-forced against the oracle by the rules of the plain fused tests; and the
  DR instance on rows of defaults against the plain instance.  Inputs and rules: tests/dr_ref.py; the oracle's fp32
  twin through the same rules on the CPU: tests/test_dr_parity_host.py.
* make() with task.randomize for Ant / Humanoid / ShadowHand: the shipped randomization_params run
  through the fused step, properties land in their ranges, and the per-env rows differ.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import copy

import parity_stats as PS
import pyoracle as O
from migym import _abi, configs, model as M, taskdefs
import dr_ref as DRR
from dr_ref import _dr_explained, _physics_sensitive, agreement, random_props   # shared with tests/test_dr_parity_host.py
from dr_trace import defaults, layout
from test_dr import replay_dr_trace

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


class DeviceBackend:
    """mg_dr_apply / mg_dr_noise: the argument struct's host arrays are mirrored on the device"""

    OUT = {"x", "corr", "env_props", "randomize_buf"}

    def __init__(self, lib):
        self.lib = lib

    def _run(self, fn, args_bufs):
        a, bufs = args_bufs
        dev = {}
        for k, v in bufs.items():
            if v is None:
                continue
            t = torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
            dev[k] = t
            setattr(a, k, t.data_ptr())
        _abi.check(fn(C.byref(a), torch.cuda.current_stream().cuda_stream), self.lib)
        torch.cuda.synchronize()
        for k in self.OUT & dev.keys():
            bufs[k][...] = dev[k].cpu().numpy().reshape(bufs[k].shape)

    def apply(self, args_bufs):
        self._run(self.lib.mg_dr_apply, args_bufs)

    def noise(self, args_bufs):
        self._run(self.lib.mg_dr_noise, args_bufs)


def test_dr_trace_matches_reference_gpu(lib):
    replay_dr_trace(DeviceBackend(lib))


@pytest.mark.parametrize("layout", ["auto", "compact"])
@pytest.mark.parametrize("solver", ["pgs", "tgs"])
def test_dr_physics_matches_oracle_ant(lib, solver, layout, monkeypatch):
    """env_props rows on the GPU vs the oracle (solver tgs: the DR instance of the TGS kernels); at this
    batch the default picks the classic team layout, `compact` pins the 12-wave one (big batches)"""
    monkeypatch.setenv("MIGYM_LAYOUT", layout)
    cfg = configs.task_config("Ant", 16)
    cfg["sim"]["physx"]["solver"] = solver
    spec = M.load_builtin("ant")
    sp = taskdefs.sim_params(cfg, 16)
    n = 384
    rng = np.random.default_rng(21)
    props = random_props(spec, n, rng)
    root = np.zeros((n, 13), np.float32)
    root[:, 2] = rng.uniform(0.3, 0.6, n)
    q = rng.normal(0, 1, (n, 4)) * np.array([0.15, 0.15, 1.0, 1.0])
    root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    root[:, 7:13] = rng.normal(0, 0.5, (n, 6))
    lo = np.array([x.lower for x in spec.nodes[1:]])
    hi = np.array([x.upper for x in spec.nodes[1:]])
    dof = np.stack([lo + (hi - lo) * rng.uniform(0, 1, (n, 8)), rng.normal(0, 1, (n, 8))], -1).astype(np.float32)
    act = rng.uniform(-15, 15, (n, 8)).astype(np.float32)
    sens = np.zeros((n, 24), np.float32)
    mnp = M.pack_model(spec)
    # oracle
    h = O.HostEnv(taskdefs.task_params("Ant", cfg, spec), spec, n)
    h.root[:], h.dof[:], h.act_eff[:] = root, dof, act
    h.env_props = np.ascontiguousarray(props, np.float32)
    pre = copy.deepcopy(h)
    O.lib().orc_simulate_views(mnp.ctypes.data, C.byref(sp), n, C.byref(h.views()), 8)
    # GPU
    tr, td, ta = (torch.from_numpy(x).to(DEV) for x in (root, dof, act))
    ts, tf = torch.zeros((n, 24), device=DEV), torch.zeros((n, 8), device=DEV)
    tp = torch.from_numpy(np.ascontiguousarray(props, np.float32)).to(DEV)
    v = _abi.StateViews()
    v.root_states, v.dof_state, v.dof_actuation, v.sensors, v.dof_force = (x.data_ptr() for x in (tr, td, ta, ts, tf))
    v.env_props, v.env_props_stride = tp.data_ptr(), props.shape[1]
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    _abi.check(lib.mg_sim_bind(sim, C.byref(v)), lib)
    _abi.check(lib.mg_sim_simulate(sim, torch.cuda.current_stream().cuda_stream), lib)
    torch.cuda.synchronize()
    lib.mg_sim_destroy(sim)
    rg, dg = tr.cpu().numpy(), td.cpu().numpy()
    assert np.isfinite(rg).all() and np.isfinite(dg).all()
    _dr_explained(f"test_dr_physics_matches_oracle_ant[{solver}-{layout}]", mnp, sp, pre,
                  [("root pose", rg[:, 0:7], h.root[:, 0:7], 2e-4, 0, lambda g: g.root[0, 0:7]),
                   ("root twist", rg[:, 7:13], h.root[:, 7:13], 2e-3, 2e-3, lambda g: g.root[0, 7:13]),
                   ("dof pos", dg[..., 0], h.dof[..., 0], 2e-4, 0, lambda g: g.dof[0, :, 0]),
                   ("dof vel", dg[..., 1], h.dof[..., 1], 2e-3, 2e-3, lambda g: g.dof[0, :, 1])], hand=False)
    # the properties matter: the same states without them end elsewhere
    h2 = O.HostEnv(taskdefs.task_params("Ant", cfg, spec), spec, n)
    h2.root[:], h2.dof[:], h2.act_eff[:] = root, dof, act
    O.lib().orc_simulate_views(mnp.ctypes.data, C.byref(sp), n, C.byref(h2.views()), 8)
    assert agreement(h2.dof[..., 1], h.dof[..., 1], 2e-3, 2e-3) < 0.5


@pytest.mark.parametrize("kind,solver", [("block", "pgs"), ("egg", "pgs"), ("pen", "pgs"), ("block", "tgs")])
def test_dr_physics_matches_oracle_hand(lib, kind, solver):
    """env_props rows (masses, drives, friction, object mass / friction / scale) on the GPU vs the oracle;
    the object's scale reaches every shape's size (box half extents, egg semi-axes, pen radius + length)."""
    from test_gpu_hand import DevHandEnv, PALM_DZ, hand_states, setup
    spec, sp, tp = setup(kind=kind)
    sp.solver_type = _abi.MG_SOLVER_TGS if solver == "tgs" else _abi.MG_SOLVER_PGS
    n = 192
    rng = np.random.default_rng(23)
    h = hand_states(spec, tp, n, rng, PALM_DZ[kind], pen=kind == "pen")
    props = np.ascontiguousarray(random_props(spec, n, rng), np.float32)
    e = DevHandEnv(h)
    mnp = M.pack_model(spec)
    h.env_props = props
    pre = copy.deepcopy(h)
    O.lib().orc_simulate_views(mnp.ctypes.data, C.byref(sp), n, C.byref(h.views()), 8)
    tp_ = torch.from_numpy(props).to(DEV)
    vg = e.views()
    vg.env_props, vg.env_props_stride = tp_.data_ptr(), props.shape[1]
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    _abi.check(lib.mg_sim_bind(sim, C.byref(vg)), lib)
    _abi.check(lib.mg_sim_simulate(sim, torch.cuda.current_stream().cuda_stream), lib)
    torch.cuda.synchronize()
    lib.mg_sim_destroy(sim)
    rg, dg = e.root.cpu().numpy(), e.dof.cpu().numpy()
    assert np.isfinite(rg).all() and np.isfinite(dg).all()
    _dr_explained(f"test_dr_physics_matches_oracle_hand[{kind}{'-tgs' if solver == 'tgs' else ''}]", mnp, sp, pre,
                  [("object pose", rg[:, 1, 0:7], h.root[:, 1, 0:7], 2e-4, 0, lambda g: g.root[0, 1, 0:7]),
                   ("object twist", rg[:, 1, 7:13], h.root[:, 1, 7:13], 2e-3, 2e-3, lambda g: g.root[0, 1, 7:13]),
                   ("dof pos", dg[..., 0], h.dof[..., 0], 2e-4, 0, lambda g: g.dof[0, :, 0]),
                   ("dof vel", dg[..., 1], h.dof[..., 1], 2e-3, 2e-3, lambda g: g.dof[0, :, 1])], hand=True)


# -------------------------------------------------------------------------- the fused step under domain randomization
# k_env_step<DR> / k_hand_step<DR> are what a run with task.randomize launches every step.  The cases (tests/dr_ref.py
# fused_case: random_props' rows, the oracle rolled on with them, time limits inside the run) go through the harness
# of the plain fused tests unchanged -- DevEnv / DevHandEnv bind the host's env_props, and the deepcopy / env_slice
# copies that step_flags, the sensitivity fallback and the fp32 twin take carry the rows.  tests/test_dr_parity_host.py
# puts the oracle's fp32 twin through the same rule on the CPU.
def _gpu_final_step(lib, spec, sp, tp, pre, hand, props):
    """the observations after one mg_env_step from `pre` (dr_ref.final_step_input) with the rows bound or not"""
    from test_gpu_hand import DevHandEnv
    from test_gpu_parity import DevEnv
    g = copy.deepcopy(pre)
    if not props:
        g.env_props = None
    e = (DevHandEnv if hand else DevEnv)(g)
    mnp = M.pack_model(spec)
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), g.n, 0, C.byref(sim)), lib)
    try:
        _abi.check(lib.mg_sim_bind(sim, C.byref(e.views())), lib)
        _abi.check(lib.mg_env_step(sim, C.byref(tp), C.byref(e.buffers(seed=DRR.STEP_SEED, step=DRR.FUSED_STEPS - 1)),
                                   torch.cuda.current_stream().cuda_stream), lib)
        torch.cuda.synchronize()
    finally:
        lib.mg_sim_destroy(sim)
    return e.obs.cpu().numpy()


def _assert_props_matter(lib, spec, sp, tp, h0, acts, hand):
    """the last teacher-forced step once more with env_props unbound, on both sides: fewer than half the envs then
    end where the domain-randomized step ends (and the device's own DR step does end there)"""
    pre = DRR.final_step_input(spec, sp, tp, h0, acts)
    dr = DRR.oracle_final_step(spec, sp, tp, pre, props=True).obs
    assert agreement(DRR.oracle_final_step(spec, sp, tp, pre, props=False).obs, dr, 2e-3, 2e-3) < 0.5
    assert agreement(_gpu_final_step(lib, spec, sp, tp, pre, hand, props=False), dr, 2e-3, 2e-3) < 0.5
    assert agreement(_gpu_final_step(lib, spec, sp, tp, pre, hand, props=True), dr, 2e-3, 2e-3) > 0.9


@pytest.mark.parametrize("name,layout", [("Cartpole", "classic"), ("Ant", "classic"), ("Ant", "compact"),
                                         ("Humanoid", "classic"), ("Humanoid", "compact"), ("MAAnt", "classic"),
                                         ("Ant-tgs", "classic")])
def test_dr_fused_env_step_matches_oracle(lib, name, layout, monkeypatch):
    """mg_env_step with env_props bound (k_env_step<DR>: the 8-, 16- and 32-lane instances, both team layouts, MA-Ant,
    TGS) against orc_env_step applying the same rows, over 4 teacher-forced control steps with device-RNG resets: the
    rule and the numbers of test_fused_env_step_matches_oracle"""
    from test_gpu_parity import _teacher_forced, assert_north_star_rtol, kernel_layout
    monkeypatch.setenv("MIGYM_LAYOUT", layout)
    spec, sp, tp, h, acts = DRR.fused_case(name)
    lanes = {"Cartpole": 8, "Humanoid": 32}.get(DRR.FUSED[name][0], 16)
    assert kernel_layout(lib, spec, sp, h.n) == (lanes, layout == "compact")
    h0 = copy.deepcopy(h)
    res = _teacher_forced(lib, f"test_dr_fused_env_step_matches_oracle[{name}-{layout}]", spec, sp, tp, h,
                          DRR.FUSED_STEPS, acts, seed=DRR.STEP_SEED)
    assert_north_star_rtol(res)
    _assert_props_matter(lib, spec, sp, tp, h0, acts, hand=False)


@pytest.mark.parametrize("name", DRR.HAND_FUSED)
def test_dr_fused_hand_step_matches_oracle(lib, name):
    """mg_env_step of the ShadowHand with env_props bound (k_hand_step<DR>: block, egg, pen, block under TGS; masses,
    drives, effort limits, tendons, friction, object mass / friction / scale randomized) against orc_hand_env_step
    applying the same rows: the rule and the numbers of test_hand_fused_env_step_matches_oracle, 4 steps"""
    from test_gpu_hand import _hand_teacher_forced
    spec, sp, tp, h, acts = DRR.fused_case(name)
    h0 = copy.deepcopy(h)
    _hand_teacher_forced(lib, f"test_dr_fused_hand_step_matches_oracle[{name}]", spec, sp, tp, h, DRR.FUSED_STEPS, acts,
                         DRR.STEP_SEED)
    _assert_props_matter(lib, spec, sp, tp, h0, acts, hand=True)


# -------------------------------------------------------------------------- k_simulate<DR> on its other capacities
def _gpu_simulate_dr(lib, spec, sp, pre, props="rows"):
    """(result, team lanes, compact) of one mg_sim_simulate of the host `pre` on the device; props: "rows" binds
    pre.env_props, "defaults" rows of mg_env_props_defaults (the DR instance on the model's own values), None nothing
    (the plain instance)"""
    import types
    mnp = M.pack_model(spec)
    d = {k: torch.from_numpy(np.array(getattr(pre, k))).to(DEV) for k in ("root", "dof", "act_eff", "sensors", "dof_force")}
    v = _abi.StateViews()
    v.root_states, v.dof_state, v.dof_actuation = d["root"].data_ptr(), d["dof"].data_ptr(), d["act_eff"].data_ptr()
    v.sensors, v.dof_force = d["sensors"].data_ptr(), d["dof_force"].data_ptr()
    if props == "rows":
        tp_ = torch.from_numpy(np.array(pre.env_props)).to(DEV)
    elif props == "defaults":
        tp_ = _default_rows(lib, mnp, pre.n)
    if props is not None:
        v.env_props, v.env_props_stride = tp_.data_ptr(), tp_.shape[1]
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), pre.n, 0, C.byref(sim)), lib)
    try:
        t, lay = C.c_int32(), C.c_int32()
        _abi.check(lib.mg_sim_kernel_layout(sim, C.byref(t), C.byref(lay)), lib)
        _abi.check(lib.mg_sim_bind(sim, C.byref(v)), lib)
        _abi.check(lib.mg_sim_simulate(sim, torch.cuda.current_stream().cuda_stream), lib)
        torch.cuda.synchronize()
    finally:
        lib.mg_sim_destroy(sim)
    got = types.SimpleNamespace(**{k: x.cpu().numpy() for k, x in d.items()})
    for x in vars(got).values():
        assert np.isfinite(x).all()
    return got, t.value, lay.value


def _default_rows(lib, mnp, n):
    offs = (C.c_int32 * 4)()
    stride = lib.mg_env_props_layout(mnp.ctypes.data, offs)
    row = np.zeros(stride, np.float32)
    _abi.check(lib.mg_env_props_defaults(mnp.ctypes.data, row.ctypes.data), lib)
    return torch.from_numpy(row).to(DEV).repeat(n, 1).contiguous()


SIM_LANES = {"Cartpole": 8, "Humanoid-pgs": 32, "Humanoid-tgs": 32}


@pytest.mark.parametrize("name,layout", [("Cartpole", "classic"), ("Humanoid-pgs", "classic"), ("Humanoid-pgs", "compact"),
                                         ("Humanoid-tgs", "classic"), ("Humanoid-tgs", "compact")]
                         + [(k, "classic") for k in DRR.TREE_SIM + ("T16-fixed-tgs",)])
def test_dr_physics_matches_oracle_other_capacities(lib, name, layout, monkeypatch):
    """k_simulate<DR> where test_dr_physics_matches_oracle_ant / _hand do not take it: Cartpole's 8-lane instance, the
    Humanoid's (32, 24, 32, 24, 160) in both layouts and under TGS, and the three tree capacities (self pairs: the
    friction of a pair averages two randomized shape frictions; more geoms than team lanes: a second round of the
    lane-per-geom loops reads the rows' geom frictions) -- one mg_sim_simulate from identical states against
    orc_simulate_views with the same rows, by _dr_explained with the bars of the Ant and hand tests; sensors and DOF
    forces (which read the randomized damping, stiffness and frictionloss) by tests/tree_physics_ref.py's rule"""
    monkeypatch.setenv("MIGYM_LAYOUT", layout)
    spec, sp, pre, ref = DRR.sim_case(name)
    got, lanes, compact = _gpu_simulate_dr(lib, spec, sp, pre)
    want = SIM_LANES[name] if name in SIM_LANES else int(name[1:3])
    assert (lanes, compact) == (want, int(layout == "compact")), (lanes, compact)
    _dr_explained(f"test_dr_physics_matches_oracle_other_capacities[{name}-{layout}]", M.pack_model(spec), sp, pre,
                  DRR.sim_checks(spec, got, ref), hand=False)
    # the properties matter: the same states without them end elsewhere
    plain, _, _ = _gpu_simulate_dr(lib, spec, sp, pre, props=None)
    assert agreement(plain.dof[..., 1], ref.dof[..., 1], 2e-3, 2e-3) < 0.5


# -------------------------------------------------------------------------- rows of defaults change nothing
@pytest.mark.parametrize("name", ["Ant", "Humanoid", "hand-block"])
def test_default_rows_equal_the_plain_instance(lib, name):
    """env_props bound to rows of mg_env_props_defaults: the DR instance runs on the model's own values -- the inertia
    scale is mass / mass = 1 (an IEEE division), the averaged friction 0.5 (1 + 1), every node property a copy -- from
    the same state as the plain instance, independent of the oracle.  The two are separate instantiations of code
    compiled with FMA contraction on (team_physics.hpp: fp contract(fast)): what the plain one folds at compile time
    (the scale 1.0f, a null row pointer) the DR one multiplies at run time, so the compiler fuses the sums around
    them differently, and the results are NOT bit-identical.  Measured on the MI355X: at most 4.5e-8 in
    a pose, 4.4e-6 in a twist, 8.9e-7 / 1.1e-4 in a DOF position / velocity, 3.7e-4 in a DOF force and 5.3e-3 in a
    sensor (the Humanoid's, of forces ~1e3); a scratch build with contraction off gave the plain instance's bits in
    every quantity of all three cases, so contraction is the whole difference.  So every env of the pair is held to
    the one-step bars of the oracle tests (positions 2e-4, velocities 2e-3 + 2e-3 |v|, DOF forces and sensors 1 % of
    the batch's largest; the hand's rigid bodies 2e-3 + 2e-3 |x|), with no exemption."""
    spec, sp, tp, h, acts = DRR.fused_case(name)
    mnp = M.pack_model(spec)
    if name == "hand-block":
        from test_gpu_hand import DevHandEnv
        h.pre_physics(mnp, tp, seed=DRR.STEP_SEED, step=0)   # PD targets for the drives
        h.env_props = None                                   # (DevHandEnv would bind the case's random rows)
        outs = []
        for rows in (False, True):
            e = DevHandEnv(h)
            v = e.views()
            if rows:
                tp_ = _default_rows(lib, mnp, h.n)
                v.env_props, v.env_props_stride = tp_.data_ptr(), tp_.shape[1]
            sim = C.c_void_p()
            _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), h.n, 0, C.byref(sim)), lib)
            try:
                _abi.check(lib.mg_sim_bind(sim, C.byref(v)), lib)
                _abi.check(lib.mg_sim_simulate(sim, torch.cuda.current_stream().cuda_stream), lib)
                torch.cuda.synchronize()
            finally:
                lib.mg_sim_destroy(sim)
            outs.append({k: getattr(e, k).cpu().numpy() for k in ("root", "dof", "sensors", "dof_force", "rbs")})
    else:
        h.act_eff[:] = np.random.default_rng(3).uniform(-1, 1, h.act_eff.shape) * (15.0 if name == "Ant" else 50.0)
        outs = [vars(_gpu_simulate_dr(lib, spec, sp, h, props=p)[0]) for p in (None, "defaults")]
    moved = np.abs(outs[0]["dof"][..., 0] - h.dof[..., 0]).max()
    assert moved > 1e-3, "the step moved nothing"
    plain, dr = outs
    n = h.n
    root_p, root_d = (o["root"].reshape(n, -1, 13)[:, -2 if name == "hand-block" else 0] for o in (plain, dr))
    checks = [("root pose", root_d[:, 0:7], root_p[:, 0:7], 2e-4, 0), ("root twist", root_d[:, 7:13], root_p[:, 7:13], 2e-3, 2e-3),
              ("dof pos", dr["dof"][..., 0], plain["dof"][..., 0], 2e-4, 0),
              ("dof vel", dr["dof"][..., 1], plain["dof"][..., 1], 2e-3, 2e-3),
              ("dof force", dr["dof_force"], plain["dof_force"], 1e-2 * max(1.0, np.abs(plain["dof_force"]).max()), 0),
              ("sensors", dr["sensors"], plain["sensors"], 1e-2 * max(1.0, np.abs(plain["sensors"]).max()), 0)]
    if name == "hand-block":
        checks.append(("rigid bodies", dr["rbs"], plain["rbs"], 2e-3, 2e-3))
    test = f"test_default_rows_equal_the_plain_instance[{name}]"
    outside = {}
    for k, a, b, atol, rtol in checks:
        st = PS.record(test, k, a, b, atol=atol, rtol=rtol, differing=int((a != b).sum()))
        print(f"{test} {k}: max |DR(defaults) - plain| = {st['max']:.3e}, {int((a != b).sum())} of {a.size} elements differ")
        if PS.env_bad(a, b, atol, rtol).any():
            outside[k] = st["max"]
    assert not outside, f"{name}: the DR instance on default rows leaves the one-step bars of the plain instance: {outside}"


@pytest.mark.parametrize("task,n", [("Ant", 4096), ("Humanoid", 2048), ("ShadowHand", 1024)])
def test_make_with_randomize(task, n):
    """the shipped randomization_params of each task YAML through make() and the fused step"""
    import migym
    cfg = configs.task_config(task, n, sim_device=DEV)
    cfg["task"]["randomize"] = True
    env = migym.make(seed=3, task=task, num_envs=n, sim_device=DEV, rl_device=DEV, headless=True, cfg={"task": cfg})
    assert env.randomize and env.env_props.shape[0] == env.num_actors
    spec = env.model_spec
    props = env.env_props.cpu().numpy()
    base = defaults(spec)
    W = _abi.MG_EP_NODE_WIDTH
    mass = np.stack([props[:, W * b.node] for b in spec.bodies], 1)
    m0 = np.array([base[W * b.node] for b in spec.bodies])
    r = mass / np.where(m0 > 0, m0, 1)
    assert r[:, m0 > 0].min() >= 0.5 - 1e-6 and r[:, m0 > 0].max() <= 1.5 + 1e-6
    if task == "Humanoid":   # mass is setup_only with a linear schedule: scale 0 at setup, never randomized
        assert np.all(r[:, m0 > 0] == 1.0)
    else:
        assert np.std(r[:, m0 > 0]) > 0.1        # per-env draws differ
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(20):
        obs, rew, reset, extras = env.step(torch.rand((env.num_actors, env.num_actions), device=DEV, generator=g) * 2 - 1)
    torch.cuda.synchronize()
    assert torch.isfinite(obs["obs"]).all() and torch.isfinite(rew).all()
    assert "actions" in env.dr_randomizations and "observations" in env.dr_randomizations
    if task == "ShadowHand":   # gravity noise without a schedule (Humanoid's starts at scale 0)
        assert tuple(env.sim_params.gravity) != (0.0, 0.0, -9.81)
    env.close()


class _Gen:
    """actor_params_generator stand-in: a known vector per call (vec_task.py:736-760)"""

    def __init__(self, n):
        self.n, self.calls = n, 0

    def sample(self):
        self.calls += 1
        return 1.0 + 0.01 * np.arange(self.n) + 0.1 * self.calls


def test_actor_params_generator_ant():
    """get_actor_params_info + actor_params_generator: the randomized envs take og * sample (scaling) /
    og + sample (additive) from the generator's vector, setup_only entries (mass) are ignored, the other
    envs keep their rows, and a vector of the wrong length raises."""
    import migym
    n = 64
    cfg = configs.task_config("Ant", n, sim_device=DEV)
    cfg["task"]["randomize"] = True
    env = migym.make(seed=3, task="Ant", num_envs=n, sim_device=DEV, rl_device=DEV, headless=True, cfg={"task": cfg})
    dr = env.randomization_params
    params, names, lows, highs = env.get_actor_params_info(dr, 5)
    assert len(params) == len(names) == len(lows) == len(highs)
    nd = env.num_dof
    assert "dof_properties_0_damping_0" in names and f"dof_properties_0_damping_{nd - 1}" in names
    assert "rigid_body_properties_0_mass" in names
    i_lo = names.index("dof_properties_0_lower_0")
    assert lows[i_lo] == -np.inf and highs[i_lo] == np.inf          # gaussian: unbounded
    i_d = names.index("dof_properties_0_damping_3")
    assert (lows[i_d], highs[i_d]) == (0.5, 1.5)
    spec = env.model_spec
    base = defaults(spec)
    stride, offs = layout(spec)
    assert params[i_d] == pytest.approx(float(env.env_props[5, offs[0] + _abi.MG_EP_NODE_WIDTH * 4 + 2]), rel=0, abs=0)
    before = env.env_props.clone()
    gen = _Gen(len(names))
    env.actor_params_generator = gen
    ids = torch.tensor([2, 9, 40], device=DEV)
    mask = torch.zeros(n, dtype=torch.long, device=DEV)
    mask[ids] = 1
    env.randomize_buf_actors[:] = 10 ** 6
    env.apply_randomizations(dr, reset_mask=mask, increment=False)
    torch.cuda.synchronize()
    assert gen.calls == 3 and sorted(env.extern_actor_params) == [2, 9, 40]
    props = env.env_props.cpu().numpy()
    keep = np.ones(n, bool)
    keep[ids.cpu().numpy()] = False
    assert np.array_equal(props[keep], before.cpu().numpy()[keep])
    for e in (2, 9, 40):
        ext = env.extern_actor_params[e]
        for d in range(nd):
            col = offs[0] + _abi.MG_EP_NODE_WIDTH * (d + 1)
            j = names.index(f"dof_properties_0_damping_{d}")
            assert props[e, col + 2] == pytest.approx(base[col + 2] * ext[j], rel=1e-6, abs=1e-7)
            j = names.index(f"dof_properties_0_lower_{d}")
            assert props[e, col + 4] == pytest.approx(base[col + 4] + ext[j], rel=1e-6, abs=1e-6)
        # mass is setup_only: unchanged by the generator
        W = _abi.MG_EP_NODE_WIDTH
        assert np.array_equal(props[e, offs[0]::W][:len(spec.nodes)], before.cpu().numpy()[e, offs[0]::W][:len(spec.nodes)])
    env.actor_params_generator = _Gen(len(names) + 1)
    env.randomize_buf_actors[:] = 10 ** 6      # the call above restarted the randomized envs' counters
    with pytest.raises(Exception, match="extern_sample size"):
        env.apply_randomizations(dr, reset_mask=mask, increment=False)
    env.close()
