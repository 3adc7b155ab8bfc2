"""Sim parameters away from the tasks' YAML values: the points, and the task models' states, oracle steps and
comparison at them, shared by tests/test_simparams_host.py (the oracle's fp32 twin on the CPU) and
tests/test_gpu_simparams.py (the kernels).

Every other GPU-versus-oracle physics test runs at a task's own mg_sim_params (substeps 2, gravity along z or zero,
friction 1, 4 or 8 position iterations, baumgarte 0.2, ...), so the branches of csrc/team_physics.hpp that read these
fields see one value each.  POINTS moves one field (or one pair of fields that belong together) at a time.

A (model, point) pair is admitted on the CPU by the reference alone: on its states the oracle's fp32
twin leaves no env outside the one-step rule without a flag, the flags reach at most parity_stats.REACH_CAP, and the
fp64 oracle's own result at the point leaves the tolerances of its result at the task's parameters in at least a
quarter of the states (`moved`; 5 states on the trees at limit_margin 0, where only the joints between the limit and
the margin feel it).  Where a pair does not qualify at the first seed the next one is taken, twice at most; for an
iteration count the next lower count is allowed too.  TAKEN records what was taken, LEFT_OUT what never qualified.

The tree cases (tree_physics_ref: T16-free, T32-fixed, T64-free, dropped states) take a point through
tree_physics_ref.sim_params / states / compare(point=...).  The task models' states are random_states (the draw of
test_gpu_parity.test_physics_step_matches_oracle, its seed and heights) and, for the hand, test_gpu_hand's palm
states.
"""
import copy
import types

import numpy as np

import parity_stats as PS
import pyoracle as O
from migym import _abi, configs, model as M, taskdefs

# name -> the mg_sim_params fields it sets
POINTS = {
    "substeps1": dict(substeps=1),
    "substeps4": dict(substeps=4, dt=1.0 / 30.0),
    "gravity": dict(gravity=(3.0, -2.0, -8.0)),
    "friction0.2": dict(friction=0.2),
    "friction0": dict(friction=0.0),
    "depen0.3": dict(max_depen_vel=0.3),
    "rest5mm": dict(rest_offset=0.005, contact_offset=0.01),
    "iters1": dict(pos_iters=1),
    "iters16": dict(pos_iters=16),
    "margin0": dict(limit_margin=0.0),
    "baumgarte0.8": dict(baumgarte=0.8),
    "tgs2-6": dict(solver_type=_abi.MG_SOLVER_TGS, pos_iters=2, vel_iters=6),
}
TREE_CASES = ("T16-free", "T32-fixed", "T64-free")
SMALL_POINTS = ("substeps4", "tgs2-6")       # the trees also run these at tree_physics_ref.SMALL_N actors
# task -> (envs, root heights, the points it runs)
TASKS = {"Ant": (256, (0.25, 0.7), tuple(POINTS)), "Humanoid": (128, (0.6, 1.4), tuple(POINTS)),
         "Cartpole": (64, (2.0, 2.0), ("substeps1", "substeps4", "gravity"))}
SEED = 7                                      # test_physics_step_matches_oracle's
# the ShadowHand block on the palm (test_gpu_hand.test_hand_physics_step_matches_oracle's states, seed 5); tilted
# gravity reaches the free object's own gravity term
HAND, HAND_N, HAND_SEED = "ShadowHand", 256, 5
HAND_POINTS = ("substeps1", "substeps4", "gravity", "friction0.2", "rest5mm", "depen0.3")
# what the admission rule took where the first choice did not qualify: (model, point) -> dict(seed=k (the k-th next
# seed), over=fields replacing the point's); and the pairs that never qualified, with the twin's figure
TAKEN = {}
# the hand at max_depen_vel 0.3: its contacts are shallow (the clamp engages below 12.5 mm at the hand's h), so the
# oracle's result moves in 54, 61 and 54 of 256 states at seeds 5, 6 and 7, under the quarter (64) the rule asks for;
# the twin had 0 unflagged disagreements at each
LEFT_OUT = {(HAND, "depen0.3"): "moved 54 / 61 / 54 of 256 at seeds 5 / 6 / 7 (floor 64); twin: 0 unflagged"}


def pairs(models=None):
    """the admitted (model, point) pairs, trees first"""
    out = [(m, p) for m in TREE_CASES for p in POINTS]
    out += [(t, p) for t, (_, _, pts) in TASKS.items() for p in pts]
    out += [(HAND, p) for p in HAND_POINTS]
    return [mp for mp in out if mp not in LEFT_OUT and (models is None or mp[0] in models)]


def fields(point, model=None):
    f = dict(POINTS[point])
    f.update(TAKEN.get((model, point), {}).get("over", {}))
    return f


def seed_shift(point, model=None):
    return TAKEN.get((model, point), {}).get("seed", 0)


def apply(sp, point, model=None):
    """a copy of sp moved to the point (None: sp itself, untouched)"""
    if point is None:
        return sp
    sp = copy.copy(sp)
    for k, v in fields(point, model).items():
        if k == "gravity":
            for i in range(3):
                sp.gravity[i] = v[i]
        else:
            setattr(sp, k, v)
    return sp


def moved(at_point, at_task, checks):
    """per env: the result `at_point` leaves the one-step tolerances of `at_task` (both the fp64 oracle's, from the
    same states); checks(got, ref, n) -> [(name, got, ref, atol, rtol)]"""
    n = len(at_point.root)
    out = np.zeros(n, bool)
    for _, a, b, atol, rtol in checks(at_point, at_task, n):
        out |= PS.env_bad(a, b, atol, rtol)
    return out


def moved_floor(model, point, n):
    if point == "margin0" and model in TREE_CASES:
        return 5
    return (n + 3) // 4


# ------------------------------------------------------------------------------------------------ the task models
def random_states(spec, tp, n, rng, z_range, contact_frac=0.5):
    nd = spec.num_dofs
    root = np.zeros((n, 13), np.float32)
    root[:, 0:2] = rng.uniform(-2, 2, (n, 2))
    root[:, 2] = rng.uniform(*z_range, n)
    yaw = rng.uniform(-np.pi, np.pi, n)
    tilt = rng.normal(0, 0.3, (n, 2))
    q = np.stack([tilt[:, 0] * 0.5, tilt[:, 1] * 0.5, np.sin(yaw / 2), np.cos(yaw / 2)], -1)
    root[:, 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    root[:, 7:13] = rng.normal(0, 0.5, (n, 6))
    lo, hi = np.array(tp.dof_lower[:nd]), np.array(tp.dof_upper[:nd])
    dof = np.zeros((n, nd, 2), np.float32)
    dof[:, :, 0] = lo + (hi - lo) * rng.uniform(-0.05, 1.05, (n, nd))
    dof[:, :, 1] = rng.normal(0, 1.0, (n, nd))
    return root, dof


_cache = {}


def task_setup(task):
    """(spec, packed model, sim params at the task's values, task params)"""
    if ("setup", task) not in _cache:
        cfg = configs.task_config(task, 16)
        spec = M.load_builtin(taskdefs.TASK_INFO[task][1])
        sp = taskdefs.sim_params(cfg, taskdefs.TASK_INFO[task][5])
        _cache["setup", task] = spec, M.pack_model(spec), sp, taskdefs.task_params(task, cfg, spec)
    return _cache["setup", task]


def task_sim_params(task, point):
    return apply(task_setup(task)[2], point, task)


def task_host(task, root, dof, act):
    """a HostEnv holding a physics input, with every output gym.simulate writes bound"""
    spec, _, _, tp = task_setup(task)
    h = O.HostEnv(tp, spec, len(root))
    h.root[:], h.dof[:], h.act_eff[:] = root, dof, act
    h.ncf = np.zeros((len(root), len(spec.bodies), 3), np.float32)
    return h


def task_states(task, point):
    """(root, dof, act, ref, base): the task's states before the step (read-only; test_physics_step_matches_oracle's
    draw at seed SEED + the seed the admission rule took), the fp64 oracle's HostEnv after one simulate at the point,
    and the same at the task's own parameters; computed once"""
    key = ("states", task, point)
    if key in _cache:
        return _cache[key]
    spec, mnp, sp, tp = task_setup(task)
    n, z, _ = TASKS[task]
    rng = np.random.default_rng(SEED + seed_shift(point, task))
    root, dof = random_states(spec, tp, n, rng, z)
    if task == "Cartpole":
        root[:, :] = 0
        root[:, 2] = 2.0
        root[:, 6] = 1.0
    act = (rng.uniform(-1, 1, (n, spec.num_dofs)) * (15.0 if task == "Ant" else 50.0)).astype(np.float32)
    for x in (root, dof, act):
        x.setflags(write=False)
    ref, base = task_host(task, root, dof, act), task_host(task, root, dof, act)
    ref.simulate(mnp, task_sim_params(task, point), threads=8)
    base.simulate(mnp, sp, threads=8)
    _cache[key] = root, dof, act, ref, base
    return _cache[key]


def task_twin(task, point):
    root, dof, act, _, _ = task_states(task, point)
    h = task_host(task, root, dof, act)
    h.simulate(task_setup(task)[1], task_sim_params(task, point), threads=8, fp32=True)
    return h


def task_outside(got, ref, n):
    """the one-step tolerances (tree_physics_ref.outside) on HostEnv-like results"""
    f_h, s_h, c_h = ref.dof_force[:n], ref.sensors[:n], ref.ncf[:n]
    return [("root pose", got.root[:, 0:7], ref.root[:n, 0:7], 2e-4, 0),
            ("dof pos", got.dof[..., 0], ref.dof[:n, :, 0], 2e-4, 0),
            ("root twist", got.root[:, 7:13], ref.root[:n, 7:13], 2e-3, 2e-3),
            ("dof vel", got.dof[..., 1], ref.dof[:n, :, 1], 2e-3, 2e-3),
            ("dof force", got.dof_force, f_h, 1e-2 * max(1.0, np.abs(f_h).max()), 0),
            ("sensors", got.sensors, s_h, 1e-2 * max(1.0, np.abs(s_h).max()), 0),
            ("net contact forces", got.ncf, c_h, 1e-2 * max(1.0, np.abs(c_h).max()), 0)]


def task_compare(test, task, point, got):
    """`got`: a HostEnv-like result (root, dof, sensors, dof_force, ncf) of one simulate of the task's states at the
    point by the implementation under test, held to the fp64 oracle by the one-step rule (tree_physics_ref.compare).
    Returns the exemption record."""
    _, mnp, _, _ = task_setup(task)
    root, dof, act, ref, _ = task_states(task, point)
    n = len(root)
    for x in (got.root, got.dof, got.sensors, got.dof_force, got.ncf):
        assert np.isfinite(x).all()
    assert np.abs(got.dof[..., 0] - dof[..., 0]).max() > 1e-3, "the step moved nothing"
    bad = np.zeros(n, bool)
    for name, a, b, atol, rtol in task_outside(got, ref, n):
        eb = PS.env_bad(a, b, atol, rtol)
        PS.record(test, name, a, b, envs_outside=int(eb.sum()), atol=atol, rtol=rtol)
        bad |= eb
    flags = PS.step_flags(mnp, task_sim_params(task, point), task_host(task, root, dof, act))
    return PS.assert_steps_explained(test, bad[None], flags[None], sens=None, reach_cap=PS.REACH_CAP,
                                     allow_unexplained=0.0)


def task_candidates(task, point):
    """(before, after): per env, the fp64 oracle's count of contact candidates at the point, before and after the step"""
    _, mnp, _, _ = task_setup(task)
    sp = task_sim_params(task, point)
    root, dof, _, ref, _ = task_states(task, point)
    cnt = lambda r, d: np.array([len(O.contacts(mnp, sp, r[a], d[a], 64)) for a in range(len(r))])
    return cnt(root, dof), cnt(ref.root, ref.dof)


# ------------------------------------------------------------------------------------------------ the hand
def hand_setup():
    """(spec, packed model, sim params at the task's values, task params) of the ShadowHand block"""
    if "hand" not in _cache:
        cfg = configs.task_config("ShadowHand", 16)
        cfg["env"]["objectType"] = "block"
        spec = taskdefs.hand_spec("block")
        _cache["hand"] = (spec, M.pack_model(spec), taskdefs.sim_params(cfg, taskdefs.TASK_INFO[HAND][5]),
                          taskdefs.task_params("ShadowHand", cfg, spec))
    return _cache["hand"]


def hand_sim_params(point):
    return apply(hand_setup()[2], point, HAND)


def hand_states(point):
    """(h0, ref, base): the physics input (a HandHostEnv: the palm states with object forces on half of the envs and
    the net contact force tensor bound, as test_gpu_hand._physics_vs_oracle makes it; do not write to it), the fp64
    oracle's result at the point and at the task's own parameters"""
    key = ("hand states", point)
    if key not in _cache:
        import test_gpu_hand as H
        spec, mnp, sp, tp = hand_setup()
        rng = np.random.default_rng(HAND_SEED + seed_shift(point, HAND))
        h0 = H.hand_states(spec, tp, HAND_N, rng, H.PALM_DZ["block"])
        h0.rb_forces[: HAND_N // 2, len(spec.bodies)] = rng.normal(0, 0.3, (HAND_N // 2, 3))
        h0.ncf = np.zeros((HAND_N, len(spec.bodies) + 2, 3), np.float32)
        ref, base = copy.deepcopy(h0), copy.deepcopy(h0)
        ref.simulate(mnp, hand_sim_params(point), threads=8)
        base.simulate(mnp, sp, threads=8)
        _cache[key] = h0, ref, base
    return _cache[key]


def hand_twin(point):
    h = copy.deepcopy(hand_states(point)[0])
    h.simulate(hand_setup()[1], hand_sim_params(point), threads=8, fp32=True)
    return h


def hand_outside(got, ref, n):
    """the hand's one-step tolerances (test_gpu_hand._physics_vs_oracle)"""
    return [("net contact forces", got.ncf, ref.ncf[:n], 1e-2 * max(1.0, np.abs(ref.ncf[:n]).max()), 0),
            ("object pose", got.root[:, 1, 0:7], ref.root[:n, 1, 0:7], 2e-4, 0),
            ("object twist", got.root[:, 1, 7:13], ref.root[:n, 1, 7:13], 2e-3, 2e-3),
            ("dof pos", got.dof[..., 0], ref.dof[:n, :, 0], 2e-4, 0),
            ("dof vel", got.dof[..., 1], ref.dof[:n, :, 1], 2e-3, 2e-3),
            ("dof force", got.dof_force, ref.dof_force[:n], 1e-2, 1e-2),
            ("rigid bodies", got.rbs, ref.rbs[:n], 2e-3, 2e-3),
            ("sensors", got.sensors, ref.sensors[:n], 1e-2 * max(1.0, np.abs(ref.sensors[:n]).max()), 0)]


def hand_compare(test, point, got):
    """as task_compare, for a HandHostEnv-like result (root, dof, sensors, dof_force, rbs, ncf)"""
    h0, ref, _ = hand_states(point)
    n = h0.n
    for x in (got.root, got.dof, got.sensors, got.dof_force, got.rbs, got.ncf):
        assert np.isfinite(x).all()
    assert np.abs(got.dof[..., 0] - h0.dof[..., 0]).max() > 1e-3, "the step moved nothing"
    np.testing.assert_array_equal(got.root[:, 0], ref.root[:, 0])       # fixed hand root untouched
    np.testing.assert_array_equal(got.root[:, 2], ref.root[:, 2])       # goal actor untouched
    bad = np.zeros(n, bool)
    for name, a, b, atol, rtol in hand_outside(got, ref, n):
        eb = PS.env_bad(a, b, atol, rtol)
        PS.record(test, name, a, b, envs_outside=int(eb.sum()), atol=atol, rtol=rtol)
        bad |= eb
    flags = PS.step_flags(hand_setup()[1], hand_sim_params(point), h0)
    return PS.assert_steps_explained(test, bad[None], flags[None], sens=None, reach_cap=PS.REACH_CAP,
                                     allow_unexplained=0.0)


def hand_candidates(point):
    _, mnp, _, _ = hand_setup()
    sp = hand_sim_params(point)
    h0, ref, _ = hand_states(point)
    cnt = lambda h: np.array([len(O.contacts(mnp, sp, h.root[a].ravel(), h.dof[a], 64)) for a in range(h.n)])
    return cnt(h0), cnt(ref)


# ------------------------------------------------------------------------------------------------ the fused step
# mg_env_step at substeps 1, and at substeps 4 with controlFrequencyInv 2: nsub = 1 and 8 in csrc/step_kernels.hpp
FUSED = {"substeps1": dict(substeps=1, dt=None, cfi=1), "substeps4x2": dict(substeps=4, dt=1.0 / 30.0, cfi=2)}
FUSED_STEPS, FUSED_RNG_SEED = 2, 5
FUSED_CASES = (("Ant", 256), ("Humanoid", 128), (HAND, 128))
# What the admission rule took (conditions on the inputs, asserted in tests/test_simparams_host.py: flags within
# REACH_CAP and the fp32 twin without an unflagged disagreement).  The hand at 16 substeps over the two steps never
# qualifies: from the palm states the flags reach 5.5 % of the env-steps at seed 5 and 7.4 % at seed 7, and at seed 6
# (4.7 %) the twin itself leaves the tolerances in one unflagged env-step (an observation 0.69 off); from the reset
# pose of test_hand_fused_env_step_matches_oracle they reach 5.1 %.  So the hand takes the next lower count,
# controlFrequencyInv 1: nsub = 4.
FUSED_TAKEN = {(HAND, "substeps4x2"): dict(cfi=1)}


def fused_setup(task, point):
    """(spec, sim params, task params) with the task's config moved through the YAML fields themselves (sim.substeps,
    sim.dt, env.controlFrequencyInv), so that the task's own dt follows"""
    f = dict(FUSED[point], **FUSED_TAKEN.get((task, point), {}))
    cfg = configs.task_config(task, 16)
    cfg["sim"]["substeps"] = f["substeps"]
    if f["dt"] is not None:
        cfg["sim"]["dt"] = f["dt"]
    cfg["env"]["controlFrequencyInv"] = f["cfi"]
    if task == HAND:
        cfg["env"]["objectType"] = "block"
        spec = taskdefs.hand_spec("block")
    else:
        spec = M.load_builtin(taskdefs.TASK_INFO[task][1])
    sp = taskdefs.sim_params(cfg, taskdefs.TASK_INFO[task][5])
    tp = taskdefs.task_params(task, cfg, spec)
    assert (sp.substeps, tp.control_freq_inv) == (f["substeps"], f["cfi"])
    return spec, sp, tp


def fused_input(task, n, point):
    """(host env, actions per step): the one-step tests' states (random_states half in contact; the hand's palm states),
    no reset pending, and FUSED_STEPS random actions"""
    spec, sp, tp = fused_setup(task, point)
    shift = FUSED_TAKEN.get((task, point), {}).get("seed", 0)
    if task == HAND:
        import test_gpu_hand as H
        rng = np.random.default_rng(HAND_SEED + shift)
        h = H.hand_states(spec, tp, n, rng, H.PALM_DZ["block"])
        h.prev_targets[:] = h.targets
        h.reset_goal[:] = 0
    else:
        rng = np.random.default_rng(SEED + shift)
        h = O.HostEnv(tp, spec, n)
        h.root[:], h.dof[:] = random_states(spec, tp, n, rng, TASKS[task][1])
    h.reset[:] = 0
    return h, [rng.uniform(-1.2, 1.2, (n, tp.num_actions)).astype(np.float32) for _ in range(FUSED_STEPS)]


def fused_flags(task, n, point):
    """(flags, twin_bad), each (FUSED_STEPS, n): orc_step_flips of each teacher-forced step's physics input, by the
    fp64 oracle alone; and where the oracle's fp32 twin, stepped from the same state, leaves the fused tests'
    tolerances (obs 2e-3 + 2e-3 |x|, reward 5e-3 + 5e-3 |r|, the same resets)"""
    spec, sp, tp = fused_setup(task, point)
    mnp = M.pack_model(spec)
    h, acts = fused_input(task, n, point)
    flags, bad = [], []
    for t in range(FUSED_STEPS):
        h.actions[:] = acts[t]
        pre = (PS.hand_physics_input(h, mnp, tp, FUSED_RNG_SEED, t) if task == HAND else
               PS.loco_physics_input(h, mnp, sp, tp, FUSED_RNG_SEED, t, threads=8))
        flags.append(PS.step_flags(mnp, sp, pre))
        g = copy.deepcopy(h)
        h.env_step(mnp, sp, tp, seed=FUSED_RNG_SEED, step=t, threads=8)
        g.env_step(mnp, sp, tp, seed=FUSED_RNG_SEED, step=t, threads=8, fp32=True)
        bad.append(PS.env_bad(g.obs, h.obs, 2e-3, 2e-3) | PS.env_bad(g.rew[:, None], h.rew[:, None], 5e-3, 5e-3)
                   | (g.reset != h.reset))
    # the hand resets in pre_physics, which would replace the palm states (a locomotion env that falls resets after
    # its step's physics, and starts the next step in the air)
    assert task != HAND or not h.reset.any()
    return np.array(flags), np.array(bad)


def result(**arrays):
    return types.SimpleNamespace(**arrays)
