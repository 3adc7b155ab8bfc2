"""numpy restatement of Anymal's pre_physics_step, post_physics_step and the VecTask.step tail (anymal.py:226-304,
311-386; vec_task.py step tail), in float32 and the reference's operation order, with the helpers the Anymal tests
share: the reference trace, the task config it was generated for, the dispatcher's choice of kernel instance, and
host views of the task model for the fp64 oracle.

Test infrastructure: tests/test_anymal_host.py holds the restatement to the reference's own output
(tests/golden/trace_anymal.npz); the GPU tests use it where no recorded trace exists (the device RNG).

State (a dict of arrays, updated in place by ``post_step``):
  progress, reset (N) int64; root (N, 13), dof (N, 12, 2), commands (N, 3) float32.
Per-step inputs: torques (N, 12) and ncf (N, nB, 3) as simulate left them, actions (N, 12) (clamped inside), noise
(N, 27) U(0,1) rows [positions_offset 12 | velocities 12 | command x | y | yaw].
"""
import functools
import os

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "trace_anymal.npz")
ANYMAL_JSON = os.path.join(HERE, "golden", "anymal_c.json")
STATE_KEYS = ("root", "dof", "commands")


def params_from(ap):
    """the constants the restatement reads, from a ctypes mg_anymal_params (taskdefs.anymal_params)"""
    return dict(lin=F(ap.lin_vel_scale), ang=F(ap.ang_vel_scale), dof_pos=F(ap.dof_pos_scale),
                dof_vel=F(ap.dof_vel_scale), action_scale=F(ap.action_scale),
                rew=np.array([ap.rew_lin_vel_xy, ap.rew_ang_vel_z, ap.rew_torque], F),
                default=np.array(list(ap.default_dof_pos), F), base_init=np.array(list(ap.base_init_state), F),
                cmd_lo=np.array(list(ap.command_lo), F), cmd_span=np.array(list(ap.command_span), F),
                base=int(ap.base_body), knees=list(ap.knee_body), clip_actions=F(ap.clip_actions),
                clip_obs=F(ap.clip_obs), max_episode_length=int(ap.max_episode_length))


def pre_step(p, actions):
    """(actions_out, targets): the clamp of VecTask.step, then targets = action_scale * a + default (two roundings)"""
    a = np.clip(actions.astype(F), -p["clip_actions"], p["clip_actions"])
    return a, ((p["action_scale"] * a).astype(F) + p["default"][None]).astype(F)


def reset_envs(p, st, env_ids, noise):
    """reset_idx (anymal.py:283-303) but for its reset_buf[env_ids] = 1, which compute_reward overwrites"""
    for e in env_ids:
        u = noise[e].astype(F)
        st["dof"][e, :, 0] = p["default"] * (F(1.5 - 0.5) * u[0:12] + F(0.5))
        st["dof"][e, :, 1] = F(0.1 - -0.1) * u[12:24] + F(-0.1)
        st["root"][e] = p["base_init"]
        st["commands"][e] = p["cmd_span"] * u[24:27] + p["cmd_lo"]
        st["progress"][e] = 0


def quat_rotate(q, v, inverse):
    qw, qv = q[:, 3:4], q[:, :3]
    a = v * (F(2.0) * qw * qw - F(1.0))
    b = np.cross(qv, v).astype(F) * qw * F(2.0)
    c = qv * (qv * v).sum(-1, dtype=F, keepdims=True) * F(2.0)
    return ((a - b if inverse else a + b) + c).astype(F)


def observe(p, st, act):
    root, N = st["root"], len(st["root"])
    q = root[:, 3:7]
    lin = quat_rotate(q, root[:, 7:10], True)
    ang = quat_rotate(q, root[:, 10:13], True)
    grav = quat_rotate(q, np.tile(np.array([0, 0, -1], F), (N, 1)), False)
    scale = np.array([p["lin"], p["lin"], p["ang"]], F)
    obs = np.concatenate([lin * p["lin"], ang * p["ang"], grav, st["commands"] * scale,
                          (st["dof"][..., 0] - p["default"]) * p["dof_pos"], st["dof"][..., 1] * p["dof_vel"], act],
                         -1).astype(F)
    return obs, lin, ang


def reward(p, st, lin, ang, torques, ncf):
    cmd = st["commands"]
    d = cmd[:, :2] - lin[:, :2]
    lin_err = (d * d).sum(-1, dtype=F)
    ang_err = np.square(cmd[:, 2] - ang[:, 2])
    r = np.exp(-lin_err / F(0.25)).astype(F) * p["rew"][0] + np.exp(-ang_err / F(0.25)).astype(F) * p["rew"][1]
    r = r + (torques * torques).sum(-1, dtype=F) * p["rew"][2]
    r = np.maximum(r, F(0.0)).astype(F)
    norm = lambda x: np.sqrt((x * x).sum(-1, dtype=F))   # noqa: E731
    rst = norm(ncf[:, p["base"]]) > 1.0
    rst |= (norm(ncf[:, p["knees"]]) > 1.0).any(-1)
    rst |= st["progress"] >= p["max_episode_length"] - 1
    return r, rst.astype(np.int64)


def post_step(p, st, torques, ncf, actions, noise):
    """returns dict(obs, obs_clamped, rew, timeout); st holds reset / progress and the task state"""
    act = np.clip(actions.astype(F), -p["clip_actions"], p["clip_actions"])
    st["progress"] += 1
    done = np.nonzero(st["reset"])[0]
    reset_envs(p, st, done, noise)
    obs, lin, ang = observe(p, st, act)
    rew, st["reset"][:] = reward(p, st, lin, ang, torques.astype(F), ncf.astype(F))
    timeout = (st["progress"] >= p["max_episode_length"] - 1) & (st["reset"] != 0)
    return dict(obs=obs, obs_clamped=np.clip(obs, -p["clip_obs"], p["clip_obs"]), rew=rew, timeout=timeout)


def close(x, ref):
    """the project's 1e-4 rule: |x - ref| <= 1e-4 max(1, |ref|)"""
    return np.abs(x.astype(np.float64) - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref))


# ---- the reference trace (tests/golden/trace_anymal.npz, written by tests/golden/make_anymal_golden.py)
@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(GOLDEN))
    for v in g.values():
        v.setflags(write=False)
    return g


def golden_cfg(N, **env):
    """the task config the trace was generated for (env overrides on top)"""
    from migym import configs
    over = {"env.learn.episodeLength_s": float(golden()["episode_length_s"]),
            "env.asset": {"modelTable": ANYMAL_JSON}}
    over.update({"env." + k: v for k, v in env.items()})
    return configs.task_config("Anymal", N, overrides=over)


def task_cfg(N, **env):
    """the built-in Anymal config on the fixture table"""
    from migym import configs
    over = {"env.asset": {"modelTable": ANYMAL_JSON}}
    over.update({"env." + k: v for k, v in env.items()})
    return configs.task_config("Anymal", N, overrides=over)


def golden_state0(g, N):
    return dict(root=np.zeros((N, 13), F), dof=np.zeros((N, 12, 2), F), commands=g[f"N{N}_commands_0"].copy(),
                progress=np.zeros(N, np.int64), reset=np.zeros(N, np.int64))


# ---- the dispatcher's choice (csrc/dispatch.hpp: mgi::team_size), asked of the library itself; no device needed
def dispatch_team_size(spec, max_contacts):
    """lanes of the first kernel instance that fits ``spec`` (0: none): mg_model_team_lanes"""
    import ctypes as C
    from migym import _abi, model as M
    mnp, lanes = M.pack_model(spec), C.c_int32(-1)
    lib = _abi.lib()
    _abi.check(lib.mg_model_team_lanes(mnp.ctypes.data, int(max_contacts), C.byref(lanes)), lib)
    return lanes.value


# ---- the task model under the fp64 oracle
class AnymalHost:
    """host views of the task's robots for orc_simulate_views / orc_step_flips: PD targets, DOF forces and the net
    contact force tensor bound, as the task binds them"""

    def __init__(self, spec, root, dof, tgt):
        import pyoracle as O
        self.O = O
        self.n = len(root)
        self.root, self.dof, self.tgt = (np.array(x, F) for x in (root, dof, tgt))
        self.act_eff = np.zeros((self.n, spec.num_dofs), F)
        self.dof_force = np.zeros((self.n, spec.num_dofs), F)
        self.ncf = np.zeros((self.n, len(spec.bodies), 3), F)

    def views(self):
        from migym import _abi
        O, v = self.O, _abi.StateViews()
        v.root_states, v.dof_state, v.dof_actuation = O.p(self.root), O.p(self.dof), O.p(self.act_eff)
        v.dof_targets, v.dof_force, v.net_contact_forces = O.p(self.tgt), O.p(self.dof_force), O.p(self.ncf)
        return v

    def simulate(self, mnp, sp):
        v = self.views()
        self.O.lib().orc_simulate_views(mnp.ctypes.data, self.O.C.byref(sp), self.n, self.O.C.byref(v), 8)
        return self


def task_model(cfg):
    """(spec, packed model, sim params, anymal params) of the task as configured by ``cfg``"""
    from migym import model as M, taskdefs
    spec = taskdefs.anymal_spec(M.load_json(ANYMAL_JSON), cfg)
    return spec, M.pack_model(spec), taskdefs.sim_params(cfg, taskdefs.TASK_INFO["Anymal"][5], 1), \
        taskdefs.anymal_params(cfg, spec)


def reset_state(p, n, seed):
    """n envs in the reference's reset distribution, from injected U(0,1) draws: (root, dof, noise)"""
    noise = np.random.default_rng(seed).uniform(0, 1, (n, 27)).astype(F)
    st = dict(root=np.zeros((n, 13), F), dof=np.zeros((n, 12, 2), F), commands=np.zeros((n, 3), F),
              progress=np.zeros(n, np.int64), reset=np.ones(n, np.int64))
    reset_envs(p, st, np.arange(n), noise)
    return st["root"], st["dof"], noise


def num_candidates(mnp, sp, root, dof):
    import pyoracle as O
    return np.array([len(O.contacts(mnp, sp, root[a], dof[a], 64)) for a in range(len(root))])


# ---- one-step physics states, chosen by the fp64 oracle alone (as tests/tree_physics_ref.py chooses its own)
PHYS_ACTORS, PHYS_SMALL, PHYS_POOL = 66, 6, 160
STANDING_STEPS, FALLEN_STEPS = 25, 30
_phys = {}


def physics_states(kind):
    """(spec, mnp, sp, root, dof, tgt, ref): PHYS_ACTORS states of the task model before the step, read-only, random
    PD targets within the action range, and the fp64 oracle's AnymalHost after one simulate from them.
      standing: reset draws rolled STANDING_STEPS zero-action steps by the oracle, until the feet rest;
      fallen: the base 2 cm above touching, rolled by up to 3.1 rad (some on their backs) and pitched by up to 0.6 rad, joints from the reset
      draws, rolled FALLEN_STEPS steps, so that it lies on its base and thighs.
    Taken in pool order where the contact candidates before and after the step stay within max_contacts; the first
    PHYS_SMALL have no discontinuity in their step (orc_step_flips == 0)."""
    if kind in _phys:
        return _phys[kind]
    import parity_stats as PS
    import tree_physics_ref as TP
    from migym import model as M
    spec, mnp, sp, ap = task_model(task_cfg(PHYS_ACTORS))
    p = params_from(ap)
    rng = np.random.default_rng({"standing": 31, "fallen": 32}[kind])
    root, dof, _ = reset_state(p, PHYS_POOL, int(rng.integers(1 << 30)))
    if kind == "fallen":
        roll, pitch = rng.uniform(-3.1, 3.1, PHYS_POOL), rng.uniform(-0.6, 0.6, PHYS_POOL)
        for a in range(PHYS_POOL):
            root[a, 3:7] = M.quat_from_rpy(roll[a], pitch[a], 0.0)
            root[a, 2] = 0.0
            root[a, 2] = 0.02 - TP.lowest_point(spec, root[a], dof[a, :, 0])
    h = AnymalHost(spec, root, dof, np.tile(p["default"], (PHYS_POOL, 1)))
    for _ in range(STANDING_STEPS if kind == "standing" else FALLEN_STEPS):
        h.simulate(mnp, sp)
    root, dof = h.root.copy(), h.dof.copy()
    tgt = (p["default"][None] + p["action_scale"] * rng.uniform(-1, 1, (PHYS_POOL, 12))).astype(F)
    after = AnymalHost(spec, root, dof, tgt).simulate(mnp, sp)
    fits = np.isfinite(root).all(1) & (num_candidates(mnp, sp, root, dof) <= sp.max_contacts) & \
        (num_candidates(mnp, sp, after.root, after.dof) <= sp.max_contacts)
    flags = PS.step_flags(mnp, sp, AnymalHost(spec, root, dof, tgt))
    keep = []
    for a in np.flatnonzero(fits):
        if len(keep) >= PHYS_SMALL or flags[a] == 0:
            keep.append(a)
        if len(keep) == PHYS_ACTORS:
            break
    assert len(keep) == PHYS_ACTORS, f"{kind}: the pool holds only {len(keep)} usable states"
    root, dof, tgt = (np.ascontiguousarray(x[keep]) for x in (root, dof, tgt))
    for x in (root, dof, tgt):
        x.setflags(write=False)
    _phys[kind] = spec, mnp, sp, root, dof, tgt, AnymalHost(spec, root, dof, tgt).simulate(mnp, sp)
    return _phys[kind]


def compare_step(test, kind, n, got, reach_cap=None):
    """the one-step rule of tree_physics_ref.compare on the first n states of ``kind``: every env within positions
    2e-4, velocities 2e-3 + 2e-3 |v|, DOF forces and net contact forces 1 % of the batch's largest, unless
    orc_step_flips puts its step at a discontinuity (at most 5 % of the envs, nothing unexplained); finite; moved.
    ``got``: root, dof (n, 12, 2), dof_force, ncf."""
    import parity_stats as PS
    spec, mnp, sp, root, dof, tgt, ref = physics_states(kind)
    for x in (got.root, got.dof, got.dof_force, got.ncf):
        assert np.isfinite(x).all()
    assert np.abs(got.dof[..., 0] - dof[:n, :, 0]).max() > 1e-3, "the step moved nothing"
    f_h, c_h = ref.dof_force[:n], ref.ncf[:n]
    checks = [("root pose", got.root[:, 0:7], ref.root[:n, 0:7], 2e-4, 0),
              ("dof pos", got.dof[..., 0], ref.dof[:n, :, 0], 2e-4, 0),
              ("root twist", got.root[:, 7:13], ref.root[:n, 7:13], 2e-3, 2e-3),
              ("dof vel", got.dof[..., 1], ref.dof[:n, :, 1], 2e-3, 2e-3),
              ("dof force", got.dof_force, f_h, 1e-2 * max(1.0, np.abs(f_h).max()), 0),
              ("net contact forces", got.ncf, c_h, 1e-2 * max(1.0, np.abs(c_h).max()), 0)]
    bad = np.zeros(n, bool)
    for name, a, b, atol, rtol in checks:
        eb = PS.env_bad(a, b, atol, rtol)
        err = np.abs(a.astype(np.float64) - b)
        print(f"{test} {name}: max err {err.max():.3g} (atol {atol:.3g}), envs outside {int(eb.sum())} / {n}")
        PS.record(test, name, a, b, envs_outside=int(eb.sum()), atol=atol, rtol=rtol)
        bad |= eb
    flags = PS.step_flags(mnp, sp, AnymalHost(spec, root[:n], dof[:n], tgt[:n]))
    return PS.assert_steps_explained(test, bad[None], flags[None], sens=None,
                                     reach_cap=PS.REACH_CAP if reach_cap is None else reach_cap, allow_unexplained=0.0)
