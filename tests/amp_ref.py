"""HumanoidAMP's task layer restated in numpy fp32, and the fixtures of its tests.

A second statement of what include/migym.h promises of mg_amp_pre / mg_amp_post / mg_amp_reset_idx / mg_amp_obs_demo,
written from the reference's expressions (humanoid_amp.py, amp/humanoid_amp_base.py, amp/utils_amp/motion_lib.py,
utils/torch_jit_utils.py) without its code: tests/test_amp_host.py holds it to the recorded traces of the reference's
own methods (tests/golden/make_amp_golden.py) on the CPU, tests/test_gpu_amp.py feeds it the counter RNG's host twin.
It samples the packed table of migym.motion.MotionTable, the array the kernels read, so the CPU suite covers the
table's layout as well.
"""
import functools
import os

import numpy as np

from migym import _abi, configs, taskdefs
from migym import model as M
from migym.motion import DOF_BODY_IDS, DOF_OFFSETS, F_DOF_VEL, F_KEY, F_ROT, MotionTable

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_TABLE = os.path.join(GOLDEN, "amp_humanoid.json")
MOTIONS_YAML = os.path.join(GOLDEN, "amp_motions.yaml")
CLIPS = ["amp_humanoid_walk", "amp_humanoid_run", "amp_humanoid_walk_flip"]
SIZES = [6, 67]
CONFIGS = {   # make_amp_golden.CONFIGS
    "default": dict(state_init="Default", steps=2, local=False, pd=False),
    "start": dict(state_init="Start", steps=3, local=True, pd=True),
    "random": dict(state_init="Random", steps=2, local=True, pd=True),
    "hybrid": dict(state_init="Hybrid", steps=3, local=False, pd=True),
}
TOL = 1e-4   # the project's task-layer tolerance: |x - ref| <= TOL * max(1, |ref|)
f32 = np.float32
OBS_OFFSETS = [0, 6, 12, 18, 19, 25, 26, 32, 33, 39, 45, 46]


@functools.lru_cache(maxsize=None)
def _npz(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def trace(N, name):
    """the arrays of one trace, keys without the config prefix"""
    if N == SIZES[0]:
        g = _npz("trace_amp_N6.npz")
        out = {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "_")}
        out.update({k: g[k] for k in ("steps", "episode_length", "sim_dt", "control_freq_inv", "hybrid_prob",
                                      "termination_height")})
        return out
    return _npz(f"trace_amp_N{N}_{name}.npz")


def motionlib():
    return _npz("amp_motionlib.npz")


def demo():
    return _npz("trace_amp_demo.npz")


@functools.lru_cache(maxsize=None)
def table():
    return MotionTable(MOTIONS_YAML, [5, 8, 11, 14])


def golden_cfg(N, name):
    """the task config the traces were recorded under"""
    c, g = CONFIGS[name], trace(SIZES[0], name)
    cfg = configs.task_config("HumanoidAMP", N)
    cfg["env"].update({"stateInit": c["state_init"], "numAMPObsSteps": c["steps"], "localRootObs": c["local"],
                       "pdControl": c["pd"], "episodeLength": int(g["episode_length"]),
                       "hybridInitProb": float(g["hybrid_prob"]), "motion_file": MOTIONS_YAML})
    cfg["env"]["asset"] = {"modelTable": MODEL_TABLE}
    return cfg


def task_model(cfg):
    spec = taskdefs.amp_spec(M.load_json(MODEL_TABLE), cfg)
    return spec, _abi.model_bytes(spec), taskdefs.sim_params(cfg, taskdefs.TASK_INFO["HumanoidAMP"][5], 1), \
        taskdefs.amp_params(cfg, spec)


def params_from(ap):
    return dict(offset=np.array(list(ap.pd_action_offset), f32), scale=np.array(list(ap.pd_action_scale), f32),
                effort=np.array(list(ap.motor_effort), f32), power_scale=f32(ap.power_scale),
                initial_dof_pos=np.array(list(ap.initial_dof_pos), f32), initial_root=np.array(list(ap.initial_root), f32),
                dt=float(ap.dt), termination_height=f32(ap.termination_height), hybrid_prob=f32(ap.hybrid_init_prob),
                clip_actions=f32(ap.clip_actions), clip_obs=f32(ap.clip_obs), max_len=int(ap.max_episode_length),
                early=bool(ap.enable_early_termination), local=bool(ap.local_root_obs), pd=bool(ap.pd_control),
                state_init=int(ap.state_init), steps=int(ap.num_amp_obs_steps), key=list(ap.key_body),
                contact=[b for b in range(ap.num_bodies) if (ap.contact_body_mask >> b) & 1], nb=int(ap.num_bodies))


def close(x, ref, tol=TOL):
    """the project's 1e-4 rule, |x - ref| <= 1e-4 max(1, |ref|): the largest |x - ref| / max(1, |ref|) and whether it
    is within tol (a NaN on either side is outside)"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    err = float((np.abs(x - ref) / np.maximum(1.0, np.abs(ref))).max()) if x.size else 0.0
    return err, bool(err <= tol)


# ---------------------------------------------------------------------------------------------- quaternion algebra (fp32)
def _rotate(q, v):
    """my_quat_rotate"""
    qw, qv = q[..., 3:4], q[..., :3]
    a = v * (f32(2.0) * qw * qw - f32(1.0))
    b = np.cross(qv, v).astype(f32) * qw * f32(2.0)
    c = qv * (qv * v).sum(-1, keepdims=True, dtype=f32) * f32(2.0)
    return (a + b + c).astype(f32)


def _quat_mul(a, b):
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x2, y2, z2, w2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = f32(0.5) * (xx + (z1 - x1) * (x2 - y2))
    w = qq - ww + (z1 - y1) * (y2 - z2)
    x = qq - xx + (x1 + w1) * (x2 + w2)
    y = qq - yy + (w1 - x1) * (y2 + z2)
    z = qq - zz + (z1 + y1) * (w2 - x2)
    return np.stack([x, y, z, w], -1).astype(f32)


def _normalize(x):
    n = np.sqrt((x * x).sum(-1, keepdims=True, dtype=f32))
    return (x / np.maximum(n, f32(1e-9))).astype(f32)


def _normalize_angle(x):
    return np.arctan2(np.sin(x), np.cos(x)).astype(f32)


def _quat_from_angle_axis(angle, axis):
    theta = (angle / f32(2.0))[..., None]
    return _normalize(np.concatenate([_normalize(axis) * np.sin(theta), np.cos(theta)], -1).astype(f32))


def _heading_inv(q):
    ex = np.zeros(q.shape[:-1] + (3,), f32)
    ex[..., 0] = 1
    d = _rotate(q, ex)
    heading = np.arctan2(d[..., 1], d[..., 0]).astype(f32)
    ez = np.zeros_like(ex)
    ez[..., 2] = 1
    return _quat_from_angle_axis(-heading, ez)


def _tan_norm(q):
    ex = np.zeros(q.shape[:-1] + (3,), f32)
    ex[..., 0] = 1
    ez = np.zeros_like(ex)
    ez[..., 2] = 1
    return np.concatenate([_rotate(q, ex), _rotate(q, ez)], -1)


def _exp_map_to_quat(e):
    with np.errstate(invalid="ignore", divide="ignore"):
        angle = np.sqrt((e * e).sum(-1, dtype=f32))
        axis = e / angle[..., None]
    angle = _normalize_angle(angle)
    mask = angle > f32(1e-5)
    angle = np.where(mask, angle, f32(0))
    default = np.zeros_like(e)
    default[..., 2] = 1
    axis = np.where(mask[..., None], axis, default).astype(f32)
    return _quat_from_angle_axis(angle, axis)


def _quat_to_angle_axis(q):
    with np.errstate(invalid="ignore", divide="ignore"):
        sin_theta = np.sqrt(f32(1) - q[..., 3] * q[..., 3])
        angle = _normalize_angle(f32(2) * np.arccos(q[..., 3]))
        axis = q[..., :3] / sin_theta[..., None]
    mask = sin_theta > f32(1e-5)
    default = np.zeros_like(axis)
    default[..., 2] = 1
    return np.where(mask, angle, f32(0)).astype(f32), np.where(mask[..., None], axis, default).astype(f32)


def _slerp(q0, q1, t):
    """t broadcasts against q[..., 0]"""
    cos = q0[..., 3] * q1[..., 3] + q0[..., 0] * q1[..., 0] + q0[..., 1] * q1[..., 1] + q0[..., 2] * q1[..., 2]
    q1 = np.where((cos < 0)[..., None], -q1, q1)
    cos = np.abs(cos)[..., None]
    t = np.broadcast_to(t, cos.shape[:-1])[..., None].astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        half = np.arccos(cos)
        sin_half = np.sqrt(f32(1.0) - cos * cos)
        ra = np.sin((f32(1) - t) * half) / sin_half
        rb = np.sin(t * half) / sin_half
        new = ra * q0 + rb * q1
    new = np.where(np.abs(sin_half) < f32(0.001), f32(0.5) * q0 + f32(0.5) * q1, new)
    new = np.where(np.abs(cos) >= 1, q0, new)
    return new.astype(f32)


# ---------------------------------------------------------------------------------------------- the task layer
def observations(root, dof_pos, dof_vel, key_pos, local):
    """compute_humanoid_observations = build_amp_observations: (n, 105)"""
    root, dof_pos, dof_vel, key_pos = (np.asarray(a, f32) for a in (root, dof_pos, dof_vel, key_pos))
    n = root.shape[0]
    q = root[:, 3:7]
    h = _heading_inv(q)
    rot_obs = _tan_norm(_quat_mul(h, q) if local else q)
    vel, ang = _rotate(h, root[:, 7:10]), _rotate(h, root[:, 10:13])
    key = _rotate(np.repeat(h[:, None], 4, 1).reshape(-1, 4), (key_pos.reshape(n, 4, 3) - root[:, None, 0:3]).reshape(-1, 3))
    dof_obs = np.zeros((n, 52), f32)
    for j, o in enumerate(DOF_OFFSETS[:-1]):
        size = DOF_OFFSETS[j + 1] - o
        if size == 3:
            dof_obs[:, OBS_OFFSETS[j]:OBS_OFFSETS[j] + 6] = _tan_norm(_exp_map_to_quat(dof_pos[:, o:o + 3]))
        else:
            dof_obs[:, OBS_OFFSETS[j]] = dof_pos[:, o]
    return np.concatenate([root[:, 2:3], rot_obs, vel, ang, dof_obs, dof_vel, key.reshape(n, 12)], -1).astype(f32)


def pre_step(p, actions):
    a = np.clip(np.asarray(actions, f32), -p["clip_actions"], p["clip_actions"])
    if p["pd"]:
        return a, (p["offset"] + p["scale"] * a).astype(f32)
    return a, (a * p["effort"] * p["power_scale"]).astype(f32)


def post_step(p, st, root, dof, rb_pos, ncf):
    """mg_amp_post on the state dict st (progress, reset, terminate, timeout, obs, rew, amp), in place"""
    st["progress"] = st["progress"] + 1
    st["obs"] = observations(root, dof[..., 0], dof[..., 1], rb_pos[:, p["key"]].reshape(len(root), 12), p["local"])
    st["rew"] = np.ones(len(root), f32)
    mask = np.ones(p["nb"], bool)
    mask[p["contact"]] = False
    fallen = (ncf[:, mask] > f32(0.1)).any((1, 2)) & (rb_pos[:, mask, 2] < p["termination_height"]).any(1)
    term = (fallen & (st["progress"] > 1) & p["early"]).astype(np.int64)
    time_out = st["progress"] >= p["max_len"] - 1
    st["terminate"] = term
    st["reset"] = np.where(time_out, 1, term).astype(np.int64)
    st["timeout"] = time_out & (st["reset"] != 0)
    st["amp"] = np.concatenate([st["obs"][:, None], st["amp"][:, :-1]], 1)


def pick_motion(tb, u):
    return np.minimum(tb.cdf.searchsorted(np.asarray(u, f32).astype(np.float64), side="right"), tb.num_motions() - 1)


def motion_state(tb, mids, times):
    """MotionLib.get_motion_state off the packed table: root (n, 13), dof_pos, dof_vel, key (n, 12); and idx0"""
    mids, times = np.asarray(mids), np.asarray(times, np.float64)
    length, nf, dt = tb.lengths[mids], tb.num_frames[mids], tb.dt[mids]
    phase = np.clip(times / length, 0.0, 1.0)
    i0 = (phase * (nf - 1)).astype(int)
    i1 = np.minimum(i0 + 1, nf - 1)
    blend = ((times - i0 * dt) / dt).astype(f32)[:, None]
    f0, f1 = tb.frames[tb.first_frame[mids] + i0], tb.frames[tb.first_frame[mids] + i1]
    n = len(mids)
    root = np.zeros((n, 13), f32)
    root[:, 0:3] = (f32(1.0) - blend) * f0[:, 0:3] + blend * f1[:, 0:3]
    root[:, 3:7] = _slerp(f0[:, 3:7], f1[:, 3:7], blend[:, 0])
    root[:, 7:13] = f0[:, 7:13]
    key = ((f32(1.0) - blend) * f0[:, F_KEY:] + blend * f1[:, F_KEY:]).astype(f32)
    local = _slerp(f0[:, F_ROT:F_DOF_VEL].reshape(n, 15, 4), f1[:, F_ROT:F_DOF_VEL].reshape(n, 15, 4), blend)
    dof_pos = np.zeros((n, 28), f32)
    for j, b in enumerate(DOF_BODY_IDS):
        o, size = DOF_OFFSETS[j], DOF_OFFSETS[j + 1] - DOF_OFFSETS[j]
        angle, axis = _quat_to_angle_axis(local[:, b])
        if size == 3:
            dof_pos[:, o:o + 3] = angle[:, None] * axis
        else:
            dof_pos[:, o] = _normalize_angle(angle * axis[:, 1])
    return root, dof_pos, f0[:, F_DOF_VEL:F_KEY].copy(), key, i0


def reset_idx(p, tb, st, ids, noise, rb_pos):
    """mg_amp_reset_idx: st holds root (N, 13), dof (N, 28, 2), obs, amp, progress, reset, terminate; noise (n, 3) by
    list position; rb_pos (N, 15, 3) the rigid-body positions as bound"""
    ids, noise = np.asarray(ids), np.asarray(noise, f32)
    mode = p["state_init"]
    ref = np.full(len(ids), mode in (1, 2)) | ((mode == 3) & (noise[:, 0] < p["hybrid_prob"]))
    mids = pick_motion(tb, noise[:, 1])
    t0 = np.zeros(len(ids)) if mode == 1 else noise[:, 2].astype(np.float64) * tb.lengths[mids]
    for i, e in enumerate(ids):
        if ref[i]:
            root, dp, dv, _, _ = motion_state(tb, mids[i:i + 1], t0[i:i + 1])
            st["root"][e], st["dof"][e, :, 0], st["dof"][e, :, 1] = root[0], dp[0], dv[0]
        else:
            st["root"][e], st["dof"][e, :, 0], st["dof"][e, :, 1] = p["initial_root"], p["initial_dof_pos"], 0.0
        st["progress"][e] = st["reset"][e] = st["terminate"][e] = 0
        cur = observations(st["root"][e:e + 1], st["dof"][e:e + 1, :, 0], st["dof"][e:e + 1, :, 1],
                           rb_pos[e:e + 1, p["key"]].reshape(1, 12), p["local"])[0]
        st["obs"][e] = cur
        st["amp"][e, 0] = cur
        for k in range(1, p["steps"]):
            if ref[i]:
                root, dp, dv, key, _ = motion_state(tb, mids[i:i + 1], t0[i:i + 1] + -p["dt"] * k)
                st["amp"][e, k] = observations(root, dp, dv, key, p["local"])[0]
            else:
                st["amp"][e, k] = cur
    return ref, mids, t0


def obs_demo(p, tb, noise):
    """mg_amp_obs_demo: (n, steps, 105) from (n, 2) uniforms [motion | phase]"""
    noise = np.asarray(noise, f32)
    mids = pick_motion(tb, noise[:, 0])
    t0 = noise[:, 1].astype(np.float64) * tb.lengths[mids]
    out = np.zeros((len(noise), p["steps"], 105), f32)
    for k in range(p["steps"]):
        root, dp, dv, key, _ = motion_state(tb, mids, t0 + -p["dt"] * k)
        out[:, k] = observations(root, dp, dv, key, p["local"])
    return out


# ---------------------------------------------------------------------------------------------- the task model under the fp64 oracle
class AmpHost:
    """host views of the task's humanoids for orc_simulate_views / orc_step_flips, bound as the task binds them: PD
    targets, DOF forces, rigid-body states, foot sensors and the net contact force tensor"""

    def __init__(self, spec, root, dof, tgt):
        import pyoracle as O
        self.O, self.n = O, len(root)
        self.root, self.dof, self.tgt = (np.array(x, f32) for x in (root, dof, tgt))
        nd, nb = spec.num_dofs, len(spec.bodies)
        self.act_eff, self.dof_force = np.zeros((self.n, nd), f32), np.zeros((self.n, nd), f32)
        self.ncf, self.rb = np.zeros((self.n, nb, 3), f32), np.zeros((self.n, nb, 13), f32)
        self.sensors = np.zeros((self.n, max(len(spec.sensors), 1), 6), f32)

    def views(self):
        O, v = self.O, _abi.StateViews()
        v.root_states, v.dof_state, v.dof_actuation = O.p(self.root), O.p(self.dof), O.p(self.act_eff)
        v.dof_targets, v.dof_force, v.net_contact_forces = O.p(self.tgt), O.p(self.dof_force), O.p(self.ncf)
        v.rigid_body_states, v.sensors = O.p(self.rb), O.p(self.sensors)
        return v

    def simulate(self, mnp, sp):
        v = self.views()
        self.O.lib().orc_simulate_views(mnp.ctypes.data, self.O.C.byref(sp), self.n, self.O.C.byref(v), 8)
        return self


def num_candidates(mnp, sp, root, dof):
    import pyoracle as O
    return np.array([len(O.contacts(mnp, sp, root[a], dof[a], 96)) for a in range(len(root))])


# one-step physics states, chosen by the fp64 oracle alone (as tests/tree_physics_ref.py chooses its own)
PHYS_ACTORS, PHYS_SMALL, PHYS_POOL = 66, 6, 200
CLIP_STEPS, FALLEN_STEPS = 12, 30
_phys = {}


def physics_cfg(N):
    cfg = golden_cfg(N, "random")
    cfg["env"]["episodeLength"] = 300
    return cfg


def physics_states(kind):
    """(spec, mnp, sp, root, dof, tgt, ref, passed_over): PHYS_ACTORS states of the task model before the step,
    read-only, random position targets inside the action range (offset + scale U(-1, 1)), and the fp64 oracle's
    AmpHost after one simulate from them.
      clip: poses sampled from the walk clip (motion_state at seeded uniform phases), held at their own pose as PD
        target and rolled CLIP_STEPS simulates by the oracle, until the feet rest;
      fallen: the same poses with the root rolled by up to 3.1 rad and pitched by up to 0.6 rad, lowered to 2 cm above
        touching, rolled FALLEN_STEPS simulates, until non-foot rows carry force.
    Taken in pool order where the state is finite, the contact candidates before and after the step stay within
    max_contacts and orc_step_flips reports no discontinuity in the step: stricter than "no flip among the first 6",
    so that no env is exempt from the comparison.  passed_over: the pool indices skipped before the last one taken."""
    if kind in _phys:
        return _phys[kind]
    import parity_stats as PS
    import tree_physics_ref as TP
    spec, mnp, sp, ap = task_model(physics_cfg(PHYS_ACTORS))
    p, tb = params_from(ap), table()
    rng = np.random.default_rng({"clip": 41, "fallen": 42}[kind])
    u = rng.uniform(0, 1, PHYS_POOL)
    root, dof_pos, dof_vel, _, _ = motion_state(tb, np.zeros(PHYS_POOL, int), u * tb.lengths[0])
    dof = np.stack([dof_pos, dof_vel], -1).astype(f32)
    root[:, 0:2] = 0.0
    if kind == "fallen":
        roll, pitch = rng.uniform(-3.1, 3.1, PHYS_POOL), rng.uniform(-0.6, 0.6, PHYS_POOL)
        root[:, 7:13], dof[..., 1] = 0.0, 0.0
        for a in range(PHYS_POOL):
            root[a, 3:7] = M.quat_from_rpy(roll[a], pitch[a], 0.0)
            root[a, 2] = 0.0
            root[a, 2] = 0.02 - TP.lowest_point(spec, root[a], dof[a, :, 0])
    h = AmpHost(spec, root, dof, dof[..., 0].copy())
    for _ in range(CLIP_STEPS if kind == "clip" else FALLEN_STEPS):
        h.simulate(mnp, sp)
    root, dof = h.root.copy(), h.dof.copy()
    tgt = (p["offset"][None] + p["scale"][None] * rng.uniform(-1, 1, (PHYS_POOL, 28))).astype(f32)
    after = AmpHost(spec, root, dof, tgt).simulate(mnp, sp)
    ok = np.isfinite(root).all(1) & np.isfinite(dof).all((1, 2)) & np.isfinite(after.root).all(1)
    ok[ok] &= num_candidates(mnp, sp, root[ok], dof[ok]) <= sp.max_contacts
    ok[ok] &= num_candidates(mnp, sp, after.root[ok], after.dof[ok]) <= sp.max_contacts
    flags = PS.step_flags(mnp, sp, AmpHost(spec, root, dof, tgt))
    keep = [a for a in np.flatnonzero(ok) if flags[a] == 0][:PHYS_ACTORS]
    assert len(keep) == PHYS_ACTORS, f"{kind}: the pool holds only {len(keep)} usable states"
    passed_over = [a for a in range(keep[-1]) if a not in keep]
    root, dof, tgt = (np.ascontiguousarray(x[keep]) for x in (root, dof, tgt))
    for x in (root, dof, tgt):
        x.setflags(write=False)
    _phys[kind] = spec, mnp, sp, root, dof, tgt, AmpHost(spec, root, dof, tgt).simulate(mnp, sp), passed_over
    return _phys[kind]


def compare_step(test, kind, n, got):
    """the one-step rule of tree_physics_ref.compare on the first n states of ``kind``: every env within positions
    2e-4, velocities 2e-3 + 2e-3 |v|, DOF forces and net contact forces 1 % of the batch's largest; the states were
    chosen with no flagged discontinuity, so nothing is exempt.  ``got``: root, dof (n, 28, 2), dof_force, ncf."""
    import parity_stats as PS
    spec, mnp, sp, root, dof, tgt, ref, _ = physics_states(kind)
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
    flags = PS.step_flags(mnp, sp, AmpHost(spec, root[:n], dof[:n], tgt[:n]))
    return PS.assert_steps_explained(test, bad[None], flags[None], sens=None, reach_cap=PS.REACH_CAP,
                                     allow_unexplained=0.0)
