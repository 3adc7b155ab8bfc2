"""Helpers of the GPU-vs-oracle physics tests (test infrastructure): error statistics, and the
discontinuities of the build's physics that let an fp32 (GPU) and an fp64 (oracle) step of the same state
part ways.

The tests compare one physics step, or fused steps teacher-forced step by step (both sides restarted from the
oracle's state every step, so a step's rounding difference cannot grow chaotically over the next).  An env-step
whose GPU and oracle results disagree is accepted only when the oracle's orc_step_flips puts that step, in one of
its substeps, at a discontinuity:

  * a contact within STEP_DELTA of its threshold (contact_offset; 0 for the hand's explicit MJCF pairs) whose row
    the solve uses: present on one side and absent on the other, it changes the result only if its impulse leaves
    zero at some PGS visit (a row whose impulse stays zero changes nothing);
  * a joint-limit row within STEP_DELTA of the limit margin, used by the solve (the same rule);
  * a PD drive whose explicit force is within STEP_DF (relative) of its effort limit (implicit <-> saturated);
  * a capsule core inside a box whose two least push-out faces tie (seg_box_sat);
  * past max_contacts, a contact candidate within STEP_DELTA of its threshold on either side (or an ambiguous one)
    that precedes the cut: used or not, it shifts which later contact the cut drops (bit 128);

or where the oracle is itself sensitive (one step of the env alone with positions moved by 1e-6 moves its
observation by >= 1/4 of the GPU-vs-oracle gap).  The fraction of ALL env-steps these predicates exempt is
recorded and capped (REACH_CAP), so a test cannot pass by exempting the contact-rich envs wholesale.

The older per-state predicates (contact_flips, limit_flips, drive_flips, deep_contacts) remain for the
diagnostic tools.  Set MIGYM_PARITY_REPORT=<path> to collect the error statistics and exemptions of every check
into a JSON file.
"""
import copy
import json
import os

import numpy as np

import pyoracle as O

_REPORT = {}


def err_stats(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).ravel()
    if d.size == 0:
        return {"max": 0.0, "p999": 0.0, "p99": 0.0}
    return {"max": float(d.max()), "p999": float(np.quantile(d, 0.999)), "p99": float(np.quantile(d, 0.99))}


def record(test, name, a, b, **extra):
    st = err_stats(a, b)
    st.update({k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in extra.items()})
    _REPORT.setdefault(test, {})[name] = st
    return st


def write_report():
    path = os.environ.get("MIGYM_PARITY_REPORT")
    if path and _REPORT:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        old.update(_REPORT)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


# observation column groups of the locomotion tasks (ant.py:325-351 compute_ant_observations, humanoid.py:382-413):
# [height | vel_loc | angvel_loc | yaw roll angle_to_target | up_proj heading_proj | dof pos | dof vel | ... | actions]
OBS_GROUPS = {
    60: {"height": [0], "vel_loc": [1, 2, 3], "angvel_loc": [4, 5, 6], "yaw/roll/angle_to_target": [7, 8, 9],
         "up/heading proj": [10, 11], "dof pos (scaled)": list(range(12, 20)), "dof vel": list(range(20, 28)),
         "foot force-torques": list(range(28, 52)), "actions": list(range(52, 60))},
    108: {"height": [0], "vel_loc": [1, 2, 3], "angvel_loc": [4, 5, 6], "yaw/roll/angle_to_target": [7, 8, 9],
          "up/heading proj": [10, 11], "dof pos (scaled)": list(range(12, 33)), "dof vel": list(range(33, 54)),
          "dof force": list(range(54, 75)), "foot force-torques": list(range(75, 87)), "actions": list(range(87, 108))},
    # ShadowHand full_state (shadow_hand.py:528-575)
    211: {"dof pos (unscaled)": list(range(0, 24)), "dof vel": list(range(24, 48)), "dof force": list(range(48, 72)),
          "object pose": list(range(72, 79)), "object linvel": list(range(79, 82)), "object angvel": list(range(82, 85)),
          "goal pose": list(range(85, 92)), "object-goal rot": list(range(92, 96)),
          "fingertip states": list(range(96, 161)), "fingertip force-torques": list(range(161, 191)),
          "actions": list(range(191, 211))},
}
# MA-Ant: the Ant layout plus the other agents' torso positions relative to self (3 (A - 1), taskdefs.task_params)
for _A in (2, 4, 8):
    OBS_GROUPS[60 + 3 * (_A - 1)] = dict(OBS_GROUPS[60], **{"other agents": list(range(60, 60 + 3 * (_A - 1)))})
NORTH_STAR_RTOL = 1e-4   # BASELINE.json north_star: "obs/reward parity to CPU reference within 1e-4 rel"


def column_stats(test, name, a, b, keep, groups, rtol=NORTH_STAR_RTOL):
    """per column group over the env-steps in `keep` (unflagged): max |a - b|, max relative error |a - b| / |b| (over
    |b| > 1e-3), the fraction of elements within rtol |b| alone, and the atol that rtol needs to hold everywhere
    (max(|a - b| - rtol |b|)); recorded under test/name and returned"""
    a = np.asarray(a, np.float64)[keep]
    b = np.asarray(b, np.float64)[keep]
    out = {}
    for g, cols in groups.items():
        x, y = a[:, cols], b[:, cols]
        d = np.abs(x - y)
        big = np.abs(y) > 1e-3
        out[g] = {"max_abs": float(d.max()) if d.size else 0.0,
                  "max_rel": float((d[big] / np.abs(y[big])).max()) if big.any() else 0.0,
                  "frac_within_rtol": float((d <= rtol * np.abs(y)).mean()) if d.size else 1.0,
                  "atol_needed": float(np.maximum(d - rtol * np.abs(y), 0.0).max()) if d.size else 0.0,
                  "scale": float(np.abs(y).max()) if d.size else 0.0}
    _REPORT.setdefault(test, {})[name] = out
    return out


def env_bad(a, b, atol, rtol):
    """per-env: some element outside atol + rtol |b|"""
    a = np.asarray(a).reshape(len(a), -1)
    b = np.asarray(b).reshape(len(b), -1)
    return ~((np.abs(a - b) <= atol + rtol * np.abs(b)).all(axis=1))


def contact_flips(mnp, sp, roots, dofs, delta=1e-4, cap=64):
    """per env: the oracle's contact set changes when contact_offset moves by +-delta"""
    lo, hi = copy.copy(sp), copy.copy(sp)
    lo.contact_offset = sp.contact_offset - delta
    hi.contact_offset = sp.contact_offset + delta
    out = np.zeros(len(roots), bool)
    for i in range(len(roots)):
        r = np.ascontiguousarray(roots[i], np.float32).ravel()
        d = np.ascontiguousarray(dofs[i], np.float32)
        out[i] = len(O.contacts(mnp, lo, r, d, cap)) != len(O.contacts(mnp, hi, r, d, cap))
    if int(mnp["pair_mjcf"]) and int(mnp["num_pairs"]) > 0:
        # explicit MJCF pairs switch on at distance 0, not at the offset: count the pair contacts alone (the
        # model with pairs minus the model without) with the pairs' threshold moved to +-delta
        mp, m0 = mnp.copy(), mnp.copy()
        mp["pair_mjcf"] = 0
        m0["num_pairs"] = 0
        lo0, hi0 = copy.copy(sp), copy.copy(sp)
        lo0.contact_offset, hi0.contact_offset = -delta, delta
        for i in range(len(roots)):
            r = np.ascontiguousarray(roots[i], np.float32).ravel()
            d = np.ascontiguousarray(dofs[i], np.float32)
            npl = len(O.contacts(mp, lo0, r, d, cap)) - len(O.contacts(m0, lo0, r, d, cap))
            nph = len(O.contacts(mp, hi0, r, d, cap)) - len(O.contacts(m0, hi0, r, d, cap))
            out[i] |= npl != nph
    return out


def deep_contacts(mnp, sp, roots, dofs, depth=5e-3, cap=64):
    """per env: an oracle contact deeper than `depth`"""
    out = np.zeros(len(roots), bool)
    for i in range(len(roots)):
        cs = O.contacts(mnp, sp, np.ascontiguousarray(roots[i], np.float32).ravel(),
                        np.ascontiguousarray(dofs[i], np.float32), cap)
        out[i] = any(c[7] < -depth for c in cs)
    return out


def limit_flips(q, lower, upper, margin, dq=1e-4):
    """per env: a DOF position within dq of the joint-limit row threshold (limit_margin from a limit)"""
    q = np.asarray(q, np.float64)
    lo = np.abs((q - np.asarray(lower)) - margin) < dq
    hi = np.abs((np.asarray(upper) - q) - margin) < dq
    return (lo | hi).reshape(len(q), -1).any(axis=1)


def drive_flips(q, qd, targets, kp, damping, effort, df=1e-2):
    """per env: an explicit PD force kp (q* - q) - b qd within df (relative) of its effort limit"""
    fe = np.asarray(kp) * (np.asarray(targets) - q) - np.asarray(damping) * qd
    lim = np.asarray(effort)
    near = (np.asarray(kp) > 0) & (np.abs(np.abs(fe) - lim) < df * np.maximum(lim, 1e-6))
    return near.reshape(len(q), -1).any(axis=1)


# thresholds of the per-step predicates (orc_step_flips): a teacher-forced step starts the GPU and the oracle
# from the same state, so the two stay within fp32 rounding (~1e-6 m) of each other through its substeps
STEP_DELTA = 1e-5    # m / rad from a contact, pair or joint-limit threshold (with the row in use)
STEP_DF = 2e-4       # relative distance of a PD drive's explicit force from its effort limit
# at most this fraction of the env-steps of a test may be exempt (flagged) at all: beyond it the predicates would
# excuse too much for the test to see a bug in contact-rich envs ("What's weak" 2)
REACH_CAP = 0.05
SENS_CAP = 0.01      # and at most this fraction by the oracle-sensitivity fallback


def spin_bad(ra, da, rb, db, root0, dof0, dt, atol_p=2e-4, atol_v=2e-3, rtol_v=2e-3, k_spin=1e-4):
    """per env of the fast-spin stress states (tests/test_gpu_parity.py, fast = 1): result a vs the checker's b
    (root states (n, 13), dof states (n, ndof, 2)) from the same pre-step state (root0, dof0).  A velocity may
    differ by atol_v + rtol_v |v| + k_spin x the env's largest initial rate (fp32 rounding of the spin-sized
    Coriolis and cap terms, |w|^2 h, reaches every velocity of the env, also the ones that end near 0); a position
    by atol_p + dt x the tolerance of its velocity (the step integrates q' = q + dt v', the quaternion with
    |dq| <= dt |dw| / 2)"""
    n = len(ra)
    spin = np.maximum(np.abs(dof0[..., 1]).reshape(n, -1).max(axis=1), np.abs(root0[:, 10:13]).max(axis=1))
    base = atol_v + k_spin * spin[:, None]
    tv_d = base + rtol_v * np.abs(db[..., 1])
    tv_r = base + rtol_v * np.abs(rb[:, 7:13])
    bad = (np.abs(da[..., 1] - db[..., 1]) > tv_d).any(axis=1)
    bad |= (np.abs(ra[:, 7:13] - rb[:, 7:13]) > tv_r).any(axis=1)
    bad |= (np.abs(da[..., 0] - db[..., 0]) > atol_p + dt * tv_d).any(axis=1)
    bad |= (np.abs(ra[:, 0:3] - rb[:, 0:3]) > atol_p + dt * tv_r[:, 0:3]).any(axis=1)
    bad |= (np.abs(ra[:, 3:7] - rb[:, 3:7]) > atol_p + 0.5 * dt * tv_r[:, 3:6].max(axis=1, keepdims=True)).any(axis=1)
    return bad


def first_substep_drift(mnp, sp, root0, dof0, act, floor=1e-6):
    """per env: how far apart an fp32 and an fp64 first substep put the positions (root position, joint
    positions; max abs), measured with the oracle's fp32 build (liboracle_f32) against the checker, at least
    `floor`: the input perturbation simulate_sensitive uses (the rest of the step starts from states this far apart)"""
    sp1 = copy.copy(sp)
    sp1.substeps, sp1.dt = 1, sp.dt / sp.substeps
    out = []
    for fp32 in (False, True):
        r, d = np.array(root0, np.float32), np.array(dof0, np.float32)
        O.simulate(mnp, sp1, r, d, np.ascontiguousarray(act, np.float32), threads=8, fp32=fp32)
        out.append((r.astype(np.float64), d.astype(np.float64)))
    (r64, d64), (r32, d32) = out
    n = len(r64)
    dq = np.maximum(np.abs(r32[:, 0:3] - r64[:, 0:3]).max(axis=1),
                    np.abs(d32[..., 0] - d64[..., 0]).reshape(n, -1).max(axis=1))
    return np.maximum(dq, floor)


def simulate_sensitive(mnp, sp, root0, dof0, act, i, out_a, out_b, eps=1e-6, ratio=0.25, log=None):
    """the oracle's own sensitivity at env i of a direct simulate from (root0, dof0, act): one simulate of env i
    alone, once as given and once with its positions (root position, joint positions) moved by eps (e.g. its
    first_substep_drift); True if its result (root states and dof states) moves by >= ratio x the gap
    |out_a - out_b| of env i (log: a list collecting (i, moved, gap))"""
    runs = []
    for pert in (0.0, eps):
        r = np.array(root0[i:i + 1], np.float64)
        d = np.array(dof0[i:i + 1], np.float64)
        r[:, 0:3] += pert
        d[..., 0] += pert
        r, d = r.astype(np.float32), d.astype(np.float32)
        O.simulate(mnp, sp, r, d, np.ascontiguousarray(act[i:i + 1], np.float32))
        runs.append(np.concatenate([r.ravel(), d.ravel()]).astype(np.float64))
    moved = np.abs(runs[1] - runs[0]).max()
    gap = np.abs(np.asarray(out_a[i], np.float64).ravel() - np.asarray(out_b[i], np.float64).ravel()).max()
    if log is not None:
        log.append((i, float(moved), float(gap)))
    return moved >= ratio * gap


def step_flags(mnp, sp, host, delta=STEP_DELTA, df=STEP_DF):
    """per env: orc_step_flips of the physics input `host` holds (a HostEnv with act_eff / a HandHostEnv after
    pre_physics, optionally with env_props): bit 1 contact threshold in use, 2 limit threshold in use, 4 drive
    near saturation, 8 seg_box_sat tie, 16 a narrowphase decision within its ambiguity band, 32 an
    ill-conditioned contact normal (core distance / MPR depth below 0.5 mm), 64 the angular-velocity cap clipped a
    hinge rate to an ill-conditioned interval end, 128 more candidates than max_contacts with one near its
    threshold (or ambiguous) at or before the cut (never set while the candidates fit; the input must have fewer
    than 64 of them)"""
    return O.step_flips(mnp, sp, host, delta, df)


def loco_physics_input(h, mnp, sp, tp, seed, step, threads=1):
    """a HostEnv copy holding step `step`'s physics input: the state as the step starts (the locomotion resets
    run in post_physics) and the actuation pre_physics computes from h.actions"""
    g, tmp = copy.deepcopy(h), copy.deepcopy(h)
    tmp.env_step(mnp, sp, tp, seed=seed, step=step, threads=threads)
    g.act_eff[:] = tmp.act_eff
    return g


def hand_physics_input(h, mnp, tp, seed, step):
    """a HandHostEnv copy after pre_physics of step `step` (goal / env resets, PD targets, object forces)"""
    g = copy.deepcopy(h)
    g.pre_physics(mnp, tp, seed=seed, step=step)
    return g


def assert_steps_explained(test, bad, flags, sens=None, reach_cap=REACH_CAP, sens_cap=SENS_CAP, allow_unexplained=0.0):
    """bad, flags: (steps, envs).  Every disagreeing env-step must be flagged by orc_step_flips at that step (or,
    through `sens(t, i)`, sit where the oracle itself is sensitive); the flags' reach (the fraction of ALL env-steps
    they would exempt) and the sensitivity fallback's use are recorded and capped.  allow_unexplained: a stated
    fraction of env-steps that may disagree with neither (the fast-spin stress states; recorded)"""
    bad = np.asarray(bad, bool)
    flagged = np.asarray(flags) != 0
    why = flagged.copy()
    nsens = 0
    if sens is not None:
        for t, i in zip(*np.nonzero(bad & ~why)):
            if sens(int(t), int(i)):
                why[t, i] = True
                nsens += 1
    total = bad.size
    rec = {"env_steps": int(total), "disagreeing": int(bad.sum()), "flagged_reach": float(flagged.mean()),
           "explained_by_flags": int((bad & flagged).sum()), "explained_by_sensitivity": nsens,
           "bits": {str(b): float(((np.asarray(flags) & b) != 0).mean()) for b in (1, 2, 4, 8, 16, 32, 64, 128)}}
    unexplained = np.argwhere(bad & ~why)
    rec["unexplained"] = int(len(unexplained))
    rec["allowed_unexplained"] = float(allow_unexplained)
    _REPORT.setdefault(test, {})["exemptions"] = rec
    assert len(unexplained) <= allow_unexplained * total, (
        f"{test}: {len(unexplained)} of {int(bad.sum())} disagreeing env-steps are not at a discontinuity "
        f"(allowed {allow_unexplained} x {total}) (step, env): {unexplained[:10].tolist()}")
    assert flagged.mean() <= reach_cap, f"{test}: the predicates exempt {flagged.mean():.3f} of the env-steps (cap {reach_cap})"
    assert nsens <= sens_cap * total, f"{test}: {nsens} env-steps excused by oracle sensitivity (cap {sens_cap} x {total})"
    return rec


def oracle_sensitive_step(mnp, sp, tp, pre, action, i, gpu_out, oracle_out, seed, step, hand, eps=1e-6, ratio=0.25):
    """one teacher-forced step of env i alone from `pre` (its state before the step), once as recorded and once
    with positions moved by eps: True if the final observation moves by >= ratio x the GPU-vs-oracle gap"""
    runs = []
    for pert in (0.0, eps):
        g = env_slice(pre, i)
        if hand:
            g.root[:, 1, 0:3] += pert
        else:
            g.root[:, 0:3] += pert
        g.dof[..., 0] += pert
        g.actions[:] = action[i:i + 1]
        g.env_step(mnp, sp, tp, seed=seed, step=step, threads=1, env_offset=i)
        runs.append(g.obs[0].astype(np.float64).copy())
    moved = np.abs(runs[1] - runs[0]).max()
    gap = np.abs(np.asarray(gpu_out, np.float64) - np.asarray(oracle_out, np.float64)).max()
    return moved >= ratio * gap


def assert_explained(bad, explained, what):
    """every disagreeing env must sit at one of the discontinuities"""
    unexplained = np.flatnonzero(bad & ~explained)
    assert unexplained.size == 0, (f"{what}: {unexplained.size} of {int(bad.sum())} disagreeing envs are not at a "
                                   f"contact / limit / drive threshold or a deep penetration: {unexplained[:10].tolist()}")


def env_slice(h, i):
    """a one-env copy of a pyoracle HostEnv / HandHostEnv (every per-env array sliced)"""
    g = copy.copy(h)
    for k, v in vars(h).items():
        if isinstance(v, np.ndarray):
            setattr(g, k, v[i:i + 1].copy() if v.shape[:1] == (h.n,) else v.copy())
    g.n = 1
    return g


def oracle_sensitive(mnp, sp, tp, pre, actions, i, gpu_out, oracle_out, seed, hand, t0=1, eps=1e-6, ratio=0.25):
    """the oracle's own sensitivity at env i: replay steps t0.. of env i alone (RNG keyed by its index), once as
    recorded and once with its positions perturbed by eps; True if the perturbed replay's final observation
    moves by >= ratio x the GPU-vs-oracle difference"""
    runs = []
    for pert in (0.0, eps):
        g = env_slice(pre[t0], i)
        if hand:
            g.root[:, 1, 0:3] += pert
        else:
            g.root[:, 0:3] += pert
        g.dof[..., 0] += pert
        for t in range(t0, len(actions)):
            g.actions[:] = actions[t][i:i + 1]
            g.env_step(mnp, sp, tp, seed=seed, step=t, threads=1, env_offset=i)
        runs.append(g.obs[0].astype(np.float64).copy())
    moved = np.abs(runs[1] - runs[0]).max()
    gap = np.abs(np.asarray(gpu_out, np.float64) - np.asarray(oracle_out, np.float64)).max()
    return moved >= ratio * gap
