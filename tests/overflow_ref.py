"""The task models and the hand with max_contacts lowered below what their states hold: the inputs, the fp64 oracle's
step at that capacity and the comparison, shared by tests/test_gpu_overflow.py (the kernels) and
tests/test_overflow_host.py (the oracle's fp32 twin through the same rule).

Capacity is a per-task constant (Ant 16, Humanoid 32, ShadowHand 24) that the task states of the other tests never
reach.  Here the states are theirs -- contacts_ref.task_set (Ant and Humanoid on their feet after a short rollout) and
contacts_ref.hand_set (the object on the palm, or against the forearm hull) -- and max_contacts is lowered to k, so
that collide() drops contacts (csrc/team_physics.hpp, cap = min(max_contacts, MC)) and everything behind it -- rows,
the solve, sensors, DOF forces, net contact forces -- runs on a cut list.  One simulate against the oracle at the same
k; every env within the one-step tolerances unless orc_step_flips flags its step (bit 128: a candidate near its
threshold before the cut), flags reaching at most 5 %, no sensitivity fallback, nothing unexplained.
"""
import copy

import numpy as np

import contacts_ref as CR
import parity_stats as PS
import pyoracle as O

TASKS = (("Ant", 256, 2), ("Humanoid", 128, 4))      # (task, envs, max_contacts)
TASK_OVER = {"Ant": 16, "Humanoid": 20}              # at least this many envs hold more candidates than that
HANDS = (("palm-block", 4), ("palm-egg", 4), ("palm-pen", 4), ("hull-block", 8))
# palm-egg: contacts_ref.hand_set's states (seed 5) leave the rule with the fp32 twin at every capacity, the task's own
# 24 included (envs 2 and 142, 2.2 and 2.8 x the tolerance, unflagged: the twin's fp32 egg narrowphase, not the cut),
# so the egg states are the same builder's next draw
HAND_SEED = {"palm-egg": 6}
HAND_FORCE_SEED = 29                                 # the object forces of test_gpu_hand._physics_vs_oracle
_cache = {}


def candidates(mnp, sp, root, dof):
    """per env: the fp64 oracle's count of contact candidates (its list ends at 64)"""
    return np.array([len(O.contacts(mnp, sp, np.asarray(root[i]).ravel(), dof[i], 64)) for i in range(len(root))])


class LocoStep:
    """a locomotion task's states, k, and the fp64 oracle's simulate at max_contacts = k and with room for all"""

    def __init__(self, task, n, k):
        self.spec, sp, self.tp, self.mnp, self.root, self.dof, self.act = CR.task_set(task, n)
        self.n, self.k, self.sp = n, k, CR.with_max_contacts(sp, k)
        self.before = candidates(self.mnp, sp, self.root, self.dof)
        self.ref = self.simulate(self.sp)
        self.roomy = self.simulate(sp)

    def simulate(self, sp, fp32=False):
        """(root, dof, sensors, dof force) after one simulate"""
        r, d = self.root.copy(), self.dof.copy()
        s = np.zeros((self.n, max(len(self.spec.sensors), 1) * 6), np.float32)
        f = np.zeros((self.n, self.spec.num_dofs), np.float32)
        O.simulate(self.mnp, sp, r, d, self.act, s, f, threads=8, fp32=fp32)
        return r, d, s, f

    def outside(self, got, ref=None):
        """per env: outside the one-step tolerances of test_gpu_parity's physics step (positions 2e-4, velocities
        2e-3 + 2e-3 |v|, sensors and DOF forces 1 % of the batch's largest), as [(name, got, ref, atol, rtol)]"""
        rg, dg, sg, fg = got
        r_h, d_h, s_h, f_h = ref or self.ref
        return [("root pose", rg[:, 0:7], r_h[:, 0:7], 2e-4, 0), ("dof pos", dg[..., 0], d_h[..., 0], 2e-4, 0),
                ("root twist", rg[:, 7:13], r_h[:, 7:13], 2e-3, 2e-3), ("dof vel", dg[..., 1], d_h[..., 1], 2e-3, 2e-3),
                ("sensors", sg, s_h, 1e-2 * max(1.0, np.abs(s_h).max()), 0),
                ("dof force", fg, f_h, 1e-2 * max(1.0, np.abs(f_h).max()), 0)]

    def cut_moves(self):
        """per env: the oracle's step with the task's own capacity leaves the tolerances of its step at k"""
        bad = np.zeros(self.n, bool)
        for _, a, b, atol, rtol in self.outside(self.roomy):
            bad |= PS.env_bad(a, b, atol, rtol)
        return bad

    def compare(self, test, got):
        for x in got:
            assert np.isfinite(x).all()
        bad = np.zeros(self.n, bool)
        for name, a, b, atol, rtol in self.outside(got):
            eb = PS.env_bad(a, b, atol, rtol)
            PS.record(test, name, a, b, envs_outside=int(eb.sum()), atol=atol, rtol=rtol)
            bad |= eb
        pre = O.HostEnv(self.tp, self.spec, self.n)
        pre.root[:], pre.dof[:], pre.act_eff[:] = self.root, self.dof, self.act
        flags = PS.step_flags(self.mnp, self.sp, pre)
        rec = PS.assert_steps_explained(test, bad[None], flags[None], sens=None, allow_unexplained=0.0)
        PS._REPORT[test]["counts"] = {"over_capacity": int((self.before > self.k).sum()),
                                      "most": int(self.before.max()), "cut_moves_oracle": int(self.cut_moves().sum())}
        return rec


def loco_step(task, n, k):
    if ("loco", task, n, k) not in _cache:
        _cache["loco", task, n, k] = LocoStep(task, n, k)
    return _cache["loco", task, n, k]


FUSED = ("Humanoid", 128, 4)    # one teacher-forced fused step (observations: sensors and DOF forces) at max_contacts 4
FUSED_SEED = 7                  # contacts_ref.task_set's rollout seed: the step continues it


def fused_input(task, n):
    """(spec, sp, tp, mnp, HostEnv, step index, actions) for one more control step after contacts_ref.task_set's
    rollout (the same rollout, kept as a HostEnv with its task buffers)"""
    if ("fused", task, n) not in _cache:
        from test_gpu_parity import setup
        from migym import model as M
        spec, sp, tp = setup(task)
        mnp = M.pack_model(spec)
        h = O.HostEnv(tp, spec, n)
        rng = np.random.default_rng(23)
        for t in range(CR.TASK_ROLLOUT[task]):
            h.actions[:] = rng.uniform(-1.0, 1.0, (n, tp.num_actions)).astype(np.float32)
            h.env_step(mnp, sp, tp, seed=FUSED_SEED, step=t, threads=8)
        np.testing.assert_array_equal(h.root, CR.task_set(task, n)[4])
        acts = rng.uniform(-1.0, 1.0, (n, tp.num_actions)).astype(np.float32)
        _cache["fused", task, n] = spec, sp, tp, mnp, h, CR.TASK_ROLLOUT[task], acts
    spec, sp, tp, mnp, h, t, acts = _cache["fused", task, n]
    return spec, sp, tp, mnp, copy.deepcopy(h), t, acts


# ------------------------------------------------------------------------------------------------ hand
def hand_states(name):
    """(spec, sp, mnp, HandHostEnv, candidate counts) of a hand set: contacts_ref.hand_set's, or the same recipe
    drawn with HAND_SEED"""
    if ("hand", name) not in _cache:
        if name in HAND_SEED:
            import test_gpu_hand as H
            from migym import model as M
            kind = name.split("-")[1]
            spec, sp, tp = H.setup(kind=kind)
            h = H.hand_states(spec, tp, 256, np.random.default_rng(HAND_SEED[name]), H.PALM_DZ[kind], pen=kind == "pen")
            mnp = M.pack_model(spec)
        else:
            spec, sp, mnp, _, _, h = CR.hand_set(name)
        _cache["hand", name] = spec, sp, mnp, h, candidates(mnp, sp, h.root.reshape(h.n, -1), h.dof)
    return _cache["hand", name]


def hand_input(name, k):
    """(spec, sp at max_contacts k, mnp, a fresh HandHostEnv of the set's states, candidate counts)"""
    spec, sp, mnp, h, before = hand_states(name)
    return spec, CR.with_max_contacts(sp, k), mnp, copy.deepcopy(h), before


def hand_twin_compare(test, name, k):
    """the checks of test_gpu_hand._physics_vs_oracle with the oracle's fp32 twin in the kernel's place"""
    spec, sp, mnp, h, before = hand_input(name, k)
    n = h.n
    rng = np.random.default_rng(HAND_FORCE_SEED)
    h.rb_forces[: n // 2, len(spec.bodies)] = rng.normal(0, 0.3, (n // 2, 3))
    h.ncf = np.zeros((n, len(spec.bodies) + 2, 3), np.float32)
    h0, g = copy.deepcopy(h), copy.deepcopy(h)
    h.simulate(mnp, sp, threads=8)
    g.simulate(mnp, sp, threads=8, fp32=True)
    roomy = copy.deepcopy(h0)
    roomy.simulate(mnp, hand_states(name)[1], threads=8)
    scale, ncf_scale = max(1.0, np.abs(h.sensors).max()), max(1.0, np.abs(h.ncf).max())

    def checks(x):
        return [("net contact forces", x.ncf, h.ncf, 1e-2 * ncf_scale, 0),
                ("object pose", x.root[:, 1, 0:7], h.root[:, 1, 0:7], 2e-4, 0),
                ("object twist", x.root[:, 1, 7:13], h.root[:, 1, 7:13], 2e-3, 2e-3),
                ("dof pos", x.dof[..., 0], h.dof[..., 0], 2e-4, 0),
                ("dof vel", x.dof[..., 1], h.dof[..., 1], 2e-3, 2e-3),
                ("dof force", x.dof_force, h.dof_force, 1e-2, 1e-2), ("rigid bodies", x.rbs, h.rbs, 2e-3, 2e-3),
                ("sensors", x.sensors, h.sensors, 1e-2 * scale, 0)]
    bad, moves = np.zeros(n, bool), np.zeros(n, bool)
    for name_, a, b, atol, rtol in checks(g):
        eb = PS.env_bad(a, b, atol, rtol)
        PS.record(test, name_, a, b, envs_outside=int(eb.sum()), atol=atol, rtol=rtol)
        bad |= eb
    for _, a, b, atol, rtol in checks(roomy):
        moves |= PS.env_bad(a, b, atol, rtol)
    rec = PS.assert_steps_explained(test, bad[None], PS.step_flags(mnp, sp, h0)[None])
    rec["over_capacity"], rec["cut_moves_oracle"] = int((before > k).sum()), int(moves.sum())
    PS._REPORT[test]["counts"] = {"over_capacity": rec["over_capacity"], "most": int(before.max()),
                                  "cut_moves_oracle": rec["cut_moves_oracle"]}
    return rec
