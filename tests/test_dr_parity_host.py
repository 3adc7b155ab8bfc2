"""The cases of the domain-randomization GPU tests (tests/test_gpu_dr.py) on the CPU: the oracle's fp32 twin in place
of the GPU, through the same rules.

The GPU tests accept an env outside the tolerances only where orc_step_flips (evaluated with the env's own env_props
row) flags its step or the fp64 oracle is itself sensitive there, and only while the flags reach at most REACH_CAP of
the env-steps and the sensitivity fallback at most SENS_CAP.  All three are properties of the inputs and the oracle,
so they are pinned here without a GPU: the oracle's fp32 build (the same C in float, rounding unlike the kernel and
unlike the fp64 checker) takes the identical inputs through the identical rule and must end with no unexplained env
and both caps held.  Each case's seed is the first from dr_ref.SEED_BASE at which that holds (written next to the
case in tests/dr_ref.py); the rule's numbers are the project's own and never move.

Also pinned: what the rows reach.  random_props perturbs the effort limit where the model has one -- the ShadowHand's
position drives; the locomotion models and the trees are torque-actuated, their effort column is 0, unused by the
oracle and the kernel alike, and stays 0 -- and in every hand case some env starts a step with a drive saturated at
its row's limit where the model's own limit would decide otherwise; and the same inputs stepped without the rows end
elsewhere in more than half of the envs.
"""
import copy

import numpy as np
import pytest

import dr_ref as R
import parity_stats as PS
from migym import model as M


def _within_caps(rec):
    assert rec["unexplained"] == 0
    assert rec["flagged_reach"] <= PS.REACH_CAP
    assert rec["explained_by_sensitivity"] <= PS.SENS_CAP * rec["env_steps"]


@pytest.mark.parametrize("name", list(R.FUSED))
def test_fp32_twin_dr_fused_step_matches_oracle(name):
    spec, sp, tp, h, acts = R.fused_case(name)
    assert h.env_props is not None and h.n == R.FUSED[name][1]
    hand = name in R.HAND_FUSED
    h0 = copy.deepcopy(h)
    rec = R.twin_teacher_forced(f"test_fp32_twin_dr_fused_step_matches_oracle[{name}]", spec, sp, tp, h, acts, hand)
    _within_caps(rec)
    assert rec["resets"] > 0, "no reset inside the run: the device-RNG reset path would go unchecked"
    # the rows matter: the last step without them ends elsewhere in more than half of the envs
    pre = R.final_step_input(spec, sp, tp, h0, acts)
    dr = R.oracle_final_step(spec, sp, tp, pre, props=True).obs
    assert R.agreement(R.oracle_final_step(spec, sp, tp, pre, props=False).obs, dr, 2e-3, 2e-3) < 0.5


@pytest.mark.parametrize("name", list(R.SIM))
def test_fp32_twin_dr_one_step_matches_oracle(name):
    spec, sp, pre, ref = R.sim_case(name)
    assert pre.n == (66 if name[0] == "T" else 67)
    _within_caps(R.twin_one_step(f"test_fp32_twin_dr_one_step_matches_oracle[{name}]", name))
    assert np.abs(ref.dof[..., 0] - pre.dof[..., 0]).max() > 1e-3, "the step moved nothing"
    plain = R.DrTreeHost(spec, pre.root, pre.dof, pre.act_eff, None).simulate(M.pack_model(spec), sp)
    assert R.agreement(plain.dof[..., 1], ref.dof[..., 1], 2e-3, 2e-3) < 0.5


def _saturated(spec, h, limit):
    """per (env, DOF): a position drive whose explicit force kp (target - q) - b qd, with the row's kp and damping,
    exceeds `limit` (oracle_physics.c dof_term: then a constant +-limit force)"""
    W, nn = R.W, len(spec.nodes)
    p = h.env_props
    kp, b = p[:, 6:W * nn:W][:, 1:], p[:, 2:W * nn:W][:, 1:]
    fe = kp * (h.targets - h.dof[..., 0]) - b * h.dof[..., 1]
    return (kp > 0) & (np.abs(fe) > limit[:, 1:])


@pytest.mark.parametrize("name", list(R.FUSED))
def test_effort_column_is_randomized_and_reached(name):
    """the effort column of random_props differs from the model's wherever the model has a limit, and in the hand
    cases a drive starts a teacher-forced step saturated under its row's limit but not under the model's, or the
    other way round (the column decides the step).  The locomotion models have no position drive and no effort limit
    (kp = effort = 0 on every node): their column stays the model's and neither side reads it."""
    spec, sp, tp, h, acts = R.fused_case(name)
    rows, base = R.effort_columns(spec, h.env_props)
    has = base > 0
    assert np.array_equal(rows[:, ~has], np.tile(base[~has], (h.n, 1)))
    if name not in R.HAND_FUSED:
        assert not has.any() and all(x.drive_kp == 0 for x in spec.nodes)
        return
    assert has.sum() >= 20 and (rows[:, has] != base[has]).all()
    r = rows[:, has] / base[has]
    assert r.min() >= 0.5 - 1e-6 and r.max() <= 1.5 + 1e-6 and r.std() > 0.2
    mnp = M.pack_model(spec)
    decided = at_limit = 0
    for t in range(R.FUSED_STEPS):
        h.actions[:] = acts[t]
        g = PS.hand_physics_input(h, mnp, tp, R.STEP_SEED, t)
        row_sat, base_sat = _saturated(spec, g, rows), _saturated(spec, g, np.tile(base, (h.n, 1)))
        at_limit += int(row_sat.any(axis=1).sum())
        decided += int((row_sat != base_sat).any(axis=1).sum())
        h.env_step(mnp, sp, tp, seed=R.STEP_SEED, step=t, threads=8)
    assert at_limit >= 1 and decided >= 1, (at_limit, decided)
