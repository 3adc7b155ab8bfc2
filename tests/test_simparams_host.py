"""The (model, point) pairs of tests/test_gpu_simparams.py on the CPU: the admission rule of tests/simparams_ref.py,
with the oracle's fp32 twin in place of the GPU.

Every pair the GPU test runs goes through the identical comparison here (tree_physics_ref.compare for the trees,
simparams_ref.task_compare / hand_compare for the task models) with the fp32 build of the oracle as the implementation
under test: 0 unexplained envs, flags within parity_stats.REACH_CAP.  The conditions on the inputs are asserted too:
the fp64 oracle's own result at the point leaves the tolerances of its result at the task's parameters in at least a
quarter of the states (5 on the trees at limit_margin 0), so a kernel that ignored the field would fail; and no state
has more contact candidates than max_contacts, before or after the step.  The per-pair figures go to the parity
report (MIGYM_PARITY_REPORT) under "simparams inputs[...]".

The GPU test's 6-actor repeats (the trees at substeps4 and tgs2-6) are not repeated here: this file's time is the
36 selections of tree states, and the 6 are a prefix of the 66, unflagged by construction
(tree_physics_ref.states).
"""
import numpy as np
import pytest

import parity_stats as PS
import simparams_ref as SR
import tree_physics_ref as TP
from migym import model as M

KIND = "dropped"


def _inputs(model, point, n, moved, before, after, cap):
    PS._REPORT.setdefault(f"simparams inputs[{model}-{point}]", {})["counts"] = {
        "envs": int(n), "moved": int(moved.sum()), "most_candidates": int(max(before.max(), after.max())),
        "max_contacts": int(cap)}
    assert moved.sum() >= SR.moved_floor(model, point, n), f"{model}/{point}: the oracle moves in {moved.sum()} of {n}"
    assert max(before.max(), after.max()) <= cap, f"{model}/{point}: {max(before.max(), after.max())} candidates"


def _tree_twin(case, point, n):
    spec = TP.spec_of(case)
    root, dof, act, _ = TP.states(case, KIND, point=point)
    return TP.TreeHost(spec, root[:n], dof[:n], act[:n]).simulate(M.pack_model(spec), TP.sim_params(case, point=point),
                                                                  fp32=True)


@pytest.mark.parametrize("name,point", SR.pairs(SR.TREE_CASES))
def test_fp32_twin_tree_step_matches_oracle_at_point(name, point):
    case = TP.CASES[name]
    n = TP.CASE_ACTORS
    got = _tree_twin(case, point, n)
    rec = TP.compare(f"test_fp32_twin_tree_step_matches_oracle_at_point[{name}-{point}]", case, KIND, n, got,
                     point=point)
    assert rec["unexplained"] == 0 and rec["flagged_reach"] <= PS.REACH_CAP
    spec, mnp = TP.spec_of(case), M.pack_model(TP.spec_of(case))
    root, dof, act, ref = TP.states(case, KIND, point=point)
    sp = TP.sim_params(case, point=point)
    assert sp.max_contacts == case.max_contacts
    base = TP.TreeHost(spec, root, dof, act).simulate(mnp, TP.sim_params(case))
    _inputs(name, point, n, SR.moved(ref, base, TP.outside), np.abs(TP.num_candidates(mnp, sp, root, dof)),
            np.abs(TP.num_candidates(mnp, sp, ref.root, ref.dof)), case.max_contacts)


@pytest.mark.parametrize("task,point", SR.pairs(tuple(SR.TASKS)))
def test_fp32_twin_task_step_matches_oracle_at_point(task, point):
    rec = SR.task_compare(f"test_fp32_twin_task_step_matches_oracle_at_point[{task}-{point}]", task, point,
                          SR.task_twin(task, point))
    assert rec["unexplained"] == 0 and rec["flagged_reach"] <= PS.REACH_CAP
    root, _, _, ref, base = SR.task_states(task, point)
    before, after = SR.task_candidates(task, point)
    _inputs(task, point, len(root), SR.moved(ref, base, SR.task_outside), before, after,
            SR.task_sim_params(task, point).max_contacts)


@pytest.mark.parametrize("model,point", SR.pairs((SR.HAND,)))
def test_fp32_twin_hand_step_matches_oracle_at_point(model, point):
    rec = SR.hand_compare(f"test_fp32_twin_hand_step_matches_oracle_at_point[{point}]", point, SR.hand_twin(point))
    assert rec["unexplained"] == 0 and rec["flagged_reach"] <= PS.REACH_CAP
    h0, ref, base = SR.hand_states(point)
    before, after = SR.hand_candidates(point)
    _inputs(model, point, h0.n, SR.moved(ref, base, SR.hand_outside), before, after,
            SR.hand_sim_params(point).max_contacts)
    # tilted gravity reaches the free object: its own velocity moves, not the fingers' alone
    if point == "gravity":
        assert np.abs(ref.root[:, 1, 7:9] - base.root[:, 1, 7:9]).max() > 1e-2


@pytest.mark.parametrize("point", list(SR.FUSED))
@pytest.mark.parametrize("task,n", SR.FUSED_CASES)
def test_fused_inputs_are_admitted(task, n, point):
    """the inputs of the fused-step tests: the flags of the teacher-forced steps reach at most REACH_CAP of the
    env-steps, and the fp32 twin leaves the fused tolerances in no unflagged env-step"""
    flags, twin_bad = SR.fused_flags(task, n, point)
    PS._REPORT.setdefault(f"simparams fused inputs[{task}-{point}]", {})["counts"] = {
        "env_steps": int(flags.size), "flagged_reach": float((flags != 0).mean()),
        "twin_disagreeing": int(twin_bad.sum()), "twin_unflagged": int((twin_bad & (flags == 0)).sum())}
    assert (flags != 0).mean() <= PS.REACH_CAP, f"{task}/{point}: the flags reach {(flags != 0).mean():.3f}"
    assert not (twin_bad & (flags == 0)).any()


def test_points_and_pairs():
    """the twelve points; every pair is admitted or listed as left out; apply() leaves its argument alone and None
    returns it untouched"""
    assert len(SR.POINTS) == 12
    assert len(SR.pairs()) + len(SR.LEFT_OUT) == 3 * 12 + 2 * 12 + 3 + len(SR.HAND_POINTS)
    sp = TP.sim_params(TP.CASES["T16-free"])
    assert SR.apply(sp, None) is sp
    for point, f in SR.POINTS.items():
        moved = SR.apply(sp, point)
        assert (sp.substeps, sp.pos_iters, sp.friction, sp.baumgarte) == (2, 4, 1.0, np.float32(0.2))   # untouched
        for k, v in f.items():
            got = tuple(moved.gravity) if k == "gravity" else getattr(moved, k)
            assert got == (v if k == "gravity" else type(got)(np.float32(v) if isinstance(v, float) else v)), (point, k)
        same = [k for k, _ in sp._fields_ if k not in f and k != "gravity"]
        assert all(getattr(moved, k) == getattr(sp, k) for k in same)
