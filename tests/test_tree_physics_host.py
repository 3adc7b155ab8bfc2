"""The cases of tests/test_gpu_tree_physics.py on the CPU: what their inputs are, and the oracle's fp32 twin in place
of the GPU.

The GPU test accepts an env outside the one-step tolerances only where orc_step_flips puts its step at a
discontinuity, and only while such flags reach at most 5 % of the envs (parity_stats.assert_steps_explained).  Both
are conditions on the inputs, so they are pinned here, without a GPU: the oracle's fp32 build (liboracle_f32.so, the
same C in float, rounding unlike the kernel and unlike the fp64 checker) steps the identical states and goes through
the identical comparison (tree_physics_ref.compare).  It must end with no unexplained env and the flags within the
cap, for every case, state kind and actor count the GPU test runs; the states' seeds and recipe
(tree_physics_ref.states) were fixed against this test, never the rule.

Past capacity (the overflow states, and the dropped states at a lowered max_contacts) the same holds, and two more
conditions on the inputs are pinned: every overflow state has more candidates than max_contacts, and in at least
half of them the cut moves the fp64 oracle's own result beyond the tolerances.
"""
import numpy as np
import pytest

import dynamics_ref as D
import parity_stats as PS
import tree_physics_ref as TP
from migym import model as M


def _twin(case, kind, n, tgs=False, cap=None):
    spec, sp = TP.spec_of(case), TP.sim_params(case, tgs, cap)
    root, dof, act, _ = TP.states(case, kind, tgs, cap)
    return TP.TreeHost(spec, root[:n], dof[:n], act[:n]).simulate(M.pack_model(spec), sp, fp32=True)


@pytest.mark.parametrize("n", TP.ACTOR_COUNTS)
@pytest.mark.parametrize("kind", TP.KINDS)
@pytest.mark.parametrize("name", list(TP.CASES))
def test_fp32_twin_step_matches_oracle(name, kind, n):
    case = TP.CASES[name]
    got = _twin(case, kind, n)
    ref = TP.states(case, kind)[3]
    assert np.abs(got.dof[..., 1] - ref.dof[:n, :, 1]).max() > 0   # two implementations, not one
    rec = TP.compare(f"test_fp32_twin_step_matches_oracle[{name}-{kind}-{n}]", case, kind, n, got)
    assert rec["unexplained"] == 0 and rec["flagged_reach"] <= PS.REACH_CAP


@pytest.mark.parametrize("name", TP.TGS_CASES)
def test_fp32_twin_tgs_step_matches_oracle(name):
    case = TP.CASES[name]
    got = _twin(case, "dropped", TP.CASE_ACTORS, tgs=True)
    rec = TP.compare(f"test_fp32_twin_tgs_step_matches_oracle[{name}]", case, "dropped", TP.CASE_ACTORS, got, tgs=True)
    assert rec["unexplained"] == 0 and rec["flagged_reach"] <= PS.REACH_CAP
    # the solver really is another one: the same states under PGS end elsewhere
    assert np.abs(got.dof[..., 1] - TP.pgs_step_of_tgs_states(case, "dropped").dof[..., 1]).max() > 1e-2


# ------------------------------------------------------------------------------------------------ past capacity
@pytest.mark.parametrize("n", TP.ACTOR_COUNTS)
@pytest.mark.parametrize("name", TP.OVERFLOW_CASES)
def test_fp32_twin_overflow_step_matches_oracle(name, n):
    """more candidates than max_contacts = the instance's MC: the twin keeps the oracle's prefix of the list"""
    case = TP.CASES[name]
    got = _twin(case, "overflow", n)
    rec = TP.compare(f"test_fp32_twin_overflow_step_matches_oracle[{name}-{n}]", case, "overflow", n, got)
    assert rec["unexplained"] == 0 and rec["flagged_reach"] <= PS.REACH_CAP


@pytest.mark.parametrize("n", TP.ACTOR_COUNTS)
@pytest.mark.parametrize("name,cap", TP.LOWERED)
def test_fp32_twin_lowered_capacity_step_matches_oracle(name, cap, n):
    """the dropped states with max_contacts lowered below the instance's MC"""
    case = TP.CASES[name]
    got = _twin(case, "dropped", n, cap=cap)
    rec = TP.compare(f"test_fp32_twin_lowered_capacity_step_matches_oracle[{name}-{cap}-{n}]", case, "dropped", n, got,
                     cap=cap)
    assert rec["unexplained"] == 0 and rec["flagged_reach"] <= PS.REACH_CAP


def test_fp32_twin_tgs_overflow_step_matches_oracle():
    case = TP.CASES["T32-free"]
    got = _twin(case, "overflow", TP.CASE_ACTORS, tgs=True)
    rec = TP.compare("test_fp32_twin_tgs_overflow_step_matches_oracle", case, "overflow", TP.CASE_ACTORS, got, tgs=True)
    assert rec["unexplained"] == 0 and rec["flagged_reach"] <= PS.REACH_CAP
    assert np.abs(got.dof[..., 1] - TP.pgs_step_of_tgs_states(case, "overflow").dof[..., 1]).max() > 1e-2
    assert 2 * TP.truncation_moves(case, "overflow", tgs=True).sum() >= TP.CASE_ACTORS


def _record_counts(key, before, cap, moves):
    PS._REPORT.setdefault(key, {})["counts"] = {"over_capacity": int((before > cap).sum()), "most": int(before.max()),
                                                "cut_moves_oracle": int(moves.sum())}


@pytest.mark.parametrize("name", TP.OVERFLOW_CASES)
def test_overflow_states_are_past_capacity_and_the_cut_matters(name):
    """every overflow state has more candidates than max_contacts (= the instance's MC) and fewer than the oracle can
    count; in at least half of them the fp64 oracle's own step with room for every candidate leaves the tolerances
    of its step at capacity, so a kernel that ignored the cut would fail"""
    case = TP.CASES[name]
    before = TP.candidates_before(case, "overflow")
    assert len(before) == TP.CASE_ACTORS
    assert before.min() > case.max_contacts and before.max() < TP.ORACLE_MAXC, (before.min(), before.max())
    moves = TP.truncation_moves(case, "overflow")
    _record_counts(f"overflow inputs[{name}]", before, case.max_contacts, moves)
    assert 2 * moves.sum() >= TP.CASE_ACTORS, f"{name}: the cut matters to the oracle in only {moves.sum()} states"


# (envs over the lowered capacity, envs where the cut moves the oracle's result): pinned, the states are seeded
LOWERED_COUNTS = {("T16-fixed", 8): (17, 17), ("T32-free", 8): (22, 19)}


@pytest.mark.parametrize("name,cap", TP.LOWERED)
def test_lowered_capacity_cuts_the_dropped_states(name, cap):
    case = TP.CASES[name]
    before = TP.candidates_before(case, "dropped")
    moves = TP.truncation_moves(case, "dropped", cap=cap)
    _record_counts(f"overflow inputs[{name}-{cap}]", before, cap, moves)
    assert not moves[before <= cap].any()   # a list that fits is left alone
    assert (int((before > cap).sum()), int(moves.sum())) == LOWERED_COUNTS[name, cap]


@pytest.mark.parametrize("name", list(TP.CASES))
def test_case_inputs_reach_their_paths(name):
    """the spec is past the next smaller instance, every state within capacity, and the states reach what the case
    is there for"""
    TP.assert_case_inputs(TP.CASES[name])


def test_step_options_leave_the_tree_unchanged():
    """random_tree's step options draw from a generator of their own: nodes and bodies equal the plain tree's in
    every field the plain tree sets"""
    plain = D.random_tree(17, 1)
    full = D.random_tree(17, 1, physics=True, num_geoms=20, num_pairs=8, num_sensors=4)
    for a, b in zip(plain.nodes, full.nodes):
        for k in ("parent", "jtype", "t", "r0", "axis", "body", "mass", "com", "inertia", "armature", "lower", "upper",
                  "limited"):
            assert getattr(a, k) == getattr(b, k)
    assert plain.bodies == full.bodies
    assert not plain.geoms and not plain.pairs and not plain.sensors and plain.gravity_off == 1
    assert len(full.geoms) == 20 and len(full.pairs) == 8 and len(full.sensors) == 4 and full.gravity_off == 0
    free = D.random_tree(17, 1, free_base=True)
    assert free.fixed_base == 0 and free.nodes[0].jtype == M.JT_FREE and free.nodes[0].mass > 0
