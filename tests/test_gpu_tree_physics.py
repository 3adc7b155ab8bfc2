"""mg_sim_simulate on the three step-kernel instances that no task model selects, against the fp64 oracle.

csrc/dispatch.hpp builds eleven instances of the step kernel (T team lanes, MN nodes, MC contacts, MG geoms, MP
pairs, OBJ, LAY), and mg_sim_create launches the smallest that fits.  A GPU test that launches each:

  (8, 4, 8, 4, 0)                      Cartpole: test_gpu_parity.test_physics_step_matches_oracle[Cartpole-*]
  (16, 9, 16, 16, 0) classic           Ant, MA-Ant: test_gpu_parity.test_physics_step_matches_oracle[Ant-*]
  (16, 9, 16, 16, 0) compact           test_gpu_parity.test_pinned_layout_matches_oracle[Ant-256-compact]
  (16, 16, 24, 24, 32)                 here: T16-fixed, T16-free
  (32, 24, 32, 24, 160) classic        Humanoid: test_gpu_parity.test_physics_step_matches_oracle[Humanoid-*]
  (32, 24, 32, 24, 160) compact        test_gpu_parity.test_pinned_layout_matches_oracle[Humanoid-128-compact]
  (32, 32, 48, 48, 192)                here: T32-fixed, T32-free
  (64, 40, 48, 48, 192)                here: T64-fixed, T64-fixed-chain, T64-free
  (32, 25, 24, 24, 24, box)            ShadowHand block: test_gpu_hand.test_hand_physics_step_matches_oracle[block]
  (32, 25, 24, 24, 24, capsule)        ShadowHand pen: test_gpu_hand.test_hand_physics_step_matches_oracle[pen]
  (32, 25, 24, 24, 24, ellipsoid)      ShadowHand egg: test_gpu_hand.test_hand_physics_step_matches_oracle[egg]

The cases (tests/tree_physics_ref.py) are synthetic trees with gravity, joint damping / stiffness / frictionloss,
sphere / capsule / box geoms on the ground, self pairs and sensors, fixed and free bases, chosen as the smallest
shapes that reach what the task models leave dead in csrc/team_physics.hpp: the one-actor-per-wave team (the
shfl_xor(., 32) halves of the team reductions, the full-wave masks); the second round of the lane-per-geom loops
(more geoms than lanes); box corners that touch the ground in the two-pass ground path; slides below hinges, hinges
below slides, slides in a free-base tree; a free base with more than 21 DOFs; a fixed base with several DOF chains;
limit and contact rows beyond the team's lanes.  Each case runs 1, 6 and 66 actors (a lone team; a partial wave at 4
and at 2 actors per wave; several blocks with a ragged tail), from dropped and from settled states, and once per
instance with the TGS solver.  Past contact capacity: the overflow states (max_contacts = MC, every candidate
list longer) on six of the cases, once with TGS, and the dropped states of two cases at max_contacts = 8.

One mg_sim_simulate from the states of the oracle's step; every env within the project's one-step tolerances
(positions 2e-4, velocities 2e-3 + 2e-3 |v|, DOF forces, sensors and net contact forces 1 % of the batch's largest)
unless orc_step_flips puts its step at a discontinuity, flags reaching at most 5 % of the envs, no sensitivity
fallback, nothing unexplained (tree_physics_ref.compare); a second run bit-identical; outputs finite; the states
moved.  tests/test_tree_physics_host.py puts the oracle's fp32 twin through the same comparison on the CPU, and
asserts what the inputs reach.

All of this runs at one point of mg_sim_params, the Ant's (tree_physics_ref.sim_params).  tests/test_gpu_simparams.py
takes T16-free, T32-fixed and T64-free (dropped states) to twelve other points -- substeps, tilted gravity, low and zero
friction, the depenetration clamp, rest_offset, 1 and 16 iterations, limit_margin 0, baumgarte, TGS with vel_iters --
through the same comparison (tree_physics_ref.compare(point=...)).
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import tree_physics_ref as TP
from migym import _abi, model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, torch.float32).contiguous()


def _gpu_step(lib, case, kind, n, tgs=False, cap=None):
    """(result, team lanes, compact) of one mg_sim_simulate of the case's first n states; a second simulate from the
    same states must be bit-identical.  cap: max_contacts lowered below the case's"""
    spec, sp = TP.spec_of(case), TP.sim_params(case, tgs, cap)
    mnp = M.pack_model(spec)
    root, dof, act, _ = TP.states(case, kind, tgs, cap)
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    runs = []
    try:
        t, lay = C.c_int32(), C.c_int32()
        _abi.check(lib.mg_sim_kernel_layout(sim, C.byref(t), C.byref(lay)), lib)
        for _ in range(2):
            h = TP.TreeHost(spec, root[:n], dof[:n], act[:n])
            d = {k: T(getattr(h, k)) for k in ("root", "dof", "act_eff", "sensors", "dof_force")}
            d["ncf"] = torch.full((n, len(spec.bodies), 3), float("nan"), device=DEV)   # every row must be written
            v = _abi.StateViews()
            v.root_states, v.dof_state, v.dof_actuation = d["root"].data_ptr(), d["dof"].data_ptr(), d["act_eff"].data_ptr()
            v.sensors, v.dof_force, v.net_contact_forces = d["sensors"].data_ptr(), d["dof_force"].data_ptr(), d["ncf"].data_ptr()
            _abi.check(lib.mg_sim_bind(sim, C.byref(v)), lib)
            _abi.check(lib.mg_sim_simulate(sim, torch.cuda.current_stream().cuda_stream), lib)
            torch.cuda.synchronize()
            runs.append(types.SimpleNamespace(**{k: x.cpu().numpy() for k, x in d.items()}))
    finally:
        lib.mg_sim_destroy(sim)
    for k in ("root", "dof", "sensors", "dof_force", "ncf"):
        np.testing.assert_array_equal(getattr(runs[0], k), getattr(runs[1], k), err_msg=f"{k}: the second run differs")
    return runs[0], t.value, lay.value


def _assert_instance(case, lanes, compact):
    """the intended instance ran, and the spec's counts keep the case off the next smaller one"""
    assert (lanes, compact) == (case.lanes, 0), f"{case.name()}: ran on the {lanes}-lane instance (compact {compact})"
    cnt = TP.counts(TP.spec_of(case))
    for what, more_than in case.past:
        assert cnt[what] > more_than, f"{case.name()}: {what} = {cnt[what]} fits a smaller instance (<= {more_than})"


@pytest.mark.parametrize("n", TP.ACTOR_COUNTS)
@pytest.mark.parametrize("kind", TP.KINDS)
@pytest.mark.parametrize("name", list(TP.CASES))
def test_tree_physics_step_matches_oracle(lib, name, kind, n):
    case = TP.CASES[name]
    got, lanes, compact = _gpu_step(lib, case, kind, n)
    _assert_instance(case, lanes, compact)
    if n == TP.CASE_ACTORS and kind == "dropped":
        TP.assert_case_inputs(case)
    TP.compare(f"test_tree_physics_step_matches_oracle[{name}-{kind}-{n}]", case, kind, n, got)


@pytest.mark.parametrize("name", TP.TGS_CASES)
def test_tree_tgs_physics_step_matches_oracle(lib, name):
    """the same with solver_type TGS (as tests/test_gpu_tgs.py), against the oracle's TGS"""
    case = TP.CASES[name]
    got, lanes, compact = _gpu_step(lib, case, "dropped", TP.CASE_ACTORS, tgs=True)
    _assert_instance(case, lanes, compact)
    pgs = TP.pgs_step_of_tgs_states(case, "dropped")
    assert np.abs(got.dof[..., 1] - pgs.dof[..., 1]).max() > 1e-2   # the TGS kernel ran: PGS ends elsewhere
    TP.compare(f"test_tree_tgs_physics_step_matches_oracle[{name}]", case, "dropped", TP.CASE_ACTORS, got, tgs=True)


# ------------------------------------------------------------------------------------------------ past capacity
# More contact candidates than max_contacts: collide() keeps the first cap = min(max_contacts, MC) of the emission
# order, as the oracle does.  The overflow states have max_contacts = MC, so slot cap is the first one past the
# per-team contact arrays in LDS; the lowered runs take the max_contacts < MC branch.  The rows, PGS / TGS, sensors,
# DOF forces and net contact forces all run on a full list.  tests/test_tree_physics_host.py asserts that the cut
# matters to the oracle itself in at least half of the overflow states.
@pytest.mark.parametrize("n", TP.ACTOR_COUNTS)
@pytest.mark.parametrize("name", TP.OVERFLOW_CASES)
def test_tree_overflow_step_matches_oracle(lib, name, n):
    case = TP.CASES[name]
    got, lanes, compact = _gpu_step(lib, case, "overflow", n)
    _assert_instance(case, lanes, compact)
    TP.compare(f"test_tree_overflow_step_matches_oracle[{name}-{n}]", case, "overflow", n, got)


@pytest.mark.parametrize("n", TP.ACTOR_COUNTS)
@pytest.mark.parametrize("name,cap", TP.LOWERED)
def test_tree_lowered_capacity_step_matches_oracle(lib, name, cap, n):
    case = TP.CASES[name]
    got, lanes, compact = _gpu_step(lib, case, "dropped", n, cap=cap)
    _assert_instance(case, lanes, compact)
    TP.compare(f"test_tree_lowered_capacity_step_matches_oracle[{name}-{cap}-{n}]", case, "dropped", n, got, cap=cap)


def test_tree_tgs_overflow_step_matches_oracle(lib):
    case = TP.CASES["T32-free"]
    got, lanes, compact = _gpu_step(lib, case, "overflow", TP.CASE_ACTORS, tgs=True)
    _assert_instance(case, lanes, compact)
    pgs = TP.pgs_step_of_tgs_states(case, "overflow")
    assert np.abs(got.dof[..., 1] - pgs.dof[..., 1]).max() > 1e-2   # the TGS kernel ran: PGS ends elsewhere
    TP.compare("test_tree_tgs_overflow_step_matches_oracle", case, "overflow", TP.CASE_ACTORS, got, tgs=True)
