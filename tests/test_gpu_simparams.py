"""The step kernels against the fp64 oracle away from the tasks' sim parameters (tests/simparams_ref.py).

Every other GPU-versus-oracle physics test runs at the mg_sim_params of a task YAML, so these branches of
csrc/team_physics.hpp see one value each under the rest of the suite: the depenetration clamp (build_rows, the limit
rows and once more inside the TGS sweep), the friction bound at low and at zero mu, the x and y components of gravity
(links and the hand's free object), the substep loops of k_simulate and of the two fused kernels, the vel_iters side
of the TGS sweep count, rest_offset, limit_margin 0 with limits on, and mg_sim_set_params.

  * One mg_sim_simulate per admitted (model, point) pair -- three trees, Ant and Humanoid in both layouts, Cartpole,
    the ShadowHand block -- by the project's one-step rule (tree_physics_ref.compare: positions 2e-4, velocities
    2e-3 + 2e-3 |v|, DOF forces / sensors / net contact forces 1 % of the batch's largest; flags may exempt, reach at
    most 5 %; nothing unexplained, no sensitivity fallback), a second run bit-identical, the instance and layout
    asserted.  tests/test_simparams_host.py admits the pairs on the CPU and puts the oracle's fp32 twin through the
    same comparison.
  * mg_env_step, teacher-forced for 2 steps, at substeps 1 and at substeps 4 with controlFrequencyInv 2 (8 substeps
    per launch): the nsub loops of csrc/step_kernels.hpp.
  * mg_sim_set_params moves a sim to a point and back bit for bit, and a refused call changes nothing.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import simparams_ref as SR
import test_gpu_hand as GH
import test_gpu_parity as GP
import tree_physics_ref as TP
from migym import _abi, model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MG_OK, MG_EINVAL = 0, -1     # include/migym.h
LANES = {"Cartpole": 8, "Ant": 16, "Humanoid": 32, SR.HAND: 32}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, torch.float32).contiguous()


class Sim:
    """an mg_sim of n envs; run(inputs) binds fresh device copies of a host's arrays and simulates once"""

    def __init__(self, lib, mnp, sp, n):
        self.lib, self.n, self.h = lib, n, C.c_void_p()
        _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(self.h)), lib)

    def layout(self):
        t, lay = C.c_int32(), C.c_int32()
        _abi.check(self.lib.mg_sim_kernel_layout(self.h, C.byref(t), C.byref(lay)), self.lib)
        return t.value, lay.value

    def run(self, host, nbodies):
        """one mg_sim_simulate from the first n envs of `host` (root, dof, act_eff): the outputs as numpy arrays"""
        n = self.n
        d = {"root": T(host.root[:n]), "dof": T(host.dof[:n]), "act_eff": T(host.act_eff[:n]),
             "sensors": torch.zeros_like(T(host.sensors[:n])), "dof_force": torch.zeros_like(T(host.dof_force[:n])),
             "ncf": torch.full((n, nbodies, 3), float("nan"), device=DEV)}   # every row must be written
        v = _abi.StateViews()
        v.root_states, v.dof_state, v.dof_actuation = d["root"].data_ptr(), d["dof"].data_ptr(), d["act_eff"].data_ptr()
        v.sensors, v.dof_force, v.net_contact_forces = d["sensors"].data_ptr(), d["dof_force"].data_ptr(), d["ncf"].data_ptr()
        _abi.check(self.lib.mg_sim_bind(self.h, C.byref(v)), self.lib)
        _abi.check(self.lib.mg_sim_simulate(self.h, torch.cuda.current_stream().cuda_stream), self.lib)
        torch.cuda.synchronize()
        return SR.result(**{k: x.cpu().numpy() for k, x in d.items()})

    def run_hand(self, h0):
        e = GH.DevHandEnv(h0)
        _abi.check(self.lib.mg_sim_bind(self.h, C.byref(e.views())), self.lib)
        _abi.check(self.lib.mg_sim_simulate(self.h, torch.cuda.current_stream().cuda_stream), self.lib)
        torch.cuda.synchronize()
        return SR.result(**{k: GH.np_(getattr(e, k)) for k in ("root", "dof", "sensors", "dof_force", "rbs", "ncf")})

    def set_params(self, sp):
        return self.lib.mg_sim_set_params(self.h, C.byref(sp))

    def close(self):
        self.lib.mg_sim_destroy(self.h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


FIELDS = ("root", "dof", "sensors", "dof_force", "ncf")


def assert_same_bits(a, b, what, fields=FIELDS):
    for k in fields:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{k}: {what}")


def differs(a, b, fields=FIELDS):
    return any(not np.array_equal(getattr(a, k), getattr(b, k)) for k in fields)


# ------------------------------------------------------------------------------------------------ one step per pair
def _tree_step(lib, name, point, n):
    case = TP.CASES[name]
    spec = TP.spec_of(case)
    root, dof, act, _ = TP.states(case, "dropped", point=point)
    host = TP.TreeHost(spec, root, dof, act)
    with Sim(lib, M.pack_model(spec), TP.sim_params(case, point=point), n) as sim:
        assert sim.layout() == (case.lanes, 0), f"{name}: ran on {sim.layout()}"
        got, again = sim.run(host, len(spec.bodies)), sim.run(host, len(spec.bodies))
    assert_same_bits(got, again, "the second run differs")
    return case, got


@pytest.mark.parametrize("name,point", SR.pairs(SR.TREE_CASES))
def test_tree_step_matches_oracle_at_point(lib, name, point):
    case, got = _tree_step(lib, name, point, TP.CASE_ACTORS)
    TP.compare(f"test_tree_step_matches_oracle_at_point[{name}-{point}]", case, "dropped", TP.CASE_ACTORS, got,
               point=point)


@pytest.mark.parametrize("point", SR.SMALL_POINTS)
@pytest.mark.parametrize("name", SR.TREE_CASES)
def test_tree_step_matches_oracle_at_point_partial_wave(lib, name, point):
    """SMALL_N actors: a partial wave at 4 and at 2 actors per wave, at the longest substep loop and at TGS"""
    case, got = _tree_step(lib, name, point, TP.SMALL_N)
    TP.compare(f"test_tree_step_matches_oracle_at_point_partial_wave[{name}-{point}]", case, "dropped", TP.SMALL_N, got,
               point=point)


def _task_cases():
    out = []
    for task, point in SR.pairs(tuple(SR.TASKS)):
        out += [(task, point, lay) for lay in (("auto",) if task == "Cartpole" else ("classic", "compact"))]
    return out


@pytest.mark.parametrize("task,point,layout", _task_cases())
def test_task_step_matches_oracle_at_point(lib, task, point, layout, monkeypatch):
    """the task models at a point, the locomotion models in both team layouts (MIGYM_LAYOUT, as
    test_gpu_parity.test_pinned_layout_matches_oracle pins them)"""
    monkeypatch.setenv("MIGYM_LAYOUT", layout)
    spec, mnp, _, _ = SR.task_setup(task)
    root, dof, act, _, _ = SR.task_states(task, point)
    host = SR.task_host(task, root, dof, act)
    with Sim(lib, mnp, SR.task_sim_params(task, point), len(root)) as sim:
        assert sim.layout() == (LANES[task], int(layout == "compact")), f"{task}: ran on {sim.layout()}"
        got, again = sim.run(host, len(spec.bodies)), sim.run(host, len(spec.bodies))
    assert_same_bits(got, again, "the second run differs")
    SR.task_compare(f"test_task_step_matches_oracle_at_point[{task}-{point}-{layout}]", task, point, got)


HAND_FIELDS = ("root", "dof", "sensors", "dof_force", "rbs", "ncf")


@pytest.mark.parametrize("model,point", SR.pairs((SR.HAND,)))
def test_hand_step_matches_oracle_at_point(lib, model, point):
    """the ShadowHand block on the palm; tilted gravity reaches the free object's own gravity term"""
    spec, mnp, _, _ = SR.hand_setup()
    h0 = SR.hand_states(point)[0]
    with Sim(lib, mnp, SR.hand_sim_params(point), h0.n) as sim:
        assert sim.layout() == (LANES[SR.HAND], 0)
        got, again = sim.run_hand(h0), sim.run_hand(h0)
    assert_same_bits(got, again, "the second run differs", HAND_FIELDS)
    SR.hand_compare(f"test_hand_step_matches_oracle_at_point[{point}]", point, got)


# ------------------------------------------------------------------------------------------------ the fused step
@pytest.mark.parametrize("point", list(SR.FUSED))
@pytest.mark.parametrize("task,n,layout", [("Ant", 256, "compact"), ("Humanoid", 128, "auto")])
def test_fused_env_step_matches_oracle_at_substeps(lib, task, n, layout, point, monkeypatch):
    """mg_env_step over 2 teacher-forced control steps from test_physics_step_matches_oracle's random states (half of
    them in contact), no reset pending: nsub = substeps x controlFrequencyInv = 1 and 8"""
    assert (task, n) in SR.FUSED_CASES
    monkeypatch.setenv("MIGYM_LAYOUT", layout)
    spec, sp, tp = SR.fused_setup(task, point)
    if layout != "auto":
        assert GP.kernel_layout(lib, spec, sp, n) == (LANES[task], 1)
    h, acts = SR.fused_input(task, n, point)
    GP._teacher_forced(lib, f"test_fused_env_step_matches_oracle_at_substeps[{task}-{point}]", spec, sp, tp, h,
                       SR.FUSED_STEPS, acts, seed=SR.FUSED_RNG_SEED)


@pytest.mark.parametrize("point", list(SR.FUSED))
def test_hand_fused_env_step_matches_oracle_at_substeps(lib, point):
    """the same on the ShadowHand block, 128 envs from the palm states, no reset pending"""
    n = 128
    assert (SR.HAND, n) in SR.FUSED_CASES
    spec, sp, tp = SR.fused_setup(SR.HAND, point)
    h, acts = SR.fused_input(SR.HAND, n, point)
    ncon = GH._hand_teacher_forced(lib, f"test_hand_fused_env_step_matches_oracle_at_substeps[{point}]", spec, sp, tp, h,
                                   SR.FUSED_STEPS, acts, SR.FUSED_RNG_SEED)
    assert ncon >= n // 2   # the objects are on the hand


# ------------------------------------------------------------------------------------------------ mg_sim_set_params
SET_POINTS = ("substeps4", "gravity", "friction0.2", "depen0.3", "rest5mm", "margin0", "tgs2-6")


@pytest.mark.parametrize("point", SET_POINTS)
def test_set_params_equals_create(lib, point):
    """a sim created at the Ant's parameters and moved to a point with mg_sim_set_params gives the bits of a sim
    created at the point; moved back, the bits of the original"""
    task = "Ant"
    spec, mnp, sp, _ = SR.task_setup(task)
    root, dof, act, _, _ = SR.task_states(task, point)
    host, nb, n = SR.task_host(task, root, dof, act), len(spec.bodies), len(root)
    at = SR.task_sim_params(task, point)
    with Sim(lib, mnp, at, n) as sim:
        want = sim.run(host, nb)
    with Sim(lib, mnp, sp, n) as sim:
        orig = sim.run(host, nb)
        assert differs(orig, want), "the point changes nothing"
        assert sim.set_params(at) == MG_OK
        assert_same_bits(sim.run(host, nb), want, f"set_params({point}) differs from create({point})")
        assert sim.set_params(sp) == MG_OK
        assert_same_bits(sim.run(host, nb), orig, "moved back, the result differs from the original")


def test_set_params_refusals_change_nothing(lib):
    """changed max_contacts or agents, substeps 0, a bad solver, negative vel_iters, dt 0: MG_EINVAL, and the next
    simulate is bit-equal to one without the call"""
    task, point = "Ant", "gravity"
    spec, mnp, sp, _ = SR.task_setup(task)
    root, dof, act, _, _ = SR.task_states(task, point)
    host, nb, n = SR.task_host(task, root, dof, act), len(spec.bodies), len(root)
    with Sim(lib, mnp, sp, n) as sim:
        orig = sim.run(host, nb)
        for field, value in (("max_contacts", sp.max_contacts - 1), ("agents", sp.agents + 1), ("substeps", 0),
                             ("solver_type", 2), ("vel_iters", -1), ("dt", 0.0)):
            bad = SR.apply(sp, point, task)   # a refused call must not take the rest of the struct either
            setattr(bad, field, value)
            assert sim.set_params(bad) == MG_EINVAL, field
            assert_same_bits(sim.run(host, nb), orig, f"a refused set_params ({field}) changed the result")
