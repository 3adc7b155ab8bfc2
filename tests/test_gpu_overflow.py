"""The task models and the hand past contact capacity, against the fp64 oracle (tests/overflow_ref.py).

max_contacts lowered below what the states hold -- Ant to 2 and Humanoid to 4 on their feet, in the classic and the
compact layout; the hand with the block, the egg and the pen on the palm to 4, with the block against the forearm
hull to 8 -- so collide() cuts the list and the rows, the solve, sensors, DOF forces and net contact forces run on
the oracle's prefix of the emission order.  One mg_sim_simulate each through the comparison of the physics-step tests
(tolerances unchanged, orc_step_flips with bit 128, reach at most 5 %, no sensitivity fallback, nothing unexplained),
and one teacher-forced mg_env_step of the Humanoid at max_contacts 4 (observations carry sensors and DOF forces).
tests/test_overflow_host.py pins the inputs (how many envs are past capacity, that the cut matters to the oracle) and
puts the oracle's fp32 twin through the same comparison.
"""
import numpy as np
import pytest
import torch

import contacts_ref as CR
import overflow_ref as OV
import test_gpu_hand as H
import test_gpu_parity as GP
from migym import _abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


@pytest.mark.parametrize("layout", ["classic", "compact"])
@pytest.mark.parametrize("task,n,k", OV.TASKS)
def test_task_step_past_capacity_matches_oracle(lib, task, n, k, layout, monkeypatch):
    monkeypatch.setenv("MIGYM_LAYOUT", layout)
    c = OV.loco_step(task, n, k)
    assert (c.before > k).sum() >= OV.TASK_OVER[task]
    assert GP.kernel_layout(lib, c.spec, c.sp, n)[1] == (layout == "compact")
    got = GP._gpu_simulate(lib, c.mnp, c.sp, c.root, c.dof, c.act, max(len(c.spec.sensors), 1))
    again = GP._gpu_simulate(lib, c.mnp, c.sp, c.root, c.dof, c.act, max(len(c.spec.sensors), 1))
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)
    c.compare(f"test_task_step_past_capacity_matches_oracle[{task}-{k}-{layout}]", got)


@pytest.mark.parametrize("name,k", OV.HANDS)
def test_hand_step_past_capacity_matches_oracle(lib, name, k):
    """test_gpu_hand's physics comparison (determinism, net contact forces, rigid bodies, sensors) at max_contacts k"""
    spec, sp, mnp, h, before = OV.hand_input(name, k)
    assert (before > k).sum() >= 16
    H._physics_vs_oracle(lib, spec, sp, h, np.random.default_rng(OV.HAND_FORCE_SEED), h.n)


def test_fused_step_past_capacity_matches_oracle(lib):
    task, n, k = OV.FUSED
    spec, sp, tp, mnp, h, t, acts = OV.fused_input(task, n)
    assert (OV.candidates(mnp, sp, h.root, h.dof) > k).sum() >= OV.TASK_OVER[task]
    # (the step index only keys the reset draws: the fused harness counts its steps from 0)
    GP._teacher_forced(lib, "test_fused_step_past_capacity_matches_oracle", spec, CR.with_max_contacts(sp, k), tp, h, 1,
                       [acts], seed=OV.FUSED_SEED)
