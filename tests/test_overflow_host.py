"""The cases of tests/test_gpu_overflow.py on the CPU (tests/overflow_ref.py): how many envs are past the lowered
capacity, that the cut matters to the fp64 oracle itself, and the oracle's fp32 twin through the comparison the GPU
test applies -- 0 unexplained, flags within the 5 % cap."""
import copy

import pytest

import overflow_ref as OV
import parity_stats as PS


@pytest.mark.parametrize("task,n,k", OV.TASKS)
def test_fp32_twin_task_step_past_capacity_matches_oracle(task, n, k):
    c = OV.loco_step(task, n, k)
    over = c.before > k
    assert over.sum() >= OV.TASK_OVER[task], f"{task}: {over.sum()} envs hold more than {k} candidates"
    assert 2 * c.cut_moves()[over].sum() >= over.sum()   # the cut changes the oracle's own result in most of them
    rec = c.compare(f"test_fp32_twin_task_step_past_capacity_matches_oracle[{task}-{k}]", c.simulate(c.sp, fp32=True))
    assert rec["unexplained"] == 0 and rec["flagged_reach"] <= PS.REACH_CAP


# envs of 256 with more candidates than k (the fp64 oracle's count; pinned, the states are seeded)
HAND_OVER = {("palm-block", 4): 56, ("palm-egg", 4): 49, ("palm-pen", 4): 92, ("hull-block", 8): 21}


@pytest.mark.parametrize("name,k", OV.HANDS)
def test_fp32_twin_hand_step_past_capacity_matches_oracle(name, k):
    rec = OV.hand_twin_compare(f"test_fp32_twin_hand_step_past_capacity_matches_oracle[{name}-{k}]", name, k)
    assert rec["unexplained"] == 0 and rec["flagged_reach"] <= PS.REACH_CAP
    assert rec["over_capacity"] == HAND_OVER[name, k]
    assert 2 * rec["cut_moves_oracle"] >= rec["over_capacity"]


def test_fp32_twin_fused_step_past_capacity_matches_oracle():
    """one teacher-forced env step of the Humanoid on its feet at max_contacts 4: observations (sensors and DOF forces
    among them) and rewards of the twin against the oracle, test_gpu_parity._teacher_forced's tolerances and rule"""
    import contacts_ref as CR
    task, n, k = OV.FUSED
    spec, sp, tp, mnp, h, t, acts = OV.fused_input(task, n)
    spk = CR.with_max_contacts(sp, k)
    assert (OV.candidates(mnp, sp, h.root, h.dof) > k).sum() >= OV.TASK_OVER[task]
    h.actions[:] = acts
    flags = PS.step_flags(mnp, spk, PS.loco_physics_input(h, mnp, spk, tp, OV.FUSED_SEED, t, threads=8))
    g, roomy = copy.deepcopy(h), copy.deepcopy(h)
    h.env_step(mnp, spk, tp, seed=OV.FUSED_SEED, step=t, threads=8)
    g.env_step(mnp, spk, tp, seed=OV.FUSED_SEED, step=t, threads=8, fp32=True)
    roomy.env_step(mnp, sp, tp, seed=OV.FUSED_SEED, step=t, threads=8)
    bad = (PS.env_bad(g.obs, h.obs, 2e-3, 2e-3) | PS.env_bad(g.rew[:, None], h.rew[:, None], 5e-3, 5e-3)
           | (g.reset != h.reset))
    rec = PS.assert_steps_explained("test_fp32_twin_fused_step_past_capacity_matches_oracle", bad[None], flags[None])
    assert rec["unexplained"] == 0 and rec["flagged_reach"] <= PS.REACH_CAP
    # the cut shows in the observations
    assert PS.env_bad(roomy.obs, h.obs, 2e-3, 2e-3).sum() >= OV.TASK_OVER[task] // 2
