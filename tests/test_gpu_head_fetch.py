"""GPU tests of the step kernels' head fetch: the static-grid k_env_step instances request
the wave's order entry and its actors' raw inputs (reset flag, root row, DOF pairs, actions) before the model tile is
in LDS and the block has met at its barrier, every wave of the block included -- also one that has no work item.

The shapes are the small ones at which that fetch can go wrong (larger batches repeat them):

  * Ant on the compact layout (two-wave blocks of four envs per wave), n = 1 (the block's second wave has no item),
    4 (a full wave beside an empty one), 5 (a partial second wave) and 257 (a ragged last block);
  * Ant on the classic layout (one-wave blocks), n = 5;  MA-Ant, 3 envs x 4 agents;  Cartpole (8-lane teams, fixed
    base, one action), n = 9;  Humanoid (the work-queue instance, whose items fetch inside the loop), n = 3, both
    layouts;  ShadowHand block (k_hand_step, Team::load() on its object and target rows), n = 3.

Each shape runs four fused steps -- the first resets every env (reset_buf starts at 1), the third a hand-set subset --
unordered (MIGYM_ORDER=off) and sorted (MIGYM_ORDER=sort: the order entry is what the fetch starts from), and the two
must agree bit for bit on every output and state tensor.  Each shape and ordering mode is also put through the parity
tests' teacher-forced comparison with the fp64 oracle (their helpers and tolerances, imported).  With the sensors
bound, Ant's first five envs give the same sensor rows alone (n = 5) as inside a 257-env batch.
"""
import numpy as np
import pytest
import torch

import migym
import pyoracle as O
from migym import configs
from test_gpu_hand import _hand_teacher_forced, setup as hand_setup
from test_gpu_parity import _teacher_forced, assert_north_star_rtol, lib, ma_setup, setup  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 4
HAND_SET_STEP = 2   # the step before which a subset of reset_buf is set by hand

# (id, task, env count, MIGYM_LAYOUT or None, env config)
SHAPES = [("ant-compact-1", "Ant", 1, "compact", {}),
          ("ant-compact-4", "Ant", 4, "compact", {}),
          ("ant-compact-5", "Ant", 5, "compact", {}),
          ("ant-compact-257", "Ant", 257, "compact", {}),
          ("ant-classic-5", "Ant", 5, "classic", {}),
          ("maant-3x4", "MAAnt", 3, None, {"numAgents": 4}),
          ("humanoid-classic-3", "Humanoid", 3, "classic", {}),
          ("humanoid-compact-3", "Humanoid", 3, "compact", {}),
          ("cartpole-9", "Cartpole", 9, None, {}),
          ("hand-block-3", "ShadowHand", 3, None, {"objectType": "block"})]
IDS = [s[0] for s in SHAPES]


def _subset(actors, agents):
    """the hand-set resets: every other env (all of its agents, so MA-Ant's AND filter resets it), the first included"""
    m = torch.zeros(actors, dtype=torch.long)
    m.view(-1, agents)[::2] = 1
    return m


def _rollout(monkeypatch, task, n, layout, env_cfg, mode, act_envs=None):
    """STEPS fused steps with MIGYM_ORDER = mode; every step's outputs and state tensors, cloned.  act_envs: draw
    the actions for that many envs and use the first n rows (the same actions for an env in batches of two sizes)"""
    monkeypatch.setenv("MIGYM_ORDER", mode)
    if layout:
        monkeypatch.setenv("MIGYM_LAYOUT", layout)
    else:
        monkeypatch.delenv("MIGYM_LAYOUT", raising=False)
    cfg = configs.task_config(task, n, sim_device=DEV)
    cfg["env"].update(env_cfg)
    env = migym.make(seed=17, task=task, num_envs=n, sim_device=DEV, rl_device=DEV, headless=True, cfg={"task": cfg})
    A = env.num_agents
    g = torch.Generator().manual_seed(23)
    out = []
    assert bool((env.reset_buf == 1).all())
    for k in range(STEPS):
        a = torch.rand(((act_envs or n) * A, env.num_actions), generator=g) * 2.4 - 1.2
        if k == HAND_SET_STEP:
            env.reset_buf.copy_(torch.maximum(env.reset_buf.cpu(), _subset(env.num_actors, A)).to(DEV))
        obs, rew, reset, _ = env.step(a[:n * A].to(DEV))
        out.append({"obs": obs["obs"].clone(), "rew": rew.clone(), "reset": reset.clone(),
                    "progress": env.progress_buf.clone(), "root": env.root_states.reshape(n * A, -1).clone(),
                    "dof": env.dof_state.reshape(n * A, -1).clone(), "sensors": env.vec_sensor_tensor.clone()})
    env.close()
    return out


_cache = {}


def _cached_rollout(monkeypatch, sid, mode, **kw):
    """one rollout per (shape, mode), shared by the tests below and never modified"""
    if (sid, mode) not in _cache:
        _, task, n, layout, env_cfg = SHAPES[IDS.index(sid)]
        _cache[sid, mode] = _rollout(monkeypatch, task, n, layout, env_cfg, mode, **kw)
    return _cache[sid, mode]


@pytest.mark.parametrize("sid", IDS)
def test_ordering_modes_agree_bit_for_bit(sid, monkeypatch):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    kw = {"act_envs": 257} if sid.startswith("ant-compact") else {}
    off = _cached_rollout(monkeypatch, sid, "off", **kw)
    on = _cached_rollout(monkeypatch, sid, "sort", **kw)
    for k, (x, y) in enumerate(zip(off, on)):
        assert torch.isfinite(x["obs"]).all(), f"{sid} step {k}: non-finite observations"
        for name in x:
            assert torch.equal(x[name], y[name]), f"{sid} step {k}: {name} differ between MIGYM_ORDER=off and sort"
    # the hand-set resets took: the step's reset_idx restarted their envs (progress_buf = 0)
    if not sid.startswith("hand"):   # (the hand's reset_idx runs in pre_physics_step and the step then counts 1)
        _, task, n, _, env_cfg = SHAPES[IDS.index(sid)]
        A = env_cfg.get("numAgents", 1)
        sub = _subset(n * A, A).bool()
        assert bool((off[HAND_SET_STEP]["progress"].cpu()[sub] == 0).all())


@pytest.mark.parametrize("mode", ["off", "sort"])
def test_sensor_rows_do_not_depend_on_the_batch(mode, monkeypatch):
    """Ant, compact layout: envs 0..4 alone (n = 5) and as the head of a 257-env batch (same seed, global ids and
    actions) give the same sensor, observation and state rows: a wave's fetch reads its own actors' rows only"""
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    small = _cached_rollout(monkeypatch, "ant-compact-5", mode, act_envs=257)
    big = _cached_rollout(monkeypatch, "ant-compact-257", mode, act_envs=257)
    for k, (x, y) in enumerate(zip(small, big)):
        assert float(y["sensors"].abs().max()) > 0.0 or k == 0
        for name in ("sensors", "obs", "root", "dof"):
            assert torch.equal(x[name], y[name][:5]), f"step {k}: {name} rows of envs 0..4 differ between n = 5 and 257"


@pytest.mark.parametrize("mode", ["off", "sort"])
@pytest.mark.parametrize("sid", IDS)
def test_shape_matches_oracle(lib, sid, mode, monkeypatch):  # noqa: F811
    """the parity tests' teacher-forced comparison (progress exact; obs, reward and resets within their per-env
    tolerances, exemptions explained) at each shape and ordering mode, a subset's reset set by hand before step 2"""
    _, task, n, layout, env_cfg = SHAPES[IDS.index(sid)]
    monkeypatch.setenv("MIGYM_ORDER", mode)
    if layout:
        monkeypatch.setenv("MIGYM_LAYOUT", layout)
    else:
        monkeypatch.delenv("MIGYM_LAYOUT", raising=False)
    rng = np.random.default_rng(3)
    name = f"test_shape_matches_oracle[{sid}-{mode}]"
    if task == "ShadowHand":
        spec, sp, tp = hand_setup(kind=env_cfg["objectType"])
        h = O.HandHostEnv(tp, spec, n)
        acts = [rng.uniform(-1.2, 1.2, (n, tp.num_actions)).astype(np.float32) for _ in range(STEPS)]
        _hand_teacher_forced(lib, name, spec, sp, tp, h, STEPS, acts, 5)
        return
    A = env_cfg.get("numAgents", 1)
    spec, sp, tp = ma_setup(A) if task == "MAAnt" else setup(task)
    h = O.HostEnv(tp, spec, n * A)
    assert (h.reset == 1).all()
    acts = [rng.uniform(-1.2, 1.2, (n * A, tp.num_actions)).astype(np.float32) for _ in range(STEPS)]
    sub = _subset(n * A, A).numpy()

    def mutate(t, hh):
        if t == HAND_SET_STEP:
            hh.reset[:] = np.maximum(hh.reset, sub)
    res = _teacher_forced(lib, name, spec, sp, tp, h, STEPS, acts, seed=5, mutate=mutate)
    # the column-group statistics against 1e-4 relative compare fractions of entries to within 0.5 %: only the
    # 257-env shape has the hundreds of entries per group that takes
    if n >= 256:
        assert_north_star_rtol(res)
