"""The ABA backward pass of the 16-lane compact teams (DESIGN.md §3 ABA step 2, §9 round 9): the root's child sum
runs over the team's lanes where the root has two to seven children (common.hpp mg_root_sum_slot: the root's own 27
values go to the level slot its children leave free, lane l adds the children's entries l and l + 16 in the children's
order, lane 0 reads the sums back), and on the root's own lane otherwise.

Ant and MA-Ant (four children of the torso: the team-wide sum) on the compact layout, at the small shapes at which a
wave's teams can go wrong: Ant n = 1 (three idle teams, and the block's second wave without an item), 4 (a full
wave), 5 (a partial second wave), 67 (a ragged last block); MA-Ant 3 envs x 4 agents.  Four fused steps -- the first
resets every env, the third a hand-set subset -- unordered and sorted, which must agree bit for bit, and each put
through the parity tests' teacher-forced comparison with the fp64 oracle (their helpers and tolerances, unchanged).

Tree shapes, one mg_sim_simulate each on the compact 9-node instance (MIGYM_LAYOUT=compact), free base, against the
fp64 oracle by tree_physics_ref.compare's rules, at 5 actors (a partial second wave) and 66:

  * star    eight children of the root: level 1 fills all eight slots, none is free -> the root's own sum;
  * chain   depth 8, one child per node                                            -> the root's own sum;
  * root2   two children of the root, the fewest the team-wide sum takes           (slot 2);
  * root7   seven children, the most it takes                                      (slot 7, the last one);
  * mixed   a level of three nodes, and a node below the root with two children    (slot 3; the serial sum deeper);
  * random  dynamics_ref.random_tree(9, 1) as drawn                                (parents from [i - 6, i)).

test_fp32_twin_tree_shapes (no GPU) puts the oracle's fp32 twin through the same comparison on the same states: the
trees and seeds were fixed against it, never the rule.
"""
import dataclasses

import numpy as np
import pytest
import torch

import dynamics_ref as D
import parity_stats as PS
import pyoracle as O
import tree_physics_ref as TP
from migym import model as M
from test_gpu_head_fetch import HAND_SET_STEP, STEPS, _rollout, _subset
from test_gpu_parity import _teacher_forced, lib, ma_setup, setup  # noqa: F401  (lib: fixture)
from test_gpu_tree_physics import _gpu_step

gpu = pytest.mark.gpu

# (id, task, env count, env config): all on the compact layout
SHAPES = [("ant-1", "Ant", 1, {}), ("ant-4", "Ant", 4, {}), ("ant-5", "Ant", 5, {}), ("ant-67", "Ant", 67, {}),
          ("maant-3x4", "MAAnt", 3, {"numAgents": 4})]
IDS = [s[0] for s in SHAPES]


@gpu
@pytest.mark.parametrize("sid", IDS)
def test_ordering_modes_agree_bit_for_bit(sid, monkeypatch):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    _, task, n, env_cfg = SHAPES[IDS.index(sid)]
    off = _rollout(monkeypatch, task, n, "compact", env_cfg, "off")
    on = _rollout(monkeypatch, task, n, "compact", env_cfg, "sort")
    for k, (x, y) in enumerate(zip(off, on)):
        assert torch.isfinite(x["obs"]).all(), f"{sid} step {k}: non-finite observations"
        for name in x:
            assert torch.equal(x[name], y[name]), f"{sid} step {k}: {name} differ between MIGYM_ORDER=off and sort"
    A = env_cfg.get("numAgents", 1)
    assert bool((off[HAND_SET_STEP]["progress"].cpu()[_subset(n * A, A).bool()] == 0).all())   # the hand-set resets took


@gpu
@pytest.mark.parametrize("mode", ["off", "sort"])
@pytest.mark.parametrize("sid", IDS)
def test_shape_matches_oracle(lib, sid, mode, monkeypatch):  # noqa: F811
    """the parity tests' teacher-forced comparison at each shape and ordering mode, a subset reset by hand"""
    _, task, n, env_cfg = SHAPES[IDS.index(sid)]
    monkeypatch.setenv("MIGYM_ORDER", mode)
    monkeypatch.setenv("MIGYM_LAYOUT", "compact")
    A = env_cfg.get("numAgents", 1)
    spec, sp, tp = ma_setup(A) if task == "MAAnt" else setup(task)
    h = O.HostEnv(tp, spec, n * A)
    assert (h.reset == 1).all()
    rng = np.random.default_rng(3)
    acts = [rng.uniform(-1.2, 1.2, (n * A, tp.num_actions)).astype(np.float32) for _ in range(STEPS)]
    sub = _subset(n * A, A).numpy()

    def mutate(t, hh):
        if t == HAND_SET_STEP:
            hh.reset[:] = np.maximum(hh.reset, sub)
    _teacher_forced(lib, f"test_quad_aba_shape_matches_oracle[{sid}-{mode}]", spec, sp, tp, h, STEPS, acts, seed=5,
                    mutate=mutate)


# ------------------------------------------------------------------------------------------------ tree shapes
@dataclasses.dataclass(frozen=True)
class ShapeCase(TP.Case):
    """a tree_physics_ref case whose tree is random_tree's nine nodes hung on given parents (None: as drawn)"""
    label: str = ""
    parents: tuple = None

    def name(self):
        return self.label


TREE_SEED = 1        # random_tree's first seed with a hinge below a slide and a slide below a hinge at nine nodes
NUM_GEOMS = 12       # of the instance's 16; no self pairs (the 9-node instance has none)
MAXC = 16            # the instance's MC
TREES = {c.label: c for c in (
    ShapeCase(16, {}, MAXC, 201, (), (), label="star", parents=(0, 0, 0, 0, 0, 0, 0, 0)),
    ShapeCase(16, {}, MAXC, 202, (), (), label="chain", parents=(0, 1, 2, 3, 4, 5, 6, 7)),
    ShapeCase(16, {}, MAXC, 203, (), (), label="root2", parents=(0, 0, 1, 1, 2, 2, 3, 4)),
    ShapeCase(16, {}, MAXC, 204, (), (), label="root7", parents=(0, 0, 0, 0, 0, 0, 0, 1)),
    ShapeCase(16, {}, MAXC, 205, (), (), label="mixed", parents=(0, 0, 0, 1, 1, 2, 4, 4)),
    ShapeCase(16, {}, MAXC, 206, (), (), label="random"))}
# (children of the root, the widest level): what decides the path (common.hpp mg_root_sum_slot, kCompactLevelSlots)
SHAPE_OF = {"star": (8, 8), "chain": (1, 1), "root2": (2, 4), "root7": (7, 7), "mixed": (3, 3)}
TREE_ACTORS = (5, TP.CASE_ACTORS)


def _spec(case):
    """the case's spec, entered where tree_physics_ref.spec_of looks it up"""
    key = ("spec", case.name())
    if key not in TP._cache:
        spec = D.random_tree(9, TREE_SEED)
        for i, p in enumerate(case.parents or ()):
            spec.nodes[i + 1].parent = p
            spec.bodies[i + 1].parent_body = p
        D._step_ready(spec, np.random.default_rng([TREE_SEED, 1]), True, True, NUM_GEOMS, 0, M.MAX_SENSORS, True)
        spec.name = f"tree9_{case.label}"
        TP._cache[key] = spec
    return TP._cache[key]


def _shape(spec):
    par = [n.parent for n in spec.nodes]
    depth = [0] * len(par)
    for i in range(1, len(par)):
        depth[i] = depth[par[i]] + 1
    return par.count(0), max(depth.count(d) for d in set(depth[1:]))


@pytest.mark.parametrize("name", list(TREES))
def test_fp32_twin_tree_shapes(name):
    """no GPU: the tree has the shape its label says, fits the 9-node instance, and the oracle's fp32 twin passes the
    comparison the GPU is held to, on the same states"""
    case = TREES[name]
    spec = _spec(case)
    if name in SHAPE_OF:
        assert _shape(spec) == SHAPE_OF[name]
    cnt = TP.counts(spec)
    assert cnt["nodes"] == 9 and cnt["lanes"] <= 16 and cnt["geoms"] <= 16 and cnt["pairs"] == 0 and not spec.fixed_base
    root, dof, act, ref = TP.states(case, "dropped")
    for n in TREE_ACTORS:
        got = TP.TreeHost(spec, root[:n], dof[:n], act[:n]).simulate(M.pack_model(spec), TP.sim_params(case), fp32=True)
        rec = TP.compare(f"test_fp32_twin_tree_shapes[{name}-{n}]", case, "dropped", n, got)
        assert rec["unexplained"] == 0 and rec["flagged_reach"] <= PS.REACH_CAP


@gpu
@pytest.mark.parametrize("n", TREE_ACTORS)
@pytest.mark.parametrize("name", list(TREES))
def test_tree_shape_step_matches_oracle(lib, name, n, monkeypatch):  # noqa: F811
    monkeypatch.setenv("MIGYM_LAYOUT", "compact")
    case = TREES[name]
    _spec(case)
    got, lanes, compact = _gpu_step(lib, case, "dropped", n)
    assert (lanes, compact) == (16, 1), f"{name}: ran on the {lanes}-lane instance (compact {compact})"
    TP.compare(f"test_tree_shape_step_matches_oracle[{name}-{n}]", case, "dropped", n, got)
