"""Inputs of the row-sizing tests (tests/test_row_census_host.py admits them on the CPU, tests/test_gpu_row_sizing.py
runs them): Ant states rolled by the oracle whose constraint-row counts cover every size at which the step kernel's
row batches and sweeps take another path -- 0 rows, the 3- and 6-column test-solve batches, the sweep blocks of 4, the
12 register rows -- and the rule that says which envs' counts hang on a threshold.

A state's rows are 3 min(contacts, max_contacts) + its joint-limit rows (tools/row_census.py, from the fp64 oracle's
contact list and build_rows()'s comparisons).  An env is *marginal* when a contact candidate lies within DELTA of its
threshold (orc_contacts_marks) or a limit comparison within BAND of the margin: fp32 rounding may put the kernel on the
other side, so nothing is asserted about that env's count.
"""
import os
import sys

import numpy as np

import pyoracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import row_census as RC  # noqa: E402

N, SEED = 2048, 3
DELTA, BAND = 1e-4, 1e-5
MARGINAL_CAP, RESET_CAP = 0.02, 0.01
COUNTS = tuple(range(0, 21))   # the row counts the shapes test places
PER_COUNT = 4                  # envs of one count: a pure wave of the 16-lane teams
_cache = {}


def setup():
    if "setup" not in _cache:
        _cache["setup"] = RC.task_setup("Ant", N)[:4]
    return _cache["setup"]


def rolled(kind):
    """(host env, rows, marginal, reset in the last step) of a state set: 'pool4' = the state 12 control steps of a
    cycling pool of 4 U(-1, 1) action tensors leave (rows 2 .. 20), 'fresh' = the state 24 steps of fresh U(-1, 1)
    actions leave (the low counts: 0 and 1 rows)"""
    if kind in _cache:
        return _cache[kind]
    spec, sp, tp, mnp = setup()
    h = O.HostEnv(tp, spec, N)
    rng = np.random.default_rng(SEED)
    steps = 12 if kind == "pool4" else 24
    pool = rng.uniform(-1, 1, (4, N, tp.num_actions)).astype(np.float32) if kind == "pool4" else None
    was_reset = np.zeros(N, bool)
    for t in range(steps):
        h.actions[:] = pool[t % 4] if pool is not None else rng.uniform(-1, 1, (N, tp.num_actions)).astype(np.float32)
        pending = h.reset.copy() != 0
        h.env_step(mnp, sp, tp, seed=SEED, step=t, threads=8)
        was_reset = pending & (t > 0)   # (the first step resets every env: the rollout's start)
    rows, marginal = RC.row_counts(mnp, sp, h.root, h.dof, DELTA, BAND)
    _cache[kind] = (h, rows, marginal, was_reset)
    return _cache[kind]


def pick(count):
    """(kind, env indices) of PER_COUNT envs with `count` rows: from 'pool4' for 2 .. 20, from 'fresh' for 0 and 1;
    envs that are not marginal first, and none with a reset pending"""
    kind = "pool4" if count >= 2 else "fresh"
    h, rows, marginal, _ = rolled(kind)
    ok = (rows == count) & (h.reset == 0)
    idx = np.concatenate([np.flatnonzero(ok & ~marginal), np.flatnonzero(ok & marginal)])
    return kind, idx[:PER_COUNT]


PER_ENV = ("root", "dof", "act_eff", "sensors", "dof_force", "actions", "actions_out", "obs", "obs_clamped", "rew",
           "reset", "progress", "timeout", "potentials", "prev_potentials", "up", "heading")


def gather(sel):
    """a HostEnv holding the envs sel = [(kind, index), ...] in that order (every per-env buffer copied)"""
    spec, sp, tp, mnp = setup()
    g = O.HostEnv(tp, spec, len(sel))
    for j, (kind, i) in enumerate(sel):
        h = rolled(kind)[0]
        for name in PER_ENV:
            getattr(g, name)[j] = getattr(h, name)[i]
    return g


def placements():
    """(pure, mixed): two lists of (kind, index), each a multiple of four long (a wave holds four 16-lane teams, in
    env order with the work ordering off).  pure: for every count c four envs of count c.  mixed: the first env of
    count c with the first envs of counts max(c - 1, 0), max(c - 4, 0) and 0 as its wave-mates -- so every env of
    `mixed` also sits in `pure`, in a wave whose row count is its own"""
    first = {}
    pure = []
    for c in COUNTS:
        kind, idx = pick(c)
        assert len(idx) == PER_COUNT, f"{len(idx)} envs with {c} rows"
        first[c] = (kind, int(idx[0]))
        pure += [(kind, int(i)) for i in idx]
    mixed = []
    for c in COUNTS:
        mixed += [first[c], first[max(c - 1, 0)], first[max(c - 4, 0)], first[0]]
    return pure, mixed
