#!/usr/bin/env python3
"""Time the AnymalTerrain control step on the GPU and where it goes.  Per env count, on the default
10 x 20 curriculum terrain, with device events, warm-up steps and then `--steps` timed control steps of seeded random
actions, medians with p10-p90:

  step       AnymalTerrain.step: (mg_anymal_terrain_pre, mg_sim_simulate) x 4, mg_anymal_terrain_post
  split      the same launches issued by hand with an event between the groups: the four pre launches (each timed with
             the simulate that follows it cut off by an event, so a launch boundary is inside the figure), the four
             simulates, post with its finishing pass.  The events add their own packets: the parts sum to more than
             `step`
  sim_world  after a step, four mg_sim_simulate launches alone from the rollout's state, the field in world
             coordinates (the task's choice: the ground cull takes the field's global maximum)
  sim_local  the same four launches from the same state in a second sim whose field has per-actor origins (roots in
             each env's own frame: the cull still takes the global maximum, but the positions are small numbers)

Prints one JSON line per env count.  Recorded, not asserted: a tool, not a test.  The model is the test fixture
tests/golden/anymal_c.json.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isaacgymenvs-ma_amd"))
import migym  # noqa: E402
from migym import _abi, configs  # noqa: E402

ANYMAL_JSON = os.path.join(ROOT, "tests", "golden", "anymal_c.json")
DEV = "cuda:0"


def make(n):
    np.random.seed(0)
    cfg = configs.task_config("AnymalTerrain", n, overrides={"env.asset": {"modelTable": ANYMAL_JSON}})
    return migym.make(seed=0, task="AnymalTerrain", num_envs=n, sim_device=DEV, rl_device=DEV, headless=True,
                      cfg={"task": cfg})


def stats(t):
    t = np.array(t)
    return {"median": float(np.median(t)), "p10": float(np.percentile(t, 10)), "p90": float(np.percentile(t, 90))}


def event():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def run(n, warmup, steps):
    env, loc = make(n), make(n)
    # the second sim: the same field with per-actor origins, roots in each env's own frame
    t = loc.terrain
    origins = loc.env_origins.clone()
    loc.set_heightfield(loc.height_samples, t.horizontal_scale, t.vertical_scale,
                        origin=(-t.border_size, -t.border_size), env_origins=origins)
    g = torch.Generator(device=DEV).manual_seed(0)
    acts = [torch.rand((n, 12), device=DEV, generator=g) * 2 - 1 for _ in range(8)]
    lib, check = env._lib, _abi.check
    for k in range(warmup):
        env.step(acts[k % 8])
    torch.cuda.synchronize()
    rec = {k: [] for k in ("step", "pre4", "sim4", "post", "sim_world", "sim_local")}
    marks = []
    for k in range(steps):
        a = acts[k % 8]
        e0 = event()
        env.step(a)
        e1 = event()
        # the same launches by hand, an event between the groups
        tb, st = env._tb, env._stream()
        tb.actions, tb.step_counter = a.data_ptr(), env.control_steps
        p, v, b = env._params_ref, env._views_ref, _abi.C.byref(tb)
        ev = [event()]
        for _ in range(env.decimation):
            check(env._pre(env.sim, p, v, b, st), lib)
            ev.append(event())
            check(env._simulate(env.sim, st), lib)
            ev.append(event())
        env._task_views.push_now = 0
        check(env._post(env.sim, p, v, b, None, st), lib)
        ev.append(event())
        env.control_steps += 1
        # four simulates alone, from the same state, in the two coordinate conventions
        loc.root_states.copy_(env.root_states)
        loc.root_states[:, :3] -= origins
        loc.dof_state.copy_(env.dof_state)
        loc.dof_actuation.copy_(env.dof_actuation)
        w0 = event()
        for _ in range(4):
            check(lib.mg_sim_simulate(env.sim, st), lib)
        w1 = event()
        for _ in range(4):
            check(lib.mg_sim_simulate(loc.sim, st), lib)
        w2 = event()
        marks.append((e0, e1, ev, w0, w1, w2))
    torch.cuda.synchronize()
    for e0, e1, ev, w0, w1, w2 in marks:
        rec["step"].append(e0.elapsed_time(e1))
        rec["pre4"].append(sum(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(4)))
        rec["sim4"].append(sum(ev[2 * i + 1].elapsed_time(ev[2 * i + 2]) for i in range(4)))
        rec["post"].append(ev[8].elapsed_time(ev[9]))
        rec["sim_world"].append(w0.elapsed_time(w1))
        rec["sim_local"].append(w1.elapsed_time(w2))
    res = {"tool": "anymal_terrain_bench", "envs": n, "steps": steps, "warmup": warmup,
           "finite": bool(torch.isfinite(env.obs_buf).all() and torch.isfinite(env.root_states).all()),
           "mean_terrain_level": float(env.terrain_levels.float().mean()),
           "field_cells": list(env.height_samples.shape)}
    for k, t in rec.items():
        res[k + "_ms"] = stats(t)
    res["env_steps_per_s"] = n / (res["step_ms"]["median"] * 1e-3)
    res["pre4_share_of_split"] = res["pre4_ms"]["median"] / (res["pre4_ms"]["median"] + res["sim4_ms"]["median"] +
                                                             res["post_ms"]["median"])
    env.close()
    loc.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "anymal_terrain_bench needs the MI355X"
    for n in a.envs:
        print(json.dumps(run(n, a.warmup, a.steps)), flush=True)


if __name__ == "__main__":
    main()
