#!/usr/bin/env python3
"""What heightfield terrain costs a step: the Anymal control step (mg_anymal_pre, mg_sim_simulate,
mg_anymal_post) on the plane (the plain k_simulate), on a zero field and on a rough field (k_simulate_hf; 256 x 256
samples 0.1 m apart, +-5 cm, the actors spread over it by env_origins so that a wave's candidates gather from cells far
apart), and mg_height_scan at 187 points per env.

One env, one rollout, as tools/linkforce_bench.py: after the warm-up the three grounds alternate in blocks of 50 timed
control steps, device events around each, so that all see the same machine state and states of a real rollout.  The
zero field has the rough field's grid and origins: the same loads at the same addresses, other values.  Medians and
p10-p90.  Prints one JSON line.  Recorded, not asserted: a tool, not a test.  The model is the test fixture
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
GRID, DX, AMP, POINTS = 256, 0.1, 0.05, 187


def timed(f, n):
    evs = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def stats(t):
    t = np.array(t)
    return {"median": float(np.median(t)), "p10": float(np.percentile(t, 10)), "p90": float(np.percentile(t, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "heightfield_bench needs the MI355X"
    dev = "cuda:0"
    cfg = configs.task_config("Anymal", a.envs, overrides={"env.asset": {"modelTable": ANYMAL_JSON}})
    env = migym.make(seed=0, task="Anymal", num_envs=a.envs, sim_device=dev, rl_device=dev, headless=True,
                     cfg={"task": cfg})
    n = env.num_envs
    g = torch.Generator(device=dev).manual_seed(0)
    acts = [torch.rand((n, 12), device=dev, generator=g) * 2 - 1 for _ in range(8)]
    k = [0]

    def step():
        env.step(acts[k[0] % 8])
        k[0] += 1

    size = (GRID - 1) * DX
    origins = torch.zeros((n, 3), device=dev)
    origins[:, 0:2] = 2.0 + (size - 4.0) * torch.rand((n, 2), device=dev, generator=g)
    tables = {"zero_field": torch.zeros((GRID, GRID), device=dev),
              "rough_field": (torch.rand((GRID, GRID), device=dev, generator=g) * 2 - 1) * AMP}
    fields = {name: _abi.Heightfield(heights=t.data_ptr(), nx=GRID, ny=GRID, dx=DX, x0=0.0, y0=0.0, hmax=float(t.max()),
                                     env_origins=origins.data_ptr()) for name, t in tables.items()}

    def ground(name):
        hf = fields.get(name)
        _abi.check(env._lib.mg_sim_set_heightfield(env.sim, _abi.C.byref(hf) if hf is not None else None), env._lib)

    names = ("plane", "zero_field", "rough_field")
    for name in names:
        ground(name)
        for _ in range(a.warmup):
            step()
    torch.cuda.synchronize()
    times = {name: [] for name in names}
    for start in range(0, a.steps, 50):
        for name in names:
            ground(name)
            times[name] += timed(step, min(50, a.steps - start))
    # the scan: the reference's 187 measured points (a 17 x 11 grid, 0.1 m apart) around every actor on the rough field
    ground("rough_field")
    xs, ys = torch.arange(-8, 9, device=dev) * 0.1, torch.arange(-5, 6, device=dev) * 0.1
    pts = torch.stack(torch.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2).contiguous()
    assert pts.shape[0] == POINTS
    out = torch.empty((n, POINTS), device=dev)
    for _ in range(a.warmup):
        env.height_scan(pts, out)
    scan = timed(lambda: env.height_scan(pts, out), a.steps)
    res = {"tool": "heightfield_bench", "envs": n, "steps": a.steps,
           "finite": bool(torch.isfinite(env.obs_buf).all() and torch.isfinite(out).all())}
    for name, t in times.items():
        res[name + "_step_ms"] = stats(t)
    for name in names[1:]:
        res[name + "_overhead_of_median"] = float(np.median(times[name]) / np.median(times["plane"]) - 1.0)
    res["height_scan_ms"] = stats(scan)
    res["height_scan_points"] = POINTS
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
