#!/usr/bin/env python3
"""What link forces cost a step that applies none: the Anymal control step (mg_anymal_pre,
mg_sim_simulate, mg_anymal_post) with mg_sim_set_link_forces on and an all-zero force tensor bound -- k_simulate_xf,
which loads the rows and finds every one zero -- against the same step with the switch off (the plain k_simulate).

One env, one rollout: after the warm-up the switch alternates in blocks of 50 timed control steps, device events
around each, so that both variants see the same machine state and states of a real rollout (resets included; a
repeated k_simulate without the post kernel between would run on states no rollout has).  Medians and p10-p90; the two
variants' results differ only by the one-step tolerances (tests/test_gpu_linkforce.py), so the rollout does not
depend on which block ran which.  Prints one JSON line.  Recorded, not asserted: a tool, not a test.  The model is
the test fixture tests/golden/anymal_c.json.
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
    assert torch.cuda.is_available(), "linkforce_bench needs the MI355X"
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

    forces = torch.zeros((n, env.num_bodies, 3), device=dev)
    env.apply_rigid_body_force_tensors(forces, None, migym.ENV_SPACE)     # binds the tensor and switches on
    switch = lambda on: _abi.check(env._lib.mg_sim_set_link_forces(env.sim, int(on)), env._lib)   # noqa: E731
    for on in (True, False):
        switch(on)
        for _ in range(a.warmup):
            step()
    torch.cuda.synchronize()
    times = {"plain": [], "link_forces_zero": []}
    for start in range(0, a.steps, 50):
        for name, on in (("plain", False), ("link_forces_zero", True)):
            switch(on)
            times[name] += timed(step, min(50, a.steps - start))
    res = {"tool": "linkforce_bench", "envs": n, "steps": a.steps, "finite": bool(torch.isfinite(env.obs_buf).all())}
    for name, t in times.items():
        res[name + "_step_ms"] = stats(t)
    res["overhead_of_median"] = float(np.median(times["link_forces_zero"]) / np.median(times["plain"]) - 1.0)
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
