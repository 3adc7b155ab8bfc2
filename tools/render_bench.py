#!/usr/bin/env python3
"""Time the ray caster (mg_render: k_render_setup + k_render_trace) next to the same task's control step
(DESIGN.md §12).  Writes profiles/render_bench.txt.

Cases: Ant at 1,024 envs x 64 x 64; one 640 x 480 frame of an Ant env; ShadowHand at 256 envs x 64 x 64 (the hull).
Each: 20 warm-up and 200 timed launches with device events around each render call (both launches, RGB + depth + ids
bound), and around each env.step of the same env in the same run, the two alternating in blocks of 50; medians with
p10-p90, Mrays/s and the render as a fraction of a step.  The envs are stepped with random actions first, so that the
images are of a rollout's states.  Recorded, not asserted: a tool, not a test."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isaacgymenvs-ma_amd"))
import migym  # noqa: E402
from migym import configs  # noqa: E402

CASES = [("Ant", 1024, None, 64, 64), ("Ant", 1024, [0], 640, 480), ("ShadowHand", 256, None, 64, 64)]


def stats(ms):
    ms = np.asarray(ms)
    return {"median": float(np.median(ms)), "p10": float(np.percentile(ms, 10)), "p90": float(np.percentile(ms, 90))}


def run_case(task, envs, sel, W, H, warmup, steps, block=50):
    cfg = configs.task_config(task, envs, sim_device="cuda:0")
    cfg["env"]["render"] = {"width": W, "height": H}
    env = migym.make(seed=0, task=task, num_envs=envs, sim_device="cuda:0", rl_device="cuda:0", headless=True,
                     cfg={"task": cfg})
    g = torch.Generator().manual_seed(0)
    acts = [(torch.rand((env.num_actors, env.num_actions), generator=g) * 2 - 1).cuda() for _ in range(16)]
    for k in range(30):
        env.step(acts[k % 16])
    kw = dict(rgb=True, depth=True, ids=True)
    n_img = envs if sel is None else len(sel)

    def timed(fn, n):
        out = []
        for k in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(k)
            e1.record()
            out.append((e0, e1))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in out]

    render = lambda k: env.render_envs(sel, **kw)   # noqa: E731
    step = lambda k: env.step(acts[k % 16])         # noqa: E731
    timed(render, warmup)
    timed(step, warmup)
    r_ms, s_ms = [], []
    for _ in range(steps // block):
        r_ms += timed(render, block)
        s_ms += timed(step, block)
    out = env.render_envs(sel, **kw)
    torch.cuda.synchronize()
    ids = out["ids"]
    r, s = stats(r_ms), stats(s_ms)
    res = {"task": task, "envs": envs, "images": n_img, "width": W, "height": H, "render_ms": r, "step_ms": s,
           "mrays_per_s": n_img * W * H / (r["median"] * 1e-3) / 1e6, "render_over_step": r["median"] / s["median"],
           "primitives": int(out["ids"].max().item()) + 1,
           "model_pixel_share": float(((ids >= 0) & (ids < ids.max())).float().mean().item())}
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("render_bench: needs the GPU (a CPU run gives no time)")
    lines = ["Ray caster (mg_render: k_render_setup + k_render_trace), one MI355X, tools/render_bench.py",
             f"{a.warmup} warm-up and {a.steps} timed calls, device events around each render call (RGB + depth + ids) and "
             "around each env.step of the same env, alternating in blocks of 50", ""]
    raw = []
    for task, envs, sel, W, H in CASES:
        r = run_case(task, envs, sel, W, H, a.warmup, a.steps)
        raw.append(r)
        what = f"{r['images']} image{'s' if r['images'] > 1 else ''} of {W} x {H}"
        lines += [f"{task}, {envs} envs, {what} ({r['primitives']} primitives per env, the model on "
                  f"{100 * r['model_pixel_share']:.1f} % of the pixels)",
                  f"    render  median {r['render_ms']['median']:.3f} ms (p10-p90 {r['render_ms']['p10']:.3f}-"
                  f"{r['render_ms']['p90']:.3f}), {r['mrays_per_s']:.0f} Mrays/s",
                  f"    step    median {r['step_ms']['median']:.3f} ms (p10-p90 {r['step_ms']['p10']:.3f}-"
                  f"{r['step_ms']['p90']:.3f})",
                  f"    render / step: {r['render_over_step']:.2f}", ""]
    lines += ["raw: " + json.dumps(r) for r in raw]
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
