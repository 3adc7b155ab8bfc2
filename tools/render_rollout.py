#!/usr/bin/env python3
"""Render a rollout of a task with the HIP ray caster (migym/render.py): PPM frames or one .npy.

    python tools/render_rollout.py --task Ant --steps 60 --envs 4 --out frames/       # frames/env0_0000.ppm ...
    python tools/render_rollout.py --task ShadowHand --steps 30 --envs 2 --out roll.npy   # (steps, envs, H, W, 3) uint8

Random actions from a seeded generator; the image shows the collision geometry.  No dependency beyond
numpy and torch."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isaacgymenvs-ma_amd"))
import migym  # noqa: E402
from migym import configs  # noqa: E402
from migym.render import write_ppm  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--task", default="Ant")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--envs", type=int, default=1, help="envs simulated; all of them are rendered")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="frames", help="a directory (PPM frames) or a path ending in .npy")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("render_rollout: needs the GPU")
    cfg = configs.task_config(a.task, a.envs, sim_device="cuda:0")
    over = {k: v for k, v in (("width", a.width), ("height", a.height)) if v}
    if over:
        cfg["env"]["render"] = dict(cfg["env"].get("render", {}), **over)
    env = migym.make(seed=a.seed, task=a.task, num_envs=a.envs, sim_device="cuda:0", rl_device="cuda:0", headless=True,
                     virtual_screen_capture=True, cfg={"task": cfg})
    g = torch.Generator().manual_seed(a.seed)
    frames = []
    for _ in range(a.steps):
        act = torch.rand((env.num_actors, env.num_actions), generator=g) * 2 - 1
        env.step(act.cuda())
        frames.append(env.render_envs(None, rgb=True)["rgb"].cpu().numpy())
    roll = np.stack(frames)
    if a.out.endswith(".npy"):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        np.save(a.out, roll)
    else:
        os.makedirs(a.out, exist_ok=True)
        for t in range(roll.shape[0]):
            for e in range(roll.shape[1]):
                write_ppm(os.path.join(a.out, f"env{e}_{t:04d}.ppm"), roll[t, e])
    print(f"render_rollout: {a.task}, {roll.shape[0]} steps x {roll.shape[1]} envs of {roll.shape[3]} x {roll.shape[2]} "
          f"-> {a.out}")
    env.close()


if __name__ == "__main__":
    main()
