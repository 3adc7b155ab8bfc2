#!/usr/bin/env python3
"""Time the Quadcopter control step on the GPU, two ways:

  (a) task:      Quadcopter.step -- mg_quadcopter_pre, mg_sim_simulate with link forces, mg_quadcopter_post;
  (b) composed:  the step a user could compose from the link-force switch alone: the reference's pre_physics_step and
                 post_physics_step as batched, mask-based torch ops on the device (tests/quadcopter_ref.py's
                 restatement, no host synchronisation) around mg_sim_simulate.

Each path: warm-up steps, then `--steps` timed control steps with device events around each, the two paths alternating
in blocks of 50 on the task's own sim and tensors, so that both see the same machine state and one rollout; medians and
p10-p90.  Prints one JSON line.  Recorded, not asserted: a tool, not a test.  For k_simulate with link forces on against
the plain instance see tools/linkforce_bench.py.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isaacgymenvs-ma_amd"))
import migym  # noqa: E402
from migym import _abi  # noqa: E402


class Composed:
    """path (b) on the task's own sim and tensors: quadcopter.py:280-418 as batched torch ops"""

    def __init__(self, env):
        self.e, p = env, env.quadcopter_params
        d = env.device
        self.init_root = torch.tensor(list(p.init_root), device=d)
        self.span = torch.tensor([3.0, 3.0, 1.7], device=d)
        self.lo = torch.tensor([-1.5, -1.5, -0.2], device=d)
        self.dof_step, self.thrust_step = float(p.dof_step), float(p.thrust_step)
        self.clip_a, self.clip_o, self.max_len = float(p.clip_actions), float(p.clip_obs), int(p.max_episode_length)
        self.rotors = torch.tensor(list(p.rotor_body), device=d)

    def step(self, actions):
        e, N = self.e, self.e.num_envs
        # pre_physics_step: reset_idx under the mask of done envs, targets, thrusts, the force rows
        done = e.reset_buf != 0
        u = torch.rand(N, 11, device=e.device)
        fresh_root = self.init_root.expand(N, 13).clone()
        fresh_root[:, 0:3] += self.span * u[:, 0:3] + self.lo
        e.root_states.copy_(torch.where(done.view(N, 1), fresh_root, e.root_states))
        dof = e.dof_states
        fresh_dof = torch.stack((0.4 * u[:, 3:11] - 0.2, torch.zeros(N, 8, device=e.device)), -1)
        dof.copy_(torch.where(done.view(N, 1, 1), fresh_dof, dof))
        e.progress_buf.mul_((~done).long())
        e.reset_buf.zero_()
        a = actions.clamp(-self.clip_a, self.clip_a)
        tgt = torch.maximum(torch.minimum(e.dof_position_targets + self.dof_step * a[:, 0:8], e.dof_upper_limits),
                            e.dof_lower_limits)
        thr = (e.thrusts + self.thrust_step * a[:, 8:12]).clamp(0.0, 2.0)
        e.forces[:, self.rotors, 2] = thr
        e.thrusts.copy_(torch.where(done.view(N, 1), torch.zeros_like(thr), thr))
        e.forces.mul_((~done).view(N, 1, 1).float())
        e.dof_position_targets.copy_(torch.where(done.view(N, 1), dof[..., 0], tgt))
        _abi.check(e._lib.mg_sim_simulate(e.sim, e._stream()), e._lib)
        # post_physics_step: observations, compute_quadcopter_reward, the tail
        e.progress_buf += 1
        r = e.root_states
        e.obs_buf[:, 0:2] = (0.0 - r[:, 0:2]) / 3
        e.obs_buf[:, 2] = (1.0 - r[:, 2]) / 3
        e.obs_buf[:, 3:7] = r[:, 3:7]
        e.obs_buf[:, 7:10] = r[:, 7:10] / 2
        e.obs_buf[:, 10:13] = r[:, 10:13] / math.pi
        e.obs_buf[:, 13:21] = dof[..., 0]
        dist = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + (1 - r[:, 2]) * (1 - r[:, 2]))
        pos = 1.0 / (1.0 + dist * dist)
        qw = r[:, 6]
        upz = (2.0 * qw * qw - 1.0) + 2.0 * r[:, 5] * r[:, 5]     # quat_axis(q, 2)[2]
        tilt = (1 - upz).abs()
        spin = r[:, 12].abs()
        e.rew_buf.copy_(pos + pos * (1.0 / (1.0 + tilt * tilt) + 1.0 / (1.0 + spin * spin)))
        late = e.progress_buf >= self.max_len - 1
        e.reset_buf.copy_(late | (dist > 3.0) | (r[:, 2] < 0.3))
        e.timeout_buf.copy_(late & (e.reset_buf != 0))
        e.obs_clamped.copy_(e.obs_buf.clamp(-self.clip_o, self.clip_o))
        e.actions.copy_(a)


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
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_bench needs the MI355X"
    dev = "cuda:0"
    env = migym.make(seed=0, task="Quadcopter", num_envs=a.envs, sim_device=dev, rl_device=dev, headless=True)
    n = env.num_envs
    g = torch.Generator(device=dev).manual_seed(0)
    acts = [torch.rand((n, 12), device=dev, generator=g) * 2 - 1 for _ in range(8)]
    k = [0]
    comp = Composed(env)

    def task_step():
        env.step(acts[k[0] % 8])
        k[0] += 1

    def composed_step():
        comp.step(acts[k[0] % 8])
        k[0] += 1

    paths = {"task_step": task_step, "composed_step": composed_step}
    for f in paths.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {p: [] for p in paths}
    for start in range(0, a.steps, 50):
        for p, f in paths.items():
            times[p] += timed(f, min(50, a.steps - start))
    res = {"tool": "quad_bench", "envs": n, "steps": a.steps, "finite": bool(torch.isfinite(env.obs_buf).all()),
           "resets_in_last_step": int((env.progress_buf == 0).sum())}
    for p, t in times.items():
        res[p + "_ms"] = stats(t)
        res[p + "_env_steps_per_s"] = n / (np.median(t) * 1e-3)
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
