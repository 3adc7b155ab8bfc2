#!/usr/bin/env python3
"""Time the Anymal control step on the GPU, two ways:

  (a) task:      Anymal.step -- mg_anymal_pre, mg_sim_simulate, mg_anymal_post, three launches;
  (b) composed:  the step a user could compose before the task existed: torch ops for the action clamp and the PD
                 targets, mg_sim_simulate, and the post-physics part (progress, resets, observations,
                 compute_anymal_reward, timeouts, the observation clamp) as batched, mask-based torch ops on the device
                 (tests/anymal_ref.py's restatement, no host synchronisation).

Each path: warm-up steps, then `--steps` timed control steps with device events around each, the two paths alternating
in blocks of 50 so that both see the same machine state; medians and p10-p90.  `--profile-run` runs path (a) alone, for
a kernel trace taken by a profiler in a run of its own: the kernels' times and k_anymal_post's share of the HBM peak
come from that trace, inside real steps, not from events around repeated single launches (without the post kernel
between them no env resets, so a repeated k_simulate works on states no rollout has).  Prints one JSON line.
Recorded, not asserted: a tool, not a test.  The model is the test fixture tests/golden/anymal_c.json.
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


def post_bytes_per_env(clamp=True):
    """what k_anymal_post must read and write per env-step, from the shapes (a step without a reset)"""
    read = 8 + 8 + 12 * 4 + 24 * 4 + 13 * 4 + 3 * 4 + 12 * 4 + 5 * 3 * 4   # progress, reset, actions, DOF state, root,
    #                                                                        commands, torques, base + 4 thigh force rows
    write = 48 * 4 * (2 if clamp else 1) + 4 + 8 + 8 + 1                    # obs (+ clamped), rew, reset, progress, timeout
    return read + write


def rotate(q, v, sign):
    """v rotated by the unit quaternion q (xyzw; sign = +1) or by its inverse (-1), rows of (N, 4) and (N, 3)"""
    u, w = q[:, :3], q[:, 3:4]
    return v * (2.0 * w * w - 1.0) + sign * 2.0 * w * torch.linalg.cross(u, v) + 2.0 * u * (u * v).sum(-1, keepdim=True)


class Composed:
    """path (b) on the task's own sim and tensors (the two paths never run interleaved within a step): the steps of
    tests/anymal_ref.py (pre_step, reset_envs under a mask, observe, reward, the tail) as batched torch ops"""

    def __init__(self, env):
        self.e, self.p = env, env.anymal_params
        p, d = self.p, env.device
        t = lambda x: torch.tensor(list(x), device=d)   # noqa: E731
        self.default, self.base_init = t(p.default_dof_pos), t(p.base_init_state)
        self.cmd_lo, self.cmd_span = t(p.command_lo), t(p.command_span)
        self.cmd_scale = t([p.lin_vel_scale, p.lin_vel_scale, p.ang_vel_scale])
        self.rew = t([p.rew_lin_vel_xy, p.rew_ang_vel_z, p.rew_torque])
        self.rows = t([p.base_body] + list(p.knee_body)).long()
        self.down = t([0.0, 0.0, -1.0])

    def step(self, actions):
        e, p, N = self.e, self.p, self.e.num_envs
        # pre_step
        act = actions.clamp(-p.clip_actions, p.clip_actions)
        e.dof_targets.view(N, 12).copy_(p.action_scale * act + self.default)
        _abi.check(e._lib.mg_sim_simulate(e.sim, e._stream()), e._lib)
        # post_step: counters, reset_envs under the mask of done envs
        e.progress_buf += 1
        done = (e.reset_buf != 0).view(N, 1)
        u = torch.rand(N, 27, device=e.device)
        dof = e.dof_state.view(N, 12, 2)
        fresh = torch.stack((self.default * (u[:, 0:12] + 0.5), 0.2 * u[:, 12:24] - 0.1), -1)
        dof.copy_(torch.where(done.view(N, 1, 1), fresh, dof))
        e.root_states.copy_(torch.where(done, self.base_init, e.root_states))
        e.commands.copy_(torch.where(done, self.cmd_span * u[:, 24:27] + self.cmd_lo, e.commands))
        e.progress_buf.mul_((~done.view(N)).long())
        # observe
        quat = e.root_states[:, 3:7]
        lin, ang = rotate(quat, e.root_states[:, 7:10], -1.0), rotate(quat, e.root_states[:, 10:13], -1.0)
        e.obs_buf[:, 0:3] = lin * p.lin_vel_scale
        e.obs_buf[:, 3:6] = ang * p.ang_vel_scale
        e.obs_buf[:, 6:9] = rotate(quat, self.down.expand(N, 3), 1.0)
        e.obs_buf[:, 9:12] = e.commands * self.cmd_scale
        e.obs_buf[:, 12:24] = (dof[..., 0] - self.default) * p.dof_pos_scale
        e.obs_buf[:, 24:36] = dof[..., 1] * p.dof_vel_scale
        e.obs_buf[:, 36:48] = act
        # reward and the reset predicate
        err = torch.stack(((e.commands[:, :2] - lin[:, :2]).square().sum(-1), (e.commands[:, 2] - ang[:, 2]).square()), -1)
        terms = torch.cat((torch.exp(-err / 0.25), e.torques.square().sum(-1, keepdim=True)), -1)
        e.rew_buf.copy_((terms * self.rew).sum(-1).clamp_min(0.0))
        hit = (e.contact_forces[:, self.rows].square().sum(-1) > 1.0).any(-1)    # |f| > 1  <=>  |f|^2 > 1
        late = e.progress_buf >= p.max_episode_length - 1
        e.reset_buf.copy_(hit | late)
        # the tail
        e.timeout_buf.copy_(late & (e.reset_buf != 0))
        e.obs_clamped.copy_(e.obs_buf.clamp(-p.clip_obs, p.clip_obs))
        e.actions.copy_(act)


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
    ap.add_argument("--profile-run", action="store_true", help="path (a) alone, for a profiler's kernel trace")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "anymal_bench needs the MI355X"
    dev = "cuda:0"
    cfg = configs.task_config("Anymal", a.envs, overrides={"env.asset": {"modelTable": ANYMAL_JSON}})
    env = migym.make(seed=0, task="Anymal", num_envs=a.envs, sim_device=dev, rl_device=dev, headless=True,
                     cfg={"task": cfg})
    n = env.num_envs
    g = torch.Generator(device=dev).manual_seed(0)
    acts = [torch.rand((n, 12), device=dev, generator=g) * 2 - 1 for _ in range(8)]
    k = [0]

    def task_step():
        env.step(acts[k[0] % 8])
        k[0] += 1

    for _ in range(a.warmup):
        task_step()
    torch.cuda.synchronize()
    if a.profile_run:
        for _ in range(a.steps):
            task_step()
        torch.cuda.synchronize()
        print(json.dumps({"tool": "anymal_bench", "profile_run": True, "steps": a.steps, "envs": n,
                          "post_bytes_per_env": post_bytes_per_env()}))
        env.close()
        return
    comp = Composed(env)

    def composed_step():
        comp.step(acts[k[0] % 8])
        k[0] += 1

    for _ in range(a.warmup):
        composed_step()
    torch.cuda.synchronize()
    paths = {"task_step": task_step, "composed_step": composed_step}
    times = {p: [] for p in paths}
    for start in range(0, a.steps, 50):
        for p, f in paths.items():
            times[p] += timed(f, min(50, a.steps - start))
    res = {"tool": "anymal_bench", "envs": n, "steps": a.steps, "finite": bool(torch.isfinite(env.obs_buf).all()),
           "resets_in_last_step": int((env.progress_buf == 0).sum())}
    for p, t in times.items():
        res[p + "_ms"] = stats(t)
        res[p + "_env_steps_per_s"] = n / (np.median(t) * 1e-3)
    res["post_bytes_per_env"] = post_bytes_per_env()
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
