#!/usr/bin/env python3
"""Time the HumanoidAMP control step on the GPU, two ways:

  (a) task:      HumanoidAMP.step -- mg_amp_pre, mg_sim_simulate x controlFrequencyInv, mg_amp_post -- followed by
                 reset_done() (its nonzero() is the one host synchronisation, as in the reference; mg_amp_reset_idx
                 samples the motion table on the device);
  (b) composed:  what a user could compose before the task existed: torch ops for the PD targets, the observations,
                 compute_humanoid_reset and the AMP history, mg_sim_simulate, and for the resets a host-side numpy
                 motion sampler (tests/amp_ref.py's restatement of MotionLib.get_motion_state on numpy's global
                 generator) whose results are copied to the device, as the reference does on every reset.

Each path: warm-up steps, then `--steps` timed control steps with device events around each (the reset included), the
two paths alternating in blocks of 50 so that both see the same machine state; medians and p10-p90.  `--profile-run`
runs path (a) alone, for a kernel trace taken by a profiler in a run of its own.  Prints one JSON line.  Recorded, not
asserted: a tool, not a test.  The model and the clips are the test fixtures under tests/golden/; the episode length is
shortened (`--episode`) so that time-outs and resets occur within the timed steps.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isaacgymenvs-ma_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import amp_ref as R  # noqa: E402
import migym  # noqa: E402
from migym import _abi, configs  # noqa: E402
from migym.motion import DOF_OFFSETS  # noqa: E402


def post_bytes_per_env(steps, clamp=False):
    """what k_amp_post must read and write per env-step, from the shapes"""
    read = 8 + 13 * 4 + 56 * 4 + 4 * 3 * 4 + 13 * 3 * 4 + 13 * 4 + (steps - 1) * 105 * 4   # progress, root, DOF state,
    #          key rows, 13 non-contact force rows and heights, the AMP slots that shift
    write = 105 * 4 * (2 if clamp else 1) + 4 + 8 + 8 + 8 + 1 + steps * 105 * 4   # obs, rew, reset, terminate,
    #          progress, timeout, the AMP buffer
    return read + write


# ---- the observation expressions as batched torch ops (utils/torch_jit_utils.py)
def rotate(q, v):
    u, w = q[:, :3], q[:, 3:4]
    return v * (2.0 * w * w - 1.0) + 2.0 * w * torch.linalg.cross(u, v) + 2.0 * u * (u * v).sum(-1, keepdim=True)


def quat_mul(a, b):
    x1, y1, z1, w1 = a.unbind(-1)
    x2, y2, z2, w2 = b.unbind(-1)
    return torch.stack((w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                        w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2), -1)


def quat_from_angle_axis(angle, axis):
    theta = (angle / 2).unsqueeze(-1)
    q = torch.cat((torch.nn.functional.normalize(axis, dim=-1, eps=1e-9) * theta.sin(), theta.cos()), -1)
    return torch.nn.functional.normalize(q, dim=-1, eps=1e-9)


def tan_norm(q):
    ex, ez = torch.zeros_like(q[:, :3]), torch.zeros_like(q[:, :3])
    ex[:, 0], ez[:, 2] = 1, 1
    return torch.cat((rotate(q, ex), rotate(q, ez)), -1)


def observations(root, dof_pos, dof_vel, key_pos, local):
    n, q = root.shape[0], root[:, 3:7]
    ex, ez = torch.zeros_like(q[:, :3]), torch.zeros_like(q[:, :3])
    ex[:, 0], ez[:, 2] = 1, 1
    d = rotate(q, ex)
    h = quat_from_angle_axis(-torch.atan2(d[:, 1], d[:, 0]), ez)
    parts = [root[:, 2:3], tan_norm(quat_mul(h, q) if local else q), rotate(h, root[:, 7:10]), rotate(h, root[:, 10:13])]
    for j, o in enumerate(DOF_OFFSETS[:-1]):
        if DOF_OFFSETS[j + 1] - o == 3:
            e = dof_pos[:, o:o + 3]
            angle = e.norm(dim=-1)
            axis = e / angle.unsqueeze(-1)
            angle = torch.atan2(angle.sin(), angle.cos())
            mask = angle > 1e-5
            angle = torch.where(mask, angle, torch.zeros_like(angle))
            axis = torch.where(mask.unsqueeze(-1), axis, ez)
            parts.append(tan_norm(quat_from_angle_axis(angle, axis)))
        else:
            parts.append(dof_pos[:, o:o + 1])
    parts.append(dof_vel)
    rel = (key_pos.view(n, 4, 3) - root[:, None, 0:3]).reshape(n * 4, 3)
    parts.append(rotate(h.repeat_interleave(4, 0), rel).view(n, 12))
    return torch.cat(parts, -1)


class Composed:
    """path (b) on the task's own sim and tensors (the two paths never run interleaved within a step)"""

    def __init__(self, env):
        self.e, self.p = env, R.params_from(env.amp_params)
        d = env.device
        self.offset, self.scale = torch.tensor(self.p["offset"], device=d), torch.tensor(self.p["scale"], device=d)
        mask = torch.ones(15, dtype=torch.bool, device=d)
        mask[self.p["contact"]] = False
        self.mask, self.key = mask, torch.tensor(self.p["key"], device=d)
        self.table = env._motion_lib

    def step(self, actions):
        e, p, N = self.e, self.p, self.e.num_envs
        e.dof_targets.view(N, 28).copy_(self.offset + self.scale * actions)
        for _ in range(e.control_freq_inv):
            _abi.check(e._lib.mg_sim_simulate(e.sim, e._stream()), e._lib)
        e.progress_buf += 1
        dof, rb = e.dof_state.view(N, 28, 2), e.rigid_body_states.view(N, 15, 13)
        e.obs_buf.copy_(observations(e.root_states, dof[..., 0], dof[..., 1], rb[:, self.key, 0:3].reshape(N, 12), p["local"]))
        e.rew_buf.fill_(1.0)
        fallen = (e._contact_forces[:, self.mask] > 0.1).any(-1).any(-1) & \
            (rb[:, self.mask, 2] < float(p["termination_height"])).any(-1) & (e.progress_buf > 1)
        late = e.progress_buf >= p["max_len"] - 1
        e._terminate_buf.copy_(fallen)
        e.reset_buf.copy_(fallen | late)
        e._amp_obs_buf[:, 1:] = e._amp_obs_buf[:, :-1].clone()
        e._amp_obs_buf[:, 0] = e.obs_buf
        e.timeout_buf.copy_(late & (e.reset_buf != 0))
        e.actions.copy_(actions)
        # reset_done with the reference's host-side sampler
        ids = e.reset_buf.nonzero().flatten()
        n = len(ids)
        if n == 0:
            return
        tb, dev = self.table, e.device
        mids = np.random.choice(tb.num_motions(), size=n, replace=True, p=tb.weights)
        t0 = np.random.uniform(0.0, 1.0, n) * tb.lengths[mids]
        root, dp, dv, _, _ = R.motion_state(tb, mids, t0)
        e.root_states[ids] = torch.from_numpy(root).to(dev)
        dof[ids] = torch.from_numpy(np.stack([dp, dv], -1)).to(dev)
        e.progress_buf[ids] = 0
        e.reset_buf[ids] = 0
        e._terminate_buf[ids] = 0
        cur = observations(e.root_states[ids], dof[ids][..., 0], dof[ids][..., 1], rb[ids][:, self.key, 0:3].reshape(n, 12),
                           p["local"])
        e.obs_buf[ids] = cur
        e._amp_obs_buf[ids, 0] = cur
        for k in range(1, p["steps"]):
            root, dp, dv, key, _ = R.motion_state(tb, mids, t0 - p["dt"] * k)
            e._amp_obs_buf[ids, k] = observations(*(torch.from_numpy(x).to(dev) for x in (root, dp, dv, key)), p["local"])


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
    ap.add_argument("--episode", type=int, default=60)
    ap.add_argument("--profile-run", action="store_true", help="path (a) alone, for a profiler's kernel trace")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "amp_bench needs the MI355X"
    dev = "cuda:0"
    cfg = configs.task_config("HumanoidAMP", a.envs, overrides={
        "env.asset": {"modelTable": R.MODEL_TABLE}, "env.motion_file": R.MOTIONS_YAML, "env.episodeLength": a.episode})
    env = migym.make(seed=0, task="HumanoidAMP", num_envs=a.envs, sim_device=dev, rl_device=dev, headless=True,
                     cfg={"task": cfg})
    n = env.num_envs
    g = torch.Generator(device=dev).manual_seed(0)
    acts = [torch.rand((n, 28), device=dev, generator=g) * 2 - 1 for _ in range(8)]
    k, resets = [0], [0]
    env.reset_done()

    def task_step():
        env.step(acts[k[0] % 8])
        _, done = env.reset_done()
        resets[0] += len(done)
        k[0] += 1

    for _ in range(a.warmup):
        task_step()
    torch.cuda.synchronize()
    if a.profile_run:
        for _ in range(a.steps):
            task_step()
        torch.cuda.synchronize()
        print(json.dumps({"tool": "amp_bench", "profile_run": True, "steps": a.steps, "envs": n,
                          "post_bytes_per_env": post_bytes_per_env(env._num_amp_obs_steps)}))
        env.close()
        return
    comp = Composed(env)
    np.random.seed(0)

    def composed_step():
        comp.step(acts[k[0] % 8])
        k[0] += 1

    for _ in range(a.warmup):
        composed_step()
    torch.cuda.synchronize()
    paths = {"task_step": task_step, "composed_step": composed_step}
    times = {p: [] for p in paths}
    resets[0] = 0
    for start in range(0, a.steps, 50):
        for p, f in paths.items():
            times[p] += timed(f, min(50, a.steps - start))
    res = {"tool": "amp_bench", "envs": n, "steps": a.steps, "episode": a.episode,
           "finite": bool(torch.isfinite(env.obs_buf).all()), "task_resets_per_step": resets[0] / a.steps}
    for p, t in times.items():
        res[p + "_ms"] = stats(t)
        res[p + "_env_steps_per_s"] = n / (np.median(t) * 1e-3)
    res["post_bytes_per_env"] = post_bytes_per_env(env._num_amp_obs_steps)
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
