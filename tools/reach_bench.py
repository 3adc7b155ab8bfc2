#!/usr/bin/env python3
"""Time the FrankaReachMA control step for 16,384 envs x 4 arms on the GPU, two ways:

  (a) task:      FrankaReachMA.step -- mg_reach_pre, mg_sim_simulate, mg_reach_post, three launches;
  (b) composed:  the step a user could compose before the task existed: torch ops for the action clamp and scaling,
                 mg_osc_torques into dof_actuation[:, :6], mg_sim_simulate, and the post-physics part (progress, the
                 AND-filtered reset, observations, compute_franka_reward, timeouts, the observation clamp) as batched,
                 mask-based torch ops on the device (tests/franka_reach_ref.py's restatement, no host synchronisation).

Each path: warm-up steps, then `--steps` timed control steps with device events around each, the two paths alternating
in blocks of 50 so that both see the same machine state; medians and p10-p90.  The three kernels of (a) are also timed
one by one (events around single launches on the state the steps left).  `--profile-run` runs path (a) alone, for a
kernel trace taken by a profiler in a run of its own (kernel times and k_reach_post's share of the HBM peak come from
that trace, not from events).  Prints one JSON line.  Recorded, not asserted: a tool, not a test.  The model is the
test fixture tests/golden/franka_panda.json.
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
from migym.dynamics import DynamicsTensors  # noqa: E402

FRANKA_JSON = os.path.join(ROOT, "tests", "golden", "franka_panda.json")
HBM_PEAK = 8.0e12   # bytes/s, the MI355X's specified HBM3E bandwidth


def post_bytes_per_env(A, T, clamp=True):
    """what k_reach_post must read and write per env-step, from the shapes (a step without a reset)"""
    no = 10 + 3 * T + 3 * (A - 1)
    read = A * (8 + 8 + 6 * 4 + 7 * 4 + 3 * 4) + T * 3 * 4      # progress, reset, actions, eef pose, hand force; cubes
    write = A * (no * 4 * (2 if clamp else 1) + 4 + 8 + 8 + 1)   # obs (+ clamped), rew, reset, progress, timeout
    return read + write


class Composed:
    """path (b) on the task's own sim and tensors (the two paths never run interleaved within a step)"""

    def __init__(self, env):
        self.e = e = env
        self.rp = rp = e.reach_params
        self.dyn = DynamicsTensors(e._lib, e.sim, e.model_spec, e.num_actors, e.device)
        d = e.device
        self.cmd = torch.tensor(list(rp.cmd_limit), device=d)
        self.default = torch.tensor(list(rp.default_dof_pos), device=d)
        self.lower, self.upper = e.franka_dof_lower_limits, e.franka_dof_upper_limits
        self.N, self.A, self.T, self.nd, self.nb = e.num_envs, e.num_agents, e.num_targets, e.num_dof, e.num_bodies
        self.osc = dict(jac_body=rp.jac_body, arm_dofs=7, kp=list(rp.kp), kd=list(rp.kd), kp_null=list(rp.kp_null),
                        kd_null=list(rp.kd_null), default_dof_pos=list(rp.osc_default_dof_pos),
                        effort_limit=list(rp.effort_limit))

    def step(self, actions):
        e, rp, N, A, T, nd = self.e, self.rp, self.N, self.A, self.T, self.nd
        act = torch.clamp(actions, -rp.clip_actions, rp.clip_actions)
        dpose = (act * self.cmd / rp.action_scale).contiguous()
        eef_vel = e.rigid_body_states.view(N * A, self.nb, 13)[:, rp.eef_body, 7:13]
        self.dyn.osc_torques(dpose, eef_vel, out=e.dof_actuation, out_stride=nd, out_cols=6, **self.osc)
        _abi.check(e._lib.mg_sim_simulate(e.sim, e._stream()), e._lib)
        # post_physics_step, mask-based
        e.progress_buf += 1
        full = (e.reset_buf.view(N, A) != 0).all(1)
        fa = full.repeat_interleave(A)
        uz, uxy, ud = torch.rand(N, T, device=e.device), torch.rand(N, T, 2, device=e.device), \
            torch.rand(N, 9, device=e.device)
        cube = torch.zeros(N, T, 13, device=e.device)
        cube[:, :, 2] = rp.cube_z_base + uz * rp.cube_z_range
        cube[:, :, 0:2] = rp.cube_xy_scale * (uxy - 0.5)
        cube[:, :, 6] = 1.0
        m3 = full.view(N, 1, 1)
        e._init_cubeA_state.copy_(torch.where(m3, cube, e._init_cubeA_state))
        e._cubeA_state.copy_(torch.where(m3, cube, e._cubeA_state))
        pos = torch.max(torch.min(self.default + rp.dof_noise_scale * (ud - 0.5), self.upper), self.lower)
        pos[:, -2:] = self.default[-2:]
        pos = pos.repeat(1, A)
        m2 = full.view(N, 1)
        e._q.copy_(torch.where(m2, pos, e._q))
        e._qd.copy_(torch.where(m2, torch.zeros_like(pos), e._qd))
        e._pos_control.copy_(torch.where(m2, pos, e._pos_control))
        e._effort_control.copy_(torch.where(m2, torch.zeros_like(pos), e._effort_control))
        e.progress_buf.masked_fill_(fa, 0)
        e.reset_buf.masked_fill_(fa, 0)
        c, eef = e._cubeA_state[:, :, :3], e._eef_state
        a = eef[:, :, :3]
        rel = c.unsqueeze(1) - a.unsqueeze(2)
        ids = torch.argmin(rel.norm(dim=-1), dim=-1)
        min_rel = torch.gather(rel, 2, ids.view(N, A, 1, 1).expand(N, A, 1, 3)).squeeze(2)
        targets = c.reshape(N, -1).repeat_interleave(A, dim=0)
        own = torch.cat([eef[:, :, 3:7], a, min_rel], -1).view(N * A, -1)
        flat = a.reshape(N, -1)
        shifted = torch.stack([torch.cat((flat[:, 3 * i:], flat[:, :3 * i]), 1) for i in range(A)], 1)
        e.obs_buf.copy_(torch.cat([targets, own, shifted[..., 3:].reshape(N * A, -1)], -1))
        d = min_rel.reshape(-1, 3).norm(dim=-1)
        rew = 1.0 / (0.5 + d * d) - (act ** 2).sum(-1) * 0.01
        mask = torch.zeros(N, A, device=e.device, dtype=torch.long).scatter_(1, ids, 1)
        touched = (mask.sum(-1) / A).repeat_interleave(A)
        punish = (e._hands_contact_forces.reshape(-1, 3).norm(dim=-1) >= 0.1) * -10.0
        e.rew_buf.copy_(torch.clip(rew + (touched + punish), 0.0, None))
        lim = e.progress_buf >= rp.max_episode_length - 1
        e.reset_buf.copy_(torch.where(lim, torch.ones_like(e.reset_buf), e.reset_buf))
        e.timeout_buf.copy_(lim & (e.reset_buf != 0))
        e.obs_clamped.copy_(torch.clamp(e.obs_buf, -rp.clip_obs, rp.clip_obs))


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
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--arms", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--profile-run", action="store_true", help="path (a) alone, for a profiler's kernel trace")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "reach_bench needs the MI355X"
    dev = "cuda:0"
    cfg = configs.task_config("FrankaReachMA", a.envs, overrides={"env.numAgents": a.arms,
                                                                 "env.asset": {"modelTable": FRANKA_JSON}})
    env = migym.make(seed=0, task="FrankaReachMA", num_envs=a.envs, sim_device=dev, rl_device=dev, headless=True,
                     cfg={"task": cfg})
    n = env.num_actors
    g = torch.Generator(device=dev).manual_seed(0)
    acts = [torch.rand((n, 6), device=dev, generator=g) * 2 - 1 for _ in range(8)]
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
        print(json.dumps({"tool": "reach_bench", "profile_run": True, "steps": a.steps, "actors": n,
                          "post_bytes_per_env": post_bytes_per_env(a.arms, env.num_targets)}))
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
    # the three launches of (a), one by one
    lib, rp, rv, tb = env._lib, _abi.C.byref(env.reach_params), _abi.C.byref(env._task_views), env._tb
    tb.actions = acts[0].data_ptr()
    st = env._stream()
    single = {
        "k_reach_pre": lambda: _abi.check(lib.mg_reach_pre(env.sim, rp, rv, _abi.C.byref(tb), st), lib),
        "k_simulate": lambda: _abi.check(lib.mg_sim_simulate(env.sim, st), lib),
        "k_reach_post": lambda: _abi.check(lib.mg_reach_post(env.sim, rp, rv, _abi.C.byref(tb), None, st), lib),
    }
    res = {"tool": "reach_bench", "envs": a.envs, "arms": a.arms, "actors": n, "steps": a.steps,
           "finite": bool(torch.isfinite(env.obs_buf).all())}
    for p, t in times.items():
        res[p + "_ms"] = stats(t)
        res[p + "_arm_steps_per_s"] = n / (np.median(t) * 1e-3)
    for p, f in single.items():
        for _ in range(5):
            f()
        res[p + "_event_ms"] = stats(timed(f, 100))
    b = post_bytes_per_env(a.arms, env.num_targets)
    res["post_bytes_per_env"] = b
    res["post_event_share_of_hbm_peak"] = b * a.envs / (res["k_reach_post_event_ms"]["median"] * 1e-3) / HBM_PEAK
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
