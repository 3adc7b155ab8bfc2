#!/usr/bin/env python3
"""Time operational-space control for 16,384 envs x 4 Franka arms on the GPU, two ways:

  (a) fused:    one mg_osc_torques launch from the state into dof_actuation (no J or M in memory);
  (b) tensors:  mg_dynamics_refresh (J and M to memory), then the same math as batched torch ops on the same GPU
                (two batched inverses, as the reference's _compute_osc_torques, franka_reach_MA.py:770-802).

Each path: warm-up launches, then `--launches` timed ones (device events around every launch / op sequence, the two
paths alternating in blocks so that both see the same machine state), the median reported.  Prints one JSON line.
Recorded, not asserted: a tool, not a test.  The model is the test fixture tests/golden/franka_panda.json (hull-density
masses).
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isaacgymenvs-ma_amd"))
from migym import _abi, configs, model as M, taskdefs  # noqa: E402
from migym.dynamics import DynamicsTensors  # noqa: E402

DEFAULT_DOF_POS = [0, 0.1963, 0, -2.6180, 0, 2.9416, 0.7854, 0.035, 0.035]
EFFORT = [87.0] * 4 + [12.0] * 3


def osc_torch(J, Mm, q, qd, dpose, eef_vel, kp, kd, kpn, kdn, default, limit):
    """the controller's math as batched torch ops on the refreshed tensors"""
    Minv = torch.linalg.inv(Mm)
    lam = torch.linalg.inv(J @ Minv @ J.mT)
    u = J.mT @ lam @ (kp * dpose - kd * eef_vel).unsqueeze(-1)
    wrapped = torch.remainder(default - q + math.pi, 2 * math.pi) - math.pi
    un = Mm @ (kdn * -qd + kpn * wrapped).unsqueeze(-1)
    u = u + un - J.mT @ (lam @ (J @ (Minv @ un)))
    return torch.minimum(torch.maximum(u.squeeze(-1), -limit), limit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--arms", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "osc_bench needs the MI355X"
    dev = "cuda:0"
    lib = _abi.lib()
    spec = M.load_json(os.path.join(ROOT, "tests", "golden", "franka_panda.json"))
    n, nd, nb = a.envs * a.arms, spec.num_dofs, len(spec.bodies)
    hand = spec.body_index("panda_hand")
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g) * 2 - 1   # noqa: E731
    root = torch.zeros((n, 13), device=dev)
    ang = (torch.arange(n, device=dev) % a.arms).float() * (2 * math.pi / a.arms)   # arms on a circle, facing in
    root[:, 0], root[:, 1], root[:, 2] = -0.45 * torch.cos(ang), 0.45 * torch.sin(ang), 1.125
    root[:, 5], root[:, 6] = torch.sin(-ang / 2), torch.cos(-ang / 2)
    dof = torch.zeros((n, nd, 2), device=dev)
    dof[..., 0] = torch.tensor(DEFAULT_DOF_POS, device=dev)
    dof[:, :7, 0] += 0.4 * rnd(n, 7)
    dof[:, :7, 1] = rnd(n, 7)
    act = torch.zeros(n * nd, device=dev)
    dpose = rnd(n, 6) * torch.tensor([0.1, 0.1, 0.1, 0.5, 0.5, 0.5], device=dev)
    eef_vel = 0.5 * rnd(n, 6)
    v = _abi.StateViews()
    v.root_states, v.dof_state, v.dof_actuation = root.data_ptr(), dof.data_ptr(), act.data_ptr()
    sp = taskdefs.sim_params(configs.task_config("Cartpole", 4), 8)
    mnp = M.pack_model(spec)
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    _abi.check(lib.mg_sim_bind(sim, C.byref(v)), lib)
    dyn = DynamicsTensors(lib, sim, spec, n, dev)
    J, Mm = dyn.acquire_jacobian(), dyn.acquire_mass_matrix()
    kp, kpn = 150.0, 10.0
    kd, kdn = 2 * math.sqrt(kp), 2 * math.sqrt(kpn)
    default = torch.tensor(DEFAULT_DOF_POS[:7], device=dev)
    limit = torch.tensor(EFFORT, device=dev)
    out_b = [None]

    def fused():
        dyn.osc_torques(dpose, eef_vel, jac_body=hand, arm_dofs=7, kp=kp, kp_null=kpn,
                        default_dof_pos=DEFAULT_DOF_POS[:7], effort_limit=EFFORT, out=act, out_stride=nd, out_cols=7)

    def tensors():
        dyn.refresh()
        out_b[0] = osc_torch(J[:, hand - 1, :, :7], Mm[:, :7, :7], dof[:, :7, 0], dof[:, :7, 1], dpose, eef_vel,
                             kp, kd, kpn, kdn, default, limit)

    def refresh_only():
        dyn.refresh()

    paths = {"fused": fused, "refresh_plus_torch": tensors, "refresh_only": refresh_only}
    for f in paths.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    # the same math in fp64 on the refreshed tensors arbitrates between the two fp32 paths (65,536 random poses reach
    # far worse conditioning than a test fixture's 64: the two explicit fp32 inverses lose digits there)
    d = torch.float64
    ref = osc_torch(J[:, hand - 1, :, :7].to(d), Mm[:, :7, :7].to(d), dof[:, :7, 0].to(d), dof[:, :7, 1].to(d),
                    dpose.to(d), eef_vel.to(d), kp, kd, kpn, kdn, default.to(d), limit.to(d))
    err = {"fused": (act.view(n, nd)[:, :7] - ref).abs().amax(1), "torch_fp32": (out_b[0] - ref).abs().amax(1)}
    err = {k: {"median": float(e.median()), "p99": float(e.quantile(0.99)), "max": float(e.max())}
           for k, e in err.items()}
    times = {k: [] for k in paths}
    block = 50
    for start in range(0, a.launches, block):
        for k, f in paths.items():
            evs = []
            for _ in range(min(block, a.launches - start)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                evs.append((e0, e1))
            torch.cuda.synchronize()
            times[k] += [e0.elapsed_time(e1) for e0, e1 in evs]
    lib.mg_sim_destroy(sim)
    res = {"tool": "osc_bench", "envs": a.envs, "arms": a.arms, "actors": n, "launches": a.launches,
           "abs_err_vs_fp64_torch_Nm": err,
           "jm_bytes_per_arm": 4 * ((nb - 1) * 6 * nd + nd * nd)}
    for k, t in times.items():
        t = np.array(t)
        res[k + "_ms"] = {"median": float(np.median(t)), "p10": float(np.percentile(t, 10)),
                          "p90": float(np.percentile(t, 90))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
