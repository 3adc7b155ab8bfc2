#!/usr/bin/env python3
"""Bit-for-bit comparison of two builds of the library (A/B aid for changes meant to leave every result unchanged,
not a product path).  One process per library (MIGYM_LIB is read at import):

    python tools/bitcmp.py --out a.npz                          # the library in MIGYM_LIB (default: the shipped one)
    MIGYM_LIB=.../var/prev.so python tools/bitcmp.py --out b.npz
    python tools/bitcmp.py --compare a.npz b.npz               # exit status 1 on any differing bit

Each case is a make() rollout with seeded device actions (resets included); the arrays saved are every step's
obs / rew / reset and the final root and DOF state.

Those rollouts reach only the fused step kernels.  ``--simulate`` runs the other set instead: mg_sim_simulate and
mg_debug_contacts driven directly (SIMULATE_CASES: every k_simulate / k_simulate_xf / k_simulate_hf / k_contacts /
k_contacts_hf path, each at a batch that ends in a partial wave), 8 simulate calls from the tests' seeded states under
seeded actuation; the arrays saved are every state view after the last call and the contact read-out before the first.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isaacgymenvs-ma_amd"))

CASES = (("Ant", 4096, "block"), ("Humanoid", 2048, "block"), ("MAAnt", 1024, "block"), ("Cartpole", 256, "block"),
         ("ShadowHand", 1024, "block"), ("ShadowHand", 512, "pen"), ("ShadowHand", 512, "egg"))


def rollout(task, n, obj, steps):
    import torch
    import migym
    from migym import configs
    kw = {}
    if task == "ShadowHand":
        cfg = configs.task_config(task, n, sim_device="cuda:0")
        cfg["env"]["objectType"] = obj
        kw["cfg"] = {"task": cfg}
    env = migym.make(seed=0, task=task, num_envs=n, sim_device="cuda:0", rl_device="cuda:0", headless=True, **kw)
    g = torch.Generator(device="cuda:0").manual_seed(7)
    obs, rew, rst = [], [], []
    for _ in range(steps):
        a = torch.rand((env.num_actors, env.num_actions), device="cuda:0", generator=g) * 2 - 1
        o, r, d, _ = env.step(a)
        obs.append(o["obs"].clone())
        rew.append(r.clone())
        rst.append(d.clone())
    torch.cuda.synchronize()
    out = {"obs": torch.stack(obs).cpu().numpy(), "rew": torch.stack(rew).cpu().numpy(),
           "reset": torch.stack(rst).cpu().numpy(), "root": env.root_states.cpu().numpy(),
           "dof": env.dof_state.cpu().numpy()}
    env.close()
    return out


# --simulate: (name, state set, solvers, options).  State sets: the tests' own (tests/contacts_ref.py task_set / hand_set,
# tests/linkforce_ref.py pool, tests/heightfield_ref.py rough_states); options: layout (MIGYM_LAYOUT), props (env_props
# rows bound), link (link forces in that rb_force_space), rough (the rough field with env origins), contacts (the
# read-out first).  Every batch ends in a partial wave, so the teams past the batch run too.
PGS_TGS = (False, True)
SIMULATE_CASES = (
    ("Cartpole-9", ("pool", "Cartpole", 9), PGS_TGS, {}),
    ("Ant-67-classic", ("task", "Ant", 67), PGS_TGS, {"layout": "classic", "contacts": True}),
    ("Ant-67-compact", ("task", "Ant", 67), PGS_TGS, {"layout": "compact"}),
    ("Humanoid-35-classic", ("task", "Humanoid", 35), PGS_TGS, {"layout": "classic"}),
    ("Humanoid-35-compact", ("task", "Humanoid", 35), PGS_TGS, {"layout": "compact", "contacts": True}),
    ("Ant-67-props", ("task", "Ant", 67), PGS_TGS, {"props": True}),
    ("hand-block-35-props", ("hand", "palm-block", 35), PGS_TGS, {"props": True}),
    ("hand-block-35", ("hand", "palm-block", 35), PGS_TGS, {}),
    ("hand-pen-35", ("hand", "palm-pen", 35), PGS_TGS, {}),
    ("hand-egg-35", ("hand", "palm-egg", 35), PGS_TGS, {"contacts": True}),
    ("Anymal-66-link-env", ("pool", "Anymal", 66), PGS_TGS, {"link": "env"}),
    ("Anymal-66-link-local", ("pool", "Anymal", 66), PGS_TGS, {"link": "local"}),
    ("Anymal-66-rough", ("rough", "Anymal", 66), PGS_TGS, {"rough": True, "contacts": True}),
    ("T16-free-67-rough", ("rough", "T16-free", 67), PGS_TGS, {"rough": True}),
)


def simulate_case(lib, states, tgs, opt, steps):
    """one SIMULATE_CASES row under one solver: {array name: numpy array}"""
    import ctypes as C
    import numpy as np
    import torch
    import contacts_ref as CR
    import heightfield_ref as HF
    import linkforce_ref as LF
    from dr_ref import random_props
    from migym import _abi
    dev = "cuda:0"
    dt = lambda a: None if a is None else torch.tensor(np.asarray(a, dtype=np.float32), device=dev).contiguous()
    kind, model, n = states
    rng = np.random.default_rng(97)
    os.environ["MIGYM_LAYOUT"] = opt.get("layout", "auto")   # read by mg_sim_create
    fld = None
    if kind == "hand":
        from test_gpu_hand import DevHandEnv
        spec, sp, mnp, _, _, h = CR.hand_set(model, n)
        env = DevHandEnv(h)
        env.rb_forces.copy_(dt(rng.normal(0.0, 0.3, tuple(env.rb_forces.shape))))   # the object's row is applied
        v = env.views()
        d = {k: getattr(env, k) for k in ("root", "dof", "sensors", "dof_force", "rbs", "ncf")}
    else:
        act = tgt = None
        if kind == "task":
            spec, sp, _, mnp, root, dof, act = CR.task_set(model, n)
        elif kind == "pool":
            spec, mnp, sp = LF.setup(model)
            root, dof, act, tgt, _ = LF.pool(model)
        else:
            org = rng.uniform(-0.3, 0.3, (n, 3)) * np.array([1.0, 1.0, 0.1])
            fld = HF.rough_field(origins=org)
            spec, mnp, sp, root, dof, act, tgt = HF.rough_states(model, n, fld, 61)
        nd, nb, ns = spec.num_dofs, len(spec.bodies), max(len(spec.sensors), 1)
        d = {"root": dt(root[:n]), "dof": dt(dof[:n]),
             "act": dt(act[:n]) if act is not None else dt(rng.uniform(-1.0, 1.0, (n, nd))),
             "tgt": dt(None if tgt is None else tgt[:n]), "sensors": torch.zeros((n, ns * 6), device=dev),
             "dof_force": torch.zeros((n, nd), device=dev), "rbs": torch.zeros((n, nb, 13), device=dev),
             "ncf": torch.full((n, nb, 3), float("nan"), device=dev)}
        v = _abi.StateViews()
        v.root_states, v.dof_state, v.dof_actuation = d["root"].data_ptr(), d["dof"].data_ptr(), d["act"].data_ptr()
        v.sensors, v.dof_force, v.net_contact_forces = d["sensors"].data_ptr(), d["dof_force"].data_ptr(), d["ncf"].data_ptr()
        v.rigid_body_states, v.dof_targets = d["rbs"].data_ptr(), _abi.ptr(d["tgt"])
        if opt.get("link"):   # non-zero rows: a few body weights each
            m = np.array([b.mass for b in spec.bodies])
            d["f"] = dt(rng.normal(0.0, 30.0, (n, nb, 3)) * m[None, :, None])
            v.rb_forces, v.rb_force_space = d["f"].data_ptr(), int(LF.MODES[opt["link"]][0])
    if opt.get("props"):
        d["props"] = dt(random_props(spec, n, rng))
        v.env_props, v.env_props_stride = d["props"].data_ptr(), d["props"].shape[1]
    sp = LF.sp_at(sp, tgs=tgs)
    if not tgs:
        sp.solver_type = _abi.MG_SOLVER_PGS
    stream = torch.cuda.current_stream().cuda_stream
    sim, out = C.c_void_p(), {}
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    try:
        _abi.check(lib.mg_sim_bind(sim, C.byref(v)), lib)
        if opt.get("link"):
            _abi.check(lib.mg_sim_set_link_forces(sim, 1), lib)
        if fld is not None:
            tab, org = dt(fld.H), dt(fld.origins)
            hf = _abi.Heightfield(heights=tab.data_ptr(), nx=fld.nx, ny=fld.ny, dx=fld.dx, x0=fld.x0, y0=fld.y0,
                                  hmax=fld.hmax, env_origins=org.data_ptr())
            _abi.check(lib.mg_sim_set_heightfield(sim, C.byref(hf)), lib)
        if opt.get("contacts") and not tgs:   # the read-outs have no TGS instance: collide() does not depend on it
            cap = 48
            rows = torch.full((n, cap, 11), float("nan"), device=dev)
            cnt = torch.full((n,), -1, dtype=torch.int32, device=dev)
            _abi.check(lib.mg_debug_contacts(sim, rows.data_ptr(), cnt.data_ptr(), cap, stream), lib)
            out["contact_rows"], out["contact_count"] = rows.cpu().numpy(), cnt.cpu().numpy()
        for _ in range(steps):
            _abi.check(lib.mg_sim_simulate(sim, stream), lib)
        torch.cuda.synchronize()
        for k in ("root", "dof", "sensors", "dof_force", "rbs", "ncf"):
            if d[k] is not None:
                out[k] = d[k].cpu().numpy()
    finally:
        lib.mg_sim_destroy(sim)
    return out


def simulate_set(steps, only=()):
    for p in ("oracle", "tests"):
        sys.path.insert(0, os.path.join(ROOT, p))
    import torch
    from migym import _abi
    assert torch.cuda.is_available()
    lib, arrays = _abi.lib(), {}
    for name, states, solvers, opt in SIMULATE_CASES:
        if only and name not in only:
            continue
        for tgs in solvers:
            tag = f"{name}-{'tgs' if tgs else 'pgs'}"
            for k, x in simulate_case(lib, states, tgs, opt, steps).items():
                arrays[f"{tag}/{k}"] = x
            print(f"{tag}: done", flush=True)
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--simulate", action="store_true", help="the mg_sim_simulate / mg_debug_contacts set (8 steps)")
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--tasks", default="", help="comma-separated task (--simulate: case) names to run (default: every case)")
    a = ap.parse_args()
    import numpy as np
    if a.compare:
        x, y = np.load(a.compare[0]), np.load(a.compare[1])
        bad = 0
        for k in sorted(x.files):
            same = x[k].shape == y[k].shape and np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8))
            if not same:
                bad += 1
                d = np.abs(x[k].astype(np.float64) - y[k].astype(np.float64))
                print(f"DIFF {k}: {np.count_nonzero(d)} elements, max {d.max():.3e}")
        print(f"{len(x.files) - bad} of {len(x.files)} arrays bit-identical")
        sys.exit(1 if bad else 0)
    only = set(t for t in a.tasks.split(",") if t)
    if a.simulate:
        np.savez(a.out, **simulate_set(8, only))
        return
    arrays = {}
    for task, n, obj in CASES:
        if only and task not in only:
            continue
        r = rollout(task, n, obj, a.steps)
        for k, v in r.items():
            arrays[f"{task}-{obj}-{n}/{k}"] = v
        print(f"{task} {obj} {n}: done", flush=True)
    np.savez(a.out, **arrays)


if __name__ == "__main__":
    main()
