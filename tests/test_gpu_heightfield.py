"""Heightfield terrain in mg_sim_simulate and mg_height_scan on the GPU (k_simulate_hf, k_contacts_hf, k_height_scan;
DESIGN.md §15).  References and state sets: tests/heightfield_ref.py, admitted on the CPU by
tests/test_heightfield_host.py.  Tolerances are the project's one-step rule (tree_physics_ref.outside through
linkforce_ref.outside) and contacts_ref's BOUNDS["none"]; nothing here is wider.

  1. zero field: within the one-step tolerances of the plain kernel and of the fp64 oracle; after
     mg_sim_set_heightfield(NULL) bit-equal to a sim that never had a field.
  2. level field 0.37 with env origins at oz = 0.37 and random xy: the plane case; free bases also at H = 0.37, oz = 0
     against the oracle at z - 0.37.
  3. planar slopes against the oracle in the frame R^T, 2 substeps, PGS and TGS.
  4. one facet per actor on a 3 x 3 grid, each actor's own R.
  5. rough ground: mg_debug_contacts against the fp64 list of §15's definition, contact by contact.
  6. the same past capacity: the first `cap` of the emission order.
  7. the refusals, and the fused tasks' NotImplementedError.
  8. the height scan, bit for bit outside the rounding band.
  9. through make(): zero and level fields on Anymal.
 10. one launch (2 substeps, PGS and TGS, with and without env origins) on rough ground and on the task's stairs against
     the fp64 oracle stepped on the same field (orc_set_heightfield): contacts of one actor on several facets, facets
     that change between the substeps, and on the stairs tangent_basis_t's second branch (|n.x| >= 0.57735).
 11. four launches chained on the rough field, the oracle restarted from the kernel's own state at each.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import contacts_ref as CR
import heightfield_ref as HF
import linkforce_ref as LF
import parity_stats as PS
from migym import _abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("root", "dof", "sensors", "dof_force", "ncf")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


def T(a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV).contiguous()


class Sim:
    """an mg_sim of n actors; run() binds fresh device copies of a state, sets the field and simulates once"""

    def __init__(self, lib, spec, mnp, sp, n):
        self.lib, self.spec, self.n, self.h, self.keep = lib, spec, n, C.c_void_p(), None
        _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(self.h)), lib)

    def lanes(self):
        t, lay = C.c_int32(), C.c_int32()
        _abi.check(self.lib.mg_sim_kernel_layout(self.h, C.byref(t), C.byref(lay)), self.lib)
        return t.value

    def bind(self, root, dof, act=None, tgt=None, env_props=None, f=None):
        n, spec = self.n, self.spec
        nd, nb, ns = spec.num_dofs, len(spec.bodies), max(len(spec.sensors), 1)
        d = {"root": T(root[:n]), "dof": T(dof[:n]),
             "act_eff": T(act[:n]) if act is not None else torch.zeros((n, nd), device=DEV),
             "tgt": T(tgt[:n]) if tgt is not None else None,
             "sensors": torch.zeros((n, ns * 6), device=DEV), "dof_force": torch.zeros((n, nd), device=DEV),
             "ncf": torch.full((n, nb, 3), float("nan"), device=DEV), "f": f, "env_props": env_props}
        v = _abi.StateViews()
        v.root_states, v.dof_state, v.dof_actuation = d["root"].data_ptr(), d["dof"].data_ptr(), d["act_eff"].data_ptr()
        v.sensors, v.dof_force, v.net_contact_forces = d["sensors"].data_ptr(), d["dof_force"].data_ptr(), d["ncf"].data_ptr()
        v.dof_targets, v.rb_forces = _abi.ptr(d["tgt"]), _abi.ptr(f)
        if env_props is not None:
            v.env_props, v.env_props_stride = env_props.data_ptr(), env_props.shape[1]
        _abi.check(self.lib.mg_sim_bind(self.h, C.byref(v)), self.lib)
        return d

    def field(self, fld):
        """set (a heightfield_ref.Field) or clear (None) the sim's heightfield; the device tensors stay alive here"""
        if fld is None:
            _abi.check(self.lib.mg_sim_set_heightfield(self.h, None), self.lib)
            self.keep = None
            return
        tab = T(fld.H)
        org = None if fld.origins is None else T(fld.origins[:self.n])
        hf = _abi.Heightfield(heights=tab.data_ptr(), nx=fld.nx, ny=fld.ny, dx=fld.dx, x0=fld.x0, y0=fld.y0, hmax=fld.hmax,
                              env_origins=_abi.ptr(org))
        _abi.check(self.lib.mg_sim_set_heightfield(self.h, C.byref(hf)), self.lib)
        self.keep = (tab, org)

    def simulate(self):
        return self.lib.mg_sim_simulate(self.h, torch.cuda.current_stream().cuda_stream)

    def run(self, fld, root, dof, act=None, tgt=None):
        d = self.bind(root, dof, act, tgt)
        self.field(fld)
        _abi.check(self.simulate(), self.lib)
        torch.cuda.synchronize()
        return types.SimpleNamespace(**{k: d[k].cpu().numpy() for k in FIELDS})

    def contacts(self, fld, root, dof, cap):
        d = self.bind(root, dof)     # (held to the end: the sim reads these tensors)
        self.field(fld)
        out = torch.full((self.n, cap, 11), float("nan"), device=DEV)
        cnt = torch.zeros(self.n, dtype=torch.int32, device=DEV)
        _abi.check(self.lib.mg_debug_contacts(self.h, out.data_ptr(), cnt.data_ptr(), cap,
                                              torch.cuda.current_stream().cuda_stream), self.lib)
        torch.cuda.synchronize()
        o, c = out.cpu().numpy(), cnt.cpu().numpy()
        del d
        return [o[e, :c[e]] for e in range(self.n)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.mg_sim_destroy(self.h)


def same_bits(a, b, what):
    for k in FIELDS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{k}: {what}")


def flat_inputs(model, tgs):
    """(spec, mnp, sp, root, dof, act, tgt, ref): linkforce_ref's admitted states of the model (its "env" case holds
    the oracle's step under plain gravity as `base`)"""
    spec, mnp, _ = LF.setup(model)
    c = LF.case(model, "env", tgs)
    return spec, mnp, c["sp"], c["root"], c["dof"], c["act"], c["tgt"], c["base"]


def sides(tgs):
    return "tgs" if tgs else "pgs"


# ------------------------------------------------------------------------------------------------ 1. zero field
ZERO = [(m, tgs, n) for m in ("Quadcopter", "T16-free", "Anymal", "AMP", "Cartpole") for tgs in (False, True)
        for n in (LF.BATCHES[m] if m != "Cartpole" else (9,))]


@pytest.mark.parametrize("model,tgs,n", ZERO)
def test_zero_field_is_the_plane(lib, model, tgs, n):
    spec, mnp, sp, root, dof, act, tgt, ref = flat_inputs(model, tgs)
    zero = HF.Field(np.zeros((9, 9)), 0.5, -2.0, -2.0)
    with Sim(lib, spec, mnp, sp, n) as sim, Sim(lib, spec, mnp, sp, n) as never:
        assert sim.lanes() == LF.LANES[model]
        plain = never.run(None, root, dof, act, tgt)
        got = sim.run(zero, root, dof, act, tgt)
        again = sim.run(zero, root, dof, act, tgt)
        cleared = sim.run(None, root, dof, act, tgt)
    same_bits(got, again, "the second run differs")
    same_bits(cleared, plain, "after mg_sim_set_heightfield(NULL) the sim is not the plain one")
    name = f"test_zero_field_is_the_plane[{model}-{sides(tgs)}-{n}]"
    HF.compare_step(name + " vs k_simulate", spec, got, plain, n)
    HF.compare_step(name + " vs oracle", spec, got, ref, n)


# ------------------------------------------------------------------------------------------------ 2. level and origins
@pytest.mark.parametrize("model,tgs,n", [(m, tgs, n) for m, ns in (("Cartpole", (9, 67)), ("Anymal", (6,)))
                                         for tgs in (False, True) for n in ns])
def test_level_field_with_origins_is_the_plane(lib, model, tgs, n):
    spec, mnp, sp, root, dof, act, tgt, ref = flat_inputs(model, tgs)
    rng = np.random.default_rng(81)
    org = np.concatenate([rng.uniform(-1, 1, (n, 2)), np.full((n, 1), 0.37)], 1)
    fld = HF.Field(np.full((9, 9), 0.37), 0.5, -2.0, -2.0, org)
    with Sim(lib, spec, mnp, sp, n) as sim:
        got = sim.run(fld, root, dof, act, tgt)
    HF.compare_step(f"test_level_field_with_origins_is_the_plane[{model}-{sides(tgs)}-{n}]", spec, got, ref, n)


@pytest.mark.parametrize("model,tgs", [(m, tgs) for m in ("Quadcopter", "T16-free", "Anymal", "AMP") for tgs in (False, True)])
def test_level_field_raises_the_ground(lib, model, tgs):
    """H = 0.37, no origins: the actors raised by 0.37 step as the oracle's do on the plane"""
    spec, mnp, sp, root, dof, act, tgt, ref = flat_inputs(model, tgs)
    n = LF.BATCHES[model][0]
    up = np.array(root[:n])
    up[:, 2] += np.float32(0.37)
    fld = HF.Field(np.full((9, 9), 0.37), 0.5, -2.0, -2.0)
    with Sim(lib, spec, mnp, sp, n) as sim:
        got = sim.run(fld, up, dof, act, tgt)
    got.root[:, 2] -= np.float32(0.37)
    HF.compare_step(f"test_level_field_raises_the_ground[{model}-{sides(tgs)}]", spec, got, ref, n)


# ------------------------------------------------------------------------------------------------ 3. / 4. planes
PLANES = [(m, tgs, n, "slope") for m in HF.SLOPE_MODELS for tgs in (False, True) for n in LF.BATCHES[m]] + \
    [(m, tgs, n, "facets") for m, n in (("Quadcopter", 67), ("Anymal", 6)) for tgs in (False, True)]


@pytest.mark.parametrize("model,tgs,n,kind", PLANES)
def test_planes_match_the_oracle_in_the_rotated_frame(lib, model, tgs, n, kind):
    """Measured (MI355X): see DESIGN.md §15"""
    c = HF.slope_case(model, tgs, kind=kind)
    spec, mnp = c["spec"], c["mnp"]
    assert c["sp"].substeps == 2
    with Sim(lib, spec, mnp, c["sp"], n) as sim:
        assert sim.lanes() == LF.LANES[model]
        got = sim.run(c["fld"], c["world"], c["dof"], c["act"], c["tgt"])
    assert np.abs(got.dof[..., 0] - c["dof"][:n, :, 0]).max() > 1e-4, "the step moved nothing"
    worst = HF.compare_step(f"test_planes[{model}-{sides(tgs)}-{n}-{kind}]", spec, HF.to_flat(c, got, n), c["ref"], n)
    PS._REPORT.setdefault(f"heightfield planes[{model}-{sides(tgs)}-{n}-{kind}]", {})["err_over_tol"] = worst


# ------------------------------------------------------------------------------------------------ 5. / 6. contact lists
_rough = {}


def rough(model, n):
    if (model, n) not in _rough:
        fld = HF.rough_field()
        spec, mnp, sp, root, dof, _, _ = HF.rough_states(model, n, fld, 61)
        _rough[model, n] = fld, spec, mnp, sp, root, dof, HF.contact_lists(spec, mnp, sp, fld, root, dof)
    return _rough[model, n]


@pytest.mark.parametrize("model,n", [("T16-free", 67), ("Anymal", 66)])
def test_rough_ground_contact_lists(lib, model, n):
    fld, spec, mnp, sp, root, dof, lists = rough(model, n)
    with Sim(lib, spec, mnp, sp, n) as sim:
        got = sim.contacts(fld, root, dof, 64)
    st = CR.compare(f"test_rough_ground_contact_lists[{model}]", got, HF.cut_lists(lists, sp.max_contacts), "none",
                    max_contacts=sp.max_contacts)
    print(st)
    assert st["matched"] >= n
    tilted = sum(int((np.abs(g[:, 9]) < 0.999).sum()) for g in got if len(g))
    assert tilted >= n // 2, "the lists hold next to no tilted normals"


def test_rough_ground_past_capacity(lib):
    fld, spec, mnp, sp, root, dof, lists = rough("Anymal", 66)
    counts = np.array([int(((m & CR.BAND_OUT) == 0).sum()) for _, m, _ in lists])
    cap = 3
    assert (counts > cap).sum() >= 8, "too few envs past the capacity"
    spc = CR.with_max_contacts(sp, cap)
    with Sim(lib, spec, mnp, spc, 66) as sim:
        got = sim.contacts(fld, root, dof, 64)
    assert max(len(g) for g in got) == cap
    CR.compare("test_rough_ground_past_capacity", got, lists, "none", max_contacts=cap)


# ------------------------------------------------------------------------------------------------ 10. / 11. stepped fields
STEPPED = [(m, tgs, n, "rough", org) for m in HF.ROUGH_MODELS for tgs in (False, True) for n in LF.BATCHES[m]
           for org in (False, True)] + \
    [(m, tgs, n, "stairs", org) for m in HF.STAIRS_MODELS for tgs in (False, True) for n in LF.BATCHES[m]
     for org in (False, True)]


def first(fld, n):
    return HF.Field(fld.H, fld.dx, fld.x0, fld.y0, None if fld.origins is None else fld.origins[:n])


@pytest.mark.parametrize("model,tgs,n,kind,origins", STEPPED)
def test_stepped_field_matches_the_oracle_on_the_field(lib, model, tgs, n, kind, origins):
    """Measured (MI355X): see DESIGN.md §15"""
    c = HF.rough_case(model, tgs, kind, origins)
    spec, mnp = c["spec"], c["mnp"]
    assert c["sp"].substeps == 2
    with Sim(lib, spec, mnp, c["sp"], n) as sim:
        assert sim.lanes() == LF.LANES[model]
        got = sim.run(first(c["fld"], n), c["root"], c["dof"], c["act"], c["tgt"])
    assert np.abs(got.dof[..., 0] - c["dof"][:n, :, 0]).max() > 1e-4, "the step moved nothing"
    name = f"[{model}-{sides(tgs)}-{n}-{kind}-{'origins' if origins else 'world'}]"
    worst = HF.compare_step("test_stepped_field" + name, spec, got, c["ref"], n)
    PS._REPORT.setdefault("heightfield stepped" + name, {})["err_over_tol"] = worst


@pytest.mark.parametrize("model,tgs", [(m, tgs) for m in ("T16-free", "Anymal") for tgs in (False, True)])
def test_chained_launches_match_the_oracle_at_every_launch(lib, model, tgs):
    """launch k starts from the kernel's output of launch k - 1; the oracle is restarted from that state, which it
    admits by rough_case's conditions (at most 5 % per launch are not).  The oracle's work between the launches is four
    one-actor passes over 67 states per launch; the whole test takes under 0.1 s"""
    c = HF.rough_case(model, tgs)
    spec, mnp, fld = c["spec"], c["mnp"], c["fld"]
    n = len(c["idx"])
    root, dof = c["root"], c["dof"]
    with Sim(lib, spec, mnp, c["sp"], n) as sim:
        for k in range(4):
            got = sim.run(fld, root, dof, c["act"], c["tgt"])
            _, ref, ok = HF.chain_admit(c, root, dof)
            print(f"launch {k}: {int((~ok).sum())} of {n} states not admitted")
            assert (~ok).sum() <= LF.DISCARD_CAP * n
            keep = np.flatnonzero(ok)
            name = f"test_chained_launches[{model}-{sides(tgs)}-launch {k}]"
            worst = HF.compare_step(name, spec, HF.take(got, keep), HF.take(ref, keep), len(keep))
            PS._REPORT.setdefault("heightfield " + name, {})["err_over_tol"] = worst
            assert np.isfinite(got.root).all() and np.isfinite(got.dof).all()
            root, dof = got.root, got.dof


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_state_alone(lib, monkeypatch):
    spec, mnp, sp, root, dof, act, tgt, _ = flat_inputs("Quadcopter", False)
    n = 6
    zero = HF.Field(np.zeros((9, 9)), 0.5, -2.0, -2.0)

    def refused(sim, d, what, call=None):
        before = {k: d[k].clone() for k in ("root", "dof", "dof_force")}
        assert (call or sim.simulate)() != 0, f"{what}: not refused"
        msg = lib.mg_last_error().decode()
        assert "heightfield" in msg, (what, msg)
        torch.cuda.synchronize()
        for k, x in before.items():
            assert torch.equal(d[k], x), f"{what}: {k} was written"

    with Sim(lib, spec, mnp, sp, n) as sim:
        # link forces on
        f = torch.zeros((n, len(spec.bodies), 3), device=DEV)
        d = sim.bind(root, dof, act, tgt, f=f)
        sim.field(zero)
        _abi.check(lib.mg_sim_set_link_forces(sim.h, 1), lib)
        refused(sim, d, "link forces")
        _abi.check(lib.mg_sim_set_link_forces(sim.h, 0), lib)
        assert sim.simulate() == 0
        # env_props bound
        width = lib.mg_env_props_layout(mnp.ctypes.data, None)
        row = np.zeros(width, np.float32)
        _abi.check(lib.mg_env_props_defaults(mnp.ctypes.data, row.ctypes.data), lib)
        d = sim.bind(root, dof, act, tgt, env_props=T(np.tile(row, (n, 1))))
        refused(sim, d, "env_props")
        # the height scan needs a field
        sim.field(None)
        pts, out = T(HF.scan_points()), torch.zeros((n, 140), device=DEV)
        assert lib.mg_height_scan(sim.h, pts.data_ptr(), 140, out.data_ptr(), None) != 0
        assert "no heightfield" in lib.mg_last_error().decode()
    # the compact layout pinned
    monkeypatch.setenv("MIGYM_LAYOUT", "compact")
    with Sim(lib, spec, mnp, sp, n) as sim:
        d = sim.bind(root, dof, act, tgt)
        sim.field(zero)
        refused(sim, d, "MIGYM_LAYOUT=compact")
    monkeypatch.delenv("MIGYM_LAYOUT")
    # a model with a free object
    import simparams_ref as SR
    import test_gpu_hand as GH
    hspec, hmnp, hsp, _ = SR.hand_setup()
    h0 = SR.hand_states("substeps1")[0]
    with Sim(lib, hspec, hmnp, hsp, h0.n) as sim:
        e = GH.DevHandEnv(h0)
        _abi.check(lib.mg_sim_bind(sim.h, C.byref(e.views())), lib)
        sim.field(zero)
        refused(sim, {"root": e.root, "dof": e.dof, "dof_force": e.dof_force}, "a model with a free object")
    # the fused step
    import isaacgymenvs
    env = isaacgymenvs.make(seed=0, task="Ant", num_envs=16, sim_device=DEV, rl_device=DEV, headless=True)
    env.step(env.zero_actions())
    tab16 = torch.zeros((9, 9), device=DEV)
    with pytest.raises(NotImplementedError, match="fused step"):
        env.set_heightfield(tab16, 0.5)
    hf = _abi.Heightfield(heights=tab16.data_ptr(), nx=9, ny=9, dx=0.5, x0=-2.0, y0=-2.0, hmax=0.0, env_origins=None)
    _abi.check(lib.mg_sim_set_heightfield(env.sim, C.byref(hf)), lib)
    before = (env.root_states.clone(), env.dof_state.clone())
    with pytest.raises(_abi.MigymError, match="heightfield"):
        env.step(env.zero_actions())
    torch.cuda.synchronize()
    assert torch.equal(env.root_states, before[0]) and torch.equal(env.dof_state, before[1])
    _abi.check(lib.mg_sim_set_heightfield(env.sim, None), lib)
    env.step(env.zero_actions())
    env.close()


# ------------------------------------------------------------------------------------------------ 8. height scan
@pytest.mark.parametrize("origins", [False, True])
def test_height_scan_matches_the_rule_bit_for_bit(lib, origins):
    spec, mnp, sp = LF.setup("Quadcopter")
    base = HF.rough_field()
    rng = np.random.default_rng(71)
    n = 67
    root = HF.scan_roots(rng, n, base)
    org = HF.scan_origins(rng, n)
    fld = HF.Field(base.H, base.dx, base.x0, base.y0, org if origins else None)
    pts = HF.scan_points()
    want, alts, band = HF.scan(fld, root, pts)
    dof = np.zeros((n, spec.num_dofs, 2), np.float32)
    with Sim(lib, spec, mnp, sp, n) as sim:
        d = sim.bind(root, dof)      # (held to the end: the sim reads these tensors)
        sim.field(fld)
        out = torch.full((n, len(pts)), float("nan"), device=DEV)
        p = T(pts)
        _abi.check(lib.mg_height_scan(sim.h, p.data_ptr(), len(pts), out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), lib)
        torch.cuda.synchronize()
        del d
    got = out.cpu().numpy()
    assert band.mean() <= 0.02
    ok = got == want
    for a in alts:
        ok |= band & (got == a)
    print(f"height scan: {int((got != want).sum())} of {got.size} differ from the fp64 cell, {int(band.sum())} in the band")
    assert ok.all(), f"{int((~ok).sum())} points differ, first {np.argwhere(~ok)[:4].tolist()}"


# ------------------------------------------------------------------------------------------------ 9. through make()
def test_anymal_through_make(lib):
    import anymal_ref as AR
    import isaacgymenvs
    N = 6

    def mk(dz=0.0):
        cfg = AR.task_cfg(N)
        cfg["env"]["baseInitState"]["pos"] = [0.0, 0.0, cfg["env"]["baseInitState"]["pos"][2] + dz]
        return isaacgymenvs.make(seed=0, task="Anymal", num_envs=N, sim_device=DEV, rl_device=DEV, headless=True,
                                 cfg={"task": cfg})
    plain, zero, level = mk(), mk(), mk(0.25)
    zero.set_heightfield(torch.zeros((9, 9), dtype=torch.int16, device=DEV), 0.5, 0.005, origin=(-2.0, -2.0))
    level.set_heightfield(torch.full((9, 9), 50, dtype=torch.int16, device=DEV), 0.5, 0.005, origin=(-2.0, -2.0))
    with pytest.raises(ValueError):
        zero.set_heightfield(torch.zeros(9, device=DEV), 0.5)
    with pytest.raises(ValueError):
        zero.set_heightfield(torch.zeros((9, 9)), 0.5)
    _, _, noise = AR.reset_state(AR.params_from(plain.anymal_params), N, 11)
    for env in (plain, zero, level):
        env.set_reset_noise(T(noise))
    rng = np.random.default_rng(5)
    for t in range(3):
        act = T(rng.uniform(-1, 1, (N, 12)))
        obs = [env.step(act)[0]["obs"].clone() for env in (plain, zero, level)]
        torch.cuda.synchronize()
        r = [env.root_states.cpu().numpy() for env in (plain, zero, level)]
        print(f"step {t}: obs diff zero {float((obs[1] - obs[0]).abs().max()):.3g}, level "
              f"{float((obs[2] - obs[0]).abs().max()):.3g}")
        assert float((obs[1] - obs[0]).abs().max()) <= 1e-6 and np.abs(r[1] - r[0]).max() <= 1e-6
        assert float((obs[2] - obs[0]).abs().max()) <= 1e-6
        assert np.abs(r[2][:, 2] - r[0][:, 2] - 0.25).max() <= 1e-6
    scan = level.height_scan(T(HF.scan_points()))
    assert scan.shape == (N, 140) and float((scan - 0.25).abs().max()) <= 1e-7
    level.clear_heightfield()
    with pytest.raises(_abi.MigymError, match="no heightfield"):
        level.height_scan(T(HF.scan_points()))
    for env in (plain, zero, level):
        env.close()
