"""The step kernels' contact lists against the fp64 oracle's, contact by contact (mg_debug_contacts).

Every other GPU physics test sees collide() through a whole mg_sim_simulate and its 2e-4 m / 2e-3 m/s tolerances.
mg_debug_contacts runs the first substep of the instance mg_sim_simulate launches up to and including collide() and
writes the list out; tests/contacts_ref.py compares it with the oracle's: the same ids in the same order, gaps, points
and normals within 4 x the error of the oracle's fp32 twin (tests/test_contacts_host.py), exemptions only inside the
oracle's threshold band and ambiguity marks and capped.  State sets: the hand tests' (palm, forearm, exact hull,
curled fingers), every tree_physics_ref case dropped and settled, Ant and Humanoid on their feet in both layouts, two
truncated lists, and lists cut by max_contacts inside every part of collide() (contacts_ref.CUTS); and the read-out
leaves no trace in the state or in a later simulate.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import contacts_ref as CR
import tree_physics_ref as TP
from migym import _abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 48   # rows per actor of the read-out: the largest instance's contact capacity


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


def T(a):
    return torch.as_tensor(np.array(a)).to(DEV, torch.float32).contiguous()   # (a copy: some sets are read-only)


def stream():
    return torch.cuda.current_stream().cuda_stream


def _loco_views(spec, root, dof, act):
    n = len(root)
    d = dict(root=T(root), dof=T(dof), act=T(act), sensors=torch.zeros((n, max(len(spec.sensors), 1) * 6), device=DEV),
             dof_force=torch.zeros((n, spec.num_dofs), device=DEV))
    v = _abi.StateViews()
    v.root_states, v.dof_state, v.dof_actuation = d["root"].data_ptr(), d["dof"].data_ptr(), d["act"].data_ptr()
    v.sensors, v.dof_force = d["sensors"].data_ptr(), d["dof_force"].data_ptr()
    return d, v


def _hand_views(h):
    from test_gpu_hand import DevHandEnv
    e = DevHandEnv(copy.deepcopy(h))
    d = dict(root=e.root, dof=e.dof, targets=e.targets, sensors=e.sensors, dof_force=e.dof_force, rbs=e.rbs)
    return d, e.views(), e


def read_contacts(lib, mnp, sp, n, make_views, cap=CAP, simulate=False):
    """(per-env lists, team lanes, compact, state after a following simulate or None): mg_debug_contacts twice from
    freshly bound states (bit-identical, state tensors untouched), then optionally mg_sim_simulate"""
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    try:
        t, lay = C.c_int32(), C.c_int32()
        _abi.check(lib.mg_sim_kernel_layout(sim, C.byref(t), C.byref(lay)), lib)
        d, v, *keep = make_views()
        before = {k: x.clone() for k, x in d.items()}
        _abi.check(lib.mg_sim_bind(sim, C.byref(v)), lib)
        runs = []
        for _ in range(2):
            out = torch.full((n, cap, 11), float("nan"), device=DEV)
            cnt = torch.full((n,), -1, dtype=torch.int32, device=DEV)
            _abi.check(lib.mg_debug_contacts(sim, out.data_ptr(), cnt.data_ptr(), cap, stream()), lib)
            torch.cuda.synchronize()
            runs.append((out.cpu().numpy(), cnt.cpu().numpy()))
        for k, x in d.items():
            assert torch.equal(x, before[k]), f"the read-out changed the {k} tensor"
        after = None
        if simulate:
            _abi.check(lib.mg_sim_simulate(sim, stream()), lib)
            torch.cuda.synchronize()
            after = {k: x.cpu().numpy() for k, x in d.items()}
    finally:
        lib.mg_sim_destroy(sim)
    (o0, c0), (o1, c1) = runs
    np.testing.assert_array_equal(c0, c1)
    np.testing.assert_array_equal(o0, o1)   # NaN-filled past each count on both: equal as bits
    kept = min(sp.max_contacts, cap)
    assert (c0 >= 0).all() and (c0 <= kept).all(), (c0.min(), c0.max())
    lists = [o0[a, :c0[a]].astype(np.float64) for a in range(n)]
    assert all(np.isfinite(x).all() for x in lists)
    assert all(np.isnan(o0[a, c0[a]:]).all() for a in range(n)), "rows past the count were written"
    return lists, t.value, lay.value, after


def _simulate_alone(lib, mnp, sp, n, make_views):
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), n, 0, C.byref(sim)), lib)
    try:
        d, v, *keep = make_views()
        _abi.check(lib.mg_sim_bind(sim, C.byref(v)), lib)
        _abi.check(lib.mg_sim_simulate(sim, stream()), lib)
        torch.cuda.synchronize()
        return {k: x.cpu().numpy() for k, x in d.items()}
    finally:
        lib.mg_sim_destroy(sim)


# ------------------------------------------------------------------------------------------------ hand
@pytest.mark.parametrize("name", CR.HAND_SETS)
def test_hand_contacts_match_oracle(lib, name):
    """the palm, near-forearm, exact-hull and curled-finger sets of tests/test_gpu_hand.py, 256 envs each"""
    spec, sp, mnp, root, dof, h = CR.hand_set(name)
    n = len(root)
    reach = CR.hand_reach(name)
    if name.startswith("forearm"):
        assert reach["hull"] >= 64, reach      # test_hand_physics_near_forearm_matches_oracle: 16 of its first 64
    if name.startswith("hull"):
        assert reach["hull"] >= n // 2, reach  # test_hand_physics_hull_exact_matches_oracle
    if name == "fingers":
        assert reach["pairs"] >= n // 2, reach
    got, lanes, compact, _ = read_contacts(lib, mnp, sp, n, lambda: _hand_views(h))
    assert (lanes, compact) == (32, 0)
    lists = CR.cached_lists(("hand", name), mnp, sp, root, dof)
    CR.compare(f"test_hand_contacts_match_oracle[{name}]", got, lists, CR.kind_of(name),
               mark_cap=CR.MARK_CAP_HULL if name.startswith("hull") else CR.MARK_CAP)


def test_hand_sets_reach_seg_mtd_mpr_and_box_edges():
    """the sets above hold an egg over a capsule's core (convex.hpp seg_mtd), an egg more than 1 mm into a box (MPR)
    and an edge-edge contact of the cube (box_box_edge), found with the oracle"""
    egg = [CR.hand_reach(f"{w}-egg") for w in ("palm", "forearm")]
    assert sum(r["seg_mtd"] for r in egg) >= 1 and sum(r["mpr"] for r in egg) >= 1, egg
    assert sum(CR.hand_reach(f"{w}-block")["edge"] for w in ("palm", "forearm", "hull")) >= 1


# ------------------------------------------------------------------------------------------------ trees
@pytest.mark.parametrize("kind", TP.KINDS)
@pytest.mark.parametrize("name", list(TP.CASES))
def test_tree_contacts_match_oracle(lib, name, kind):
    """every tree_physics_ref case at 66 actors: box corners on the ground, the second geom round, more candidates
    than lanes, the one-actor-per-wave team"""
    case = TP.CASES[name]
    spec, sp, mnp, root, dof, act = CR.tree_set(case, kind)
    got, lanes, compact, _ = read_contacts(lib, mnp, sp, len(root), lambda: _loco_views(spec, root, dof, act))
    from test_gpu_tree_physics import _assert_instance
    _assert_instance(case, lanes, compact)
    lists = CR.cached_lists(("tree", name, kind), mnp, sp, root, dof)
    CR.compare(f"test_tree_contacts_match_oracle[{name}-{kind}]", got, lists, "none")


# ------------------------------------------------------------------------------------------------ task models
@pytest.mark.parametrize("layout", ["classic", "compact"])
@pytest.mark.parametrize("task,n", [("Ant", 256), ("Humanoid", 128)])
def test_task_contacts_match_oracle_in_both_layouts(lib, task, n, layout, monkeypatch):
    """Ant and Humanoid on their feet after a short oracle rollout, MIGYM_LAYOUT pinned: the compact layout stages the
    geom frames (and the 16-lane one the gaps) over the poses in region A"""
    monkeypatch.setenv("MIGYM_LAYOUT", layout)
    spec, sp, tp, mnp, root, dof, act = CR.task_set(task, n)
    got, lanes, compact, _ = read_contacts(lib, mnp, sp, n, lambda: _loco_views(spec, root, dof, act))
    assert compact == (layout == "compact")
    lists = CR.cached_lists(("task", task, n), mnp, sp, root, dof)
    st = CR.compare(f"test_task_contacts_match_oracle_in_both_layouts[{task}-{layout}]", got, lists, "none")
    assert st["contacts"] >= n // 2


# ------------------------------------------------------------------------------------------------ truncation
def test_truncated_hand_list_is_the_oracles_prefix(lib):
    """max_contacts 4 on the palm-block states (up to 17 contacts): the kernel keeps the first 4 of the full list"""
    spec, sp, mnp, root, dof, h = CR.hand_set("palm-block")
    lists = CR.cached_lists(("hand", "palm-block"), mnp, sp, root, dof)
    assert sum(1 for r, m, _ in lists if ((m & CR.BAND_OUT) == 0).sum() > 4) >= 16
    sp4 = CR.with_max_contacts(sp, 4)
    got, _, _, _ = read_contacts(lib, mnp, sp4, len(root), lambda: _hand_views(h))
    assert max(len(g) for g in got) == 4
    CR.compare("test_truncated_hand_list_is_the_oracles_prefix", got, lists, "block", max_contacts=4)


def test_truncated_tree_list_is_the_oracles_prefix(lib):
    """max_contacts 4 on a tree case whose states hold more: ground candidates of several geoms, then pairs"""
    case = TP.CASES["T32-free"]
    spec, sp, mnp, root, dof, act = CR.tree_set(case, "settled")
    lists = CR.cached_lists(("tree", "T32-free", "settled"), mnp, sp, root, dof)
    assert sum(1 for r, m, _ in lists if ((m & CR.BAND_OUT) == 0).sum() > 4) >= 16
    sp4 = CR.with_max_contacts(sp, 4)
    got, lanes, _, _ = read_contacts(lib, mnp, sp4, len(root), lambda: _loco_views(spec, root, dof, act))
    assert lanes == case.lanes and max(len(g) for g in got) == 4
    CR.compare("test_truncated_tree_list_is_the_oracles_prefix", got, lists, "none", max_contacts=4)


@pytest.mark.parametrize("cut", CR.CUTS, ids=CR.cut_id)
def test_list_cut_in_every_phase_is_the_oracles_prefix(lib, cut, monkeypatch):
    """max_contacts = k with the cut inside one part of collide() (contacts_ref.CUTS): each pass's own capacity guard
    drops a contact in at least CUT_ENVS envs (asserted from the oracle's list), the overflow trees' at the last slot
    of the per-team arrays (k = MC), Ant and Humanoid on the compact layout"""
    phase, where, k = cut
    if phase == "compact":
        monkeypatch.setenv("MIGYM_LAYOUT", "compact")
    spec, sp, mnp, root, dof, extra, kind, key = CR.cut_set(where)
    assert len(CR.cut_envs(cut)) >= CR.CUT_ENVS
    lists = CR.cached_lists(key, mnp, sp, root, dof)
    views = (lambda: _hand_views(extra)) if where.startswith("hand") else (lambda: _loco_views(spec, root, dof, extra))
    got, lanes, compact, _ = read_contacts(lib, mnp, CR.with_max_contacts(sp, k), len(root), views)
    assert compact == (phase == "compact") and max(len(g) for g in got) == k
    if where.startswith("tree") and where.endswith("overflow"):
        assert k <= sp.max_contacts and all(len(g) == k for g in got)   # every overflow state fills the list
    CR.compare(f"test_list_cut_in_every_phase_is_the_oracles_prefix[{CR.cut_id(cut)}]", got, lists, kind,
               max_contacts=k, mark_cap=CR.MARK_CAP_HULL if where.startswith("hand:hull") else CR.MARK_CAP)


# ------------------------------------------------------------------------------------------------ non-interference
@pytest.mark.parametrize("which", ["hand-egg", "Humanoid-compact"])
def test_read_out_leaves_no_trace(lib, which, monkeypatch):
    """two read-outs are bit-identical and leave the state tensors as they were (read_contacts); a simulate after a
    read-out gives the bits of a simulate without one"""
    if which == "hand-egg":
        spec, sp, mnp, root, dof, h = CR.hand_set("palm-egg")
        mk = lambda: _hand_views(h)
    else:
        monkeypatch.setenv("MIGYM_LAYOUT", "compact")
        spec, sp, tp, mnp, root, dof, act = CR.task_set("Humanoid", 128)
        mk = lambda: _loco_views(spec, root, dof, act)
    n = len(root)
    _, _, _, after = read_contacts(lib, mnp, sp, n, mk, simulate=True)
    alone = _simulate_alone(lib, mnp, sp, n, mk)
    moved = False
    for k in alone:
        np.testing.assert_array_equal(after[k], alone[k], err_msg=f"{k}: a simulate after the read-out differs")
        moved |= k == "dof" and not np.array_equal(alone[k], np.asarray(dof, np.float32))
    assert moved


def test_read_out_rejects_bad_arguments(lib):
    spec, sp, tp, mnp, root, dof, act = CR.task_set("Ant", 256)
    sim = C.c_void_p()
    _abi.check(lib.mg_sim_create(mnp.ctypes.data, C.byref(sp), 256, 0, C.byref(sim)), lib)
    try:
        out = torch.zeros((256, CAP, 11), device=DEV)
        cnt = torch.zeros(256, dtype=torch.int32, device=DEV)
        assert lib.mg_debug_contacts(sim, out.data_ptr(), cnt.data_ptr(), CAP, stream()) == -1
        assert b"not bound" in lib.mg_last_error()
        d, v = _loco_views(spec, root, dof, act)
        _abi.check(lib.mg_sim_bind(sim, C.byref(v)), lib)
        assert lib.mg_debug_contacts(sim, out.data_ptr(), cnt.data_ptr(), sp.max_contacts - 1, stream()) == -1
        assert b"cap" in lib.mg_last_error()
        _abi.check(lib.mg_debug_contacts(sim, out.data_ptr(), cnt.data_ptr(), CAP, stream()), lib)
        torch.cuda.synchronize()
    finally:
        lib.mg_sim_destroy(sim)
