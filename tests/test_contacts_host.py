"""The contact-level comparison (tests/contacts_ref.py) on the CPU: the oracle's fp32 twin through the rule the GPU
tests apply to the kernels (tests/test_gpu_contacts.py).

Per state set: the reference alone stays inside the caps (envs with a threshold-band or ambiguity mark, marked
contacts); its list with the thresholds moved out, less the rows at or above the thresholds, is its plain list; the
twin (liboracle_f32.so, the same C in float) passes with no unexplained env and with every error within a quarter of
contacts_ref.BOUNDS, i.e. the bounds are 4 x the twin's largest error; the hand sets reach the
narrowphase paths the GPU tests are after.  And the rule has teeth: a list with one gap moved by 2e-5 m, one normal
turned by 1e-3 rad, two contacts swapped, one dropped or one geom id changed fails.
"""
import numpy as np
import pytest

import contacts_ref as CR
import tree_physics_ref as TP

TREE_SETS = [(name, kind) for name in TP.CASES for kind in TP.KINDS]


def _twin_check(test, kind, mnp, sp, root, dof, lists, mark_cap=CR.MARK_CAP):
    plain = CR.plain_lists(mnp, sp, root, dof)
    for (rows, marks, _), p in zip(lists, plain):
        np.testing.assert_array_equal(rows[(marks & CR.BAND_OUT) == 0], p)
    st = CR.compare(test, CR.twin_lists(mnp, sp, root, dof), lists, kind, mark_cap=mark_cap)
    assert st["unexplained"] == 0 and st["matched"] > 0
    for q, quarter in zip(CR.QUANT, CR.TWIN_MAX[kind]):
        assert st["max_" + q] <= quarter, f"{test}: the twin's {q} error {st['max_' + q]:.3g} is past {quarter:.3g}"
    return st


@pytest.mark.parametrize("name", CR.HAND_SETS)
def test_twin_hand_contacts_match_oracle(name):
    spec, sp, mnp, root, dof, _ = CR.hand_set(name)
    lists = CR.cached_lists(("hand", name), mnp, sp, root, dof)
    _twin_check(f"test_twin_hand_contacts_match_oracle[{name}]", CR.kind_of(name), mnp, sp, root, dof, lists,
                CR.MARK_CAP_HULL if name.startswith("hull") else CR.MARK_CAP)


def test_hand_sets_reach_the_narrowphase_paths():
    """what test_gpu_contacts.py asserts of its inputs, on the CPU too: hull contacts as the step tests' thresholds
    (64 of 256 near the forearm, half of the hull-exact envs), an egg over a capsule's core (seg_mtd), an egg more
    than 1 mm into a box (MPR), an edge-edge contact of the cube, the finger pairs in most envs"""
    for kind in ("block", "egg", "pen"):
        assert CR.hand_reach(f"forearm-{kind}")["hull"] >= 64
    for kind in ("block", "pen"):
        assert CR.hand_reach(f"hull-{kind}")["hull"] >= 128
    egg = [CR.hand_reach(f"{w}-egg") for w in ("palm", "forearm")]
    assert sum(r["seg_mtd"] for r in egg) >= 1, egg
    assert sum(r["mpr"] for r in egg) >= 1, egg
    assert sum(CR.hand_reach(f"{w}-block")["edge"] for w in ("palm", "forearm", "hull")) >= 1
    assert CR.hand_reach("fingers")["pairs"] >= 128


@pytest.mark.parametrize("name,kind", TREE_SETS)
def test_twin_tree_contacts_match_oracle(name, kind):
    spec, sp, mnp, root, dof, _ = CR.tree_set(TP.CASES[name], kind)
    lists = CR.cached_lists(("tree", name, kind), mnp, sp, root, dof)
    _twin_check(f"test_twin_tree_contacts_match_oracle[{name}-{kind}]", "none", mnp, sp, root, dof, lists)


@pytest.mark.parametrize("task,n", [("Ant", 256), ("Humanoid", 128)])
def test_twin_task_contacts_match_oracle(task, n):
    spec, sp, tp, mnp, root, dof, _ = CR.task_set(task, n)
    lists = CR.cached_lists(("task", task, n), mnp, sp, root, dof)
    st = _twin_check(f"test_twin_task_contacts_match_oracle[{task}]", "none", mnp, sp, root, dof, lists)
    assert st["contacts"] >= n // 2   # the feet are on the ground


def test_truncated_list_is_a_prefix():
    """max_contacts below an env's count: the first rows of the full list pass, the last rows do not"""
    spec, sp, mnp, root, dof, _ = CR.hand_set("palm-block")
    lists = CR.cached_lists(("hand", "palm-block"), mnp, sp, root, dof)
    plain = CR.plain_lists(mnp, sp, root, dof)
    assert max(len(p) for p in plain) > 4
    CR.compare("truncated", [p[:4] for p in plain], lists, "block", max_contacts=4, record=False)
    with pytest.raises(AssertionError):
        CR.compare("truncated", [p[-4:] for p in plain], lists, "block", max_contacts=4, record=False)
    with pytest.raises(AssertionError):
        CR.compare("truncated", [p[:3] for p in plain], lists, "block", max_contacts=4, record=False)


@pytest.mark.parametrize("cut", CR.CUTS, ids=CR.cut_id)
def test_twin_list_cut_in_every_phase(cut):
    """max_contacts = k with the cut inside one part of collide() (contacts_ref.CUTS) in at least CUT_ENVS envs,
    decided from the oracle's list; the twin's list at that capacity is the oracle's prefix, through the unchanged rule.
    And the rule sees a cut one slot late (k + 1 rows where more are due) or early"""
    phase, where, k = cut
    spec, sp, mnp, root, dof, _, kind, key = CR.cut_set(where)
    hits = CR.cut_envs(cut)
    assert len(hits) >= CR.CUT_ENVS, f"{cut}: the cut falls inside the phase in {len(hits)} envs"
    lists = CR.cached_lists(key, mnp, sp, root, dof)
    mark_cap = CR.MARK_CAP_HULL if where.startswith("hand:hull") else CR.MARK_CAP
    test = f"test_twin_list_cut_in_every_phase[{CR.cut_id(cut)}]"
    st = CR.compare(test, CR.twin_lists(mnp, sp, root, dof, cap=k), lists, kind, max_contacts=k, mark_cap=mark_cap)
    CR.PS._REPORT[test]["cut"] = {"envs_in_phase": len(hits), "k": k}
    assert st["unexplained"] == 0 and st["matched"] > 0
    for late in (k + 1, k - 1):
        with pytest.raises(AssertionError):
            CR.compare(test, CR.twin_lists(mnp, sp, root, dof, cap=late), lists, kind, max_contacts=k,
                       mark_cap=mark_cap, record=False)


def _turn(n, angle):
    a = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    return np.cos(angle) * n + np.sin(angle) * a


def _perturbations(plain, lists):
    """the five perturbed copies of the oracle's own lists, each changed in one env at contacts without marks"""
    env = next(e for e, (rows, marks, _) in enumerate(lists)
               if len(rows) >= 2 and not marks.any() and CR._ids(rows[0]) != CR._ids(rows[1]))

    def edit(fn):
        out = [p.copy() for p in plain]
        out[env] = fn(out[env])
        return out

    def gap(r):
        r[0, 10] += 2e-5
        return r

    def normal(r):
        r[0, 7:10] = _turn(r[0, 7:10], 1e-3)
        return r

    def swap(r):
        r[[0, 1]] = r[[1, 0]]
        return r

    def geom(r):
        r[0, 1] += 1
        return r
    return {"gap": edit(gap), "normal": edit(normal), "swapped": edit(swap), "dropped": edit(lambda r: r[1:]),
            "geom id": edit(geom)}


@pytest.mark.parametrize("name", ["palm-block", "palm-egg", "palm-pen", "tree"])
def test_perturbed_lists_fail(name):
    if name == "tree":
        spec, sp, mnp, root, dof, _ = CR.tree_set(TP.CASES["T32-free"], "settled")
        key, kind = ("tree", "T32-free", "settled"), "none"
    else:
        spec, sp, mnp, root, dof, _ = CR.hand_set(name)
        key, kind = ("hand", name), CR.kind_of(name)
    lists = CR.cached_lists(key, mnp, sp, root, dof)
    plain = CR.plain_lists(mnp, sp, root, dof)
    CR.compare("unperturbed", plain, lists, kind, record=False)   # the oracle's own list passes
    for what, got in _perturbations(plain, lists).items():
        if kind == "egg" and what == "normal":
            # the egg's normal bound is 4 x 3.4e-3 (its twin's MPR normals near the medial axis): 1e-3 rad is inside
            CR.compare(what, got, lists, kind, record=False)
            continue
        with pytest.raises(AssertionError):
            CR.compare(what, got, lists, kind, record=False)
