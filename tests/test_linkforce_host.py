"""The inputs of tests/test_gpu_linkforce.py, admitted on the CPU by the reference alone (tests/linkforce_ref.py).

  * The momentum identity holds for the fp64 oracle and for its fp32 twin on the passive copies of the quadcopter,
    Anymal and AMP models, on the contact-free states the GPU test uses; both residuals go to the parity report.  The
    residual is relative to the impulse h M |a| with |P| / (h M |a|) about 25 (|v| about 1 m/s, h |a| about 0.04 m/s),
    so a value that passed through fp32 once carries 25 x 2^-24 = 1.5e-6 at most per rounding and far less on
    average: the fp64 oracle, whose inputs and outputs are fp32, is held to 1e-5 and the twin, fp32 throughout, to
    1e-4.  (Measured: 1.6e-6 to 3.9e-6 and 1.2e-6 to 2.6e-6: both sit on the rounding of the fp32 rows the momenta
    are computed from.)  The passive copy is a condition of the identity, not a convenience: drives, dampers, limit
    rows and the angular-velocity cap all change a velocity by something that is not a force on the body.
  * The gravity-equivalence states: contact candidates within capacity before and after, no orc_step_flips flag at g
    or at g + a, at most 5 % of the states drawn passed over; the admitted a moves the oracle's own result out of the
    one-step tolerances in at least a quarter of the states (tests/test_simparams_host.py's rule), so a kernel that
    ignored the forces would fail; and the fp32 twin at g + a passes the comparison the GPU test makes.
"""
import numpy as np
import pytest

import linkforce_ref as LF
import parity_stats as PS
from migym import model as M

CASES = [(m, mode, tgs) for m in LF.LANES for mode in LF.MODES for tgs in (False, True)]


@pytest.mark.parametrize("model", LF.MOMENTUM_MODELS)
def test_momentum_identity_holds_for_the_oracle(model):
    spec, mnp, sp, root, dof, body, axis = LF.momentum_setup(model)
    assert not spec.fixed_base and sp.substeps == 1
    assert sorted(set(body.tolist())) == list(range(len(spec.bodies))) and sorted(set(axis.tolist())) == [0, 1, 2]
    rec = {}
    for name, fp32, bound in (("fp64", False, 1e-5), ("fp32 twin", True, 1e-4)):
        lin, ang = LF.oracle_momentum_residuals(model, fp32)
        rec[name] = {"linear": float(lin.max()), "angular": float(ang.max())}
        print(f"{model} {name}: momentum residual linear {lin.max():.3g}, angular {ang.max():.3g} (bound {bound:g})")
        assert lin.max() <= bound and ang.max() <= bound
    PS._REPORT.setdefault(f"linkforce momentum[{model}]", {})["residuals"] = rec


@pytest.mark.parametrize("model,mode,tgs", CASES)
def test_gravity_equivalence_states_are_admitted(model, mode, tgs):
    spec, mnp, sp0 = LF.setup(model)
    c = LF.case(model, mode, tgs)
    want = max(LF.BATCHES[model])
    assert len(c["idx"]) == want and c["cand"] <= sp0.max_contacts
    passed_over = c["scanned"] - want
    assert passed_over <= LF.DISCARD_CAP * c["scanned"], \
        f"{model}/{mode}: {passed_over} of {c['scanned']} drawn states passed over"
    moved = LF.moved(model, mode, tgs)
    PS._REPORT.setdefault(f"linkforce inputs[{model}-{mode}-{'tgs' if tgs else 'pgs'}]", {})["counts"] = {
        "envs": want, "scanned": c["scanned"], "moved": int(moved.sum()), "most_candidates": c["cand"]}
    assert moved.sum() >= (want + 3) // 4, f"{model}/{mode}: the oracle moves in {moved.sum()} of {want}"
    # the forces are what the mode says: m_b a in the env frame, or turned into each body's own at the state
    m = LF.masses(spec)
    np.testing.assert_allclose(np.linalg.norm(c["f"], axis=2), m[None] * np.linalg.norm(c["a"], axis=1)[:, None],
                               rtol=1e-5, atol=1e-7)
    # the fp32 twin, run at g + a, passes the GPU test's comparison
    twin = LF.Host(spec, c["root"], c["dof"], c["act"], c["tgt"]).simulate_each(mnp, c["sps"], fp32=True)
    LF.compare(f"test_gravity_equivalence_states_are_admitted[{model}-{mode}-{tgs}]", model, mode, tgs, want, twin)


def test_tree_bodies_sit_off_their_nodes():
    """the T16-free copy is the one model whose body frames differ from its node frames: its bodies' COMs are on the
    nodes' COMs, their origins and orientations are not the nodes'"""
    spec = LF.setup("T16-free")[0]
    for b in spec.bodies:
        n = spec.nodes[b.node]
        c = np.asarray(b.pos) + M.qmat(M.qnorm(b.quat)) @ np.asarray(b.com)
        np.testing.assert_allclose(c, n.com, atol=1e-12)
        assert b.mass == n.mass
    assert max(np.linalg.norm(b.pos) for b in spec.bodies) > 0.05
    assert min(abs(M.qnorm(b.quat)[3]) for b in spec.bodies) < 0.9
