"""The inputs of tests/test_gpu_row_sizing.py, admitted by the oracle alone (CPU): the rolled Ant states hold envs at
every constraint-row count the step kernel sizes its row batches and sweeps by, few of them hang on a threshold, and
none was reset in the step that left them.  tools/row_census.py's counts are what both tests read."""
import numpy as np
import pytest

import row_sizing_ref as R


def test_pool_rollout_holds_every_row_count_from_2_to_20():
    """step 12 of the pool-of-4 rollout (Ant 2,048 envs, seed 3): at least four envs at every row count 2 .. 20"""
    h, rows, marginal, was_reset = R.rolled("pool4")
    hist = np.bincount(rows, minlength=21)
    print("rows histogram:", hist.tolist())
    assert all(hist[c] >= R.PER_COUNT for c in range(2, 21)), hist.tolist()


def test_fresh_rollout_holds_the_low_row_counts():
    """step 24 of the fresh-random rollout: at least four envs with no row at all and four with one"""
    h, rows, marginal, was_reset = R.rolled("fresh")
    hist = np.bincount(rows, minlength=2)
    print("rows histogram:", hist.tolist())
    assert hist[0] >= R.PER_COUNT and hist[1] >= R.PER_COUNT, hist.tolist()


@pytest.mark.parametrize("kind", ["pool4", "fresh"])
def test_few_states_hang_on_a_threshold_and_none_was_reset(kind):
    """envs with a contact candidate within 1e-4 of its threshold or a limit comparison within 1e-5 of the margin:
    at most 2 %; envs reset in the step that left the state: at most 1 %; no reset pending"""
    h, rows, marginal, was_reset = R.rolled(kind)
    print(f"{kind}: marginal {marginal.mean():.4f}, reset in the last step {was_reset.mean():.4f}")
    assert marginal.mean() <= R.MARGINAL_CAP
    assert was_reset.mean() <= R.RESET_CAP
    assert not h.reset.any()


def test_placements_cover_the_counts_without_a_pending_reset():
    """the shapes test's two placements: 21 pure waves and 21 mixed ones, every env of the mixed batch also in the
    pure one, the counts as labelled"""
    pure, mixed = R.placements()
    assert len(pure) == len(mixed) == 4 * len(R.COUNTS)
    assert set(mixed) <= set(pure)
    for c in R.COUNTS:
        for kind, i in pure[4 * c:4 * c + 4]:
            assert R.rolled(kind)[1][i] == c and R.rolled(kind)[0].reset[i] == 0
        want = (c, max(c - 1, 0), max(c - 4, 0), 0)
        assert tuple(int(R.rolled(k)[1][i]) for k, i in mixed[4 * c:4 * c + 4]) == want
    g = R.gather(pure)
    assert g.n == len(pure) and not g.reset.any()
