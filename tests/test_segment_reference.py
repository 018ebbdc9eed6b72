"""The yardstick of the hub route (tests/segment_reference.py) against the CPU oracle: the same bits wherever no row exceeds 512
entries, the oracle's value within the element-wise bound on hub rows, and the expected bits on a row whose segment sums are known
in closed form.  No GPU."""
import numpy as np
import pytest

import segment_reference as sr
from helpers import (HUB_LENGTHS, assert_close_elementwise, graph_from_lengths, hub_length_layout, spread_lengths)

N = 1500


def _square(hub_rows, hub_cols, seed, edge_cols=0):
    """square graph with implicit degrees: every listed column has a row of its own with entries (finite coefficients)"""
    rng = np.random.default_rng(seed)
    lay = hub_length_layout(N, rng)
    nz = lay > 0
    if hub_rows:
        row_len = lay
        col_len = np.zeros(N, np.int64)
        col_len[nz] = np.roll(lay[nz], 5) if hub_cols else spread_lengths(int(lay.sum()), nz)[nz]
    else:
        col_len = lay if hub_cols else np.minimum(lay, 512)
        row_len = spread_lengths(int(col_len.sum()), col_len > 0)
    ia, ja = graph_from_lengths(row_len, col_len, rng, edge_cols)
    assert np.array_equal(np.bincount(ja[0] - 1, minlength=N), col_len)
    assert (np.diff(ia)[ja[0] - 1] > 0).all()
    return ia, ja


def _operands(seed, F, Fe=3, E=40):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (N, F)).astype(np.float32), rng.uniform(-1, 1, (N, F)).astype(np.float32),
            rng.uniform(-1, 1, (E, Fe)).astype(np.float32))


def _rect(ia, ja, seed):
    rng = np.random.default_rng(seed)
    return (np.diff(ia) + rng.integers(1, 4, N)).astype(np.int32), rng.integers(1, 60, N).astype(np.int32)


@pytest.mark.parametrize("F", [1, 5, 64])
def test_without_hub_rows_the_yardstick_is_the_oracle(oracle, F):
    """no row and no column above 512 entries (both hold one of exactly 512): every op, bit for bit"""
    ia, ja = _square(False, False, seed=3, edge_cols=40)
    assert np.diff(ia).max() <= 512 and np.bincount(ja[0] - 1).max() == 512
    ia2, ja2 = sr.transpose(ia, ja, N)                       # ... and its transpose: a ROW of exactly 512
    assert np.diff(ia2).max() == 512
    x, gr, e = _operands(F, F)
    for a, j in ((ia, ja), (ia2, ja2)):
        assert np.array_equal(sr.kipf_propagate(x, a, j), oracle.kipf_propagate(x, a, j))
        rd, cd = _rect(a, j, 4)
        assert np.array_equal(sr.kipf_propagate(x, a, j, rd, cd), oracle.kipf_propagate_rect(x, a, j, rd, cd))
        for exact in (False, True):
            assert np.array_equal(sr.kipf_propagate_bwd(gr, a, j, exact=exact), oracle.kipf_propagate_bwd(gr, a, j, exact=exact))
        c = oracle.duvenaud_propagate(x, e, a, j)
        assert np.array_equal(sr.duvenaud_propagate(x, e, a, j), c)
        assert np.array_equal(sr.neighbour_sum(x, a, j), c[:, :F])
        assert np.array_equal(sr.duvenaud_propagate(None, e, a, j), c[:, F:])
        up = np.concatenate([gr, gr[:, :3]], axis=1)
        assert np.array_equal(sr.duvenaud_propagate_bwd_x(up, F, a, j), oracle.duvenaud_propagate_bwd_x(up, F, a, j))


@pytest.mark.parametrize("F", [1, 5, 64])
@pytest.mark.parametrize("hub_rows", [True, False])
def test_with_hub_rows_the_yardstick_is_the_oracle_but_for_association(oracle, hub_rows, F):
    """every length of HUB_LENGTHS as a row length (hub_rows) or as a column count: the oracle's bits on every row of at most 512
    entries, and on the hubs the oracle's value within 1e-5 of the magnitude of each element's own terms (the oracle run on
    |operands|).  The other side of each graph is spread evenly, so a hub sums ~L different rows.  (With hub rows AND hub columns in
    one graph a hub row lists the same few hub columns hundreds of times each; the sequential fp32 sum of such a row is itself
    1.1e-5 of its term magnitudes from the float64 value -- the yardstick 1.7e-6 -- and the bound would measure the oracle.)"""
    ia, ja = _square(hub_rows, not hub_rows, seed=5, edge_cols=40)
    deg, cdeg = np.diff(ia), np.bincount(ja[0] - 1, minlength=N)
    assert set(HUB_LENGTHS) <= set((deg if hub_rows else cdeg).tolist()) and (cdeg if hub_rows else deg).max() <= 512
    short, cshort = deg <= 512, cdeg <= 512
    x, gr, e = _operands(10 + F, F)

    def check(got, ref, mag, keep, what):
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert np.array_equal(got[keep], ref[keep]), what
        assert_close_elementwise(got[~keep], ref[~keep], mag[~keep], 1e-5, what)
        assert keep.all() or not np.array_equal(got[~keep], ref[~keep]), f"{what}: the two associations should differ on these operands"

    check(sr.kipf_propagate(x, ia, ja), oracle.kipf_propagate(x, ia, ja), oracle.kipf_propagate(np.abs(x), ia, ja), short, "fwd")
    rd, cd = _rect(ia, ja, 6)
    check(sr.kipf_propagate(x, ia, ja, rd, cd), oracle.kipf_propagate_rect(x, ia, ja, rd, cd),
          oracle.kipf_propagate_rect(np.abs(x), ia, ja, rd, cd), short, "fwd, explicit degrees")
    for exact in (False, True):
        check(sr.kipf_propagate_bwd(gr, ia, ja, exact=exact), oracle.kipf_propagate_bwd(gr, ia, ja, exact=exact),
              oracle.kipf_propagate_bwd(np.abs(gr), ia, ja, exact=exact), cshort, f"bwd exact={exact}")
    check(sr.duvenaud_propagate(x, e, ia, ja), oracle.duvenaud_propagate(x, e, ia, ja),
          oracle.duvenaud_propagate(np.abs(x), np.abs(e), ia, ja), short, "duvenaud_propagate")
    up = np.concatenate([gr, gr[:, :3]], axis=1)
    check(sr.duvenaud_propagate_bwd_x(up, F, ia, ja), oracle.duvenaud_propagate_bwd_x(up, F, ia, ja),
          oracle.duvenaud_propagate_bwd_x(np.abs(up), F, ia, ja), cshort, "duvenaud_propagate_bwd_x")


def test_the_cut_is_at_512_entries_from_the_rows_first_entry(oracle):
    """the same graph cut at 511 gives other bits on every hub row: the graphs of these tests can tell.  (A last segment of ONE entry
    adds that entry to the sum before it, as the sequential sum does: a 512-entry row cut at 511 keeps its bits, and the 513-entry
    row has the oracle's bits under the real cut -- its place in the tests is the plan, n_tasks = 2 with a one-entry task.)"""
    ia, ja = _square(True, False, seed=5)
    x = _operands(7, 8)[0]
    y = sr.kipf_propagate(x, ia, ja)
    y511 = sr.kipf_propagate(x, ia, ja, k_long=511)
    for L in HUB_LENGTHS:
        rows = np.nonzero(np.diff(ia) == L)[0]
        assert rows.size and (L <= 512) == np.array_equal(y[rows], y511[rows]), L
    beg, end, row, nth = sr.split_rows(np.asarray(ia, np.int64) - 1)
    assert {int(L): int(c) for L, c in zip(np.diff(ia), np.bincount(row)) if L in HUB_LENGTHS} == \
        {0: 1, 1: 1, 511: 1, 512: 1, 513: 2, 1023: 2, 1024: 2, 1025: 3, 1536: 3, 1537: 4, 2600: 6}
    r513 = int(np.nonzero(np.diff(ia) == 513)[0][0])
    assert (end - beg)[row == r513].tolist() == [512, 1]
    assert np.array_equal(y[r513], oracle.kipf_propagate(x, ia, ja)[r513])


def test_a_row_of_1025_entries_with_segment_sums_in_closed_form(oracle):
    """powers of two, so that every sum is known exactly.  Column 0: 2^24, then 1023 ones, then 2.  Entry by entry every 1 is
    absorbed (2^24 + 1 ties to even, back to 2^24) and the sum ends at 2^24 + 2; the segments are 2^24 (511 ones absorbed), 512 and
    2, and ((2^24 + 512) + 2) = 2^24 + 514.  Column 1: all ones, 1025 either way.  Column 2: 1024 ones, then 2^24: 2^24 + 1024 either
    way
    (row 2 lists columns 1 and 1025: 2^24 + 2, 2, and 1 + 2^24 -> 2^24).  With degrees 4 x 4 every Kipf coefficient is 16^-1/2 = 0.25 exactly and scales each term by a power of two."""
    L = 1025
    ia = np.array([1, 1 + L, 1 + L + 2], np.int32)               # row 1: the hub over columns 1..1025; row 2: two entries
    ja = np.zeros((2, L + 2), np.int32, order="F")
    ja[0, :L] = np.arange(1, L + 1)
    ja[0, L:] = [1, L]
    x = np.ones((L, 3), np.float32)
    x[0, 0], x[L - 1, 0] = 2.0 ** 24, 2.0
    x[L - 1, 2] = 2.0 ** 24
    plain = sr.neighbour_sum(x, ia, ja)
    assert plain.tolist() == [[2.0 ** 24 + 514, 1025.0, 2.0 ** 24 + 1024], [2.0 ** 24 + 2, 2.0, 2.0 ** 24]]
    sequential = oracle.kipf_propagate_rect(x, ia, ja, np.ones(2, np.int32), np.ones(L, np.int32))    # coefficient 1: the plain sum
    assert sequential.tolist() == [[2.0 ** 24 + 2, 1025.0, 2.0 ** 24 + 1024], [2.0 ** 24 + 2, 2.0, 2.0 ** 24]]
    rd, cd = np.full(2, 4, np.int32), np.full(L, 4, np.int32)
    y = sr.kipf_propagate(x, ia, ja, rd, cd)
    assert y.dtype == np.float32 and np.array_equal(y, np.float32(0.25) * plain)
    assert np.array_equal(oracle.kipf_propagate_rect(x, ia, ja, rd, cd), np.float32(0.25) * sequential)
    # the transposed side: the same graph transposed has a hub COLUMN, gathered over the rows 1..1025 in order
    t_ia, t_ja = sr.transpose(ia, ja, L)
    g = np.ones((L, 3), np.float32)
    g[0, 0], g[L - 1, 0] = 2.0 ** 24, 2.0
    d = sr.kipf_propagate_bwd(g, t_ia, t_ja, n_out=2, row_deg=cd, col_deg=rd)
    assert d[0].tolist() == [2.0 ** 24 + 514, 1025.0, 1025.0] and d[1].tolist() == [2.0 ** 24 + 2, 2.0, 2.0]
    de = sr.kipf_propagate_bwd(g, t_ia, t_ja, exact=True, n_out=2, row_deg=cd, col_deg=rd)
    assert np.array_equal(de, np.float32(0.25) * d)
