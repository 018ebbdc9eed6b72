"""CPU: the yardstick of the two-set k-nearest-neighbour builder against itself (tests/knn_bipartite_reference.py).  A Python
transcription of knn_bipartite.hip's grid search -- the file header's stop rule for a query that may lie anywhere, in float32 -- is
pinned to the brute-force transcription of the definition on every shape class the GPU tests use: queries inside and outside the
source box, on and beside cell boundaries from two cells below the grid to two above, 1000 box widths out, at +-3e38, around 1e6, on
lattices where the tie rule decides, on coincident sources, with k above the number of sources, capped and not.  One case is built
so that the search is wrong without the margin.  Also: the C ABI, ctypes and Fortran declarations of the new entries agree."""
import functools
import os
import re

import numpy as np
import pytest

import knn_bipartite_reference as kb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"athena_mp_knn_pairs_bipartite": 18, "athena_mp_knn_graph_bipartite_host": 19}
CASES = kb.shape_cases()


@functools.lru_cache(None)
def _brute(c):
    name, q, s, qoff, soff, k, r = CASES[c]
    return kb.brute_force(q, s, k, r, qoff, soff)


@pytest.mark.parametrize("c", range(len(CASES)), ids=[c[0] for c in CASES])
def test_grid_search_with_the_clamped_stop_rule_equals_brute_force(c):
    name, q, s, qoff, soff, k, r = CASES[c]
    assert q.shape[0] * s.shape[0] <= 100000
    want_nbr, want_s = _brute(c)
    nbr, sqd, stats = kb.grid_search(q, s, k, r, qoff, soff)
    print(f"{name}: {stats[1] / max(stats[0], 1):.1f} candidates and {stats[2] / max(stats[0], 1):.1f} cells per query, largest shell {stats[3]}")
    assert np.array_equal(nbr, want_nbr)
    assert np.array_equal(sqd.view(np.int32), want_s.view(np.int32))
    assert (want_nbr > 0).any()
    if "3e38" in name and r is None:
        assert np.isinf(want_s[want_nbr > 0]).any(), "the case must hold squared distances that overflow"
    if "3e38" in name and r is not None:
        assert not want_nbr[-1].any() and want_nbr[0].any(), "the cap leaves a query at +-3e38 without a partner"
    if "cell centres" in name:
        assert (want_s[:, 0] == want_s[:, 1]).all(), "the case must be decided by the tie rule"


def test_batch_equals_the_single_calls():
    q, s, qoff, soff = kb.batch()
    nbr, sqd = kb.brute_force(q, s, 8, None, qoff, soff)
    got, got_s, _ = kb.grid_search(q, s, 8, None, qoff, soff)
    assert np.array_equal(got, nbr) and np.array_equal(got_s.view(np.int32), sqd.view(np.int32))
    for b in range(qoff.size - 1):
        one, _ = kb.brute_force(q[qoff[b]:qoff[b + 1]], s[soff[b]:soff[b + 1]], 8)
        assert np.array_equal(np.where(one > 0, one + soff[b], 0), nbr[qoff[b]:qoff[b + 1]])
    assert not nbr[qoff[2]:qoff[3]].any() and (nbr[qoff[5]:qoff[6]] > 0).sum(1).max() == 1    # no sources / one source


def test_the_margin_is_exercised():
    """the probe: one query whose true nearest source sits in the next cell, hidden from a bound formed without the margin by the
    roundings of the two cell coordinates.  With the margin the search reads that cell; without it, it returns the wrong source."""
    q, s, k, a, b = kb.margin_probe()
    want, _ = kb.brute_force(q, s, k)
    assert want[0, 0] == b + 1
    got, _, stats = kb.grid_search(q, s, k)
    assert np.array_equal(got, want) and stats[3] >= 1
    wrong, _, stats0 = kb.grid_search(q, s, k, margin=0.0)
    assert wrong[0, 0] == a + 1 and stats0[3] == 0, "without the margin the search must stop in its own cell, at the wrong source"


def test_the_clamp_moves_the_cell_coordinate_only_towards_the_grid():
    """on the boundary cases the clamp acts (queries two cells outside), and the search with the unclamped, finite coordinate -- a
    valid, tighter bound -- gives the same lists while examining no more"""
    acted = 0
    for c, (name, q, s, qoff, soff, k, r) in enumerate(CASES):
        if not name.startswith("cell boundaries"):
            continue
        lo, inv_w, nc, _ = kb.kr.make_knn_grid(s)
        g = (q - lo) * inv_w
        acted += int(((g < -2) | (g > nc + 2)).sum())
        nbr, _, st = kb.grid_search(q, s, k, r)
        free, _, st_free = kb.grid_search(q, s, k, r, clamp=False)
        assert np.array_equal(nbr, free) and np.array_equal(nbr, _brute(c)[0]) and st_free[1] <= st[1]
    assert acted > 0


def test_graph_of_orders_rows_by_index():
    q = np.array([[0.0], [10.0]], np.float32)
    s = np.array([[3.0], [0.5], [9.0], [-0.25]], np.float32)
    nbr, sqd = kb.brute_force(q, s, 3)
    assert nbr.tolist() == [[4, 2, 1], [3, 1, 2]] and sqd[0].tolist() == [0.0625, 0.25, 9.0]
    i, j, c, rowptr, eoff = kb.graph_of(nbr, q, s)
    assert list(zip(i, j)) == [(0, 0), (0, 1), (0, 3), (1, 0), (1, 1), (1, 2)]
    assert rowptr.tolist() == [0, 3, 6] and eoff.tolist() == [0, 6] and c[:, 0].tolist() == [-3.0, -0.5, 0.25, 7.0, 9.5, 1.0]


@pytest.mark.parametrize("dim,fewer,more", [(1, 136, 113), (2, 126, 143), (3, 97, 180)])
def test_the_cap_case_cuts_rows_both_ways(dim, fewer, more):
    q, s, r = kb.cap_case(dim)
    inside = (kb.brute_force(q, s, 64, r)[0] > 0).sum(1)
    assert ((inside < 8).sum(), (inside > 8).sum()) == (fewer, more) and 16 <= inside.max() <= 18


def test_declarations_agree():
    from athena_amd import _capi

    header = open(os.path.join(ROOT, "include", "athena_mp.h")).read()
    fortran = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    for name, n_args in ENTRIES.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in athena_mp.h"
        assert len(m.group(1).split(",")) == n_args
        assert len(_capi._PROTOS[name]) == n_args
        m = re.search(r"function %s\(([^)]*)\)" % name, fortran)
        assert m and 'name="%s"' % name in fortran, f"{name} has no interface in athena_mp_c.f90"
        assert len(m.group(1).replace("&", "").split(",")) == n_args
