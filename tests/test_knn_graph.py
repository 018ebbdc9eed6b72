"""CPU: the yardstick of the k-nearest-neighbour builder against itself (tests/knn_reference.py).  The large form (float64 k-d
tree candidates, fp32 keys) and a Python transcription of knn_graph.hip's grid search -- the file header's stop rule and margin in
float32 -- are pinned to the brute-force transcription of the definition on every shape class the GPU tests use, at n <= 1500;
among them points on cell boundaries and coordinates around 1e6 with spacing 1, where the margin is what keeps the search right.
Also: the C ABI, ctypes and Fortran declarations of the new entries agree."""
import functools
import os
import re

import numpy as np
import pytest

import knn_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"athena_mp_knn_pairs_batched": 14, "athena_mp_knn_pairs": 11, "athena_mp_knn_graph_batched_host": 17, "athena_mp_knn_stats": 1}
CASES = kr.shape_cases()


@functools.lru_cache(None)
def _brute(c):
    name, p, off, k, r = CASES[c]
    return kr.brute_force_neighbours(p, off, k, r)


@pytest.mark.parametrize("c", range(len(CASES)), ids=[c[0] for c in CASES])
def test_large_form_equals_brute_force(c):
    name, p, off, k, r = CASES[c]
    assert p.shape[0] <= 1500
    want = _brute(c)
    assert np.array_equal(kr.large_form_neighbours(p, off, k, r), want)
    for mode in (0, 1):
        a, b = kr.graph_of(want, p, off, mode), kr.graph_of(kr.large_form_neighbours(p, off, k, r), p, off, mode)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("c", range(len(CASES)), ids=[c[0] for c in CASES])
def test_grid_search_with_the_stop_rule_equals_brute_force(c):
    name, p, off, k, r = CASES[c]
    got, stats = kr.grid_search_neighbours(p, off, k, r)
    print(f"{name}: {stats[1] / max(stats[0], 1):.1f} candidates and {stats[2] / max(stats[0], 1):.1f} cells per query, largest shell {stats[3]}")
    assert np.array_equal(got, _brute(c))
    if name == "two clusters":
        assert stats[3] > 1                                  # the smaller cluster crossed the gap
    if name.startswith("uniform"):
        assert stats[1] < p.shape[0] ** 2 / 2                # pruned, even at 600 points


def test_the_margin_is_exercised():
    """on the boundary cases a point's computed cell differs from the cell of its exact coordinate for some points -- the case the
    margin of the stop rule exists for -- and 1e6 + lattice has cells whose width is a few float32 spacings"""
    p = kr.on_cell_boundaries(2)
    lo, inv_w, nc, _ = kr.make_knn_grid(p)
    q32 = ((p - lo) * inv_w).astype(np.float64)
    exact = (p.astype(np.float64) - lo.astype(np.float64)) * inv_w.astype(np.float64)
    assert np.any(np.floor(q32) != np.floor(exact)) or np.any(q32 == np.floor(q32))
    far = kr.lattice(12, 12) + np.float32(1e6)
    assert np.all(1.0 / kr.make_knn_grid(far)[1] < 64 * np.spacing(np.float32(1e6)))


def test_graph_of_union_and_mutual():
    p = kr.lattice(5)                                         # 0 1 2 3 4 on a line, k = 1: ties go to the smaller index
    nbr = kr.brute_force_neighbours(p, [0, 5], 1)
    assert nbr.reshape(-1).tolist() == [2, 1, 2, 3, 4]
    i, j, c, eoff = kr.graph_of(nbr, p, [0, 5], 0)
    assert list(zip(i, j)) == [(0, 1), (1, 2), (2, 3), (3, 4)] and eoff.tolist() == [0, 4] and np.all(c == -1)
    i, j, _, _ = kr.graph_of(nbr, p, [0, 5], 1)
    assert list(zip(i, j)) == [(0, 1)]


def test_the_cap_case_cuts_rows_both_ways():
    """3 000 uniform points, k = 8, a radius for mean degree about 6: at least a tenth of the rows are cut by k, at least a tenth
    by the radius (the GPU test uses this seed)"""
    p, off, k, r = kr.cap_case()
    degree = (kr.large_form_neighbours(p, off, 64, r) > 0).sum(1)          # candidates inside the cap (none has 64)
    assert degree.max() < 64
    by_k, by_r = (degree > k).mean(), (degree < k).mean()
    print(f"mean degree inside the cap {degree.mean():.2f}; rows cut by k: {by_k:.3f}, rows cut by the radius: {by_r:.3f}")
    assert by_k >= 0.1 and by_r >= 0.1


def test_declarations_agree():
    from athena_amd import _capi

    header = open(os.path.join(ROOT, "include", "athena_mp.h")).read()
    fortran = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    for name, n_args in ENTRIES.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in athena_mp.h"
        assert len(m.group(1).split(",")) == n_args
        assert len(_capi._PROTOS[name]) == n_args
        assert 'name="%s"' % name in fortran
