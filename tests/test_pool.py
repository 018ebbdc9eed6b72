"""CPU: the yardstick of max pooling against itself (tests/pool_reference.py).  Hand-made rows pin the rules of the definition on
values -- ties, signed zeros, NaNs, empty rows --, the reverse steps send every dy to the one entry arg names, the float64 twin's
reverse steps agree with central differences of its own forward on inputs without ties, and the tie-heavy features of the GPU test
are as tie-heavy as that test needs.  Also: the C ABI, ctypes and Fortran declarations of the new entries agree."""
import functools
import os
import re

import numpy as np

import knn_bipartite_reference as kb
import pool_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"athena_mp_pool_max_fwd": 5, "athena_mp_pool_max_edges_fwd": 5, "athena_mp_pool_max_bwd_x": 5,
           "athena_mp_pool_max_bwd_edges": 5, "athena_mp_pool_max_host": 6, "athena_mp_pool_max_bwd_host": 6}
NAN, INF = np.float32(np.nan), np.float32(np.inf)
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)


def _rows(*rows):
    """one feature column; row r holds the given values, entry k reading source k of a source set as wide as the longest row: (A, x)"""
    width = max(len(r) for r in rows)
    i = np.concatenate([np.full(len(r), n, np.int64) for n, r in enumerate(rows)])
    j = np.concatenate([np.arange(len(r), dtype=np.int64) for r in rows])
    A = pr.arrays_of(i, j, len(rows), width)
    h = np.concatenate([np.asarray(r, np.float32) for r in rows])[:, None]
    return A, h


def _one_row(values):
    """(y, arg) of a single row through the edge form (entry k = edge k = column k), as scalars"""
    A, h = _rows(values)
    y, arg = pr.edges_fwd(A, h)
    return y[0, 0], int(arg[0, 0])


def test_a_tie_goes_to_the_first_entry():
    assert _one_row([1, 3, 3, 2, 3]) == (3, 1)
    assert _one_row([5, 5]) == (5, 0)
    assert _one_row([-2, -7]) == (-2, 0), "the first entry replaces 'none yet' even when it is negative"


def test_of_two_zeros_the_first_stays():
    y, arg = _one_row([-1, 0.0, -0.0])
    assert bits(y) == bits(np.float32(0.0)) and arg == 1
    y, arg = _one_row([-1, -0.0, 0.0])
    assert bits(y) == bits(np.float32(-0.0)) and arg == 1
    y, arg = _one_row([-0.0])
    assert bits(y) == bits(np.float32(-0.0)) and arg == 0, "a row of one -0 gives -0, not the +0 of an empty row"


def test_a_nan_beats_infinity_and_the_first_nan_stays():
    y, arg = _one_row([INF, NAN, 7])
    assert np.isnan(y) and arg == 1
    y, arg = _one_row([NAN, INF])
    assert np.isnan(y) and arg == 0
    first, second = np.array([0x7FC00001, 0x7FC00002], np.int32).view(np.float32)
    y, arg = _one_row([1, first, second, INF])
    assert bits(y) == bits(first) and arg == 1, "the first NaN's own bits come back"
    y, arg = _one_row([-INF, -INF])
    assert y == -INF and arg == 0


def test_an_empty_row_gives_plus_zero_and_minus_one():
    A, h = _rows([4, 9], [], [2])
    y, arg = pr.edges_fwd(A, h)
    assert y[:, 0].tolist() == [9, 0, 2] and arg[:, 0].tolist() == [1, -1, 0] and bits(y[1, 0]) == 0
    yx, argx = pr.fwd(A, np.array([[4], [9]], np.float32))
    assert yx[:, 0].tolist() == [9, 0, 4] and argx[:, 0].tolist() == [1, -1, 0]
    none = pr.arrays_of(np.zeros(0, np.int64), np.zeros(0, np.int64), 2, 3)
    y, arg = pr.fwd(none, np.ones((3, 2), np.float32))
    assert not bits(y).any() and (arg == -1).all() and y.shape == (2, 2)


def test_the_vertex_and_the_edge_form_agree_on_gathered_values():
    q, s, A, x, _ = _small()
    y, arg = pr.fwd(A, x)
    e_of = np.empty(A["col"].size, np.int64)
    e_of[A["eid"]] = np.arange(A["col"].size)
    y2, arg2 = pr.edges_fwd(A, x[A["col"][e_of]])
    assert np.array_equal(y, y2) and np.array_equal(arg, arg2)


# ---- the reverse steps -----------------------------------------------------------------------------------------------------------
def test_bwd_x_of_a_tie_sends_all_of_dy_to_the_first_and_an_unchosen_column_gets_plus_zero():
    # two rows over three sources: row 0 ties sources 0 and 2, row 1 takes source 0; source 1 is never chosen
    A = pr.arrays_of(np.array([0, 0, 0, 1, 1]), np.array([0, 1, 2, 0, 1]), 2, 3)
    x = np.array([[4], [1], [4]], np.float32)
    y, arg = pr.fwd(A, x)
    assert arg[:, 0].tolist() == [0, 0]
    dy = np.array([[0.25], [-3]], np.float32)
    dx = pr.bwd_x(A, arg, dy)
    assert dx[:, 0].tolist() == [-2.75, 0, 0] and not bits(dx[1:]).any()
    dh = pr.bwd_edges(A, arg, dy, 5)
    assert dh[:, 0].tolist() == [0.25, 0, 0, -3, 0] and not bits(dh[[1, 2, 4]]).any()
    minus = pr.bwd_x(A, arg, np.array([[-0.0], [-0.0]], np.float32))
    assert not bits(minus).any(), "+0 + -0 = +0: the sum starts at +0"


@functools.lru_cache(None)
def _small():
    """12 queries x 9 sources, k = 4, F = 5, as tests/test_interp.py; float64 features without ties"""
    rng = np.random.default_rng(9101)
    q, s = rng.random((12, 3)).astype(np.float32), rng.random((9, 3)).astype(np.float32)
    nbr, _ = kb.brute_force(q, s, 4)
    i, j, _, _, _ = kb.graph_of(nbr, q, s)
    return q, s, pr.arrays_of(i, j, 12, 9), rng.standard_normal((9, 5)), rng.standard_normal((12, 5))


def test_what_comes_back_is_what_went_in_on_a_knn_graph():
    """the sum of dx over j equals the sum of dy over the non-empty rows (float64, to rounding), and dh has exactly one non-zero per
    (i, f) of a non-empty row when dy has no zeros; three clouds, the middle one without sources"""
    rng = np.random.default_rng(9102)
    qoff, soff = kb.offsets_of([40, 10, 30]), kb.offsets_of([25, 0, 20])
    q, s = rng.random((80, 3)).astype(np.float32), rng.random((45, 3)).astype(np.float32)
    nbr, _ = kb.brute_force(q, s, 5, None, qoff, soff)
    i, j, _, rowptr, _ = kb.graph_of(nbr, q, s, qoff)
    A = pr.arrays_of(i, j, 80, 45)
    filled = np.diff(rowptr) > 0
    assert filled.sum() == 70
    x = rng.integers(-2, 3, (45, 6)).astype(np.float64)              # ties everywhere
    dy = rng.standard_normal((80, 6))
    assert (dy != 0).all()
    y, arg = pr.fwd(A, x)
    assert (arg[~filled] == -1).all() and (arg[filled] >= 0).all()
    dx = pr.bwd_x(A, arg, dy)
    total = dy[filled].sum(axis=0)
    assert np.abs(dx.sum(axis=0) - total).max() <= 80 * 2.0 ** -52 * np.abs(dy).sum(axis=0).max()
    dh = pr.bwd_edges(A, arg, dy, i.size)
    per_row = np.zeros((80, 6), np.int64)
    np.add.at(per_row, i, dh != 0)
    assert (per_row[filled] == 1).all() and (per_row[~filled] == 0).all()
    assert np.array_equal(dh[dh != 0], dy[i][dh != 0])


def test_the_twin_agrees_with_central_differences():
    _, _, A, x, dy = _small()
    E = A["col"].size
    rng = np.random.default_rng(9103)
    h = rng.standard_normal((E, 5))
    step = 1e-6
    for values, source, forward, n in ((x, A["col"], pr.fwd, 9), (h, A["eid"], pr.edges_fwd, E)):
        y, arg = forward(A, values)
        assert not pr.attained_more_than_once(A, values, source, y).any()
        srt = np.sort(np.stack([values[source[A["rowptr"][r]:A["rowptr"][r + 1]]] for r in range(12)]), axis=1)
        assert (srt[:, -1] - srt[:, -2]).min() > 1e3 * step, "the two largest of a row must lie further apart than the step"
        grad = pr.bwd_x(A, arg, dy) if forward is pr.fwd else pr.bwd_edges(A, arg, dy, E)
        loss = lambda v: float((dy * forward(A, v)[0]).sum())
        num = np.zeros_like(grad)
        for a in range(n):
            for f in range(5):
                up, dn = values.copy(), values.copy()
                up[a, f] += step
                dn[a, f] -= step
                num[a, f] = (loss(up) - loss(dn)) / (2 * step)
        assert np.abs(grad).max() > 0 and (grad == 0).any()
        assert np.abs(grad - num).max() <= 1e-6 * np.abs(num).max()


def test_the_tie_heavy_features_decide_most_rows_by_the_tie_rule():
    """what tests/test_gpu_pool.py asserts before it runs the device, shown here on the CPU for the same inputs"""
    import test_gpu_pool as tg

    for name in tg.CASES:
        for F in tg.ALL_F:
            for kind in tg.KINDS:
                tg.inputs_are_what_the_test_needs(name, F, kind)


def test_declarations_agree():
    from athena_amd import _capi

    header = open(os.path.join(ROOT, "include", "athena_mp.h")).read()
    fortran = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    build = open(os.path.join(ROOT, "athena_amd", "csrc", "build.sh")).read()
    assert " pool.hip " in build
    assert list(ENTRIES.values()) == [5, 5, 5, 5, 6, 6]
    for name, n_args in ENTRIES.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in athena_mp.h"
        assert len(m.group(1).split(",")) == n_args
        assert name in _capi._PROTOS and len(_capi._PROTOS[name]) == n_args, f"{name} has no ctypes prototype"
        m = re.search(r"function %s\(([^)]*)\)" % name, fortran)
        assert m and 'name="%s"' % name in fortran, f"{name} has no interface in athena_mp_c.f90"
        assert len(m.group(1).replace("&", "").split(",")) == n_args
