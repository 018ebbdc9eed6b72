"""CPU: the yardstick of attention pooling against itself (tests/attention_reference.py).  A hand-written 3 x 4 handle pins the rules
of the definition -- the head of a column, -inf -> +0, NaN and +inf, the all -inf row, the single entry's 1, empty rows and
columns, the order of the sums --, the reverse steps are the adjoint of the forward in the float64 twin, softmax_bwd is the adjoint
of alpha's Jacobian by central differences in float64, every order of bwd_alpha's sum is exact on small integers, both fp32 orders
stay far inside the bound the GPU test holds the device to, and the inputs of the GPU test are what that test needs.  Also: the C
ABI, ctypes and Fortran declarations of the new entries agree."""
import os
import re

import numpy as np
import pytest

import attention_reference as ar
import knn_bipartite_reference as kb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"athena_mp_attn_softmax_fwd": 4, "athena_mp_attn_gather_fwd": 6, "athena_mp_attn_gather_edges_fwd": 6,
           "athena_mp_attn_gather_bwd_x": 6, "athena_mp_attn_gather_bwd_edges": 6, "athena_mp_attn_gather_bwd_alpha": 7,
           "athena_mp_attn_softmax_bwd": 5, "athena_mp_attention_host": 8, "athena_mp_attention_bwd_host": 10}
NAN, INF = np.float32(np.nan), np.float32(np.inf)
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)


def _small(ns=4):
    """(A, i, j) of 3 queries x 4 sources: row 0 = sources (0, 2, 3), row 1 empty, row 2 = sources (0, 1); edge e is pair e"""
    i, j = np.array([0, 0, 0, 2, 2]), np.array([0, 2, 3, 0, 1])
    return ar.arrays_of(i, j, 3, ns), i, j


def test_the_head_of_a_column():
    assert ar.head_of(6, 2).tolist() == [0, 0, 0, 1, 1, 1] and ar.head_of(3, 3).tolist() == [0, 1, 2] and ar.head_of(4, 1).tolist() == [0] * 4
    with pytest.raises(AssertionError):
        ar.head_of(6, 4)
    A, i, j = _small()
    alpha = np.array([[1, 10], [2, 20], [3, 30], [4, 40], [5, 50]], np.float32)
    x = np.arange(16, dtype=np.float32).reshape(4, 4) + 1                  # columns 0, 1 take head 0; 2, 3 head 1
    y = ar.fwd(A, alpha, x, 2)
    want0 = alpha[0][[0, 0, 1, 1]] * x[0] + alpha[1][[0, 0, 1, 1]] * x[2] + alpha[2][[0, 0, 1, 1]] * x[3]
    assert np.array_equal(y[0], want0) and not bits(y[1]).any()
    assert np.array_equal(y[2], alpha[3][[0, 0, 1, 1]] * x[0] + alpha[4][[0, 0, 1, 1]] * x[1])
    h = np.arange(20, dtype=np.float32).reshape(5, 4)
    assert np.array_equal(ar.edges_fwd(A, alpha, h, 2)[2], alpha[3][[0, 0, 1, 1]] * h[3] + alpha[4][[0, 0, 1, 1]] * h[4])
    assert np.array_equal(ar.bwd_edges(A, alpha, x[:3], 2)[4], alpha[4][[0, 0, 1, 1]] * x[2])     # dy of row 2


def test_the_softmax_rules():
    A, i, j = _small()
    s = np.array([[0, 1], [1, -INF], [2, 1], [5, 7], [5, 7]], np.float32)
    a = ar.softmax(A, s)
    assert a.dtype == np.float32
    assert bits(a[1, 1]) == 0, "-inf beside a finite maximum gives +0"
    assert np.array_equal(a[0, 1], np.float32(0.5)) and np.array_equal(a[2, 1], np.float32(0.5))
    assert np.array_equal(a[3], [0.5, 0.5]) and np.array_equal(a[4], [0.5, 0.5])
    e = np.exp(np.array([-2, -1, 0], np.float32))
    S = (e[0] + e[1]) + e[2]
    assert np.array_equal(a[:3, 0], e / S), "p / S with S added in row order"
    for bad in (NAN, INF):
        t = s.copy()
        t[1, 0] = bad
        a = ar.softmax(A, t)
        assert np.isnan(a[:3, 0]).all() and not np.isnan(a[:3, 1]).any() and not np.isnan(a[3:]).any(), "its own (row, head) only"
        f64, scale, arg = ar.softmax64(A, t)
        assert np.array_equal(np.isnan(f64), np.isnan(a)) and scale is f64
    t = s.copy()
    t[:3, 1] = -INF
    a = ar.softmax(A, t)
    assert np.isnan(a[:3, 1]).all() and not np.isnan(a[:3, 0]).any()
    one = ar.arrays_of(np.array([1]), np.array([2]), 3, 4)
    for v in (0.0, -3e38, 88.0):
        assert bits(ar.softmax(one, np.array([[v]], np.float32)))[0, 0] == 0x3F800000, "a row of one finite entry gives exactly 1"
    f64, scale, arg = ar.softmax64(A, s)
    assert f64.dtype == np.float64 and np.array_equal(arg[:3, 0], [-2, -1, 0]) and arg[1, 1] == -np.inf
    assert np.abs(f64 - ar.softmax(A, s)).max() < 1e-7


def test_empty_rows_and_columns_give_plus_zero_and_the_sums_are_sequential():
    i, j = np.array([0, 0, 0, 2, 2]), np.array([0, 2, 3, 0, 1])
    A = ar.arrays_of(i, j, 3, 5)                                           # source 4 has no entry, query 1 none either
    alpha = np.ones((5, 1), np.float32)
    minus = np.full((5, 2), -0.0, np.float32)
    assert not bits(ar.fwd(A, alpha, minus, 1)).any(), "+0 + 1 * -0 = +0, and an empty row is +0"
    dx = ar.bwd_x(A, alpha, np.full((3, 2), -0.0, np.float32), 1)
    assert dx.shape == (5, 2) and not bits(dx).any()
    big = np.float32(2.0 ** 24)
    h = np.array([[big], [1], [1], [0], [0]], np.float32)
    assert ar.edges_fwd(A, alpha, h, 1)[0, 0] == big, "(2^24 + 1) + 1 in fp32 stays 2^24"
    h = np.array([[1], [1], [big], [0], [0]], np.float32)
    assert ar.edges_fwd(A, alpha, h, 1)[0, 0] == big + 2
    dy = np.array([[5], [9], [7]], np.float32)                             # column 0 holds queries 0 and 2 ascending: edges 0 and 3
    w = np.array([[2], [0], [0], [3], [0]], np.float32)
    assert ar.bwd_x(A, w, dy, 1)[:, 0].tolist() == [31, 0, 0, 0, 0]
    d = np.array([[big], [1], [1], [7], [7]], np.float32)                  # softmax_bwd: dot in row order
    ds = ar.softmax_bwd(A, alpha, d)
    assert ds[0, 0] == 0 and ds[1, 0] == 1 - big and ds[3, 0] == -7
    assert bits(ar.bwd_alpha(A, 5, None, np.full((5, 1), -0.0, np.float32), np.ones((3, 1), np.float32), 1))[0, 0] == bits(np.float32(-0.0)), \
        "at C = 1 dalpha is the product itself, not a sum from +0"


def _knn_case(seed):
    """80 queries x 45 sources in three clouds, the middle one without sources (its rows are empty), k = 5: (A, E, rng)"""
    rng = np.random.default_rng(seed)
    qoff, soff = kb.offsets_of([40, 10, 30]), kb.offsets_of([25, 0, 20])
    q, s = rng.random((80, 3)).astype(np.float32), rng.random((45, 3)).astype(np.float32)
    nbr, _ = kb.brute_force(q, s, 5, None, qoff, soff)
    i, j, _, _, _ = kb.graph_of(nbr, q, s, qoff)
    return ar.arrays_of(i, j, 80, 45), i.size, rng


@pytest.mark.parametrize("F,H", [(6, 1), (6, 2), (6, 6), (8, 2)])
def test_the_reverse_is_the_adjoint_of_the_forward_in_the_twin(F, H):
    """<dy, y(alpha, v)> is bilinear: = <dv, v> = <dalpha, alpha>, float64, to 1e-12 relative"""
    A, E, rng = _knn_case(9301)
    f8 = np.float64
    alpha, x, h, dy = rng.standard_normal((E, H)), rng.standard_normal((45, F)), rng.standard_normal((E, F)), rng.standard_normal((80, F))
    assert (np.diff(A["rowptr"]) == 0).any()
    for left, dv, v, da in (((dy * ar.fwd(A, alpha, x, H, f8)).sum(), ar.bwd_x(A, alpha, dy, H, f8), x, ar.bwd_alpha(A, E, x, None, dy, H, f8)),
                            ((dy * ar.edges_fwd(A, alpha, h, H, f8)).sum(), ar.bwd_edges(A, alpha, dy, H, f8), h,
                             ar.bwd_alpha(A, E, None, h, dy, H, f8))):
        assert dv.dtype == da.dtype == np.float64 and abs(left) > 1
        assert abs(left - (dv * v).sum()) <= 1e-12 * abs(left) and abs(left - (da * alpha).sum()) <= 1e-12 * abs(left)


def test_softmax_bwd_is_the_adjoint_of_the_jacobian_by_central_differences():
    A, E, rng = _knn_case(9302)
    H = 3
    s, dalpha = rng.standard_normal((E, H)), rng.standard_normal((E, H))
    alpha = ar.softmax(A, s, np.float64)
    grad = ar.softmax_bwd(A, alpha, dalpha, np.float64)
    loss = lambda t: float((dalpha * ar.softmax(A, t, np.float64)).sum())
    step, num = 1e-6, np.zeros_like(grad)
    for e in range(E):
        for k in range(H):
            up, dn = s.copy(), s.copy()
            up[e, k] += step
            dn[e, k] -= step
            num[e, k] = (loss(up) - loss(dn)) / (2 * step)
    assert np.abs(num).max() > 0.1 and np.abs(grad - num).max() <= 1e-8 * max(1.0, np.abs(num).max())
    ei, _ = ar.edge_ends(A, E)
    sums = np.zeros((80, H))
    np.add.at(sums, ei, alpha)
    assert np.abs(sums[np.diff(A["rowptr"]) > 0] - 1).max() < 1e-14 and np.abs(np.bincount(ei, grad[:, 0], 80)).max() < 1e-14


@pytest.mark.parametrize("F,H", [(8, 8), (8, 2), (64, 4), (64, 1), (6, 2), (96, 4)])
def test_on_small_integers_every_order_of_bwd_alphas_sum_is_exact(F, H):
    A, E, rng = _knn_case(9303)
    draw = lambda *shape: rng.integers(-2, 3, shape).astype(np.float32)
    x, h, dy = draw(45, F), draw(E, F), draw(80, F)
    C = F // H
    for vx, vh in ((x, None), (None, h)):
        seq = ar.bwd_alpha(A, E, vx, vh, dy, H)
        assert seq.dtype == np.float32 and seq.shape == (E, H) and np.abs(seq).max() > 2
        assert np.array_equal(seq, ar.bwd_alpha(A, E, vx, vh, dy, H, np.float64))
        if C % 4 == 0 and (C // 4) & (C // 4 - 1) == 0:
            assert np.array_equal(bits(seq), bits(ar.bwd_alpha(A, E, vx, vh, dy, H, order="tree")))
        if vh is not None:                                                 # the columns walked backwards: another order, the heads reversed
            assert np.array_equal(ar.bwd_alpha(A, E, None, vh[:, ::-1], dy[:, ::-1], H)[:, ::-1], seq)


@pytest.mark.parametrize("C", [4, 16, 64, 256, 1024])
def test_both_fp32_orders_stay_far_inside_the_bound(C):
    """the bound of the GPU test, |dev - f64| <= |seq32 - f64| + 1e-5 sum_c |dy v|, excludes no legitimate order: on standard normals
    the sequential and the four-then-tree fp32 sums both stay below 0.03 of its second term"""
    A, E, rng = _knn_case(9304 + C)
    h, dy = rng.standard_normal((E, C)).astype(np.float32), rng.standard_normal((80, C)).astype(np.float32)
    f64 = ar.bwd_alpha(A, E, None, h, dy, 1, np.float64)
    mag = np.abs(ar.alpha_terms(A, E, None, h, dy, 1, np.float64)).sum(axis=2)
    for order in ("sequential", "tree"):
        got = ar.bwd_alpha(A, E, None, h, dy, 1, order=order).astype(np.float64)
        assert (np.abs(got - f64) / (1e-5 * mag)).max() < 0.03
    ref, bnd = ar.alpha_bound(A, E, None, h, dy, 1)
    assert np.array_equal(ref, f64) and (bnd >= 1e-5 * mag * (1 - 1e-12)).all()


def test_the_inputs_of_the_gpu_test_are_what_it_needs():
    """what tests/test_gpu_attention.py asserts before it runs the device, shown here on the CPU for the same inputs"""
    import test_gpu_attention as tg

    assert sorted(tg.SHAPES) == sorted(set(tg.SHAPES)) and len(tg.SHAPES) == 17
    for name in tg.CASES:
        for H in tg.HEADS:
            tg.inputs_are_what_the_test_needs(name, H)


def test_declarations_agree():
    from athena_amd import _capi

    header = open(os.path.join(ROOT, "include", "athena_mp.h")).read()
    fortran = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    build = open(os.path.join(ROOT, "athena_amd", "csrc", "build.sh")).read()
    assert " attention.hip " in build
    declared = _capi.declared_symbols()
    for name, n_args in ENTRIES.items():
        assert name in declared, f"{name} is not among the header's symbols"
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in athena_mp.h"
        assert len(m.group(1).split(",")) == n_args
        assert name in _capi._PROTOS and len(_capi._PROTOS[name]) == n_args, f"{name} has no ctypes prototype"
        m = re.search(r"function %s\(([^)]*)\)" % name, fortran)
        assert m and 'name="%s"' % name in fortran, f"{name} has no interface in athena_mp_c.f90"
        assert len(m.group(1).replace("&", "").split(",")) == n_args
