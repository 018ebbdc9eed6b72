"""CPU: the yardstick of the edge MLP's input and its reverse against itself (tests/edge_gather_reference.py).  A hand-written 3 x 4
handle pins the rules of the definition -- the block layout, copies that keep every bit, relative, pad columns, empty rows and
columns --, the reverse is the adjoint of the forward (exactly on small integers, to rounding in the float64 twin), and the inputs
of the GPU test are what that test needs.  Also: the C ABI, ctypes and Fortran declarations of the new entries agree."""
import os
import re

import numpy as np
import pytest

import edge_gather_reference as er
import knn_bipartite_reference as kb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"athena_mp_edge_gather_fwd": 10, "athena_mp_edge_gather_bwd": 10, "athena_mp_edge_gather_host": 10,
           "athena_mp_edge_gather_bwd_host": 10}
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)
words = lambda *w: np.array(w, np.uint32).view(np.float32)


def _small():
    """(A, i, j) of 3 queries x 4 sources: row 0 = sources (0, 2, 3), row 1 empty, row 2 = sources (0, 1); edge e is pair e"""
    i, j = np.array([0, 0, 0, 2, 2]), np.array([0, 2, 3, 0, 1])
    return er.arrays_of(i, j, 3, 4), i, j


def test_the_block_layout_and_the_pad_columns():
    A, i, j = _small()
    xs = np.arange(8, dtype=np.float32).reshape(4, 2) + 10        # source j holds 10 + 2 j, 11 + 2 j
    xq = np.arange(9, dtype=np.float32).reshape(3, 3) + 100
    coords = np.arange(5, dtype=np.float32).reshape(5, 1) + 1000
    h = np.full((5, 8), -7, np.float32)
    out = er.fwd(A, xs, xq, coords, 0, h)
    assert out is h
    for e in range(5):
        assert h[e].tolist() == xs[j[e]].tolist() + xq[i[e]].tolist() + coords[e].tolist() + [-7, -7], "(xs[j], xq[i], coords[e]), pad untouched"
    only = er.fwd(A, None, xq, None, 0, np.full((5, 3), -7, np.float32))
    assert np.array_equal(only, xq[i])
    only = er.fwd(A, None, None, coords, 0, np.full((5, 2), -7, np.float32))
    assert np.array_equal(only[:, 0], coords[:, 0]) and (only[:, 1] == -7).all()


def test_copies_keep_the_bits():
    A, i, j = _small()
    special = words(0x80000000, 0x7F800000, 0x7FC12345, 0x7F800001)            # -0, inf, a NaN with a payload, a signalling NaN
    xs = np.stack([special, special[::-1]], 1)                                  # [4, 2]
    xq = np.stack([special[:3], special[1:]], 1)                                # [3, 2]
    coords = np.resize(special, (5, 3)).astype(np.float32)
    assert np.array_equal(bits(coords).ravel()[:4], bits(special)), "numpy itself changed a word"
    h = er.fwd(A, xs, xq, coords, 0, np.zeros((5, 7), np.float32))
    assert np.array_equal(bits(h[:, :2]), bits(xs)[j]) and np.array_equal(bits(h[:, 2:4]), bits(xq)[i])
    assert np.array_equal(bits(h[:, 4:]), bits(coords))
    dh = np.resize(special, (5, 9)).astype(np.float32)
    assert np.array_equal(bits(er.bwd_coords(dh, 2, 2, 3)), bits(dh)[:, 4:7])


def test_relative_subtracts_the_query_from_the_first_block_only():
    A, i, j = _small()
    xs = np.array([[1, -0.0], [2, 5], [4, 0.0], [8, 1e-38]], np.float32)
    xq = np.array([[0.5, 0.0], [9, 9], [3, 1.5e-38]], np.float32)
    h = er.fwd(A, xs, xq, None, 1, np.full((5, 5), -7, np.float32))
    assert np.array_equal(bits(h[:, :2]), bits(xs[j] - xq[i])) and np.array_equal(bits(h[:, 2:4]), bits(xq[i])) and (h[:, 4] == -7).all()
    assert bits(h[0, 1]) == bits(np.float32(-0.0)), "-0 - +0 = -0"
    assert bits(h[1, 1]) == 0, "+0 - +0 = +0"
    tiny = h[2, 1]
    assert tiny != 0 and abs(tiny) < np.finfo(np.float32).tiny, "a subnormal difference is kept"
    inf = np.float32(np.inf)
    h = er.fwd(A, np.full((4, 1), inf, np.float32), np.full((3, 1), inf, np.float32), None, 1, np.zeros((5, 2), np.float32))
    assert np.isnan(h[:, 0]).all() and (h[:, 1] == inf).all(), "inf - inf is a NaN"
    with pytest.raises(AssertionError):
        er.fwd(A, xs, xq[:, :1], None, 1, np.zeros((5, 3), np.float32))


def test_empty_rows_and_columns_give_plus_zero_and_the_sums_are_sequential():
    i, j = np.array([0, 0, 0, 2, 2]), np.array([0, 2, 3, 0, 1])
    A = er.arrays_of(i, j, 3, 5)                                                # source 4 has no entry, query 1 none either
    dh = np.full((5, 4), -0.0, np.float32)
    dxs, dxq, dc = er.bwd(A, dh, (1, 1, 1), 0)
    assert dxs.shape == (5, 1) and dxq.shape == (3, 1) and dc.shape == (5, 1)
    assert not bits(dxs).any() and not bits(dxq).any(), "+0 + -0 = +0, and an empty row or column is +0"
    assert (bits(dc) == bits(np.float32(-0.0))).all(), "dcoords is a copy"
    # three terms whose sum depends on the order: row 0 takes edges 0, 1, 2 in that order
    big = np.float32(2.0 ** 24)
    dh = np.array([[big, 0], [1, 0], [1, 0], [0, 0], [0, 0]], np.float32)
    assert er.bwd_queries(A, dh, 0, 1, 0)[0, 0] == big, "(2^24 + 1) + 1 in fp32 stays 2^24"
    dh = np.array([[1, 0], [1, 0], [big, 0], [0, 0], [0, 0]], np.float32)
    assert er.bwd_queries(A, dh, 0, 1, 0)[0, 0] == big + 2
    # relative: per entry the second block is added, then the first subtracted; the other order of the two gives 2^24 here
    dh = np.array([[-1, big], [1, 1], [0, 0], [0, 0], [0, 0]], np.float32)
    assert er.bwd_queries(A, dh, 1, 1, 1)[0, 0] == big - 1, "((0 + 2^24) + 1) = 2^24, then (2^24 + 1) - 1 = 2^24 - 1"
    # column 0 holds queries 0 and 2 ascending: edges 0 and 3
    dh = np.zeros((5, 2), np.float32)
    dh[0, 0], dh[3, 0] = 5, 7
    assert er.bwd_sources(A, dh, 1)[:, 0].tolist() == [12, 0, 0, 0, 0]


def _knn_case(seed):
    """80 queries x 45 sources in three clouds, the middle one without sources (its rows are empty), k = 5: (A, E, rng)"""
    rng = np.random.default_rng(seed)
    qoff, soff = kb.offsets_of([40, 10, 30]), kb.offsets_of([25, 0, 20])
    q, s = rng.random((80, 3)).astype(np.float32), rng.random((45, 3)).astype(np.float32)
    nbr, _ = kb.brute_force(q, s, 5, None, qoff, soff)
    i, j, _, _, _ = kb.graph_of(nbr, q, s, qoff)
    return er.arrays_of(i, j, 80, 45), i.size, rng


@pytest.mark.parametrize("relative", [0, 1])
def test_the_reverse_is_the_adjoint_of_the_forward_exactly_on_small_integers(relative):
    """<dh, fwd(xs, xq, coords)> = <dxs, xs> + <dxq, xq> + <dcoords, coords>: integers in -3 .. 3, every sum far below 2^24"""
    A, E, rng = _knn_case(9201)
    Fs = Fq = 6
    draw = lambda *shape: rng.integers(-3, 4, shape).astype(np.float32)
    xs, xq, coords, dh = draw(45, Fs), draw(80, Fq), draw(E, 3), draw(E, 17)
    h = er.fwd(A, xs, xq, coords, relative, np.zeros((E, 17), np.float32))
    assert not h[:, 15:].any()
    dh_pad = dh.copy()
    dh_pad[:, 15:] = np.nan                                                     # never read
    dxs, dxq, dc = er.bwd(A, dh_pad, (Fs, Fq, 3), relative)
    f64 = lambda a: a.astype(np.float64)
    left = (f64(dh[:, :15]) * f64(h[:, :15])).sum()
    right = (f64(dxs) * f64(xs)).sum() + (f64(dxq) * f64(xq)).sum() + (f64(dc) * f64(coords)).sum()
    assert left == right and left != 0
    assert (np.diff(A["rowptr"]) == 0).any() and np.abs(dxs).max() > 3


@pytest.mark.parametrize("relative", [0, 1])
def test_the_twin_is_its_own_adjoint_on_normal_data(relative):
    """float64, standard normal: both sides agree to 1e-12 relative -- far above float64 rounding for rows of <= 150 terms, far
    below any indexing error"""
    A, E, rng = _knn_case(9202)
    Fs = Fq = 5
    xs, xq, coords, dh = (rng.standard_normal(s) for s in ((45, Fs), (80, Fq), (E, 2), (E, 12)))
    assert np.diff(A["t_rowptr"]).max() <= 150
    h = er.fwd64(A, xs, xq, coords, relative, E)
    dxs, dxq, dc = er.bwd64(A, dh, (Fs, Fq, 2), relative)
    assert h.dtype == dxs.dtype == np.float64
    left = (dh * h).sum()
    right = (dxs * xs).sum() + (dxq * xq).sum() + (dc * coords).sum()
    assert abs(left - right) <= 1e-12 * abs(left) and abs(left) > 1


def test_the_inputs_of_the_gpu_test_are_what_it_needs():
    """what tests/test_gpu_edge_gather.py asserts before it runs the device, shown here on the CPU for the same inputs"""
    import test_gpu_edge_gather as tg

    for name in tg.CASES:
        for widths in tg.WIDTHS:
            for padded in (0, 1):
                tg.inputs_are_what_the_test_needs(name, widths, padded)


def test_declarations_agree():
    from athena_amd import _capi

    header = open(os.path.join(ROOT, "include", "athena_mp.h")).read()
    fortran = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    build = open(os.path.join(ROOT, "athena_amd", "csrc", "build.sh")).read()
    assert " edge_gather.hip " in build
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
