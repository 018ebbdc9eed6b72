"""CPU: the yardstick of inverse-distance interpolation against itself (tests/interp_reference.py).  The float64 twin's gradients
agree with central differences of its own forward, so the formulas of include/athena_mp.h are the derivative they claim to be; the
float32 yardstick keeps the properties the definition promises (rows of weights add up to 1, none above 1, a constant comes back,
s is the builder's sqdist bit for bit) and its dcoords stays inside the bound the GPU test holds the device to.  Also: the C ABI,
ctypes and Fortran declarations of the new entries agree."""
import functools
import os
import re

import numpy as np

import interp_reference as ir
import knn_bipartite_reference as kb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"athena_mp_interp_weights": 6, "athena_mp_interp_fwd": 5, "athena_mp_interp_bwd_x": 5, "athena_mp_interp_bwd_coords": 10,
           "athena_mp_interp_host": 8, "athena_mp_interp_bwd_host": 9}
EPS = 1e-16


@functools.lru_cache(None)
def _small():
    """12 queries x 9 sources, k = 4, F = 5"""
    rng = np.random.default_rng(9001)
    q, s = rng.random((12, 3)).astype(np.float32), rng.random((9, 3)).astype(np.float32)
    nbr, sqd = kb.brute_force(q, s, 4)
    i, j, coords, rowptr, _ = kb.graph_of(nbr, q, s)
    A = ir.arrays_of(i, j, 12, 9)
    x, dy = rng.standard_normal((9, 5)), rng.standard_normal((12, 5))
    return q, s, nbr, sqd, i, j, coords, A, x, dy


@functools.lru_cache(None)
def _wide():
    """300 queries x 200 sources in [2^-10, 2^10], k = 8, F = 64: the shapes of the GPU test's bound"""
    rng = np.random.default_rng(9002)
    draw = lambda *shape: (2.0 ** rng.uniform(-10, 10, shape)).astype(np.float32)
    q, s = draw(300, 3), draw(200, 3)
    nbr, _ = kb.brute_force(q, s, 8)
    i, j, coords, _, _ = kb.graph_of(nbr, q, s)
    A = ir.arrays_of(i, j, 300, 200)
    sign = lambda a: a * rng.choice([-1, 1], a.shape).astype(np.float32)
    return coords, A, sign(draw(200, 64)), sign(draw(300, 64))


def test_the_twin_agrees_with_central_differences():
    _, _, _, _, _, _, coords, A, x, dy = _small()
    c64 = coords.astype(np.float64)
    loss = lambda c, xx: float((dy * ir.forward64(A, c, EPS, xx)[2]).sum())
    dx, dc = ir.grad64(A, c64, EPS, x, dy)
    h = 1e-6
    num_c, num_x = np.zeros_like(dc), np.zeros_like(dx)
    for e in range(c64.shape[0]):
        for a in range(3):
            up, dn = c64.copy(), c64.copy()
            up[e, a] += h
            dn[e, a] -= h
            num_c[e, a] = (loss(up, x) - loss(dn, x)) / (2 * h)
    for jj in range(x.shape[0]):
        for f in range(x.shape[1]):
            up, dn = x.copy(), x.copy()
            up[jj, f] += h
            dn[jj, f] -= h
            num_x[jj, f] = (loss(c64, up) - loss(c64, dn)) / (2 * h)
    assert np.abs(dc).max() > 0 and np.abs(dx).max() > 0
    assert np.abs(dc - num_c).max() <= 1e-6 * np.abs(num_c).max()
    assert np.abs(dx - num_x).max() <= 1e-6 * np.abs(num_x).max()


def test_the_clamp_has_no_gradient_and_overflow_no_weight():
    coords = np.array([[0, 0, 0], [1e-9, 0, 0], [3e19, 3e19, 0], [1, 2, 2]], np.float32)
    A = ir.arrays_of(np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1]), 2, 2)
    w, s = ir.raw_weight(coords, EPS)
    assert s[0] == 0 and w[0] == w[1] == np.float32(1) / np.float32(EPS) and np.isinf(s[2]) and w[2] == 0 and w[3] == np.float32(1) / 9
    wts, W = ir.weights(A, coords, EPS)
    assert wts.tolist() == [0.5, 0.5, 0.0, 1.0]
    x, dy = np.ones((2, 3), np.float32), np.ones((2, 3), np.float32)
    x[1] = 2
    dc = ir.bwd_coords(A, coords, EPS, wts, x, ir.fwd(A, wts, x), dy)
    assert ir.zero_by_definition(coords, EPS).tolist() == [True, True, True, False]
    assert not dc[:3].any() and not np.signbit(dc[:3]).any() and not np.isnan(dc).any()
    only_overflow = ir.weights(ir.arrays_of(np.array([0]), np.array([0]), 1, 1), coords[2:3], EPS)
    assert only_overflow[0].tolist() == [0.0] and only_overflow[1].tolist() == [0.0], "a row whose W is 0 has weights +0, not NaN"


def test_rows_of_weights_add_up_to_one_and_a_constant_comes_back():
    for coords, A in ((_small()[6], _small()[7]), (_wide()[0], _wide()[1])):
        wts, W = ir.weights(A, coords, EPS)
        lens = np.diff(A["rowptr"])
        assert (wts <= 1).all() and (wts >= 0).all() and (W > 0).all()
        total = np.zeros(lens.size)
        np.add.at(total, ir.edge_ends(A, wts.size)[0], wts.astype(np.float64))
        assert (np.abs(total - 1) <= lens * 2.0 ** -24).all()
        const = np.full((int(A["col"].max()) + 1, 2), 3.25, np.float32)
        y = ir.fwd(A, wts, const)
        assert (np.abs(y.astype(np.float64) - 3.25) <= 3.25 * (lens + 1)[:, None] * 2.0 ** -24).all()


def test_s_is_the_builders_sqdist_bit_for_bit():
    q, s, nbr, sqd, i, j, coords, A, _, _ = _small()
    mine = ir.sqdist(coords)
    of_pair = {(a, b - 1): v for a in range(nbr.shape[0]) for b, v in zip(nbr[a], sqd[a]) if b > 0}
    want = np.array([of_pair[(a, b)] for a, b in zip(i.tolist(), j.tolist())], np.float32)
    assert np.array_equal(mine.view(np.int32), want.view(np.int32))


def test_the_fp32_yardstick_stays_inside_the_stated_bound():
    coords, A, x, dy = _wide()
    wts, _ = ir.weights(A, coords, EPS)
    y = ir.fwd(A, wts, x)
    got = ir.bwd_coords(A, coords, EPS, wts, x, y, dy)
    twin = ir.bwd_coords(A, coords, EPS, wts, x, y, dy, np.float64)
    bound = ir.dcoords_bound(coords, EPS, wts, x, y, dy, A)
    ratio = np.abs(got.astype(np.float64) - twin) / np.maximum(bound, 1e-300)
    print(f"worst |fp32 - f64| / bound = {ratio.max():.3f}")
    assert np.isfinite(got).all() and np.abs(got).max() > 0 and (np.abs(got.astype(np.float64) - twin) <= bound).all()


def test_declarations_agree():
    from athena_amd import _capi

    header = open(os.path.join(ROOT, "include", "athena_mp.h")).read()
    fortran = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    build = open(os.path.join(ROOT, "athena_amd", "csrc", "build.sh")).read()
    assert " interp.hip " in build
    for name, n_args in ENTRIES.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in athena_mp.h"
        assert len(m.group(1).split(",")) == n_args
        assert name in _capi._PROTOS and len(_capi._PROTOS[name]) == n_args, f"{name} has no ctypes prototype"
        m = re.search(r"function %s\(([^)]*)\)" % name, fortran)
        assert m and 'name="%s"' % name in fortran, f"{name} has no interface in athena_mp_c.f90"
        assert len(m.group(1).replace("&", "").split(",")) == n_args
