"""CPU: the yardstick of the bond-angle triplets (tests/triplets_reference.py) against itself -- its plain loops and its vectorised
form agree word for word on random CSRs with multi-edges, self-image entries, id-less self loops and rows of 0, 1 and 2
participants --, its float64 twin against central differences, the count of a star, and the C-ABI surface of the new entries: the
header, the ctypes prototypes and the Fortran interfaces declare the same functions."""
import os
import re

import numpy as np
import pytest

import triplets_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"athena_mp_triplet_pairs": 8, "athena_mp_entry_vectors_fwd": 4, "athena_mp_entry_vectors_bwd": 4,
           "athena_mp_triplet_cos_fwd": 4, "athena_mp_triplet_cos_bwd": 6, "athena_mp_triplet_stats": 1,
           "athena_mp_triplets_host": 10, "athena_mp_triplet_cos_bwd_host": 7}

bits = lambda a: np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def random_graph(seed, n=24, E=70, dim=3, self_loops=True):
    """(A, E, vec): a square CSR the way the builders leave it -- edge e = (i, j), i <= j, is the entry (i, j, e) and, when i < j,
    the entry (j, i, e) -- with repeated pairs (multi-edges: same column, another edge id), edges with i == j (self images: one
    entry each), a self loop without an edge id in front of every row, the last three vertices without any edge, and vertices that
    hold one and two edges; vec of unit scale, no vector shorter than 0.3"""
    rng = np.random.default_rng(seed)
    m = n - 3
    i, j = rng.integers(0, m - 4, E - 14), rng.integers(0, m - 4, E - 14)
    i, j = np.concatenate([i, i[:6], [2, 2, 5], [m - 4, m - 3, m - 3, m - 2, m - 1]]), \
        np.concatenate([j, j[:6], [2, 2, 5], [0, 1, 3, m - 1, m - 1]])          # repeats, self images, short rows (m - 1: images only)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    order = np.lexsort((hi, lo))
    lo, hi = lo[order], hi[order]
    E = lo.size
    rows = np.concatenate([lo, hi[lo < hi]])
    cols = np.concatenate([hi, lo[lo < hi]])
    eids = np.concatenate([np.arange(E), np.arange(E)[lo < hi]])
    if self_loops:
        rows, cols, eids = (np.concatenate([a, b]) for a, b in ((rows, np.arange(n)), (cols, np.arange(n)), (eids, np.full(n, -1))))
    order = np.lexsort((eids, cols, rows))
    rows, cols, eids = rows[order], cols[order], eids[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    vec = rng.standard_normal((E, dim))
    norm = np.sqrt((vec * vec).sum(axis=1, keepdims=True))
    vec = np.where(norm < 0.3, vec * (0.3 / norm), vec)
    return tr.graph_arrays(rowptr, cols, eids, E), E, vec


def _row_participants(A, take):
    return np.bincount(tr.rows_of(A["rowptr"])[take], minlength=A["rowptr"].size - 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("cutoff3", [np.inf, 1.6])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_the_two_forms_agree_word_for_word(dim, cutoff3, dtype):
    A, E, vec = random_graph(4100 + dim, dim=dim, self_loops=dim != 2)
    vec = vec.astype(np.float32)
    rng = np.random.default_rng(7)
    draw = lambda T: rng.standard_normal(T).astype(np.float32)
    rows, col, eid = tr.rows_of(A["rowptr"]), A["col"], A["eid"]
    take = tr.participants(A, vec, dim, cutoff3, dtype)
    m = _row_participants(A, take)
    assert {0, 1, 2} <= set(m.tolist()) and m.max() > 4
    assert ((rows == col) & (eid >= 0)).any(), "self-image entries"
    assert ((rows == col) & (eid < 0)).any() == (dim != 2), "id-less self loops"
    same_pair = (rows[1:] == rows[:-1]) & (col[1:] == col[:-1]) & (eid[1:] != eid[:-1]) & (eid[1:] >= 0) & (eid[:-1] >= 0)
    assert same_pair.any(), "multi-edges"
    if np.isfinite(cutoff3):
        assert 0 < take.sum() < (eid >= 0).sum(), "the cutoff drops some entries and keeps some"
    rng = np.random.default_rng(7)
    loop = tr.everything(A, E, vec, dim, cutoff3, draw, dtype, "loop")
    rng = np.random.default_rng(7)
    fast = tr.everything(A, E, vec, dim, cutoff3, draw, dtype, "vector")
    T = loop["pairs"].shape[0]
    assert T == tr.count(A, take) == int((m * (m - 1)).sum()) and T > 100
    assert np.array_equal(loop["pairs"], fast["pairs"]) and np.array_equal(loop["rowptr"], fast["rowptr"])
    p = loop["pairs"]
    assert (np.diff(p[:, 0] * (p.max() + 1) + p[:, 1]) > 0).all() and (p[:, 0] != p[:, 1]).all(), "strictly ascending, no (k, k)"
    assert (rows[p[:, 0]] == rows[p[:, 1]]).all() and take[p].all()
    assert np.array_equal(loop["rowptr"], np.searchsorted(p[:, 0], np.arange(rows.size + 1)))
    for key in ("dir", "cos", "ddir", "dvec"):
        assert loop[key].dtype == dtype and np.array_equal(bits(loop[key]), bits(fast[key])), key
    assert np.abs(loop["cos"]).max() <= 1 + 1e-6
    assert dim == 1 or np.abs(loop["dvec"]).max() > 0.1            # on a line every cosine is 1 or -1: the gradient is rounding only
    no_triplet = np.ones(rows.size, bool)
    no_triplet[p.reshape(-1)] = False
    assert no_triplet.any() and not loop["ddir"][no_triplet].any()


def test_coincident_points_give_plus_zero_in_both_forms():
    A, E, vec = random_graph(4200)
    vec = vec.astype(np.float32)
    vec[::5] = 0.0
    vec[3] = -0.0
    draw = lambda T: np.linspace(-1, 1, T).astype(np.float32)
    for form in ("loop", "vector"):
        r = tr.everything(A, E, vec, 3, np.inf, draw, np.float32, form)
        flat =(~r["dir"][r["pairs"][:, 0]].any(axis=1)) | (~r["dir"][r["pairs"][:, 1]].any(axis=1))
        assert flat.sum() > 20 and not bits(r["cos"])[flat].any(), "den == 0 gives +0, not -0 or NaN"
        assert np.isfinite(r["ddir"]).all() and np.isfinite(r["dvec"]).all()


@pytest.mark.parametrize("cutoff3", [np.inf, 1.6])
def test_the_float64_twin_agrees_with_central_differences(cutoff3):
    """L = sum_t w_t cos_t.  h = 1e-6 on vectors of unit scale: truncation about h^2 = 1e-12, round-off about 2^-53 / h = 1e-10, so
    the bound 1e-6 of the largest gradient component has four digits of margin"""
    A, E, vec = random_graph(4300, n=16, E=34)
    f32 = vec.astype(np.float32)
    r = np.sqrt((f32.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(r - 1.6).min() > 1e-3, "no edge so close to the cutoff that a step of h moves it across"
    take = tr.participants(A, f32, 3, cutoff3)
    pairs, _ = tr.triplets(A, take)
    TA = tr.triplet_arrays(pairs, int(A["rowptr"][-1]))
    w = np.random.default_rng(5).standard_normal(pairs.shape[0])
    x = f32.astype(np.float64)
    loss_dir = lambda d: float((w * tr.cos(pairs, d, np.float64)).sum())
    loss_vec = lambda v: loss_dir(tr.entry_vectors(A, v, 3, np.float64))
    dirs = tr.entry_vectors(A, x, 3, np.float64)
    ddir = tr.cos_bwd(TA, dirs, tr.cos(pairs, dirs, np.float64), w, np.float64)
    dvec = tr.entry_vectors_bwd(A, ddir, E, np.float64)
    h = 1e-6
    for grad, at, loss in ((ddir, dirs, loss_dir), (dvec, x, loss_vec)):
        num = np.zeros_like(grad)
        for idx in np.ndindex(*grad.shape):
            up, dn = at.copy(), at.copy()
            up[idx] += h
            dn[idx] -= h
            num[idx] = (loss(up) - loss(dn)) / (2 * h)
        top = np.abs(num).max()
        assert top > 0.5 and np.abs(grad - num).max() <= 1e-6 * top, (np.abs(grad - num).max(), top)
    # an entry without an edge id carries no gradient, and a row's entries that do not take part none either
    assert not ddir[A["eid"] < 0].any() and not ddir[~take].any()


def test_the_star_of_46341_leaves_has_2147441940_triplets():
    leaves = 46341
    rowptr = np.concatenate([[0], [leaves], leaves + 1 + np.arange(leaves)])
    A = {"rowptr": rowptr, "col": np.concatenate([1 + np.arange(leaves), np.zeros(leaves, np.int64)]),
         "eid": np.concatenate([np.arange(leaves), np.arange(leaves)])}
    T = tr.count(A, np.ones(2 * leaves, bool))
    assert T == tr.star_count(leaves) == 2147441940 and T < 2 ** 31
    assert tr.star_count(leaves + 1) == 2147534622 and tr.star_count(leaves + 1) >= 2 ** 31


def test_declarations_agree():
    from athena_amd import _capi

    header = open(os.path.join(ROOT, "include", "athena_mp.h")).read()
    fortran = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    build = open(os.path.join(ROOT, "athena_amd", "csrc", "build.sh")).read()
    assert " triplets.hip " in build
    declared = _capi.declared_symbols()
    public = ",".join(line.split("::", 1)[1] for line in fortran.splitlines() if line.strip().startswith("public ::"))
    public = {name.strip() for name in public.split(",")}
    for name, n_args in ENTRIES.items():
        assert name in declared, f"{name} is not among the header's symbols"
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in athena_mp.h"
        assert len(m.group(1).split(",")) == n_args
        assert name in _capi._PROTOS and len(_capi._PROTOS[name]) == n_args, f"{name} has no ctypes prototype"
        m = re.search(r"function %s\(([^)]*)\)" % name, fortran)
        assert m and 'name="%s"' % name in fortran, f"{name} has no interface in athena_mp_c.f90"
        assert len(m.group(1).replace("&", "").split(",")) == n_args
        assert name in public, f"{name} is not public in athena_mp_c.f90"
