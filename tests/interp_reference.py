"""The yardstick of inverse-distance interpolation over a two-set graph (athena_amd/csrc/interp.hip): the definition of
include/athena_mp.h in numpy float32, every operation rounded on its own, and a float64 twin of the same formulas.

A handle is the six arrays athena_mp_graph_export shows -- rowptr, col, eid of the forward CSR, t_rowptr, t_src, t_eid of the
transposed one, 0-based --, here a dict; arrays_of derives them from the lexicographic pair list that tests/bipartite_reference.py
and tests/knn_bipartite_reference.py produce (csr_of gives the forward CSR; the transposed one is its stable sort by source).  The
sums are explicit loops in CSR order: the loop runs over the POSITION inside a row, and all rows that still have an entry at
that position take their step together -- each row's sum is the sequential one.  No np.sum, no @."""
import numpy as np

import bipartite_reference as br

F32 = np.float32


def arrays_of(i, j, nq, ns):
    """pairs (i, j) 0-based, strictly ascending in (i, j) -> the handle's arrays: entry k of row i is pair k (eid = k), column j
    lists its pairs with the queries ascending"""
    ia, ja = br.csr_of(np.asarray(i, np.int64), np.asarray(j, np.int64), nq)
    t = np.argsort(j, kind="stable")
    return {"rowptr": (ia - 1).astype(np.int32), "col": (ja[0] - 1).astype(np.int32), "eid": (ja[1] - 1).astype(np.int32),
            "t_rowptr": np.concatenate([[0], np.cumsum(np.bincount(j, minlength=ns))]).astype(np.int32),
            "t_src": np.asarray(i)[t].astype(np.int32), "t_eid": t.astype(np.int32)}


def edge_ends(A, E):
    """(query, source) of every edge column, from the forward CSR"""
    rows = np.repeat(np.arange(A["rowptr"].size - 1), np.diff(A["rowptr"]))
    ei, ej = np.zeros(E, np.int64), np.zeros(E, np.int64)
    ei[A["eid"]], ej[A["eid"]] = rows, A["col"]
    return ei, ej


def sqdist(coords, dtype=F32):
    """s_e = ((d0 d0) + d1 d1) + d2 d2, the builder's own expression"""
    d = coords.astype(dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        s = d[:, 0] * d[:, 0]
        for a in range(1, d.shape[1]):
            s = s + d[:, a] * d[:, a]
    return s


def raw_weight(coords, eps, dtype=F32):
    """(w_e, s_e): w_e = 1 / m_e, m_e = eps where s_e <= eps, else s_e; eps is the float32 the device holds"""
    s = sqdist(coords, dtype)
    eps = dtype(F32(eps))
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(s <= eps, eps, s).astype(dtype)
        return (dtype(1) / m).astype(dtype), s


def _row_loop(rowptr):
    """for each position k inside a row: (the rows that have an entry there, those entries)"""
    lens = np.diff(rowptr)
    for k in range(int(lens.max()) if lens.size else 0):
        r = np.nonzero(lens > k)[0]
        yield r, rowptr[r] + k


def weights(A, coords, eps, dtype=F32):
    """(weights [E], wsum [n_rows]): W_i = +0, then + w_eid[k] in row order; weights[e] = w_e / W_i, +0 along a row with W_i = 0"""
    w, _ = raw_weight(coords, eps, dtype)
    W = np.zeros(A["rowptr"].size - 1, dtype)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for r, p in _row_loop(A["rowptr"]):
            W[r] = W[r] + w[A["eid"][p]]
        ei, _ = edge_ends(A, w.size)
        out = np.where(W[ei] == 0, dtype(0), w / W[ei]).astype(dtype)
    return out, W


def gather(rowptr, idx, eid, wts, x, dtype=F32):
    """out[r, f] = acc, acc = +0, then acc = acc + wts[eid[k]] * x[idx[k], f] over row r in order"""
    out = np.zeros((rowptr.size - 1, x.shape[1]), dtype)
    wts, x = wts.astype(dtype), x.astype(dtype)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for r, p in _row_loop(rowptr):
            out[r] = out[r] + wts[eid[p]][:, None] * x[idx[p]]
    return out


def fwd(A, wts, x, dtype=F32):
    return gather(A["rowptr"], A["col"], A["eid"], wts, x, dtype)


def bwd_x(A, wts, dy, dtype=F32):
    return gather(A["t_rowptr"], A["t_src"], A["t_eid"], wts, dy, dtype)


def bwd_coords(A, coords, eps, wts, x, y, dy, dtype=F32):
    """dcoords [E, dim]: g_e = sum_f dy[i, f] * (x[j, f] - y[i, f]) (here f ascending), t_e = -(weights[e] * w_e) * g_e,
    dcoords[e, c] = (2 d_c) * t_e; exactly +0 where s_e <= eps or w_e = 0"""
    E = coords.shape[0]
    ei, ej = edge_ends(A, E)
    w, s = raw_weight(coords, eps, dtype)
    d, wts, x, y, dy = (a.astype(dtype) for a in (coords, wts, x, y, dy))
    g = np.zeros(E, dtype)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for f in range(x.shape[1]):
            g = g + dy[ei, f] * (x[ej, f] - y[ei, f])
        t = -(wts * w) * g
        out = (dtype(2) * d) * t[:, None]
    out[(s <= dtype(F32(eps))) | (w == 0)] = 0
    return out.astype(dtype)


def zero_by_definition(coords, eps):
    """the edges whose dcoords the definition sets to +0"""
    w, s = raw_weight(coords, eps)
    return (s <= F32(eps)) | (w == 0)


def dcoords_bound(coords, eps, wts, x, y, dy, A):
    """(F + 8) 2^-24 * 2 |d_c| * weights[e] * w_e * sum_f |dy| (|x| + |y|), in float64: one rounding each for the subtraction and
    the product, at most F - 1 for a sum in any order, three for the remaining products and four that w_e carries, each relative to
    a term no larger than the one written here"""
    E, F = coords.shape[0], x.shape[1]
    ei, ej = edge_ends(A, E)
    w, _ = raw_weight(coords, eps, np.float64)
    x, y, dy = (np.abs(a.astype(np.float64)) for a in (x, y, dy))
    mag = np.zeros(E)
    for f in range(F):
        mag = mag + dy[ei, f] * (x[ej, f] + y[ei, f])
    return (F + 8) * 2.0 ** -24 * 2 * np.abs(coords.astype(np.float64)) * (wts.astype(np.float64) * w * mag)[:, None]


# ---- the float64 twin: the same formulas, weights and y its own -------------------------------------------------------------------
def forward64(A, coords, eps, x):
    """(weights, wsum, y) in float64"""
    wts, W = weights(A, coords, eps, np.float64)
    return wts, W, fwd(A, wts, x, np.float64)


def grad64(A, coords, eps, x, dy):
    """(dx, dcoords) in float64 of L = sum dy * y(coords, x)"""
    wts, _, y = forward64(A, coords, eps, x)
    return bwd_x(A, wts, dy, np.float64), bwd_coords(A, coords, eps, wts, x, y, dy, np.float64)
