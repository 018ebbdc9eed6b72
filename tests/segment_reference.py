"""The yardstick of the row gathers (athena_amd/csrc/agg.hip, capi.hip:build_long_plan): the fp32 expression every gather of a
handle evaluates, hub rows included, in numpy and the CPU oracle.  It never touches the device code.

For a row of L entries in CSR order, term_w = x[idx_w] (no coefficient) or coef_w * x[idx_w] (a rounded multiply, then a rounded add):

    L <= 512   s = 0; s = s + term_w in entry order                                  -- the oracle's sum; 512 is still a short row
    L  > 512   the entries are cut into consecutive segments of 512 from the row's first entry (the last one may be shorter);
               p_k = the same sequential sum over segment k, started at 0;  y = (((0 + p_0) + p_1) + ...) in fp32;
               an activation is applied once, to y

A sum that starts at +0 is never -0, so 0 + p_0 = p_0 bit for bit and one formula serves every row.  Entries whose index is negative
(an entry without an edge column) are skipped but keep their place: segments are cut by entry position.

The Kipf coefficient is the oracle's own number -- the host powf of the product of the full row's and the column's degree: the split
CSR, in which every hub row is replaced by its segments as rows of their own, goes through oracle.kipf_propagate_rect with row_deg =
the FULL row's degree, and the segment rows are added in order with np.float32 adds.  The exact reverse form is the same on the
transposed CSR (sources ascending, entry order kept: a stable sort by column).  Coefficient-free gathers are numpy adds alone.

Arrays are athena's: adj_ia [n + 1] 1-based, adj_ja [2, nnz] 1-based neighbour / edge column (0 = none), features [N, F] float32."""
import numpy as np

K_LONG = 512   # kLongRow of athena_amd/csrc/common.h


def _oracle():
    from oracle import oracle

    return oracle


def split_rows(rowptr, k_long=K_LONG):
    """0-based rowptr [n + 1] -> (seg_beg [S], seg_end [S], seg_row [S], seg_ord [S]): the segments of every row in row order; a row
    of at most k_long entries (an empty one too) is one segment, seg_ord counts the segments of a row from 0"""
    rowptr = np.asarray(rowptr, np.int64)
    lens = np.diff(rowptr)
    nseg = np.where(lens > k_long, -(-lens // k_long), 1)
    seg_row = np.repeat(np.arange(lens.size), nseg)
    first = np.concatenate([[0], np.cumsum(nseg)])[:-1]
    seg_ord = np.arange(seg_row.size) - first[seg_row]
    seg_beg = rowptr[seg_row] + seg_ord * k_long
    seg_end = np.minimum(seg_beg + k_long, rowptr[seg_row + 1])
    assert (seg_end >= seg_beg).all() and (seg_end - seg_beg <= k_long).all()
    assert np.array_equal(np.bincount(seg_row, seg_end - seg_beg, minlength=lens.size).astype(np.int64), lens)
    return seg_beg, seg_end, seg_row, seg_ord


def sequential_sum(beg, end, idx, x):
    """out[s] = 0; out[s] = out[s] + x[idx[w]] for w = beg[s] .. end[s] - 1 in order, every add rounded to fp32; idx < 0: skipped"""
    beg, end, idx = (np.asarray(a, np.int64) for a in (beg, end, idx))
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    out = np.zeros((beg.size, x.shape[1]), np.float32)
    lens = end - beg
    for k in range(int(lens.max()) if lens.size else 0):
        rows = np.nonzero(lens > k)[0]
        i = idx[beg[rows] + k]
        ok = i >= 0
        rows, i = rows[ok], i[ok]
        out[rows] = out[rows] + x[i]
    assert out.dtype == np.float32
    return out


def combine(partial, seg_row, seg_ord, n_rows):
    """y[r] = (((0 + p_0) + p_1) + ...) over the segments of row r in order, fp32 adds"""
    partial = np.asarray(partial)
    assert partial.dtype == np.float32
    y = np.zeros((n_rows, partial.shape[1]), np.float32)
    for j in range(int(seg_ord.max()) + 1 if seg_ord.size else 0):
        s = np.nonzero(seg_ord == j)[0]
        y[seg_row[s]] = y[seg_row[s]] + partial[s]          # a row has one segment of each ordinal: no index repeats
    assert y.dtype == np.float32
    return y


def gather_sum(rowptr, idx, x, k_long=K_LONG):
    """the coefficient-free gather of a 0-based CSR (rowptr [n + 1], idx [nnz], negative = skipped) over the rows of x"""
    beg, end, seg_row, seg_ord = split_rows(rowptr, k_long)
    return combine(sequential_sum(beg, end, idx, x), seg_row, seg_ord, np.asarray(rowptr).size - 1)


def transpose(adj_ia, adj_ja, n_cols):
    """(t_ia [n_cols + 1] 1-based, t_ja [2, nnz] 1-based sources / edge columns) with the entries of every transposed row in the
    forward CSR's entry order (sources ascending): the order of the reference's scatter, and of the handle's transposed CSR"""
    ia = np.asarray(adj_ia, np.int64)
    ja = np.asarray(adj_ja, np.int64)
    rows = np.repeat(np.arange(1, ia.size), np.diff(ia))
    order = np.argsort(ja[0], kind="stable")
    t_ia = np.concatenate([[1], 1 + np.cumsum(np.bincount(ja[0] - 1, minlength=n_cols))]).astype(np.int32)
    t_ja = np.zeros((2, ja.shape[1]), np.int32, order="F")
    t_ja[0] = rows[order]
    t_ja[1] = ja[1][order]
    return t_ia, t_ja


def _kipf(x, adj_ia, adj_ja, row_deg, col_deg, k_long):
    """the coefficient-weighted gather over the rows of (adj_ia, adj_ja): the oracle on the split CSR, then the ordered combine"""
    ia = np.asarray(adj_ia, np.int64)
    n_rows = ia.size - 1
    beg, end, seg_row, seg_ord = split_rows(ia - 1, k_long)
    seg_ia = np.concatenate([beg, end[-1:]] if beg.size else [[0]]).astype(np.int32) + 1
    assert seg_ia[0] == 1 and np.array_equal(seg_ia[1:] - 1, end)      # consecutive segments: the entries stay where they are
    seg_deg = np.ascontiguousarray(np.asarray(row_deg, np.int32)[seg_row])
    p = _oracle().kipf_propagate_rect(x, seg_ia, adj_ja, seg_deg, np.asarray(col_deg, np.int32))
    return combine(p, seg_row, seg_ord, n_rows)


def _degrees(adj_ia, n_cols, row_deg, col_deg):
    n_rows = np.asarray(adj_ia).size - 1
    if row_deg is None:
        assert col_deg is None and n_cols in (None, n_rows), "a rectangular block needs explicit degrees"
        row_deg = col_deg = np.diff(np.asarray(adj_ia)).astype(np.int32)
    return np.asarray(row_deg, np.int32), np.asarray(col_deg, np.int32)


def kipf_propagate(x, adj_ia, adj_ja, row_deg=None, col_deg=None, k_long=K_LONG):
    """athena_mp_kipf_propagate_fwd (and reverse_kipf_propagate_partial): y [n_rows, F]"""
    x = np.ascontiguousarray(x, np.float32)
    row_deg, col_deg = _degrees(adj_ia, x.shape[0], row_deg, col_deg)
    assert col_deg.size == x.shape[0]
    return _kipf(x, adj_ia, adj_ja, row_deg, col_deg, k_long)


def kipf_propagate_bwd(grad, adj_ia, adj_ja, exact=False, n_out=None, row_deg=None, col_deg=None, k_long=K_LONG):
    """athena_mp_kipf_propagate_bwd (and reverse_kipf_propagate, ..._partial_val): dx [n_out, F] over the transposed CSR; exact: with
    the coefficient of the entry, the same integer product of the two degrees"""
    grad = np.ascontiguousarray(grad, np.float32)
    n_rows = np.asarray(adj_ia).size - 1
    assert grad.shape[0] == n_rows
    n_out = n_rows if n_out is None else int(n_out)
    row_deg, col_deg = _degrees(adj_ia, n_out, row_deg, col_deg)
    t_ia, t_ja = transpose(adj_ia, adj_ja, n_out)
    if exact:
        return _kipf(grad, t_ia, t_ja, col_deg, row_deg, k_long)
    return gather_sum(t_ia.astype(np.int64) - 1, t_ja[0].astype(np.int64) - 1, grad, k_long)


def neighbour_sum(x, adj_ia, adj_ja, k_long=K_LONG):
    """the plain half of athena_mp_kipf_propagate_fwd_dual = duvenaud_propagate with F_e = 0"""
    return gather_sum(np.asarray(adj_ia, np.int64) - 1, np.asarray(adj_ja, np.int64)[0] - 1, np.ascontiguousarray(x, np.float32), k_long)


def duvenaud_propagate(x, e, adj_ia, adj_ja, k_long=K_LONG):
    """athena_mp_duvenaud_propagate_fwd: [n_rows, Fv + Fe]; x None: the edge part alone, e None: the vertex part alone"""
    rowptr = np.asarray(adj_ia, np.int64) - 1
    ja = np.asarray(adj_ja, np.int64)
    parts = []
    if x is not None:
        parts.append(gather_sum(rowptr, ja[0] - 1, np.ascontiguousarray(x, np.float32), k_long))
    if e is not None:
        parts.append(gather_sum(rowptr, ja[1] - 1, np.ascontiguousarray(e, np.float32), k_long))
    return np.ascontiguousarray(np.concatenate(parts, axis=1))


def duvenaud_propagate_bwd_x(grad, Fv, adj_ia, adj_ja, n_out=None, k_long=K_LONG):
    """athena_mp_duvenaud_propagate_bwd_x: the vertex part of packed rows [n_rows, Fv + Fe] gathered over the transposed CSR"""
    grad = np.asarray(grad, np.float32)
    n_out = np.asarray(adj_ia).size - 1 if n_out is None else int(n_out)
    t_ia, t_ja = transpose(adj_ia, adj_ja, n_out)
    return gather_sum(t_ia.astype(np.int64) - 1, t_ja[0].astype(np.int64) - 1, np.ascontiguousarray(grad[:, :Fv]), k_long)
