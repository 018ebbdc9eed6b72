"""The yardstick of max pooling over a handle's rows (athena_amd/csrc/pool.hip): the definition of include/athena_mp.h in numpy, one
loop per entry.  Nothing is computed on the values but the reverse sum: they are compared and copied, so the loops work on float32
as it stands (or on float64, the twin of the central-difference check) and every result is bit-defined.

A handle is the six arrays athena_mp_graph_export shows -- rowptr, col, eid of the forward CSR, t_rowptr, t_src, t_eid of the
transposed one, 0-based --, here a dict, as in tests/interp_reference.py (arrays_of derives them from a lexicographic pair list;
arrays_of_csr from any CSR without repeated columns in a row).  The loops run over the POSITION inside a row, and all rows that still
have an entry at that position take their step together -- each row sees its entries in CSR order.  No np.max, no np.argmax, no np.sum."""
import numpy as np

from interp_reference import arrays_of  # noqa: F401  (the handle of a two-set pair list)


def arrays_of_csr(rowptr, col, n_cols):
    """a 0-based CSR (no edge ids) -> the handle's arrays; the transposed CSR lists each column's rows ascending"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    t = np.argsort(col, kind="stable")
    return {"rowptr": rowptr.astype(np.int32), "col": col.astype(np.int32), "eid": np.full(col.size, -1, np.int32),
            "t_rowptr": np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_cols))]).astype(np.int32),
            "t_src": rows[t].astype(np.int32), "t_eid": np.full(col.size, -1, np.int32)}


def _positions(rowptr):
    """for each position k inside a row: (k, the rows that have an entry there, those entries)"""
    lens = np.diff(rowptr)
    for k in range(int(lens.max()) if lens.size else 0):
        r = np.nonzero(lens > k)[0]
        yield k, r, rowptr[r] + k


def _walk(A, values, source):
    """(y, arg) of the walk over every row: entry k's value is values[source[k]]"""
    n, F = A["rowptr"].size - 1, values.shape[1]
    y, arg = np.zeros((n, F), values.dtype), np.full((n, F), -1, np.int32)
    for k, r, p in _positions(A["rowptr"]):
        v, best = values[source[p]], y[r]
        with np.errstate(invalid="ignore"):
            take = (v > best) | (np.isnan(v) & ~np.isnan(best))
        if k == 0:
            take[:] = True                                          # there is no best yet
        y[r] = np.where(take, v, best)                              # a copy: the bits of v, NaN payload and sign of zero included
        arg[r] = np.where(take, A["col"][p][:, None], arg[r])
    return y, arg


def fwd(A, x):
    """vertex form: x [n_cols, F] -> (y [n_rows, F], arg [n_rows, F] int32)"""
    return _walk(A, x, A["col"])


def edges_fwd(A, h):
    """edge form: h [E, F] -> (y, arg); arg is again the column"""
    return _walk(A, h, A["eid"])


def bwd_x(A, arg, dy):
    """dx [n_cols, F]: acc = +0, then acc = acc + dy[i, f] over column j's rows ascending where arg[i, f] == j"""
    dx = np.zeros((A["t_rowptr"].size - 1, dy.shape[1]), dy.dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for _, c, p in _positions(A["t_rowptr"]):
            i = A["t_src"][p]
            dx[c] = np.where(arg[i] == c[:, None], dx[c] + dy[i], dx[c])
    return dx


def bwd_edges(A, arg, dy, E):
    """dh [E, F]: the entry k of row i, e = eid[k], j = col[k]: dh[e, f] = dy[i, f] where arg[i, f] == j, else +0"""
    dh = np.zeros((E, dy.shape[1]), dy.dtype)
    for _, r, p in _positions(A["rowptr"]):
        dh[A["eid"][p]] = np.where(arg[r] == A["col"][p][:, None], dy[r], dy.dtype.type(0))
    return dh


def attained_more_than_once(A, values, source, y):
    """[n_rows, F] bool: the maximum y[i, f] is attained by more than one entry of row i (by value: +0 equals -0, NaN equals NaN)"""
    count = np.zeros(y.shape, np.int64)
    for _, r, p in _positions(A["rowptr"]):
        v = values[source[p]]
        count[r] += (v == y[r]) | (np.isnan(v) & np.isnan(y[r]))
    return count > 1
