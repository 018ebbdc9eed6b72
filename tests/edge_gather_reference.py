"""The yardstick of the gather that makes the edge MLP's input over a two-set handle, and of its reverse
(athena_amd/csrc/edge_gather.hip): the definition of include/athena_mp.h in numpy float32, and a float64 twin of the same loops.

A handle is the six arrays athena_mp_graph_export shows -- rowptr, col, eid of the forward CSR, t_rowptr, t_src, t_eid of the
transposed one, 0-based --, here a dict, as in tests/interp_reference.py (arrays_of derives them from a lexicographic pair list).
The loops run over the POSITION inside a row, and all rows that still have an entry at that position take their step together --
each row sees its entries in CSR order, each sum is the sequential one.  No np.sum, no np.add.at, no concatenate: a copy is an
assignment between arrays of one dtype, which keeps every bit, and the one arithmetic operation of the forward is the subtraction.

h and dh are [E, ld] with ld >= W = Fs + Fq + dim: fwd writes into the array it is given and touches nothing beyond column W; the
reverse loops never index beyond it.  A block of width 0 is None."""
import numpy as np

from interp_reference import arrays_of  # noqa: F401  (the handle of a two-set pair list)

F32 = np.float32


def _positions(rowptr):
    """for each position k inside a row: (the rows that have an entry there, those entries)"""
    lens = np.diff(rowptr)
    for k in range(int(lens.max()) if lens.size else 0):
        r = np.nonzero(lens > k)[0]
        yield r, rowptr[r] + k


def widths_of(xs, xq, coords):
    return tuple(0 if a is None else int(a.shape[1]) for a in (xs, xq, coords))


def fwd(A, xs, xq, coords, relative, h, dtype=F32):
    """writes the W defined columns of h [E, ld] (dtype) in place and returns it: for the entry k of row i, j = col[k], e = eid[k]:
    h[e, :Fs] = xs[j] (relative: xs[j] - xq[i]), h[e, Fs:Fs + Fq] = xq[i], h[e, Fs + Fq:W] = coords[e]"""
    Fs, Fq, dim = widths_of(xs, xq, coords)
    assert h.dtype == dtype and h.shape[1] >= Fs + Fq + dim >= 1 and (not relative or Fs == Fq >= 1)
    for a in (xs, xq, coords):
        assert a is None or a.dtype == dtype
    for i, p in _positions(A["rowptr"]):
        j, e = A["col"][p], A["eid"][p]
        if Fs:
            if relative:
                with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                    h[e, :Fs] = xs[j] - xq[i]
            else:
                h[e, :Fs] = xs[j]
        if Fq:
            h[e, Fs:Fs + Fq] = xq[i]
        if dim:
            h[e, Fs + Fq:Fs + Fq + dim] = coords[e]
    return h


def bwd_sources(A, dh, Fs):
    """dxs [n_cols, Fs]: acc = +0, then acc = acc + dh[t_eid[k], f] over column j's entries in order"""
    out = np.zeros((A["t_rowptr"].size - 1, Fs), dh.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for j, p in _positions(A["t_rowptr"]):
            out[j] = out[j] + dh[A["t_eid"][p], :Fs]
    return out


def bwd_queries(A, dh, Fs, Fq, relative):
    """dxq [n_rows, Fq]: acc = +0, then per entry in row order acc = acc + dh[e, Fs + f] and, with relative, after that
    acc = acc - dh[e, f]"""
    out = np.zeros((A["rowptr"].size - 1, Fq), dh.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, p in _positions(A["rowptr"]):
            e = A["eid"][p]
            out[i] = out[i] + dh[e, Fs:Fs + Fq]
            if relative:
                out[i] = out[i] - dh[e, :Fs]
    return out


def bwd_coords(dh, Fs, Fq, dim):
    """dcoords [E, dim] = dh[:, Fs + Fq : Fs + Fq + dim], a copy"""
    out = np.zeros((dh.shape[0], dim), dh.dtype)
    out[:] = dh[:, Fs + Fq:Fs + Fq + dim]
    return out


def bwd(A, dh, widths, relative):
    """(dxs, dxq, dcoords) of dh [E, ld]"""
    Fs, Fq, dim = widths
    return bwd_sources(A, dh, Fs), bwd_queries(A, dh, Fs, Fq, relative), bwd_coords(dh, Fs, Fq, dim)


# ---- the float64 twin: the same loops on float64 arrays -----------------------------------------------------------------------------
def fwd64(A, xs, xq, coords, relative, E):
    """h [E, W] in float64 (a fresh array of zeros underneath)"""
    xs, xq, coords = (None if a is None else a.astype(np.float64) for a in (xs, xq, coords))
    return fwd(A, xs, xq, coords, relative, np.zeros((E, sum(widths_of(xs, xq, coords))), np.float64), np.float64)


def bwd64(A, dh, widths, relative):
    return bwd(A, dh.astype(np.float64), widths, relative)
