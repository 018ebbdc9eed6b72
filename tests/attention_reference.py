"""The yardstick of attention pooling over a handle's rows (athena_amd/csrc/attention.hip): the definition of include/athena_mp.h in
numpy float32, every operation rounded on its own, and a float64 twin of the same formulas (dtype=np.float64).

A handle is the six arrays athena_mp_graph_export shows, a dict as in tests/interp_reference.py (arrays_of derives them from a
lexicographic pair list).  H heads over F = H C feature columns: the head of column c is c // C.  The loops run over the POSITION
inside a row, and all rows that still have an entry at that position take their step together -- each row sees its entries in CSR
order, so every sum is the sequential one.  No np.max, no np.sum, no @.

alpha is the one result that is not bit-defined (exp): softmax64 returns it with the scale and the exp argument that
activation_reference.assert_each takes, as activation_reference.softmax does."""
import numpy as np

from activation_reference import assert_each, bound  # noqa: F401  (the per-element bound alpha is held to)
from interp_reference import _row_loop, arrays_of, edge_ends  # noqa: F401

F32 = np.float32


def head_of(F, H):
    """[F] the head of every feature column"""
    assert H >= 1 and F >= 1 and F % H == 0
    return np.arange(F) // (F // H)


# ---- the softmax over a row's entries ----------------------------------------------------------------------------------------------
def _row_max(A, s):
    """[n_rows, H]: v replaces m where v > m, from -inf: a NaN is never taken (it turns up in p)"""
    m = np.full((A["rowptr"].size - 1, s.shape[1]), -np.inf, s.dtype)
    with np.errstate(invalid="ignore"):
        for r, p in _row_loop(A["rowptr"]):
            v = s[A["eid"][p]]
            m[r] = np.where(v > m[r], v, m[r])
    return m


def softmax(A, scores, dtype=F32):
    """alpha [E, H]: m the row's maximum, p = exp(s - m), S = p_0 + p_1 + ... in row order, alpha = p / S"""
    s = np.asarray(scores).astype(dtype)
    m = _row_max(A, s)
    S = np.zeros_like(m)
    alpha = np.full(s.shape, np.nan, dtype)                         # every edge lies in one row: nothing stays
    with np.errstate(invalid="ignore", under="ignore", over="ignore", divide="ignore"):
        for r, p in _row_loop(A["rowptr"]):
            S[r] = S[r] + np.exp(s[A["eid"][p]] - m[r])
        for r, p in _row_loop(A["rowptr"]):
            e = A["eid"][p]
            alpha[e] = np.exp(s[e] - m[r]) / S[r]
    return alpha


def softmax64(A, scores):
    """(alpha, scale = alpha, a = scores - m) in float64 over the fp32 scores"""
    assert np.asarray(scores).dtype == np.float32
    alpha = softmax(A, scores, np.float64)
    m = _row_max(A, np.asarray(scores).astype(np.float64))
    ei, _ = edge_ends(A, alpha.shape[0])
    with np.errstate(invalid="ignore"):
        a = np.asarray(scores).astype(np.float64) - m[ei]
    return alpha, alpha, a


def softmax_bwd(A, alpha, dalpha, dtype=F32):
    """dscores [E, H]: dot = +0, then + alpha dalpha in row order; dscores = alpha (dalpha - dot)"""
    y, d = np.asarray(alpha).astype(dtype), np.asarray(dalpha).astype(dtype)
    dot = np.zeros((A["rowptr"].size - 1, y.shape[1]), dtype)
    out = np.full(y.shape, np.nan, dtype)
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        for r, p in _row_loop(A["rowptr"]):
            e = A["eid"][p]
            dot[r] = dot[r] + y[e] * d[e]
        for r, p in _row_loop(A["rowptr"]):
            e = A["eid"][p]
            out[e] = y[e] * (d[e] - dot[r])
    return out


# ---- the gathers ---------------------------------------------------------------------------------------------------------------
def _gather(rowptr, src, eid, alpha, values, H, dtype):
    """out[r, c] = acc, acc = +0, then acc = acc + alpha[eid[k], c // C] * values[src[k], c] over row r in order"""
    alpha, values = np.asarray(alpha).astype(dtype), np.asarray(values).astype(dtype)
    F = values.shape[1]
    head = head_of(F, H)
    out = np.zeros((rowptr.size - 1, F), dtype)
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        for r, p in _row_loop(rowptr):
            out[r] = out[r] + alpha[eid[p]][:, head] * values[src[p]]
    return out


def fwd(A, alpha, x, H, dtype=F32):
    """vertex form: y [n_rows, F]"""
    return _gather(A["rowptr"], A["col"], A["eid"], alpha, x, H, dtype)


def edges_fwd(A, alpha, h, H, dtype=F32):
    """edge form: y [n_rows, F]"""
    return _gather(A["rowptr"], A["eid"], A["eid"], alpha, h, H, dtype)


def bwd_x(A, alpha, dy, H, dtype=F32):
    """dx [n_cols, F]: the same sum over column j, queries ascending"""
    return _gather(A["t_rowptr"], A["t_src"], A["t_eid"], alpha, dy, H, dtype)


def bwd_edges(A, alpha, dy, H, dtype=F32):
    """dh [E, F] = alpha[e, c // C] * dy[i, c]"""
    alpha, dy = np.asarray(alpha).astype(dtype), np.asarray(dy).astype(dtype)
    ei, _ = edge_ends(A, alpha.shape[0])
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        return alpha[:, head_of(dy.shape[1], H)] * dy[ei]


def alpha_terms(A, E, x, h, dy, H, dtype=F32):
    """[E, H, C]: the terms dy[i, c] * v of every dalpha[e, h], v = x[j, c] or h[e, c]"""
    assert (x is None) != (h is None)
    ei, ej = edge_ends(A, E)
    dy = np.asarray(dy).astype(dtype)
    v = np.asarray(h).astype(dtype) if x is None else np.asarray(x).astype(dtype)[ej]
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        t = dy[ei] * v
    return t.reshape(E, H, dy.shape[1] // H)


def bwd_alpha(A, E, x, h, dy, H, dtype=F32, order="sequential"):
    """dalpha [E, H], the terms added in one of two orders: "sequential", t_0 + t_1 + ... over the head's columns, or "tree": each
    run of four columns sequentially, then the first half of the runs onto the second until one is left (C = 4 L, L a power of two),
    which is the kernel's __shfl_xor tree.  At C = 1 the product."""
    t = alpha_terms(A, E, x, h, dy, H, dtype)
    C = t.shape[2]
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        if order == "sequential":
            acc = t[:, :, 0]
            for c in range(1, C):
                acc = acc + t[:, :, c]
            return acc
        assert order == "tree" and C % 4 == 0 and (C // 4) & (C // 4 - 1) == 0
        q = t.reshape(E, H, C // 4, 4)
        part = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
        while part.shape[2] > 1:
            half = part.shape[2] // 2
            part = part[:, :, :half] + part[:, :, half:]
        return part[:, :, 0]


def alpha_bound(A, E, x, h, dy, H):
    """(f64, bound): |dev - f64| <= |seq32 - f64| + 1e-5 sum_c |dy v|, the project's 1e-5 relative to the sum's own terms"""
    f64 = bwd_alpha(A, E, x, h, dy, H, np.float64)
    seq = bwd_alpha(A, E, x, h, dy, H, F32).astype(np.float64)
    mag = np.abs(alpha_terms(A, E, x, h, dy, H, np.float64))
    total = mag[:, :, 0]
    for c in range(1, mag.shape[2]):
        total = total + mag[:, :, c]
    return f64, np.abs(seq - f64) + 1e-5 * total
