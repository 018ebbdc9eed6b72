"""The yardstick of the bond-angle triplets (athena_amd/csrc/triplets.hip): the definition of include/athena_mp.h in numpy, twice -- a
plain loop per entry and per triplet (form="loop") and a vectorised form (form="vector") that takes all rows' steps of one position
together, so that every row still sees its terms in the defined order.  Both are parametrised by dtype: np.float32 gives the words
the device must give, np.float64 the twin of the central-difference check.  Every operation is rounded on its own (numpy scalars
and arrays of one dtype do that); / and sqrt are correctly rounded.

A handle is a dict of the arrays athena_mp_graph_export shows, 0-based: rowptr, col, eid of the forward CSR and e_rowptr, e_row,
e_entry of the edge index for the graph g; rowptr, col, eid, t_rowptr, t_src, t_eid for the triplet handle (triplet_arrays)."""
import numpy as np

import interp_reference as ir


def rows_of(rowptr):
    """the row of every CSR entry"""
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))


def edge_index(rowptr, col, eid, E):
    """(e_rowptr, e_row, e_entry): column e lists the entries that carry it, in entry order"""
    eid = np.asarray(eid, np.int64)
    k = np.nonzero(eid >= 0)[0]
    k = k[np.argsort(eid[k], kind="stable")]
    e_rowptr = np.concatenate([[0], np.cumsum(np.bincount(eid[k], minlength=E))])
    return e_rowptr.astype(np.int32), rows_of(rowptr)[k].astype(np.int32), k.astype(np.int32)


def graph_arrays(rowptr, col, eid, E):
    e_rowptr, e_row, e_entry = edge_index(rowptr, col, eid, E)
    return {"rowptr": np.asarray(rowptr, np.int32), "col": np.asarray(col, np.int32), "eid": np.asarray(eid, np.int32),
            "e_rowptr": e_rowptr, "e_row": e_row, "e_entry": e_entry}


def _positions(rowptr):
    """for each position inside a row: (the rows that have an entry there, those entries)"""
    rowptr = np.asarray(rowptr, np.int64)
    lens = np.diff(rowptr)
    for k in range(int(lens.max()) if lens.size else 0):
        r = np.nonzero(lens > k)[0]
        yield r, rowptr[r] + k


# ---- entry vectors ---------------------------------------------------------------------------------------------------------------------
def entry_vectors(A, vec, dim, dtype=np.float32, form="vector"):
    """dir [nnz, dim]: -vec[e] when i <= c, +vec[e] when i > c, +0 when e < 0"""
    rows, col, eid = rows_of(A["rowptr"]), np.asarray(A["col"], np.int64), np.asarray(A["eid"], np.int64)
    nnz = col.size
    out = np.zeros((nnz, dim), dtype)
    if vec is None:
        assert (eid < 0).all()
        return out
    vec = np.asarray(vec, dtype).reshape(-1, dim)
    if form == "loop":
        for k in range(nnz):
            if eid[k] >= 0:
                for d in range(dim):
                    out[k, d] = -vec[eid[k], d] if rows[k] <= col[k] else vec[eid[k], d]
        return out
    has = eid >= 0
    v = vec[eid[has]]
    out[has] = np.where((rows[has] <= col[has])[:, None], -v, v)
    return out


def entry_vectors_bwd(A, ddir, E, dtype=np.float32, form="vector"):
    """dvec [E, dim]: acc = +0, then over the entries of edge column e in edge-index order acc = acc -+ ddir[k]"""
    ddir = np.asarray(ddir, dtype)
    dim = ddir.shape[1]
    col = np.asarray(A["col"], np.int64)
    out = np.zeros((E, dim), dtype)
    if form == "loop":
        for e in range(E):
            for p in range(A["e_rowptr"][e], A["e_rowptr"][e + 1]):
                i, k = A["e_row"][p], A["e_entry"][p]
                for d in range(dim):
                    out[e, d] = out[e, d] - ddir[k, d] if i <= col[k] else out[e, d] + ddir[k, d]
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        for e, p in _positions(A["e_rowptr"]):
            i, k = np.asarray(A["e_row"], np.int64)[p], np.asarray(A["e_entry"], np.int64)[p]
            out[e] = np.where((i <= col[k])[:, None], out[e] - ddir[k], out[e] + ddir[k])
    return out


# ---- participants and triplets -----------------------------------------------------------------------------------------------------
def participants(A, vec, dim, cutoff3, dtype=np.float32):
    """[nnz] bool: e >= 0, and with a finite cutoff3 r < cutoff3, r = sqrt(((x0 x0) + x1 x1) + x2 x2) over x = vec[e]"""
    eid = np.asarray(A["eid"], np.int64)
    take = eid >= 0
    if np.isinf(cutoff3):
        return take
    x = np.asarray(vec, dtype).reshape(-1, dim)[np.maximum(eid, 0)]
    with np.errstate(over="ignore", invalid="ignore"):
        s = x[:, 0] * x[:, 0]
        for d in range(1, dim):
            s = s + x[:, d] * x[:, d]
        r = np.sqrt(s)
        return take & (r < dtype(np.float32(cutoff3)))


def count(A, take):
    """the number of triplets, as a Python integer: the sum of m (m - 1) over the rows"""
    m = np.bincount(rows_of(A["rowptr"])[np.asarray(take, bool)], minlength=len(A["rowptr"]) - 1)
    return sum(int(v) * (int(v) - 1) for v in m)


def star_count(leaves):
    """T of a star: the centre's row holds every leaf, each leaf's row one entry"""
    return leaves * (leaves - 1)


def triplets(A, take, form="vector"):
    """(pairs [T, 2] int64 0-based (k, k'), rowptr [nnz + 1] int64) in lexicographic order of (k, k')"""
    rowptr = np.asarray(A["rowptr"], np.int64)
    nnz = int(rowptr[-1])
    if form == "loop":
        pairs, first = [], np.zeros(nnz + 1, np.int64)
        for i in range(rowptr.size - 1):
            ks = [k for k in range(rowptr[i], rowptr[i + 1]) if take[k]]
            for k in range(rowptr[i], rowptr[i + 1]):
                first[k] = len(pairs)
                if take[k]:
                    pairs.extend((k, k2) for k2 in ks if k2 != k)
        first[nnz] = len(pairs)
        return np.asarray(pairs, np.int64).reshape(-1, 2), first
    rows = rows_of(rowptr)
    k = np.nonzero(take)[0]
    m = np.bincount(rows[k], minlength=rowptr.size - 1)
    start = np.concatenate([[0], np.cumsum(m)])                      # the participants of row i: k[start[i] : start[i + 1]]
    mk = m[rows[k]]                                                   # per participant: its row's count
    a = np.repeat(np.arange(k.size), mk)                              # every participant against all of its row, itself included
    run = np.concatenate([[0], np.cumsum(mk)])
    b = np.arange(a.size) - run[a] + start[rows[k]][a]
    keep = a != b
    pairs = np.stack([k[a[keep]], k[b[keep]]], axis=1)
    per_entry = np.zeros(nnz, np.int64)
    per_entry[k] = mk - 1
    return pairs.reshape(-1, 2), np.concatenate([[0], np.cumsum(per_entry)])


def triplet_arrays(pairs, nnz):
    """the triplet handle's six arrays: what athena_mp_graph_create_bipartite_dev(nnz, nnz, T, pairs) builds"""
    return ir.arrays_of(pairs[:, 0], pairs[:, 1], nnz, nnz)


def triplet_csr(pairs, rowptr):
    """(adj_ia [nnz + 1], adj_ja [2, T]) 1-based: column = the second entry, edge id = the triplet"""
    ja = np.zeros((2, pairs.shape[0]), np.int32, order="F")
    ja[0], ja[1] = pairs[:, 1] + 1, np.arange(1, pairs.shape[0] + 1)
    return (np.asarray(rowptr) + 1).astype(np.int32), ja


# ---- the angle and its reverse -----------------------------------------------------------------------------------------------------
def _dot(u, v):
    s = u[..., 0] * v[..., 0]
    for d in range(1, u.shape[-1]):
        s = s + u[..., d] * v[..., d]
    return s


def cos(pairs, dir, dtype=np.float32, form="vector"):
    """cos [T]: dot / (sqrt(sa) sqrt(sb)), +0 where the denominator is 0"""
    dir = np.asarray(dir, dtype)
    zero = dtype(0)
    if form == "loop":
        out = np.zeros(pairs.shape[0], dtype)
        for t, (k, k2) in enumerate(pairs):
            a, b = dir[k], dir[k2]
            den = np.sqrt(_dot(a, a)) * np.sqrt(_dot(b, b))
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                out[t] = zero if den == 0 else _dot(a, b) / den
        return out
    a, b = dir[pairs[:, 0]], dir[pairs[:, 1]]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        den = np.sqrt(_dot(a, a)) * np.sqrt(_dot(b, b))
        return np.where(den == 0, zero, _dot(a, b) / np.where(den == 0, dtype(1), den)).astype(dtype)


def _term(u, v, cs, dc, dtype):
    """dc (v_c / den - (cs u_c) / su) per component; +0 gradient where den == 0 (then the product with dc)"""
    su, sv = _dot(u, u), _dot(v, v)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        den = np.sqrt(su) * np.sqrt(sv)
        flat = np.asarray(den == 0)
        safe_den, safe_su = np.where(flat, dtype(1), den), np.where(flat, dtype(1), su)
        g = v / safe_den[..., None] - (cs[..., None] * u) / safe_su[..., None]
        g = np.where(flat[..., None], dtype(0), g)
        return (dc[..., None] * g).astype(dtype)


def cos_bwd(T, dir, cosv, dcos, dtype=np.float32, form="vector"):
    """ddir [nnz, dim]: acc = +0; over row k of the triplet handle T acc = acc + dcos[t] ga; then over its column k acc = acc + dcos[t] gb"""
    dir, cosv, dcos = np.asarray(dir, dtype), np.asarray(cosv, dtype), np.asarray(dcos, dtype)
    out = np.zeros_like(dir)
    if form == "loop":
        dim = dir.shape[1]

        def add(k, other, t):                                         # one triplet's term of dir[k], component by component
            u, v = dir[k], dir[other]
            su, sv = _dot(u, u), _dot(v, v)
            den = np.sqrt(su) * np.sqrt(sv)
            for d in range(dim):
                g = dtype(0) if den == 0 else v[d] / den - (cosv[t] * u[d]) / su
                out[k, d] = out[k, d] + dcos[t] * g

        with np.errstate(over="ignore", invalid="ignore"):
            for k in range(dir.shape[0]):
                for p in range(T["rowptr"][k], T["rowptr"][k + 1]):
                    add(k, T["col"][p], T["eid"][p])
                for p in range(T["t_rowptr"][k], T["t_rowptr"][k + 1]):
                    add(k, T["t_src"][p], T["t_eid"][p])
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        for other, ids, ptr in ((T["col"], T["eid"], T["rowptr"]), (T["t_src"], T["t_eid"], T["t_rowptr"])):
            other, ids = np.asarray(other, np.int64), np.asarray(ids, np.int64)
            for k, p in _positions(ptr):
                t = ids[p]
                out[k] = out[k] + _term(dir[k], dir[other[p]], cosv[t], dcos[t], dtype)
    return out


def everything(A, E, vec, dim, cutoff3, dcos_of, dtype=np.float32, form="vector"):
    """the whole chain on one graph: dict of take, pairs, rowptr, T (the triplet handle's arrays), dir, cos, dcos, ddir, dvec; dcos_of(T)
    draws the upstream gradient.  Without vec: the integer results only."""
    take = participants(A, vec, dim, cutoff3, dtype)
    pairs, rowptr = triplets(A, take, form)
    nnz = int(A["rowptr"][-1])
    out = {"take": take, "pairs": pairs, "rowptr": rowptr, "T": triplet_arrays(pairs, nnz)}
    if vec is None:
        return out
    out["dir"] = entry_vectors(A, vec, dim, dtype, form)
    out["cos"] = cos(pairs, out["dir"], dtype, form)
    out["dcos"] = np.asarray(dcos_of(pairs.shape[0]), dtype)
    out["ddir"] = cos_bwd(out["T"], out["dir"], out["cos"], out["dcos"], dtype, form)
    out["dvec"] = entry_vectors_bwd(A, out["ddir"], E, dtype, form)
    return out
