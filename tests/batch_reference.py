"""The yardstick of athena_mp_batch_select (athena_amd/csrc/batch_select.hip): the definition of include/athena_mp.h in numpy, over
the thirteen arrays of a handle as DeviceGraph.export names them, plus the helpers the tests share -- the arrays of a handle from
its CSR (the host builder's stable counting sorts), the pair list behind a handle, and the renumbered pair list of a selection."""
import numpy as np

NAMES = ("rowptr", "col", "eid", "coef", "t_rowptr", "t_src", "t_eid", "t_coef", "e_rowptr", "e_row", "e_entry", "deg_row", "deg_col")


def select_reference(arrays, offsets, edge_offsets, sel):
    """arrays: dict of the thirteen parent arrays (0-based); offsets [B + 1]; edge_offsets [B + 1] or None (no edge columns);
    sel: structure ids.  Returns (child arrays, vertex_offsets int32 [m + 1], edge_offsets int64 [m + 1], vertex_map, edge_map)."""
    a = {k: np.asarray(v) for k, v in arrays.items()}
    off = np.asarray(offsets, np.int64)
    eoff = np.zeros_like(off) if edge_offsets is None else np.asarray(edge_offsets, np.int64)
    sel = np.asarray(sel, np.int64).reshape(-1)
    wst = a["rowptr"].astype(np.int64)[off]                                # first entry of every structure, forward and transposed
    assert np.array_equal(wst, a["t_rowptr"].astype(np.int64)[off])
    est = a["e_rowptr"].astype(np.int64)[eoff]                             # first entry of the edge-column index
    nv, nw, ne, nq = (np.diff(t)[sel] for t in (off, wst, eoff, est))
    cv, cw, ce, cq = (np.concatenate([[0], np.cumsum(c)]) for c in (nv, nw, ne, nq))
    parts = {k: [] for k in NAMES}
    vmap, emap = [], []
    for t, s in enumerate(sel):
        rows, ents = slice(off[s], off[s + 1]), slice(wst[s], wst[s + 1])
        ecols, eents = slice(eoff[s], eoff[s + 1]), slice(est[s], est[s + 1])
        dv, dw, de = cv[t] - off[s], cw[t] - wst[s], ce[t] - eoff[s]
        keep = lambda ids: np.where(ids < 0, -1, ids + de)
        parts["rowptr"].append(a["rowptr"][rows] + dw)
        parts["col"].append(a["col"][ents] + dv)
        parts["eid"].append(keep(a["eid"][ents]))
        parts["coef"].append(a["coef"][ents])
        parts["t_rowptr"].append(a["t_rowptr"][rows] + dw)
        parts["t_src"].append(a["t_src"][ents] + dv)
        parts["t_eid"].append(keep(a["t_eid"][ents]))
        parts["t_coef"].append(a["t_coef"][ents])
        parts["e_rowptr"].append(a["e_rowptr"][ecols] + (cq[t] - est[s]))
        parts["e_row"].append(a["e_row"][eents] + dv)
        parts["e_entry"].append(a["e_entry"][eents] + dw)
        parts["deg_row"].append(a["deg_row"][rows])
        parts["deg_col"].append(a["deg_col"][rows])
        vmap.append(np.arange(off[s], off[s + 1]))
        emap.append(np.arange(eoff[s], eoff[s + 1]))
    parts["rowptr"].append([cw[-1]])
    parts["t_rowptr"].append([cw[-1]])
    parts["e_rowptr"].append([cq[-1]])
    child = {k: np.concatenate([np.asarray(p, a[k].dtype) for p in parts[k]]).astype(a[k].dtype) for k in NAMES}
    cat = lambda p: np.concatenate(p + [np.zeros(0, np.int64)]).astype(np.int32)
    return child, cv.astype(np.int32), ce.astype(np.int64), cat(vmap), cat(emap)


def handle_arrays(adj_ia, adj_ja, n_edge_cols):
    """the thirteen arrays of the handle of a square CSR in athena's convention (1-based adj_ia / adj_ja), as graph_create's host
    builder makes them: stable counting sorts, so a transposed row lists its sources in ascending order.  coef here is numpy's fp32
    power, a function of the degree product alone: good for comparing slices with rebuilds, not for comparing with the device."""
    ia = np.asarray(adj_ia, np.int64)
    n = ia.size - 1
    rowptr = ia - 1
    col = np.asarray(adj_ja[0], np.int64) - 1
    eid = np.asarray(adj_ja[1], np.int64) - 1
    deg = np.diff(rowptr)
    row = np.repeat(np.arange(n), deg)
    coef_of = lambda r, c: (deg[r] * deg[c]).astype(np.float32) ** np.float32(-0.5)
    t_order = np.argsort(col, kind="stable")
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))])
    with_e = np.nonzero(eid >= 0)[0]
    e_order = with_e[np.argsort(eid[with_e], kind="stable")]
    e_rowptr = np.concatenate([[0], np.cumsum(np.bincount(eid[with_e], minlength=n_edge_cols))])
    i32 = lambda t: np.asarray(t).astype(np.int32)
    return {"rowptr": i32(rowptr), "col": i32(col), "eid": i32(eid), "coef": coef_of(row, col), "t_rowptr": i32(t_rowptr),
            "t_src": i32(row[t_order]), "t_eid": i32(eid[t_order]), "t_coef": coef_of(row[t_order], col[t_order]),
            "e_rowptr": i32(e_rowptr), "e_row": i32(row[e_order]), "e_entry": i32(e_order), "deg_row": i32(deg), "deg_col": i32(deg)}


def pairs_of_arrays(arrays, n_edge_cols):
    """the pair list [2, n_edge_cols] (1-based) behind a handle with edge ids: column e = (row, neighbour) of the first entry that
    carries edge column e (the smaller vertex first; a self pair has one entry).  Every edge column must be carried by an entry."""
    erp, e_row, e_entry, col = (np.asarray(arrays[k], np.int64) for k in ("e_rowptr", "e_row", "e_entry", "col"))
    assert erp.size == n_edge_cols + 1 and np.all(np.diff(erp) >= 1)
    first = erp[:-1]
    return np.asfortranarray(np.stack([e_row[first] + 1, col[e_entry[first]] + 1]).astype(np.int32))


def child_pairs(pairs, offsets, edge_offsets, sel):
    """the pair list of a selection: the selected structures' pairs in selection order, renumbered -> ([2, E'] int32 1-based, n_child)"""
    off, eoff = np.asarray(offsets, np.int64), np.asarray(edge_offsets, np.int64)
    out, base = [], 0
    for s in np.asarray(sel, np.int64).reshape(-1):
        out.append(np.asarray(pairs)[:, eoff[s]:eoff[s + 1]].astype(np.int64) - off[s] + base)
        base += off[s + 1] - off[s]
    out = np.concatenate(out + [np.zeros((2, 0), np.int64)], axis=1)
    return np.asfortranarray(out.astype(np.int32)), int(base)


def random_block_pairs(rng, sizes, pairs_per_vertex=2.0):
    """a random block-diagonal multigraph: structure s has sizes[s] vertices (0 allowed) and round(pairs_per_vertex * size) random
    pairs inside it, repeats and self pairs included (at least two self pairs on a one-vertex structure)
    -> (pairs [2, E] int32 1-based global, offsets int32 [B + 1], edge_offsets int64 [B + 1])"""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cols, eoff = [], [0]
    for s, m in enumerate(sizes):
        k = 0 if m == 0 else max(2, int(round(pairs_per_vertex * m)))
        p = rng.integers(0, max(m, 1), (2, k)) + off[s] + 1
        cols.append(np.sort(p, axis=0))
        eoff.append(eoff[-1] + k)
    pairs = np.concatenate(cols + [np.zeros((2, 0), np.int64)], axis=1)
    return np.asfortranarray(pairs.astype(np.int32)), off, np.asarray(eoff, np.int64)
