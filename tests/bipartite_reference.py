"""The yardstick of the two-set radius builder (athena_amd/csrc/bipartite_graph.hip) and of its reverse step
(athena_mp_edge_grad_to_point_sets): the definitions of include/athena_mp.h in numpy.  Brute force over every (query, source) of a
cloud, the predicate term by term in float32 as radius_reference.fp32_keep evaluates it; sequential float32 sums for the
gradient.  test_radius_bipartite.py pins both to hand-written cases and to radius_reference.reference_pairs."""
import numpy as np


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def keep(q, s, r):
    """[nq, ns] bool: d = q_i - p_j per component in float32, s = ((d0 d0) + d1 d1) + d2 d2, every multiply and add rounded to
    float32 on its own, kept iff s <= fl(r * r)"""
    assert q.dtype == np.float32 and s.dtype == np.float32
    r2 = np.float32(r) * np.float32(r)
    with np.errstate(over="ignore", invalid="ignore"):
        d = q[:, None, :] - s[None, :, :]
        t = d[..., 0] * d[..., 0]
        for a in range(1, q.shape[1]):
            t = t + d[..., a] * d[..., a]
        return t <= r2


def reference_pairs(q, s, r, qoff=None, soff=None):
    """q [nq, dim], s [ns, dim] float32, offsets [B + 1] (None: one cloud) -> (i, j, coords, rowptr, edge_offsets): 0-based global
    pairs in lexicographic order of (i, j), coords = q[i] - s[j], rowptr [nq + 1] int32, edge_offsets [B + 1] int64"""
    nq, ns = q.shape[0], s.shape[0]
    qoff = offsets_of([nq]) if qoff is None else np.asarray(qoff)
    soff = offsets_of([ns]) if soff is None else np.asarray(soff)
    ii, jj = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for b in range(qoff.size - 1):
        q0, q1, s0, s1 = int(qoff[b]), int(qoff[b + 1]), int(soff[b]), int(soff[b + 1])
        if q1 == q0 or s1 == s0:
            continue
        i, j = np.nonzero(keep(q[q0:q1], s[s0:s1], r))          # row-major: lexicographic in (i, j)
        ii.append(i.astype(np.int64) + q0)
        jj.append(j.astype(np.int64) + s0)
    i, j = np.concatenate(ii), np.concatenate(jj)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=nq))]).astype(np.int32)
    with np.errstate(over="ignore"):
        coords = (q[i] - s[j]).reshape(i.size, q.shape[1])
    return i, j, coords, rowptr, rowptr[qoff].astype(np.int64)


def csr_of(i, j, nq):
    """the directed CSR of the pair list as athena_mp_graph_create takes it: adj_ia [nq + 1] 1-based, adj_ja [2, E] = (source,
    edge id) 1-based, column-major"""
    ia = np.concatenate([[1], 1 + np.cumsum(np.bincount(i, minlength=nq))]).astype(np.int32)
    ja = np.asfortranarray(np.stack([j + 1, np.arange(1, i.size + 1)]).astype(np.int32))
    return ia, ja


def reference_grad(i, j, dcoords, nq, ns):
    """(dqueries [nq, dim], dsources [ns, dim]): acc = +0, then in edge order acc = acc + dcoords[e] for the query of e and
    acc = acc - dcoords[e] for its source, one float32 operation at a time.  Edge order is (i, j) ascending, which is CSR order
    inside a row and query-ascending order inside a column."""
    assert dcoords.dtype == np.float32
    dq = np.zeros((nq, dcoords.shape[1]), np.float32)
    ds = np.zeros((ns, dcoords.shape[1]), np.float32)
    for e in range(i.size):
        dq[i[e]] = dq[i[e]] + dcoords[e]
        ds[j[e]] = ds[j[e]] - dcoords[e]
    return dq, ds
