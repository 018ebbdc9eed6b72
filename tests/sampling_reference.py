"""The yardstick of neighbour sampling (athena_amd/csrc/neighbor_sample.hip): the definition of include/athena_mp.h in Python ints
and numpy, in two forms -- sample_hop, a loop over the rows with a dictionary for the relabelling, and sample_hop_vectorised,
whole-array numpy (what scripts/bench_neighbor_sampling.py times as the host route).  Everything here is 0-based except adj_ia /
adj_ja, which are what athena_mp_graph_create takes.  Integer only: the library's arrays are compared with np.array_equal."""
import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
HOP = 0xD1B54A32D192ED03
M1, M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def hop_seed(seed, h):
    """the seed of hop h (0-based)"""
    return (int(seed) + HOP * (h + 1)) & MASK


def key(seed, r, p):
    """the key of the entry at position p of the row of vertex r, Python ints"""
    z = (int(seed) + GOLDEN * (((int(r) << 32) | int(p)) + 1)) & MASK
    z ^= z >> 30
    z = (z * M1) & MASK
    z ^= z >> 27
    z = (z * M2) & MASK
    z ^= z >> 31
    return (z & 0xFFFFFFFF00000000) | int(p)


def keys_vectorised(seed, r, p):
    """the same for arrays r, p (any integer type; seed one int or an array of them): uint64 arithmetic wraps mod 2^64"""
    u = np.uint64
    s = u(int(seed) & MASK) if np.ndim(seed) == 0 else np.asarray(seed).astype(u)
    with np.errstate(over="ignore"):
        z = s + u(GOLDEN) * (((r.astype(u) << u(32)) | p.astype(u)) + u(1))
        z ^= z >> u(30)
        z *= u(M1)
        z ^= z >> u(27)
        z *= u(M2)
        z ^= z >> u(31)
    return (z & u(0xFFFFFFFF00000000)) | p.astype(u)


def choose(seed, r, L, k):
    """the chosen positions of a row of L entries, ascending"""
    if k == 0 or L <= k:
        return list(range(L))
    return sorted(sorted(range(L), key=lambda p: key(seed, r, p))[:k])


def parent_csr(adj_ia, adj_ja):
    """adj_ia [n + 1], adj_ja [2, nnz] (1-based) -> rowptr, col, eid (0-based; eid = -1: no edge column)"""
    ja = np.asarray(adj_ja)
    return np.asarray(adj_ia, np.int64) - 1, ja[0].astype(np.int64) - 1, ja[1].astype(np.int64) - 1


def _finish(rowptr, seeds, k, brow, entry, col, eid, local, vertex_map, degrees, deg_row, deg_col):
    m, nnz, n_cols = len(seeds), len(entry), len(vertex_map)
    has_edges = eid is not None
    adj_ja = np.zeros((2, nnz), np.int32, order="F")
    adj_ja[0] = np.asarray(local, np.int64) + 1
    if has_edges:
        adj_ja[1] = np.arange(1, nnz + 1)
    vm = np.asarray(vertex_map, np.int64)
    if degrees == "block":
        rd, cd = np.diff(brow), np.bincount(np.asarray(local, np.int64), minlength=n_cols)
    else:
        own = np.diff(rowptr)
        rd = (own if deg_row is None else np.asarray(deg_row))[vm[:m]]
        cd = (own if deg_col is None else np.asarray(deg_col))[vm]
    return dict(m=m, n_cols=n_cols, nnz=nnz, rowptr=np.asarray(brow, np.int32), vertex_map=vm.astype(np.int32),
                entry_map=np.asarray(entry, np.int64).astype(np.int32),
                edge_map=eid[np.asarray(entry, np.int64)].astype(np.int32) if has_edges else None, local=np.asarray(local, np.int64).astype(np.int32),
                adj_ia=(np.asarray(brow, np.int64) + 1).astype(np.int32), adj_ja=adj_ja, n_edge_cols=nnz if has_edges else 0,
                row_deg=np.asarray(rd, np.int64).astype(np.int32), col_deg=np.asarray(cd, np.int64).astype(np.int32))


def sample_hop(rowptr, col, eid, seeds, k, seed, degrees="block", deg_row=None, deg_col=None):
    """One hop, row by row.  rowptr / col / eid: the parent's forward CSR (eid None: no edge columns); seeds: distinct vertices."""
    assert 0 <= k <= 64 and degrees in ("block", "parent")
    seeds = [int(s) for s in seeds]
    n = len(rowptr) - 1
    assert all(0 <= s < n for s in seeds) and len(set(seeds)) == len(seeds)
    brow, entry = [0], []
    for r in seeds:
        b, L = int(rowptr[r]), int(rowptr[r + 1] - rowptr[r])
        entry += [b + p for p in choose(seed, r, L, k)]
        brow.append(len(entry))
    slot = {r: s for s, r in enumerate(seeds)}
    vertex_map = list(seeds)
    for u in sorted({int(col[w]) for w in entry} - set(seeds)):
        slot[u] = len(vertex_map)
        vertex_map.append(u)
    local = [slot[int(col[w])] for w in entry]
    return _finish(np.asarray(rowptr, np.int64), seeds, k, brow, entry, col, eid, local, vertex_map, degrees, deg_row, deg_col)


def select_vectorised(rowptr, seeds, k, seed):
    """(brow [m + 1], entry [nnz]): the chosen parent CSR positions of every seed row, whole-array numpy"""
    rowptr = np.asarray(rowptr, np.int64)
    seeds = np.asarray(seeds, np.int64).reshape(-1)
    m = seeds.size
    L = rowptr[seeds + 1] - rowptr[seeds]
    cnt = L if k == 0 else np.minimum(L, k)
    brow = np.concatenate([[0], np.cumsum(cnt)])
    start = np.concatenate([[0], np.cumsum(L)])
    idx = np.repeat(np.arange(m), L)                                   # the seed slot of every candidate entry
    p = np.arange(start[-1]) - start[idx]
    drawn = (L > cnt)[idx]
    keyv = p.astype(np.uint64)                                         # a whole row keeps every position
    if drawn.any():
        keyv[drawn] = keys_vectorised(seed, seeds[idx[drawn]], p[drawn])
    order = np.lexsort((keyv, idx))
    keep = order[(np.arange(order.size) - start[idx[order]]) < cnt[idx[order]]]
    keep.sort()                                                        # candidates are numbered by (slot, p): ascending p inside a row
    return brow, rowptr[seeds[idx[keep]]] + p[keep]


def sample_hop_vectorised(rowptr, col, eid, seeds, k, seed, degrees="block", deg_row=None, deg_col=None):
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    seeds = np.asarray(seeds, np.int64).reshape(-1)
    n, m = rowptr.size - 1, seeds.size
    brow, entry = select_vectorised(rowptr, seeds, k, seed)
    g = col[entry]
    slot = np.full(n, -1, np.int64)
    slot[seeds] = np.arange(m)
    new = np.unique(g[slot[g] < 0])
    slot[new] = m + np.arange(new.size)
    return _finish(rowptr, seeds, k, brow, entry, col, eid, slot[g], np.concatenate([seeds, new]), degrees, deg_row, deg_col)


def sample(rowptr, col, eid, seeds, fanouts, seed, degrees="block", deg_row=None, deg_col=None, hop=sample_hop):
    """Several hops: hop h draws fanouts[h] with hop_seed(seed, h) around hop h - 1's whole vertex_map; outermost block first."""
    blocks = []
    for h, k in enumerate(fanouts):
        b = hop(rowptr, col, eid, seeds, k, hop_seed(seed, h), degrees, deg_row, deg_col)
        blocks.append(b)
        seeds = b["vertex_map"]
    return blocks[::-1]


# ---- the parent graph of the GPU tests: every row length at which the draw kernel takes another path ------------------------------
FANOUTS = (1, 2, 5, 63, 64, 0)
HUB = 5000
ROW_LENGTHS = (0, 1, 2, 3, 4, 5, 6, 62, 63, 64, 65, 128, 129, HUB, 0, 1, 7, 64, 65, 130, 200, 3, 5, 66)


def shape_graph(with_edges, seed=11):
    """(adj_ia, adj_ja, n_edge_cols): rows of the lengths above (k - 1, k, k + 1 of every fan-out, the step boundaries 63 .. 65 and
    128 .. 129, a hub of 5 000), then rows of 0 .. 9 entries up to n = 160.  Every row of two entries or more starts with a self
    loop and repeats its second entry (a multigraph); columns are drawn over all vertices, so seeds are each other's neighbours.
    with_edges: every entry carries an edge column except the self loops (edge id 0)."""
    rng = np.random.default_rng(seed)
    lengths = list(ROW_LENGTHS) + [int(v) for v in rng.integers(0, 10, 160 - len(ROW_LENGTHS))]
    n = len(lengths)
    cols, ids = [], []
    n_edge_cols = sum(lengths) // 2 + 7 if with_edges else 0
    for r, L in enumerate(lengths):
        c = rng.integers(0, n, L)
        e = rng.integers(1, n_edge_cols + 1, L) if with_edges else np.zeros(L, np.int64)
        if L >= 2:
            c[0], e[0] = r, 0
        if L >= 3:
            c[2] = c[1]
        cols.append(c)
        ids.append(e)
    adj_ia = (np.concatenate([[0], np.cumsum(lengths)]) + 1).astype(np.int32)
    adj_ja = np.asfortranarray(np.stack([np.concatenate(cols) + 1, np.concatenate(ids)]).astype(np.int32))
    return adj_ia, adj_ja, n_edge_cols


def seed_sets(n, seed=12):
    """name -> seeds (0-based) of the GPU tests"""
    rng = np.random.default_rng(seed)
    hub = ROW_LENGTHS.index(HUB)
    return {"m = 0": np.zeros(0, np.int32), "m = 1, the hub": np.array([hub], np.int32), "m = 5": np.array([3, hub, 0, 12, 7], np.int32),
            "descending": np.arange(n - 1, -1, -3, dtype=np.int32), "shuffled": rng.permutation(n)[:70].astype(np.int32),
            "all vertices": np.arange(n, dtype=np.int32), "the length rows": np.arange(len(ROW_LENGTHS), dtype=np.int32)}
