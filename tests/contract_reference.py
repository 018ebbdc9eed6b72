"""The yardstick of athena_mp_contract_pairs, athena_mp_graph_pairs and athena_mp_cell_pairs (include/athena_mp.h): the definition
in numpy, twice over with nothing shared -- `contract` (a stable argsort of a key and head flags) and `brute_force` (a dictionary
filled in edge order with plain loops) -- the transcriptions of the two small entries, and the inputs the CPU and GPU tests share.

A pair list is an int32 array [E, 2]: the memory of the library's column-major [2, E], 1-based, row e = fine edge e."""
import functools

import numpy as np

KEYS = ("coarse_pairs", "rowptr", "members", "weights", "edge_pair", "coords")
LOCAL = {1: ((0, 1),), 2: ((0, 1), (0, 2), (1, 2)), 3: ((0, 1), (1, 2), (2, 3), (3, 0)),
         4: ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))}
NV = {1: 2, 2: 3, 3: 4, 4: 4}


class Refused(ValueError):
    pass


def _rng(seed):
    return np.random.default_rng(seed)


def bits_for(v):
    b = 1
    while b < 64 and (int(v) >> b):
        b += 1
    return b


def check(pairs, n_rows, n_cols, row_cluster, col_cluster, m_rows, m_cols, mode, row_points=None, col_points=None):
    """the refusals of the library, in its order; the word that names each is in the message"""
    E = pairs.shape[0]
    if mode not in (0, 1):
        raise Refused("mode")
    if E >= 2 ** 31 or min(n_rows, n_cols, m_rows, m_cols) < 0:
        raise Refused("size")
    if mode == 0 and (n_rows != n_cols or m_rows != m_cols):
        raise Refused("one set")
    if (row_cluster is None and m_rows != n_rows) or (col_cluster is None and m_cols != n_cols):
        raise Refused("identity")
    if (row_points is None) != (col_points is None):
        raise Refused("only one")
    if row_points is not None and not 1 <= row_points.shape[1] <= 3:
        raise Refused("dim")
    if bits_for(m_rows) + bits_for(m_cols) > 62:
        raise Refused("bits")
    if E == 0:
        return
    bad = np.nonzero((pairs[:, 0] < 0) | (pairs[:, 0] > n_rows) | (pairs[:, 1] < 0) | (pairs[:, 1] > n_cols))[0]
    if bad.size:
        raise Refused(f"pairs(:,{bad[0] + 1})")
    for name, c, m in (("row_cluster", row_cluster, m_rows), ("col_cluster", col_cluster, m_cols)):
        if c is not None:
            bad = np.nonzero((c < 0) | (c > m))[0]
            if bad.size:
                raise Refused(f"{name}({bad[0] + 1})")


def _result(E, P, M, cp, rowptr, members, weights, edge_pair, coords, m_rows, m_cols):
    count = np.diff(rowptr)
    return dict(P=P, M=M, coarse_pairs=cp.astype(np.int32).reshape(P, 2), rowptr=rowptr.astype(np.int32),
                members=members.astype(np.int32).reshape(M, 2), weights=weights.astype(np.float32), edge_pair=edge_pair.astype(np.int32),
                coords=coords, bits=(bits_for(m_rows) + bits_for(m_cols) + 1) if E else 0, largest=int(count.max()) if P else 0)


def contract(pairs, n_rows, n_cols, row_cluster, col_cluster, m_rows, m_cols, mode, row_points=None, col_points=None):
    """the sorted form: relabel, key, stable argsort of the edges that take part, head flags"""
    check(pairs, n_rows, n_cols, row_cluster, col_cluster, m_rows, m_cols, mode, row_points, col_points)
    E = pairs.shape[0]
    u, v = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    rc = np.arange(1, n_rows + 1) if row_cluster is None else np.asarray(row_cluster, np.int64)
    cc = np.arange(1, n_cols + 1) if col_cluster is None else np.asarray(col_cluster, np.int64)
    a = np.where(u >= 1, np.concatenate([[0], rc])[u], 0)
    b = np.where(v >= 1, np.concatenate([[0], cc])[v], 0)
    part = (a >= 1) & (b >= 1)
    if mode == 0:
        part &= a != b
        a, b = np.minimum(a, b), np.maximum(a, b)
    key = a * (m_cols + 1) + b
    idx = np.nonzero(part)[0]
    order = idx[np.argsort(key[idx], kind="stable")]
    M = order.size
    ks = key[order]
    head = np.ones(M, bool)
    head[1:] = ks[1:] != ks[:-1]
    pid = np.cumsum(head)
    P = int(pid[-1]) if M else 0
    rowptr = np.concatenate([np.nonzero(head)[0], [M]])
    cp = np.stack([a[order][head], b[order][head]], axis=1)
    members = np.stack([pid, order + 1], axis=1)
    weights = (np.float32(1) / np.diff(rowptr).astype(np.float32))[pid - 1] if M else np.zeros(0, np.float32)
    edge_pair = np.zeros(E, np.int64)
    edge_pair[order] = pid
    coords = None
    if row_points is not None:
        coords = (row_points[cp[:, 0] - 1].astype(np.float32) - col_points[cp[:, 1] - 1].astype(np.float32)).astype(np.float32)
    return _result(E, P, M, cp, rowptr, members, weights, edge_pair, coords, m_rows, m_cols)


def brute_force(pairs, n_rows, n_cols, row_cluster, col_cluster, m_rows, m_cols, mode, row_points=None, col_points=None):
    """the dictionary form: one loop over the edges in order, one over the sorted keys"""
    check(pairs, n_rows, n_cols, row_cluster, col_cluster, m_rows, m_cols, mode, row_points, col_points)
    E = pairs.shape[0]
    groups = {}
    for e in range(E):
        u, v = int(pairs[e, 0]), int(pairs[e, 1])
        if u < 1 or v < 1:
            continue
        a = u if row_cluster is None else int(row_cluster[u - 1])
        b = v if col_cluster is None else int(col_cluster[v - 1])
        if a < 1 or b < 1 or (mode == 0 and a == b):
            continue
        if mode == 0 and a > b:
            a, b = b, a
        groups.setdefault((a, b), []).append(e + 1)
    cp, rowptr, members, weights = [], [0], [], []
    edge_pair = np.zeros(E, np.int64)
    for c, k in enumerate(sorted(groups), 1):
        cp.append(k)
        for e in groups[k]:
            members.append((c, e))
            weights.append(np.float32(1) / np.float32(len(groups[k])))
            edge_pair[e - 1] = c
        rowptr.append(len(members))
    P, M = len(cp), len(members)
    coords = None
    if row_points is not None:
        coords = np.zeros((P, row_points.shape[1]), np.float32)
        for c, (a, b) in enumerate(cp):
            for k in range(row_points.shape[1]):
                coords[c, k] = np.float32(row_points[a - 1, k]) - np.float32(col_points[b - 1, k])
    return _result(E, P, M, np.array(cp, np.int64), np.array(rowptr), np.array(members, np.int64), np.array(weights, np.float32), edge_pair,
                   coords, m_rows, m_cols)


def same(got, want, keys=KEYS):
    """the names of the arrays that differ, word for word"""
    bad = []
    for k in keys:
        if want.get(k) is None:
            continue
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a.view(np.int32), b.view(np.int32)):
            bad.append(k)
    return bad


def graph_pairs(e_rowptr, e_row, e_entry, col):
    """athena_mp_graph_pairs from the handle's exported arrays: (row + 1, col + 1) of the first entry of each edge column"""
    E = e_rowptr.size - 1
    out = np.zeros((E, 2), np.int32)
    for e in range(E):
        if e_rowptr[e] < e_rowptr[e + 1]:
            at = e_rowptr[e]
            out[e] = (e_row[at] + 1, col[e_entry[at]] + 1)
    return out


def cell_pairs(cells, cell_type):
    """athena_mp_cell_pairs: slot c * ne + l = local pair l of cell c, as given"""
    loc = LOCAL[cell_type]
    out = np.zeros((cells.shape[0] * len(loc), 2), np.int32)
    for c in range(cells.shape[0]):
        for l, (i, j) in enumerate(loc):
            out[c * len(loc) + l] = (cells[c, i], cells[c, j])
    return out


# ---- structured meshes whose edge counts are known in closed form -------------------------------------------------------------
def grid_mesh(cell_type, nx, ny, nz=1):
    """(cells, n_vertices, n_edges, n_boundary_edges or None, points): cell_type 1 = the grid lines of an nx x ny lattice as segments
    (every edge once), 2 = every square cut along one diagonal, 3 = the squares, 4 = every cube of an nx x ny x nz lattice cut into
    its six Kuhn tetrahedra (one diagonal per face, one per body)"""
    if cell_type == 4:
        vid = lambda i, j, k: (k * (ny + 1) + j) * (nx + 1) + i + 1
        cells = []
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
                        at = [i, j, k]
                        tet = [vid(*at)]
                        for ax in perm:
                            at[ax] += 1
                            tet.append(vid(*at))
                        cells.append(tet)
        nvert = (nx + 1) * (ny + 1) * (nz + 1)
        edges = (nx * (ny + 1) * (nz + 1) + ny * (nx + 1) * (nz + 1) + nz * (nx + 1) * (ny + 1)
                 + nx * ny * (nz + 1) + nx * nz * (ny + 1) + ny * nz * (nx + 1) + nx * ny * nz)
        g = np.stack(np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), np.arange(nz + 1), indexing="ij"), -1).astype(np.float32)
        pts = np.ascontiguousarray(g.transpose(2, 1, 0, 3).reshape(-1, 3))
        return np.array(cells, np.int32), nvert, edges, None, pts
    vid = lambda i, j: j * (nx + 1) + i + 1
    cells = []
    for j in range(ny + 1):
        for i in range(nx + 1):
            if cell_type == 1:
                if i < nx:
                    cells.append([vid(i, j), vid(i + 1, j)])
                if j < ny:
                    cells.append([vid(i, j + 1), vid(i, j)])                  # given high-to-low: the contraction orders it
            elif i < nx and j < ny:
                q = [vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)]
                if cell_type == 3:
                    cells.append(q)
                else:
                    cells += [[q[0], q[1], q[2]], [q[2], q[3], q[0]]]
    lines = nx * (ny + 1) + ny * (nx + 1)
    edges = lines + (nx * ny if cell_type == 2 else 0)
    boundary = lines if cell_type == 1 else 2 * (nx + ny)
    g = np.stack(np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij"), -1).astype(np.float32)
    pts = np.ascontiguousarray(g.transpose(1, 0, 2).reshape(-1, 2))
    return np.array(cells, np.int32), (nx + 1) * (ny + 1), edges, boundary, pts


# ---- the shared inputs --------------------------------------------------------------------------------------------------------
def _random_case(seed, E, n_rows, n_cols, m_rows, m_cols, mode, dim, dropped=0.1, zeros=5, selfs=20, dups=40):
    r = _rng(seed)
    pairs = np.stack([r.integers(1, n_rows + 1, E), r.integers(1, n_cols + 1, E)], axis=1).astype(np.int32)
    if dups:
        pairs[r.choice(E, dups, replace=False)] = pairs[r.choice(E, dups, replace=False)]
    if selfs and mode == 0:
        at = r.choice(E, selfs, replace=False)
        pairs[at, 1] = pairs[at, 0]
    if zeros:
        pairs[r.choice(E, zeros, replace=False)] = 0
        pairs[r.choice(E, 2, replace=False), 1] = 0                         # one end only
    rc = r.integers(1, m_rows + 1, n_rows).astype(np.int32)
    rc[r.random(n_rows) < dropped] = 0
    cc = rc
    if mode == 1:
        cc = r.integers(1, m_cols + 1, n_cols).astype(np.int32)
        cc[r.random(n_cols) < dropped] = 0
    rp = cp = None
    if dim:
        rp = r.standard_normal((m_rows, dim)).astype(np.float32)
        cp = rp if mode == 0 else r.standard_normal((m_cols, dim)).astype(np.float32)
    return dict(pairs=pairs, n_rows=n_rows, n_cols=n_cols, row_cluster=rc, col_cluster=cc, m_rows=m_rows, m_cols=m_cols, mode=mode,
                row_points=rp, col_points=cp)


@functools.lru_cache(None)
def shape_cases():
    """(name, arguments of contract) of every shape class"""
    E3 = 2 * 4096 + 77
    cases = [("three tiles, 300 clusters, mode 0", _random_case(1, E3, 5000, 5000, 300, 300, 0, 3)),
             ("three tiles, 300 x 200 clusters, mode 1", _random_case(2, E3, 5000, 3000, 300, 200, 1, 2)),
             ("7 clusters, one pass", _random_case(3, 1000, 400, 400, 7, 7, 0, 1)),
             ("7 x 5 clusters, one pass, mode 1", _random_case(4, 1000, 400, 90, 7, 5, 1, 1))]
    for mode in (0, 1):
        for dim in (1, 2, 3):
            cases.append((f"mode {mode}, dim {dim}", _random_case(10 + 3 * mode + dim, 777, 333, 333 if mode == 0 else 211, 40,
                                                                  40 if mode == 0 else 23, mode, dim)))
    # the identity over 2^17 + 3 vertices: 18 + 18 + 1 key bits, the high word of the key is sorted
    n = 2 ** 17 + 3
    r = _rng(20)
    E = 4096 + 300
    pairs = np.stack([r.integers(1, n + 1, E), r.integers(1, n + 1, E)], axis=1).astype(np.int32)
    pairs[:64] = [n, n - 1]                                                   # duplicates at the top of the index space, given high-low
    pairs[64:200] = pairs[300:436]
    pairs[200] = [7, 7]
    cases.append(("identity over 2^17 + 3 vertices", dict(pairs=pairs, n_rows=n, n_cols=n, row_cluster=None, col_cluster=None, m_rows=n, m_cols=n,
                                                          mode=0, row_points=None, col_points=None)))
    # a hub: 5000 fine edges in one coarse pair, behind a few small ones and in front of others
    n, m = 6000, 20
    rc = np.zeros(n, np.int32)
    rc[:3000], rc[3000:] = 3, 9
    rc[:40] = np.arange(40) % 2 + 1                                           # coarse pair (1, 2) and pairs with 3 and 9 in front
    rc[5990:] = np.arange(10) + 11                                            # and pairs behind
    r = _rng(21)
    hub = np.stack([np.arange(41, 3001), np.arange(3001, 5961)], axis=1)      # vertices of cluster 3 with vertices of cluster 9
    hub = np.concatenate([hub, hub[:2100, ::-1]])                             # 5060 edges, some given as (9, 3)
    rest = np.stack([r.integers(1, n + 1, 400), r.integers(1, n + 1, 400)], axis=1)
    pairs = np.concatenate([hub, rest]).astype(np.int32)
    pairs = pairs[r.permutation(pairs.shape[0])]
    pts = r.standard_normal((m, 3)).astype(np.float32)
    cases.append(("hub of thousands", dict(pairs=pairs, n_rows=n, n_cols=n, row_cluster=rc, col_cluster=rc, m_rows=m, m_cols=m, mode=0,
                                           row_points=pts, col_points=pts)))
    base = _random_case(30, 500, 100, 100, 9, 9, 0, 2)
    cases.append(("E = 0", dict(base, pairs=np.zeros((0, 2), np.int32))))
    cases.append(("every edge dropped", dict(base, row_cluster=np.zeros(100, np.int32), col_cluster=np.zeros(100, np.int32))))
    one = np.where(np.arange(100) < 50, 4, 8).astype(np.int32)
    cases.append(("P = 1", dict(base, row_cluster=one, col_cluster=one)))
    return tuple(cases)


def case(name):
    names = [c[0] for c in shape_cases()]
    return shape_cases()[names.index(name)][1]


def args_of(kw):
    """the arguments in the order of contract / brute_force"""
    return (kw["pairs"], kw["n_rows"], kw["n_cols"], kw["row_cluster"], kw["col_cluster"], kw["m_rows"], kw["m_cols"], kw["mode"],
            kw["row_points"], kw["col_points"])
