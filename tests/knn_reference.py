"""The yardstick of the k-nearest-neighbour builder (athena_mp_knn_pairs_batched, athena_amd/csrc/knn_graph.hip): the definition
of include/athena_mp.h in numpy float32, in two forms, and a Python transcription of the kernel's grid search.

  brute force   the definition as it is written: the all-pairs s per cloud, np.lexsort on (j, s), the cap, union / mutual,
                lexicographic pairs.  Small n only.
  large form    the same keys over the candidates of a float64 cKDTree.  For point i take the fp32 s of its k float64-nearest
                neighbours and let S be the largest: the k-th smallest fp32 s is at most S, so every true key has s <= S, and
                every such j has exact distance at most sqrt(S) * (1 + 2^-20) (the fp32 sum of at most three squares is within a
                few 2^-24 relative of the exact one).  Query that ball, evaluate the fp32 keys, take the first k.
  grid search   knn_graph.hip's search, shell by shell, with the file header's stop rule and margin in float32 -- it returns what
                it examined as well, so a test can see the pruning.

test_knn_graph.py pins the second and third to the first."""
import numpy as np

K_MARGIN = np.float32(2.0 ** -10)
K_SHRINK = np.float32(1.0 - 2.0 ** -20)
K_GRID_POINTS = 2.0
K_MAX_CELLS_AXIS = 2048


def sq_dist(a, b):
    """s of the definition: every multiply and add rounded to float32 on its own, left to right (a, b float32 [..., dim])"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = a - b
        s = d[..., 0] * d[..., 0]
        for c in range(1, d.shape[-1]):
            s = s + d[..., c] * d[..., c]
    return s


def r2_of(radius):
    """fl(radius * radius), +inf for no cap"""
    if radius is None or np.isinf(radius):
        return np.float32(np.inf)
    with np.errstate(over="ignore"):
        return np.float32(radius) * np.float32(radius)


def _first_k(s, j, k, r2):
    """the first k of the candidates j with squared distances s in the order (s, j), after the cap"""
    keep = s <= r2
    s, j = s[keep], j[keep]
    o = np.lexsort((j, s))[:k]
    return j[o]


def graph_of(nbr, p, offsets, mode):
    """nbr [n, k] (1-based, 0 = padding) -> (i, j, coords, edge_offsets): pairs i < j, 0-based, in lexicographic order; union (0):
    j in N(i) or i in N(j); mutual (1): both"""
    n, k = nbr.shape
    a = np.repeat(np.arange(n, dtype=np.int64), k)
    b = nbr.reshape(-1).astype(np.int64) - 1
    a, b = a[b >= 0], b[b >= 0]
    key, count = np.unique(np.minimum(a, b) * n + np.maximum(a, b), return_counts=True)      # ascending: lexicographic in (i, j)
    assert count.size == 0 or count.max() <= 2
    if mode == 1:
        key = key[count == 2]
    i, j = key // max(n, 1), key % max(n, 1)
    eoff = np.searchsorted(i, np.asarray(offsets, np.int64), side="left").astype(np.int64)
    return i, j, p[i] - p[j], eoff


def brute_force_neighbours(p, offsets, k, radius=None):
    """nbr [n, k] int32: row i = N_k(i) as 1-based global ids in key order, padded with 0"""
    assert p.dtype == np.float32 and p.ndim == 2
    off = np.asarray(offsets, np.int64)
    r2 = r2_of(radius)
    nbr = np.zeros((p.shape[0], k), np.int32)
    for b in range(off.size - 1):
        q = p[off[b]:off[b + 1]]
        m = q.shape[0]
        s = sq_dist(q[:, None, :], q[None, :, :])
        idx = np.arange(m)
        for i in range(m):
            other = idx != i
            f = _first_k(s[i][other], idx[other], k, r2)
            nbr[off[b] + i, :f.size] = f + off[b] + 1
    return nbr


def large_form_neighbours(p, offsets, k, radius=None):
    from scipy.spatial import cKDTree

    assert p.dtype == np.float32 and p.ndim == 2
    off = np.asarray(offsets, np.int64)
    r2 = r2_of(radius)
    nbr = np.zeros((p.shape[0], k), np.int32)
    for b in range(off.size - 1):
        q = p[off[b]:off[b + 1]]
        m = q.shape[0]
        if m < 2:
            continue
        kk = min(k, m - 1)
        tree = cKDTree(q.astype(np.float64))
        _, near = tree.query(q.astype(np.float64), kk + 1)
        near = near.reshape(m, kk + 1)
        # k others per point: drop the point itself where it is listed, the last one otherwise (coincident points)
        me = near == np.arange(m)[:, None]
        me[~me.any(1), -1] = True
        others = np.take_along_axis(near, np.argsort(me, axis=1, kind="stable"), 1)[:, :kk]
        S = sq_dist(q[:, None, :], q[others]).max(1)
        assert np.all(np.isfinite(S)), "the large form is for clouds whose squared distances are finite in float32"
        ball = np.sqrt(S.astype(np.float64)) * (1.0 + 2.0 ** -20)
        cand = tree.query_ball_point(q.astype(np.float64), ball)
        for i in range(m):
            j = np.asarray(cand[i], np.int64)
            j = j[j != i]
            f = _first_k(sq_dist(q[i], q[j]), j, k, r2)
            nbr[off[b] + i, :f.size] = f + off[b] + 1
    return nbr


# ---- the grid search of knn_graph.hip ------------------------------------------------------------------------------------------
def _round_down32(v):
    f = np.float32(v)
    return np.nextafter(f, np.float32(0)) if float(f) > v else f


def make_knn_grid(q):
    """(lo, inv_w, nc, w_low) of one cloud q float32 [m, dim]: make_knn_grid of knn_graph.hip"""
    m, dim = q.shape
    lo = q.min(0)
    extent = q.max(0).astype(np.float64) - lo.astype(np.float64)
    extent[~((extent > 0) & (extent < 1e37))] = 0.0
    nc = np.ones(dim, np.int64)
    inv_w = np.zeros(dim, np.float32)
    w_low = np.zeros(dim, np.float32)
    act = extent > 0
    if act.any():
        w = (np.prod(extent[act]) / max(1.0, m / K_GRID_POINTS)) ** (1.0 / act.sum())
        for a in np.nonzero(act)[0]:
            c = np.floor(extent[a] / w)
            nc[a] = 1 if not c >= 1 else int(min(c, K_MAX_CELLS_AXIS))
        while np.prod(nc) > min(2 * m, 1 << 30):
            a = int(np.argmax(nc))                           # the first of the largest
            nc[a] = (nc[a] + 1) // 2
        for a in range(dim):
            if nc[a] <= 1:
                continue
            f = np.float32(nc[a] / extent[a])
            if not (f >= np.float32(1e-30) and f <= np.float32(1e30)):
                nc[a] = 1
                continue
            inv_w[a] = f
            w_low[a] = _round_down32((1.0 / float(f)) * (1.0 - 2.0 ** -30))
    return lo, inv_w, nc, w_low


def grid_search_neighbours(p, offsets, k, radius=None):
    """-> (nbr, stats): stats = [queries, candidates examined, cells visited, largest shell], as athena_mp_knn_stats"""
    assert p.dtype == np.float32 and p.ndim == 2
    off = np.asarray(offsets, np.int64)
    r2 = r2_of(radius)
    capped = np.isfinite(r2)
    dim = p.shape[1]
    nbr = np.zeros((p.shape[0], k), np.int32)
    stats = [p.shape[0], 0, 0, 0]
    f32 = np.float32
    for b in range(off.size - 1):
        q = p[off[b]:off[b + 1]]
        m = q.shape[0]
        if m == 0:
            continue
        lo, inv_w, nc, w_low = make_knn_grid(q)
        qq = (q - lo) * inv_w                                # two float32 roundings: cell_q
        assert qq.dtype == np.float32
        cell = np.minimum(qq.astype(np.int64), nc - 1)
        members = {}
        for i in range(m):
            members.setdefault(tuple(cell[i]), []).append(i)
        for i in range(m):
            c = cell[i]
            best_s, best_j = np.zeros(0, f32), np.zeros(0, np.int64)
            rho = 0
            while True:
                lo_c, hi_c = np.maximum(c - rho, 0), np.minimum(c + rho, nc - 1)
                grid = np.stack(np.meshgrid(*[np.arange(lo_c[a], hi_c[a] + 1) for a in range(dim)], indexing="ij"), -1).reshape(-1, dim)
                shell = grid[np.abs(grid - c).max(1) == rho]
                js = [j for cc in shell for j in members.get(tuple(cc), ())]
                stats[1] += len(js)
                stats[2] += shell.shape[0]
                j = np.asarray([x for x in js if x != i], np.int64)
                if j.size:
                    s = sq_dist(q[i], q[j])
                    keep = s <= r2
                    s, j = np.concatenate([best_s, s[keep]]), np.concatenate([best_j, j[keep]])
                    o = np.lexsort((j, s))[:k]
                    best_s, best_j = s[o], j[o]
                # the stop rule of the file header
                t = f32(np.inf)
                for a in range(dim):
                    if nc[a] <= 1:
                        continue
                    if c[a] + rho + 1 <= nc[a] - 1:
                        t = min(t, ((f32(c[a] + rho + 1) - qq[i, a]) - K_MARGIN) * w_low[a])
                    if c[a] - rho - 1 >= 0:
                        t = min(t, ((qq[i, a] - f32(c[a] - rho)) - K_MARGIN) * w_low[a])
                if np.isinf(t):
                    break
                with np.errstate(over="ignore", under="ignore"):
                    bound = min((t * t) * K_SHRINK, np.finfo(f32).max) if t > 0 else f32(0)
                assert isinstance(bound, f32)
                if bound < f32(2.0 ** -100):
                    bound = f32(0)
                if capped and bound > r2:
                    break
                if best_s.size == k and best_s[-1] < bound:
                    break
                rho += 1
            stats[3] = max(stats[3], rho)
            nbr[off[b] + i, :best_j.size] = best_j + off[b] + 1
    return nbr, stats


# ---- the inputs both test files use --------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def lattice(*shape):
    return np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, len(shape)).astype(np.float32)


def two_clusters():
    """20 and 30 points in unit boxes 1 000 box-widths apart: at k = 25 the smaller cluster must cross the gap"""
    rng = _rng(7)
    a, b = rng.random((20, 3)), rng.random((30, 3))
    b[:, 0] += 1000.0
    return np.concatenate([a, b]).astype(np.float32)


def on_cell_boundaries(dim, n=500, seed=11):
    """a uniform cloud in the unit box, corners included, with half of the coordinates moved onto the grid's cell boundaries c / nc
    and the float32 numbers beside them"""
    rng = _rng(seed + dim)
    p = rng.random((n, dim)).astype(np.float32)
    p[0], p[1] = 0.0, 1.0
    nc = make_knn_grid(p)[2]
    for a in range(dim):
        rows = rng.choice(np.arange(2, n), n // 2, replace=False)
        x = (rng.integers(0, nc[a] + 1, rows.size) / nc[a]).astype(np.float32)
        step = rng.integers(-1, 2, rows.size)
        x = np.where(step < 0, np.nextafter(x, np.float32(-1)), np.where(step > 0, np.nextafter(x, np.float32(2)), x))
        p[rows, a] = np.clip(x, 0.0, 1.0)
    assert np.array_equal(make_knn_grid(p)[2], nc)
    return p


def coincident():
    p = _rng(5).random((200, 3)).astype(np.float32)
    p[60:100] = p[60]
    return p


def shape_cases():
    """(name, points, offsets, k, radius) of every shape class, each small enough for brute_force"""
    rng = _rng(3)
    one = lambda q: offsets_of([q.shape[0]])
    cases = [("lattice 1-D 64", lattice(64), 4), ("lattice 12 x 12", lattice(12, 12), 4), ("lattice 6 x 6 x 6, k = 6", lattice(6, 6, 6), 6),
             ("lattice 6 x 6 x 6, k = 7", lattice(6, 6, 6), 7), ("40 coincident among 200", coincident(), 8),
             ("two clusters", two_clusters(), 25),
             ("planar in 3-D", np.concatenate([rng.random((400, 2)), np.full((400, 1), 0.25)], 1).astype(np.float32), 8),
             ("1000 : 1 : 1 box", (rng.random((400, 3)) * [1000.0, 1.0, 1.0]).astype(np.float32), 8),
             ("1e6 + lattice 12 x 12", lattice(12, 12) + np.float32(1e6), 5), ("1e6 + 1-D 200", lattice(200) + np.float32(1e6), 3),
             ("1e6 + uniform, spacing 1", (1e6 + rng.random((300, 3)) * 7.0).astype(np.float32), 8)]
    cases = [(name, q, one(q), k, None) for name, q, k in cases]
    for dim in (1, 2, 3):
        q = _rng(20 + dim).random((600, dim)).astype(np.float32)
        cases += [(f"uniform dim {dim}, k = {k}", q, one(q), k, None) for k in (1, 8, 33, 64)]
        cases.append((f"cell boundaries dim {dim}", on_cell_boundaries(dim), offsets_of([500]), 8, None))
        cases.append((f"capped dim {dim}", q, one(q), 8, degree_radius(600, 6.0, dim)))
    off = offsets_of([300, 0, 1, 450, 2, 120])
    cases.append(("batch", _rng(31).random((int(off[-1]), 3)).astype(np.float32), off, 8, None))
    cases.append(("k >= n", _rng(32).random((5, 2)).astype(np.float32), offsets_of([5]), 9, None))
    return cases


def cap_case():
    """3 000 uniform points, k = 8, a radius for a mean degree of about 6: some rows are cut by k, some by the radius"""
    p = _rng(41).random((3000, 3)).astype(np.float32)
    return p, offsets_of([3000]), 8, degree_radius(3000, 6.0, 3)


def degree_radius(n, mean_degree, dim):
    """radius for which a uniform cloud of n points in the unit box has about this mean degree"""
    vol = {1: 2.0, 2: np.pi, 3: 4.0 / 3.0 * np.pi}[dim]
    return float((mean_degree / (n * vol)) ** (1.0 / dim))
