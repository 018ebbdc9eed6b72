"""The yardstick of the voxel-grid clusters (athena_mp_grid_clusters, include/athena_mp.h): the definition transcribed into numpy
float32, every operation rounded on its own.  Two forms that share only the cell function: `clusters` orders the points with one
stable lexsort and sums the members of all clusters round by round; `brute_force` is a dictionary keyed by (cloud, cell tuple)
filled in point order, plain Python loops, no sort of the points.  `grad` is the reverse step, `centroid64` its float64 twin.
Also the inputs the tests share."""
import functools

import numpy as np

F = np.float32
KEYS = ("cluster", "pairs", "rowptr", "weights", "centroid", "nearest", "cell", "cluster_offsets", "origin_out")
MAX_AXIS = 1 << 21


class Refused(Exception):
    pass


def bits_for(v):
    return max(1, int(v).bit_length())


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def grids(p, off, size, origin=None):
    """(inv, lo [B, dim] float32, nc [B] tuples of ints, bits, passes): the cell function's constants and the key layout"""
    p = np.ascontiguousarray(p, F)
    B, dim = off.size - 1, p.shape[1]
    size = F(size)
    if not (np.isfinite(size) and size > 0):
        raise Refused("size")
    with np.errstate(over="ignore", divide="ignore"):
        inv = F(1) / size
    if not np.isfinite(inv):
        raise Refused("inverse")
    lo = np.zeros((B, dim), F)
    nc = [(1,) * dim] * B
    cells_max = 1
    for b in range(B):
        q = p[off[b]:off[b + 1]]
        if q.shape[0] == 0:
            continue
        if not np.isfinite(q).all():
            raise Refused("finite")
        lo[b] = (q.min(axis=0) + F(0)) if origin is None else np.asarray(origin, F)
        if origin is not None and (q.min(axis=0) < lo[b]).any():
            raise Refused("origin")
        with np.errstate(over="ignore", invalid="ignore"):
            ext = q.max(axis=0) - lo[b]
            if not np.isfinite(ext).all():
                raise Refused("extent")
            t = ext * inv
        if not (t < F(MAX_AXIS)).all():
            raise Refused("axis")
        nc[b] = tuple(int(v) + 1 for v in t)
        cells_max = max(cells_max, int(np.prod([int(v) for v in nc[b]], dtype=object)))
    cbits, bbits = bits_for(cells_max - 1), bits_for(max(B - 1, 0))
    if cbits + bbits > 62:
        raise Refused("bits")
    bits = cbits + bbits
    return inv, lo, nc, bits, (1 if bits <= 8 else (bits + 7) // 8)


def cells_of(p, off, inv, lo):
    """c [n, dim] int64 and the cloud of every point: c_k = floor(fl(fl(p_k - lo_k) * inv))"""
    p = np.ascontiguousarray(p, F)
    cloud = np.repeat(np.arange(off.size - 1), np.diff(off))
    with np.errstate(over="ignore", invalid="ignore"):
        c = ((p - lo[cloud]) * inv).astype(np.int64)
    return c, cloud


def _sqdist(p, c):
    """((d0*d0) + d1*d1) + d2*d2 of d = p - c, float32, term by term"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = p - c
        s = d[..., 0] * d[..., 0]
        for a in range(1, p.shape[-1]):
            s = s + d[..., a] * d[..., a]
    return s


def _finish(p, off, lo, order, rowptr, centroid, nearest, cell, extra):
    n, m = p.shape[0], rowptr.size - 1
    count = np.diff(rowptr)
    of_slot = np.repeat(np.arange(m), count)
    cluster = np.empty(n, np.int32)
    cluster[order] = of_slot + 1
    pairs = np.stack([of_slot + 1, order + 1], axis=1).astype(np.int32)          # the memory of a column-major [2, n]
    first = order[rowptr[:-1]] if m else np.zeros(0, np.int64)                    # a member of each cluster -> its cloud
    cloud_of = np.searchsorted(off, first, side="right") - 1
    coff = np.searchsorted(cloud_of, np.arange(off.size), side="left").astype(np.int32)
    out = dict(cluster=cluster, pairs=pairs, rowptr=rowptr.astype(np.int32), weights=(F(1) / count.astype(F))[of_slot].astype(F),
               centroid=centroid.astype(F), nearest=nearest.astype(np.int32), cell=cell.astype(np.int32), cluster_offsets=coff,
               origin_out=lo.copy(), m=m, largest=int(count.max()) if m else 0)
    out.update(extra)
    return out


def clusters(p, off, size, origin=None):
    """the definition through one stable sort of the points by (cloud, c_{dim-1}, .., c_0); the sums advance one member per round in
    all clusters at once"""
    p = np.ascontiguousarray(p, F)
    n, dim = p.shape
    inv, lo, nc, bits, passes = grids(p, off, size, origin)
    c, cloud = cells_of(p, off, inv, lo)
    order = np.lexsort(tuple(c[:, k] for k in range(dim)) + (cloud,)) if n else np.zeros(0, np.int64)      # stable; the last key is primary
    key = np.concatenate([cloud[order, None], c[order][:, ::-1]], axis=1)
    head = np.ones(n, bool)
    head[1:] = (key[1:] != key[:-1]).any(axis=1)
    rowptr = np.concatenate([np.nonzero(head)[0], [n]]).astype(np.int64)
    m = rowptr.size - 1
    count = np.diff(rowptr)
    l = lo[cloud[order[rowptr[:-1]]]] if m else np.zeros((0, dim), F)
    S = np.zeros((m, dim), F)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(int(count.max()) if m else 0):
            live = np.nonzero(count > r)[0]
            S[live] = S[live] + (p[order[rowptr[live] + r]] - l[live])
        centroid = l + S / count.astype(F)[:, None]
    of_slot = np.repeat(np.arange(m), count)
    s = _sqdist(p[order], centroid[of_slot]) if n else np.zeros(0, F)
    k64 = (s.view(np.uint32).astype(np.uint64) << np.uint64(32)) | order.astype(np.uint64)
    nearest = (np.minimum.reduceat(k64, rowptr[:-1]) & np.uint64(0xFFFFFFFF)).astype(np.int64) + 1 if m else np.zeros(0, np.int64)
    cell = c[order[rowptr[:-1]]] if m else np.zeros((0, dim), np.int64)
    return _finish(p, off, lo, order, rowptr, centroid, nearest, cell, dict(bits=bits, passes=passes))


def brute_force(p, off, size, origin=None):
    """the definition with a dictionary keyed by (cloud, cell tuple), filled in point order: no sort of the points"""
    p = np.ascontiguousarray(p, F)
    n, dim = p.shape
    inv, lo, nc, bits, passes = grids(p, off, size, origin)
    c, cloud = cells_of(p, off, inv, lo)
    members = {}
    for j in range(n):
        members.setdefault((int(cloud[j]),) + tuple(int(v) for v in c[j][::-1]), []).append(j)
    names = sorted(members)                                                       # of the clusters, not of the points
    m = len(names)
    centroid, nearest, cell = np.zeros((m, dim), F), np.zeros(m, np.int64), np.zeros((m, dim), np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for i, name in enumerate(names):
            l, S = lo[name[0]], [F(0)] * dim
            for j in members[name]:
                for k in range(dim):
                    S[k] = F(S[k] + F(p[j, k] - l[k]))
            cnt = F(len(members[name]))
            centroid[i] = [F(l[k] + F(S[k] / cnt)) for k in range(dim)]
            best = None
            for j in members[name]:
                key = (int(_sqdist(p[j], centroid[i]).view(np.uint32)), j)
                best = key if best is None or key < best else best
            nearest[i] = best[1] + 1
            cell[i] = name[:0:-1]
    order = np.array([j for name in names for j in members[name]], np.int64)
    rowptr = np.concatenate([[0], np.cumsum([len(members[name]) for name in names])]).astype(np.int64)
    return _finish(p, off, lo, order, rowptr, centroid, nearest, cell, dict(bits=bits, passes=passes))


def same(got, want, keys=KEYS):
    """the names of the arrays that differ, floats by their bits"""
    bad = []
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape or g.dtype != w.dtype or not np.array_equal(g.view(np.int32), w.view(np.int32)):
            bad.append(k)
    return bad


def grad(cluster, rowptr, dcentroid):
    """dpoints[j, k] = fl(dcentroid[c, k] / fl(count_c)), c = cluster[j]"""
    count = np.diff(rowptr).astype(F)
    c = cluster.astype(np.int64) - 1
    return (np.ascontiguousarray(dcentroid, F)[c] / count[c][:, None]).astype(F)


def centroid64(p64, cluster, m):
    """the float64 twin of the centroids for a FIXED membership: the mean of the members.  lo cancels"""
    out = np.zeros((m, p64.shape[1]), np.float64)
    np.add.at(out, cluster.astype(np.int64) - 1, p64)
    return out / np.bincount(cluster.astype(np.int64) - 1, minlength=m)[:, None]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def cloud_of_sizes(sizes, dim, size, seed, row=64, shift=0.0):
    """one cloud whose cluster i has sizes[i] members, shuffled: cell i = (i % row, i // row, 0) at edge `size` (a power of two), the
    first member of cell 0 exactly on the corner so that lo is the corner; `shift` (a multiple of size) moves the whole cloud"""
    rng = _rng(seed)
    parts = []
    for i, s in enumerate(sizes):
        corner = np.array([i % row, i // row, 0][:dim] if dim > 1 else [i], np.float64)
        u = rng.integers(1, 15, (s, dim)) / 16.0
        if i == 0:
            u[0] = 0.0
        parts.append((corner + u) * size + shift)
    p = np.concatenate(parts).astype(F)
    return np.ascontiguousarray(p[rng.permutation(p.shape[0])])


HUB_SIZES = (1, 3, 4, 5, 63, 64, 65, 5000)
BOUNDARY_N = {4095: [3] * 1365, 4096: [3] * 1365 + [1], 4097: [3] * 1365 + [1, 1], 8193: [3] * 1365 + [1, 1] + [2] * 2047 + [1, 1]}


def mixed_batch():
    """empty clouds first, in the middle and last; a one-point cloud; a coincident cloud; two clouds with identical coordinates; a
    lattice on multiples of size; coordinates around 1e6; negative coordinates and -0.  size = 0.25"""
    rng = _rng(7)
    twin = rng.random((300, 3)).astype(F) * 3
    lat = (np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.25).astype(F)
    far = (1e6 + rng.random((400, 3)) * 2).astype(F)
    neg = (rng.random((200, 3)) * 2 - 1.5).astype(F)
    neg[3] = [-0.0, -0.0, -0.0]
    zero = np.array([[-0.0, 0.0, -0.0], [0.1, 0.3, 0.2], [0.0, -0.0, 0.26]], F)                         # lo = -0 + 0 = +0
    clouds = [np.zeros((0, 3), F), twin, np.full((1, 3), 2.5, F), np.zeros((0, 3), F), np.tile(F([1.25, -3.0, 7.0]), (37, 1)), twin.copy(),
              lat, far, neg, zero, np.zeros((0, 3), F)]
    return np.ascontiguousarray(np.concatenate(clouds)), offsets_of([c.shape[0] for c in clouds]), 0.25


def wide_key():
    """a 3-D cloud of extent exactly 1 at size 2^-11: 2049^3 = 8.6e9 cells, 34 bits; a second cloud adds a cloud bit"""
    rng = _rng(11)
    a = rng.random((3000, 3)).astype(F)
    a[0], a[1] = 0.0, 1.0
    b = rng.random((500, 3)).astype(F) * F(0.01)
    return np.ascontiguousarray(np.concatenate([a, b])), offsets_of([3000, 500]), 2.0 ** -11


@functools.lru_cache(None)
def shape_cases():
    """(name, points, offsets, size, origin) of every shape class the GPU tests run"""
    cases = []
    for dim in (1, 2, 3):
        p = cloud_of_sizes(HUB_SIZES, dim, 0.25, 20 + dim, row=3)
        cases.append((f"sizes 1..65 and a hub, dim {dim}", p, offsets_of([p.shape[0]]), 0.25, None))
    for m in (63, 64, 65):
        p = cloud_of_sizes(_rng(30 + m).integers(1, 7, m), 3, 0.5, 40 + m, row=8)
        cases.append((f"m = {m}", p, offsets_of([p.shape[0]]), 0.5, None))
    for n, sizes in BOUNDARY_N.items():
        p = cloud_of_sizes(sizes, 2, 0.125, 50 + n % 7)
        assert p.shape[0] == n
        cases.append((f"n = {n}", p, offsets_of([n]), 0.125, None))
    p, off, size = mixed_batch()
    cases.append(("mixed batch", p, off, size, None))
    cases.append(("mixed batch, one cluster per cloud", p, off, 4e6, None))
    cases.append(("mixed batch, size 3e38", p, off, 3e38, None))
    cases.append(("n_clouds = 0", np.zeros((0, 3), F), offsets_of([]), 1.0, None))
    cases.append(("n = 0", np.zeros((0, 2), F), offsets_of([0, 0]), 1.0, None))
    p = _rng(61).random((6000, 3)).astype(F)
    p2 = (_rng(62).random((3000, 3)) ** 3).astype(F)
    cases.append(("uniform and graded clouds", np.concatenate([p, p2]), offsets_of([6000, 3000]), 0.0625, None))
    cases.append(("uniform and graded clouds, origin below", np.concatenate([p, p2]), offsets_of([6000, 3000]), 0.0625, F([-2.0, -1.03, -3.5])))
    p, off, size = wide_key()
    cases.append(("wide key", p, off, size, None))
    return cases
