"""The yardstick of farthest-point sampling (athena_mp_farthest_points, athena_amd/csrc/fps.hip), in float32 term by term.

brute_force is the definition of include/athena_mp.h transcribed: dmin = +inf, step 1 chooses start, after every choice c
dmin[j] = min(dmin[j], s(j, c)), the next choice is the point NOT YET CHOSEN with the largest dmin, ties to the smaller index.
pruned is fps.hip's stream route transcribed: the points in some order, cut into chunks of 64 with the bounding box of the points
actually in each and a cached best key; a chunk is skipped when s(c, clamp(c, box)) >= its largest live dmin (and > 0).  Both
return (sample, sample_points, sample_sqdist, cover_sqdist); pruned also (chunk tests, tests that skipped)."""
import numpy as np

CHUNK = 64
THREADS = 256           # the register route's workgroup
CAPACITY = 4096         # points the register route holds


def _rng(seed):
    return np.random.default_rng(seed)


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def sq_dist(p, c):
    """s(j, c) for every row j of p [n, dim]: ((d0*d0) + d1*d1) + d2*d2, every operation rounded to float32"""
    p = np.asarray(p, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = p - np.asarray(c, np.float32)[None, :]
        s = d[:, 0] * d[:, 0]
        for a in range(1, p.shape[1]):
            s = s + d[:, a] * d[:, a]
    assert s.dtype == np.float32
    return s


def _key(d, index):
    """fps.hip's key: dmin's bits above ~index"""
    return (int(np.float32(d).view(np.uint32)) << 32) | (~int(index) & 0xFFFFFFFF)


def _brute_cloud(p, m, start):
    n = p.shape[0]
    dmin = np.full(n, np.inf, np.float32)
    chosen = np.zeros(n, bool)
    sample, sqd = np.empty(m, np.int64), np.empty(m, np.float32)
    cur, dcur = start, np.float32(np.inf)
    for t in range(m):
        sample[t], sqd[t] = cur, dcur
        chosen[cur] = True
        dmin = np.minimum(dmin, sq_dist(p, p[cur]))
        if t + 1 < m:
            cur = int(np.argmax(np.where(chosen, np.float32(-1), dmin)))      # the first of the largest: the smaller index
            dcur = dmin[cur]
    return sample, sqd, (dmin.max() if n else np.float32(0))


def cell_order(p, cell_points=CHUNK):
    """an order like the cell order of the stream route: cells of about cell_points points, x fastest, stable inside a cell"""
    n, dim = p.shape
    lo, hi = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    extent = np.where((hi - lo > 0) & (hi - lo < 1e37), hi - lo, 0.0)
    active = int((extent > 0).sum())
    if active == 0:
        return np.arange(n)
    w = (np.prod(extent[extent > 0]) / max(1.0, n / cell_points)) ** (1.0 / active)
    nc = np.where(extent > 0, np.clip(np.floor(extent / max(w, 1e-300)), 1, 2048), 1).astype(np.int64)
    key = np.zeros(n, np.int64)
    for a in range(dim - 1, -1, -1):
        c = np.zeros(n, np.int64)
        if nc[a] > 1:
            c = np.minimum(((p[:, a].astype(np.float64) - lo[a]) * (nc[a] / extent[a])).astype(np.int64), nc[a] - 1)
        key = key * nc[a] + c
    return np.argsort(key, kind="stable")


def _pruned_cloud(p, m, start, order, bound):
    n = p.shape[0]
    ps, nch = p[order], (n + CHUNK - 1) // CHUNK
    cuts = [slice(k * CHUNK, min((k + 1) * CHUNK, n)) for k in range(nch)]
    lo = [ps[c].min(0) for c in cuts]
    hi = [ps[c].max(0) for c in cuts]
    dmin = np.full(n, np.inf, np.float32)
    chosen = np.zeros(n, bool)
    ckey = [_key(np.inf, order[c].min()) for c in cuts]
    sample, sqd = np.empty(m, np.int64), np.empty(m, np.float32)
    cur, dcur, best = start, np.float32(np.inf), 0
    examined = skipped = 0
    for t in range(m):
        sample[t], sqd[t] = cur, dcur
        c = p[cur]
        for k, cut in enumerate(cuts):
            examined += 1
            if ckey[k] == 0:
                skipped += 1
                continue
            D = np.array([ckey[k] >> 32], np.uint32).view(np.float32)[0]
            if bound == "clamp":
                q = np.minimum(np.maximum(c, lo[k]), hi[k])
                read = not (sq_dist(q[None, :], c)[0] >= D and sq_dist(q[None, :], c)[0] > 0)
            else:                                    # a bound that is none: the distance to the box's centre
                with np.errstate(over="ignore"):
                    q = (lo[k] * np.float32(0.5) + hi[k] * np.float32(0.5)).astype(np.float32)
                read = not (sq_dist(q[None, :], c)[0] >= D) or cur in order[cut]
            if not read:
                skipped += 1
                continue
            live = ~chosen[cut]
            dn = np.minimum(dmin[cut], sq_dist(ps[cut], c))
            dmin[cut] = np.where(live, dn, dmin[cut])
            chosen[cut] |= order[cut] == cur
            keys = [_key(d, i) for d, i, ch in zip(dmin[cut], order[cut], chosen[cut]) if not ch]
            ckey[k] = max(keys) if keys else 0
        best = max(ckey)
        if t + 1 < m:
            assert best != 0
            cur = ~best & 0xFFFFFFFF
            dcur = np.array([best >> 32], np.uint32).view(np.float32)[0]
    cover = np.array([best >> 32], np.uint32).view(np.float32)[0] if best else np.float32(0)
    return sample, sqd, cover, examined, skipped


def _batched(points, offsets, sample_offsets, start, one):
    points = np.ascontiguousarray(points, np.float32)
    if offsets is None:
        offsets = offsets_of([points.shape[0]])
    B = offsets.size - 1
    m_total = int(sample_offsets[-1])
    sample = np.zeros(m_total, np.int32)
    sqd = np.zeros(m_total, np.float32)
    cover = np.zeros(B, np.float32)
    extra = np.zeros(2, np.int64)
    for b in range(B):
        p0, p1, s0, s1 = int(offsets[b]), int(offsets[b + 1]), int(sample_offsets[b]), int(sample_offsets[b + 1])
        if s1 == s0:
            cover[b] = np.inf if p1 > p0 else 0
            continue
        first = 0 if start is None or start[b] == 0 else int(start[b]) - 1 - p0
        assert 0 <= first < p1 - p0 and s1 - s0 <= p1 - p0
        got = one(points[p0:p1], s1 - s0, first)
        sample[s0:s1], sqd[s0:s1], cover[b] = got[0] + p0 + 1, got[1], got[2]
        extra += np.array(got[3:5], np.int64) if len(got) > 3 else 0
    return sample, points[sample - 1].copy(), sqd, cover, extra


def brute_force(points, sample_offsets, offsets=None, start=None):
    return _batched(points, offsets, np.asarray(sample_offsets), start, _brute_cloud)[:4]


def pruned(points, sample_offsets, offsets=None, start=None, order=cell_order, bound="clamp"):
    """order: a callable cloud -> permutation (any order is correct); returns the four arrays and (chunk tests, skipped)"""
    out = _batched(points, offsets, np.asarray(sample_offsets), start, lambda p, m, s: _pruned_cloud(p, m, s, order(p), bound))
    return out[:4] + (tuple(int(v) for v in out[4]),)


# ---- the shape classes both suites use -------------------------------------------------------------------------------------------
def lattice(side=5):
    g = np.arange(side, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def repeated():
    """five points, four times over"""
    five = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0], [0, 0, 2], [1, 1, 1]], np.float32)
    return np.tile(five, (4, 1))


def clustered(n, dim, seed, clusters=12, spread=0.004):
    rng = _rng(seed)
    centres = rng.random((clusters, dim))
    return (centres[rng.integers(0, clusters, n)] + spread * rng.standard_normal((n, dim))).astype(np.float32)


def huge(seed=7):
    """points at +-3e38 beside ordinary ones: differences and squares that overflow"""
    rng = _rng(seed)
    p = rng.random((90, 3)).astype(np.float32)
    p[::9] = rng.choice(np.array([-3e38, 3e38], np.float32), (10, 3))
    return p


def mixed_batch(seed=31, dim=3):
    """empty clouds, m_b = 0, m_b = n_b and m_b = 1, sizes on both sides of a wave and of the workgroup"""
    sizes = [70, 0, 1, 300, 64, 0, 257, 5]
    m = [9, 0, 1, 0, 64, 0, 1, 5]
    return _rng(seed).random((sum(sizes), dim)).astype(np.float32), offsets_of(sizes), offsets_of(m)


def shape_cases():
    """(name, points, offsets, sample_offsets, start): one cloud unless the name says batch"""
    cases = []
    one = lambda name, p, m, start=None: cases.append((name, np.ascontiguousarray(p, np.float32), offsets_of([p.shape[0]]),
                                                       offsets_of([m]), None if start is None else np.array([start], np.int32)))
    for n in (1, 2, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1):
        one(f"n = {n}, all of it", _rng(n).random((n, 3)), n)
    for n in (CAPACITY - 1, CAPACITY, CAPACITY + 1):
        one(f"n = {n}, m = 32", _rng(n).random((n, 3)), 32, start=n // 2)
    one("three chunks and a ragged one, dim 3", _rng(3).random((3 * CHUNK + 17, 3)), 60)
    one("dim 1", _rng(11).random((333, 1)), 40, start=200)
    one("dim 2", _rng(12).random((333, 2)), 40)
    one("clustered, dim 2", clustered(700, 2, 13), 48)
    one("clustered, dim 3", clustered(900, 3, 14), 48, start=900)
    one("lattice 5^3, m = n", lattice(), 125)
    one("repeated points, m = n", repeated(), 20)
    one("around 1e6", 1e6 + 50 * _rng(15).random((400, 3)), 64)
    one("+-3e38", huge(), 90)
    p, off, soff = mixed_batch()
    cases.append(("batch, start defaulted", p, off, soff, None))
    start = np.where(np.diff(soff) > 0, off[1:], 0).astype(np.int32)           # each cloud's LAST point; unused entries 0
    start[4] = 0                                                                 # an entry of 0: the first point
    cases.append(("batch, start given", p, off, soff, start))
    return cases
