"""The yardstick of the two-set k-nearest-neighbour builder (athena_mp_knn_pairs_bipartite, athena_amd/csrc/knn_bipartite.hip): the
definition of include/athena_mp.h in numpy float32, and a Python transcription of the kernel's grid search.

  brute force   the definition as it is written: the all-pairs s of a cloud's queries and sources, a stable sort (ties to the
                smaller source index), the cap, the first k.  A few thousand points at the most.
  grid search   knn_bipartite.hip's search, shell by shell around the source cell nearest to the query, with the file header's
                stop rule in float32: the cell coordinate clamped to [-2, nc + 2], the margin, the flag for "no unread side".  It
                returns what it examined as well (the counts of athena_mp_knn_stats), and takes the margin and the clamp as
                arguments so that a test can show that a case needs them.

test_knn_bipartite.py pins the second to the first on every shape class the GPU tests use."""
import numpy as np

import knn_reference as kr

K_MARGIN, K_SHRINK = kr.K_MARGIN, kr.K_SHRINK
INF = np.float32(np.inf)
f32 = np.float32


def _rng(seed):
    return np.random.default_rng(seed)


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _offsets(q, s, qoff, soff):
    qoff = offsets_of([q.shape[0]]) if qoff is None else np.asarray(qoff)
    soff = offsets_of([s.shape[0]]) if soff is None else np.asarray(soff)
    assert qoff.shape == soff.shape
    return qoff, soff


def brute_force(q, s, k, radius=None, qoff=None, soff=None):
    """(nbr [nq, k] int32, sqdist [nq, k] float32): row i = N_k(i) as 1-based global source ids in key order padded with 0, and
    the s of each entry padded with +inf"""
    assert q.dtype == np.float32 and s.dtype == np.float32 and q.ndim == 2 and s.ndim == 2
    qoff, soff = _offsets(q, s, qoff, soff)
    r2 = kr.r2_of(radius)
    nbr = np.zeros((q.shape[0], k), np.int32)
    sqd = np.full((q.shape[0], k), INF, np.float32)
    for b in range(qoff.size - 1):
        q0, q1, s0, s1 = int(qoff[b]), int(qoff[b + 1]), int(soff[b]), int(soff[b + 1])
        if q1 == q0 or s1 == s0:
            continue
        for r0 in range(q0, q1, 512):                              # a block of rows at a time: the all-pairs array stays small
            r1 = min(r0 + 512, q1)
            S = kr.sq_dist(q[r0:r1, None, :], s[None, s0:s1, :])
            assert not np.isnan(S).any()
            o = np.argsort(S, axis=1, kind="stable")[:, :k]        # stable: ties to the smaller source index
            So = np.take_along_axis(S, o, 1)
            ok = So <= r2                                          # what the cap removes sorts behind what it keeps
            kk = o.shape[1]
            nbr[r0:r1, :kk] = np.where(ok, o + s0 + 1, 0)
            sqd[r0:r1, :kk] = np.where(ok, So, INF)
    return nbr, sqd


def graph_of(nbr, q, s, qoff=None):
    """nbr [nq, k] -> (i, j, coords, rowptr, edge_offsets): 0-based global pairs in lexicographic order of (i, j) -- the sources of
    a row ascend by index --, coords = q[i] - s[j], rowptr [nq + 1] int32, edge_offsets int64"""
    nq, k = nbr.shape
    qoff = offsets_of([nq]) if qoff is None else np.asarray(qoff)
    i = np.repeat(np.arange(nq, dtype=np.int64), k)
    j = nbr.reshape(-1).astype(np.int64) - 1
    i, j = i[j >= 0], j[j >= 0]
    o = np.lexsort((j, i))
    i, j = i[o], j[o]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=nq))]).astype(np.int32)
    with np.errstate(over="ignore"):
        coords = (q[i] - s[j]).reshape(i.size, q.shape[1])
    return i, j, coords, rowptr, rowptr[qoff].astype(np.int64)


# ---- the grid search of knn_bipartite.hip ----------------------------------------------------------------------------------------
def grid_search(q, s, k, radius=None, qoff=None, soff=None, margin=K_MARGIN, clamp=True):
    """-> (nbr, sqdist, stats): stats = [queries, candidates examined, cells visited, largest shell], as athena_mp_knn_stats.
    margin = 0 or clamp = False give the search WITHOUT that part of the rule (clamp = False is for finite cell coordinates)."""
    assert q.dtype == np.float32 and s.dtype == np.float32
    qoff, soff = _offsets(q, s, qoff, soff)
    r2 = kr.r2_of(radius)
    capped = np.isfinite(r2)
    dim = q.shape[1]
    nbr = np.zeros((q.shape[0], k), np.int32)
    sqd = np.full((q.shape[0], k), INF, np.float32)
    stats = [q.shape[0], 0, 0, 0]
    margin = f32(margin)
    for b in range(qoff.size - 1):
        q0, q1, s0, s1 = int(qoff[b]), int(qoff[b + 1]), int(soff[b]), int(soff[b + 1])
        if q1 == q0 or s1 == s0:
            continue                                         # a cloud without sources has no grid: its queries read nothing
        src = s[s0:s1]
        lo, inv_w, nc, w_low = kr.make_knn_grid(src)
        gs = (src - lo) * inv_w                              # cell_q of the sources: two float32 roundings
        cell = np.minimum(gs.astype(np.int64), nc - 1)
        members = {}
        for j in range(src.shape[0]):
            members.setdefault(tuple(cell[j]), []).append(j)
        with np.errstate(over="ignore", invalid="ignore"):
            g_all = (q[q0:q1] - lo) * inv_w
        assert g_all.dtype == np.float32
        if clamp:
            g_all = np.fmin(np.fmax(g_all, f32(-2)), (nc + 2).astype(np.float32))     # fmax(NaN, -2) = -2
        assert np.isfinite(g_all).all()
        for i in range(q1 - q0):
            g = g_all[i]
            c = np.clip(np.floor(g).astype(np.int64), 0, nc - 1)
            best_s, best_j = np.zeros(0, f32), np.zeros(0, np.int64)
            rho = 0
            while True:
                lo_c, hi_c = np.maximum(c - rho, 0), np.minimum(c + rho, nc - 1)
                grid = np.stack(np.meshgrid(*[np.arange(lo_c[a], hi_c[a] + 1) for a in range(dim)], indexing="ij"), -1).reshape(-1, dim)
                shell = grid[np.abs(grid - c).max(1) == rho]
                j = np.asarray([x for cc in shell for x in members.get(tuple(cc), ())], np.int64)
                stats[1] += j.size
                stats[2] += shell.shape[0]
                if j.size:
                    sj = kr.sq_dist(q[q0 + i], src[j])
                    keep = sj <= r2
                    sj, j = np.concatenate([best_s, sj[keep]]), np.concatenate([best_j, j[keep]])
                    o = np.lexsort((j, sj))[:k]
                    best_s, best_j = sj[o], j[o]
                # the stop rule of the file header
                t, unread = INF, False
                for a in range(dim):
                    if nc[a] <= 1:
                        continue
                    if c[a] + rho + 1 <= nc[a] - 1:
                        t = min(t, ((f32(c[a] + rho + 1) - g[a]) - margin) * w_low[a])
                        unread = True
                    if c[a] - rho - 1 >= 0:
                        t = min(t, ((g[a] - f32(c[a] - rho)) - margin) * w_low[a])
                        unread = True
                if not unread:
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
            nbr[q0 + i, :best_j.size] = best_j + s0 + 1
            sqd[q0 + i, :best_s.size] = best_s
    return nbr, sqd, stats


# ---- the inputs both test files use --------------------------------------------------------------------------------------------
def uniform_with_outside(dim, nq=300, ns=200, seed=100):
    """sources uniform in the unit box; queries uniform in the box grown by half its width on every side"""
    rng = _rng(seed + dim)
    s = rng.random((ns, dim)).astype(np.float32)
    q = (rng.random((nq, dim)) * 2.0 - 0.5).astype(np.float32)
    return q, s


def on_and_beside_cell_boundaries(dim, ns=300, seed=110):
    """sources as knn_reference.on_cell_boundaries; queries with every component on a boundary lo + c / inv_w of the source grid,
    c = -2 .. nc + 2 (two cells below the grid to two above), or the float32 beside it"""
    rng = _rng(seed + dim)
    s = kr.on_cell_boundaries(dim, ns)
    lo, inv_w, nc, _ = kr.make_knn_grid(s)
    assert np.all(nc > 1)
    q = np.zeros((240, dim), np.float32)
    for a in range(dim):
        c = rng.integers(-2, nc[a] + 3, q.shape[0])
        x = (lo[a] + c / np.float64(inv_w[a])).astype(np.float32)
        step = rng.integers(-1, 2, q.shape[0])
        q[:, a] = np.where(step < 0, np.nextafter(x, f32(-9)), np.where(step > 0, np.nextafter(x, f32(9)), x))
    return q, s


def far_gaussian():
    rng = _rng(120)
    s = rng.random((200, 3)).astype(np.float32)
    q = (rng.standard_normal((60, 3)) * 1000.0).astype(np.float32)
    return q, s


def huge_queries(dim=3):
    """queries at +-3e38 on one axis or on all, beside ordinary ones: q - p overflows, s = +inf"""
    rng = _rng(130)
    s = rng.random((200, dim)).astype(np.float32)
    q = rng.random((20 + 2 * dim + 2, dim)).astype(np.float32)
    for a in range(dim):
        q[20 + 2 * a, a], q[21 + 2 * a, a] = 3e38, -3e38
    q[-2], q[-1] = 3e38, -3e38
    return q, s


def around_1e6():
    rng = _rng(140)
    s = (1e6 + rng.random((300, 3)) * 7.0).astype(np.float32)
    q = (1e6 + rng.random((200, 3)) * 11.0 - 2.0).astype(np.float32)
    return q, s


def lattice_on_the_sources(*shape):
    s = kr.lattice(*shape)
    return s[_rng(150).permutation(s.shape[0])].copy(), s


def lattice_at_cell_centres(*shape):
    s = kr.lattice(*shape)
    q = kr.lattice(*[n - 1 for n in shape]) + f32(0.5)       # equidistant from 2^dim sources: the tie rule decides
    return q, s


def coincident_sources(m, nq=40, seed=160):
    rng = _rng(seed + m)
    s = np.repeat(rng.random((1, 3)).astype(np.float32), m, axis=0)
    return rng.random((nq, 3)).astype(np.float32), s


def batch():
    rng = _rng(170)
    qoff, soff = offsets_of([300, 0, 1, 450, 2, 120]), offsets_of([200, 5, 0, 300, 70, 1])
    shift = rng.uniform(-5, 5, (6, 3))                        # the clouds lie anywhere; a cloud's queries reach beyond its sources
    q = (rng.random((int(qoff[-1]), 3)) * 1.4 - 0.2 + np.repeat(shift, np.diff(qoff), axis=0)).astype(np.float32)
    s = (rng.random((int(soff[-1]), 3)) + np.repeat(shift, np.diff(soff), axis=0)).astype(np.float32)
    return q, s, qoff, soff


def cap_case(dim):
    """the issue's cap case: 300 queries, then 200 sources, from default_rng(5); k = 8 and a radius that cuts some rows and leaves
    others to k"""
    rng = np.random.default_rng(5)
    q = rng.random((300, dim), np.float32)
    s = rng.random((200, dim), np.float32)
    return q, s, {1: 0.02, 2: 0.12, 3: 0.25}[dim]


def margin_probe():
    """One query and 4097 sources on the line [-1.5, 1.5], built so that the search is wrong WITHOUT the margin.  The grid has 2048
    cells; around cell 1060 the positions are near 0 and fine-grained, while fl(p - lo) is rounded at the spacing of 1.5 and g at
    that of 1024: a computed cell coordinate is off by up to 10^-4 of a cell.  Source B is the first float32 whose computed cell
    is c + 1 while its exact coordinate is still below the boundary; the query's computed g is below its exact one; source A, in
    the query's own cell on its other side, lies farther than B but inside the bound that the unmargined gap gives.  Truth: B.
    -> (q, s, k = 1, index of A, index of B)"""
    L = f32(1.5)
    filler = (_rng(180).random(4093) - 1.5).astype(np.float32)            # the lower third: far from the cells probed
    ends = lambda mid: np.concatenate([[-L], filler, mid, [L]]).astype(np.float32)[:, None]
    lo, inv_w, nc, w_low = kr.make_knn_grid(ends([0.0, 0.0]))
    assert nc[0] == 2048 and lo[0] == -L
    iw = np.float64(inv_w[0])
    g_of = lambda p: f32(f32(p - lo[0]) * inv_w[0])                       # cell_q
    x_of = lambda p: (np.float64(p) + 1.5) * iw                           # the same in exact arithmetic
    best = None
    for c in range(1030, 1100):
        pb = f32((c + 1) / iw - 1.5)
        while g_of(pb) >= c + 1:                                          # down to the last float32 whose computed g is below c + 1
            pb = np.nextafter(pb, f32(-9))
        while g_of(pb) < c + 1:                                           # the first whose computed g reaches it
            pb = np.nextafter(pb, f32(9))
        qv = f32((c + 0.7) / iw - 1.5)
        for _ in range(200):                                              # the query whose g is rounded down the most
            hidden = ((c + 1) - x_of(pb)) + (x_of(qv) - np.float64(g_of(qv)))
            if best is None or hidden > best[0]:
                best = (hidden, c, pb, qv)
            qv = np.nextafter(qv, f32(9))
    hidden, c, pb, qv = best
    g = g_of(qv)
    assert hidden > 2.0 ** -15 and int(g) == c and int(g_of(pb)) == c + 1
    t0 = (f32(c + 1) - g) * w_low[0]                                      # the gap without the margin
    bound0 = (t0 * t0) * K_SHRINK
    one = lambda a, b: kr.sq_dist(np.array([a], np.float32), np.array([b], np.float32))
    s_b = one(qv, pb)
    assert s_b < bound0, "the probe found no source that the unmargined bound hides"
    pa = f32(np.float64(qv) - np.sqrt(np.float64(s_b)))                   # A: on the other side, a little farther than B
    while not one(qv, pa) > s_b:
        pa = np.nextafter(pa, f32(-9))
    assert s_b < one(qv, pa) < bound0 and int(g_of(pa)) == c, "no room for A between B and the unmargined bound"
    s = ends([pa, pb])
    grid = kr.make_knn_grid(s)
    assert s.shape[0] == 4097 and grid[2][0] == 2048 and grid[1][0] == inv_w[0] and grid[3][0] == w_low[0]
    return np.array([[qv]], np.float32), s, 1, s.shape[0] - 3, s.shape[0] - 2


def shape_cases():
    """(name, queries, sources, query_offsets, source_offsets, k, radius) of every shape class, each small enough for brute force"""
    cases = []
    one = lambda name, qs, k, r=None: cases.append((name, qs[0], qs[1], None, None, k, r))
    for dim in (1, 2, 3):
        one(f"uniform, half a box outside, dim {dim}", uniform_with_outside(dim), 8)
    for dim in (1, 2, 3):
        one(f"cell boundaries -2 .. nc + 2, dim {dim}", on_and_beside_cell_boundaries(dim), 8)
    one("gaussian 1000 box widths out", far_gaussian(), 8)
    one("+-3e38, no cap", huge_queries(), 8)
    one("+-3e38, capped", huge_queries(), 8, 0.3)
    one("+-3e38, dim 1, k = 64", huge_queries(1), 64)
    one("around 1e6", around_1e6(), 8)
    one("1e6 + lattice, on the sources", tuple(a + f32(1e6) for a in lattice_on_the_sources(12, 12)), 5)
    one("lattice 1-D, on the sources", lattice_on_the_sources(64), 3)
    one("lattice 12 x 12, cell centres", lattice_at_cell_centres(12, 12), 4)
    one("lattice 6 x 6 x 6, cell centres, k = 7", lattice_at_cell_centres(6, 6, 6), 7)
    one("lattice 6 x 6 x 6, on the sources, k = 7", lattice_on_the_sources(6, 6, 6), 7)
    one("200 coincident sources, k = 64", coincident_sources(200), 64)
    one("k above the number of sources", uniform_with_outside(2, 50, 5), 9)
    one("k = 1", uniform_with_outside(3, 200, 300), 1)
    one("k = 64", uniform_with_outside(3, 100, 300), 64)
    for dim in (1, 2, 3):
        q, s, r = cap_case(dim)
        one(f"capped dim {dim}", (q, s), 8, r)
    assert len(cases) == 23
    return cases
