"""The yardstick of athena_mp_topk_vertices and athena_mp_select_rows_fwd / _bwd (include/athena_mp.h): the selection in numpy,
twice over with nothing shared -- `select` (each graph sorted with an explicit comparison of two vertices) and `select_counting`
(the O(n_g^2) form: a vertex is kept iff fewer than k_g vertices precede it and it passes) --, the gated rows term by term in
fp32 with the gate's gradient in float64, and the named inputs the CPU and GPU tests share.

Order inside a graph: value descending, then vertex index ascending; -0 equals +0; every NaN equals every other NaN and lies below
-inf.  Graph g keeps the first min(k_g, n_g) vertices of that order, with min_score only those with score >= min_score."""
import functools

import numpy as np

KEYS = ("cluster", "selected", "order", "sel_offsets")
WAVE_MAX = 64
TILE = 4096                                                           # entries of one radix tile


class Refused(ValueError):
    pass


def _rng(seed):
    return np.random.default_rng(seed)


def bits_for(v):
    b = 1
    while b < 64 and (int(v) >> b):
        b += 1
    return b


def ratio_counts(sizes, ratio):
    """the wrapper's rule, on the host in float64: k_g = min(n_g, ceil(ratio * n_g))"""
    sizes = np.asarray(sizes, np.int64)
    return np.minimum(sizes, np.ceil(np.float64(ratio) * sizes.astype(np.float64)).astype(np.int64)).astype(np.int32)


def check(score, offsets, k):
    """the refusals of the library, in its order; the word that names each is in the message"""
    n, B = score.shape[0], offsets.shape[0] - 1
    if B < 0 or n < 0:
        raise Refused("negative")
    if B == 0:
        if n != 0:
            raise Refused("end at")
        return
    if offsets[0] != 0:
        raise Refused("offsets(1)")
    down = np.nonzero(np.diff(offsets.astype(np.int64)) < 0)[0]
    if down.size:
        raise Refused(f"offsets({down[0] + 2})")
    if offsets[-1] != n:
        raise Refused("end at")
    kk = np.broadcast_to(np.asarray(k, np.int64), (B,))
    if np.ndim(k) == 0 and k < 0:
        raise Refused("k =")
    bad = np.nonzero(kk < 0)[0]
    if bad.size:
        raise Refused(f"k({bad[0] + 1})")


def stats(offsets, route="auto"):
    """what athena_mp_topk_stats reports: graphs on the wave route, on the sort route, key bits sorted, radix passes"""
    sizes = np.diff(np.asarray(offsets, np.int64))
    B = sizes.size
    on_wave = np.ones(B, bool) if route == "wave" else np.zeros(B, bool) if route == "sort" else sizes <= WAVE_MAX
    sorted_vertices = int(sizes[~on_wave].sum())
    bits = 32 + bits_for(max(B - 1, 0)) if sorted_vertices else 0
    return (int(on_wave.sum()), int(B - on_wave.sum()), bits, (bits + 7) // 8)


def _precedes(sa, a, sb, b):
    """vertex a (score sa) comes before vertex b in the order of the definition"""
    na, nb = sa != sa, sb != sb
    if na or nb:
        return (not na) if na != nb else a < b
    if sa != sb:                                                      # -0 == +0 here
        return sa > sb
    return a < b


def _finish(n, B, kept_in_order):
    """kept_in_order: per graph the kept vertices (0-based, global) in score order -> the four arrays"""
    cluster = np.zeros(n, np.int32)
    flat = np.array([v for run in kept_in_order for v in run], np.int64)
    selected = np.sort(flat)
    cluster[selected] = np.arange(1, selected.size + 1)
    sel_offsets = np.concatenate([[0], np.cumsum([len(run) for run in kept_in_order])]).astype(np.int32) if B else np.zeros(1, np.int32)
    return dict(m=int(selected.size), cluster=cluster, selected=(selected + 1).astype(np.int32), order=(flat + 1).astype(np.int32),
                sel_offsets=sel_offsets)


def select(score, offsets, k, min_score=None):
    """the sorted form: every graph's vertices sorted with the comparison of the definition, then the prefix"""
    check(score, offsets, k)
    n, B = score.shape[0], offsets.shape[0] - 1
    kk = np.broadcast_to(np.asarray(k, np.int64), (B,))
    runs = []
    for g in range(B):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        vals = [float(s) for s in score[lo:hi]]
        cmp = lambda a, b: -1 if _precedes(vals[a], a, vals[b], b) else 1
        order = sorted(range(hi - lo), key=functools.cmp_to_key(cmp))
        run = []
        for a in order[:min(int(kk[g]), hi - lo)]:
            if min_score is not None and not np.float32(vals[a]) >= np.float32(min_score):
                break
            run.append(lo + a)
        runs.append(run)
    return _finish(n, B, runs)


def select_counting(score, offsets, k, min_score=None):
    """the counting form: v is kept iff fewer than k_g vertices of its graph precede it and it passes; its place in the graph's
    run is that count"""
    check(score, offsets, k)
    n, B = score.shape[0], offsets.shape[0] - 1
    kk = np.broadcast_to(np.asarray(k, np.int64), (B,))
    runs = []
    for g in range(B):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        s = score[lo:hi].astype(np.float32)
        ng = hi - lo
        nan = np.isnan(s)
        idx = np.arange(ng)
        before = np.zeros(ng, np.int64)
        with np.errstate(invalid="ignore"):
            for c0 in range(0, ng, 1024):                             # columns v in chunks, rows u: u precedes v
                v = slice(c0, min(ng, c0 + 1024))
                greater = s[:, None] > s[None, v]
                below_nan = ~nan[:, None] & nan[None, v]
                same = (s[:, None] == s[None, v]) | (nan[:, None] & nan[None, v])
                before[v] = (greater | below_nan | (same & (idx[:, None] < idx[None, v]))).sum(axis=0)
            passes = np.ones(ng, bool) if min_score is None else s >= np.float32(min_score)
        kept = np.nonzero((before < kk[g]) & passes)[0]
        run = np.full(kept.size, -1, np.int64)
        run[before[kept]] = lo + kept                                 # the kept are a prefix: their counts are 0 .. len - 1
        assert (run >= 0).all()
        runs.append(run.tolist())
    return _finish(n, B, runs)


def same(a, b):
    return [key for key in KEYS if not np.array_equal(a[key], b[key])] + ([] if a["m"] == b["m"] else ["m"])


# ---- the gated rows -----------------------------------------------------------------------------------------------------------------
def rows_fwd(selected, x, gate=None):
    """y[r, :] = fl(x[v, :] * gate[v]), v = selected[r] - 1; without a gate the words themselves"""
    v = selected.astype(np.int64) - 1
    if gate is None:
        return x.view(np.int32)[v].view(np.float32)
    with np.errstate(all="ignore"):
        return (x[v].astype(np.float32) * gate[v].astype(np.float32)[:, None]).astype(np.float32)


def rows_bwd_x(cluster, dy, gate=None):
    """dx[v, :] = fl(dy[c - 1, :] * gate[v]), c = cluster[v]; +0 where c = 0"""
    n, F = cluster.shape[0], dy.shape[1]
    dx = np.zeros((n, F), np.float32)
    kept = np.nonzero(cluster > 0)[0]
    rows = dy.view(np.int32)[cluster[kept].astype(np.int64) - 1].view(np.float32)
    if gate is not None:
        with np.errstate(all="ignore"):
            rows = (rows * gate[kept].astype(np.float32)[:, None]).astype(np.float32)
    dx.view(np.int32)[kept] = rows.view(np.int32)
    return dx


def rows_bwd_gate(cluster, dy, x):
    """(dgate [n] in float64 from the fp32 products, the sum of the products' magnitudes): dgate[v] = sum over the columns of
    fl(dy[c - 1, col] * x[v, col]); both 0 where c = 0"""
    n = cluster.shape[0]
    dgate, scale = np.zeros(n, np.float64), np.zeros(n, np.float64)
    kept = np.nonzero(cluster > 0)[0]
    with np.errstate(all="ignore"):
        prod = (dy[cluster[kept].astype(np.int64) - 1].astype(np.float32) * x[kept].astype(np.float32)).astype(np.float32).astype(np.float64)
        dgate[kept], scale[kept] = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    return dgate, scale


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
def _bits(words):
    return np.array(words, np.uint32).view(np.float32)


def special_values():
    """one of each kind the definition speaks of, ties included: adjacent -0 / +0, both infinities, NaNs of both signs and
    different payloads, subnormals of both signs, negatives next to positives, neighbours one ulp apart"""
    one = np.float32(1.0)
    return np.concatenate([
        _bits([0x80000000, 0x00000000, 0x00000000, 0x80000000]),                      # -0 +0 +0 -0: four equal scores
        np.array([np.inf, -np.inf, np.inf, -np.inf], np.float32),
        _bits([0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFF800001, 0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF]),   # NaNs, quiet and signalling
        _bits([0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00000002]),          # subnormals
        np.array([-1.5, 1.5, -1.5, 1.5, -3.0e38, 3.0e38], np.float32),
        np.array([one, np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0)), -one, np.nextafter(-one, np.float32(0))],
                 np.float32),
        _bits([0x00800000, 0x80800000]),                                              # the smallest normals
    ]).astype(np.float32)


def _scores(r, n, distinct=None):
    """n scores; distinct: drawn from that many values, so that ties abound"""
    if distinct is None:
        return r.standard_normal(n).astype(np.float32)
    return r.standard_normal(distinct).astype(np.float32)[r.integers(0, distinct, n)]


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _with_specials(r, n):
    """n scores that hold every special value, shuffled, the rest drawn with ties"""
    sp = special_values()
    assert n >= sp.size
    s = np.concatenate([sp, _scores(r, n - sp.size, distinct=7)])
    return s.view(np.uint32)[r.permutation(n)].view(np.float32)


SIZES = (0, 1, 2, 63, 64, 65, 128, 129)


def _sizes_case(seed, sizes, **kw):
    r = _rng(seed)
    off = _offsets(sizes)
    return dict(dict(score=_scores(r, int(off[-1]), distinct=9), offsets=off, k=None, ratio=0.5, min_score=None), **kw)


def _three_tiles(seed, distinct):
    r = _rng(seed)
    n = 2 * TILE + 9
    s = np.full(n, np.float32(0.25)) if distinct == 1 else np.array([-1.0, 0.5, 2.0], np.float32)[r.integers(0, 3, n)]
    return dict(score=s, offsets=_offsets([n]), k=n // 2 + 3, ratio=None, min_score=None)


def _specials_case(seed, n, **kw):
    r = _rng(seed)
    return dict(dict(score=_with_specials(r, n), offsets=_offsets([n]), k=n, ratio=None, min_score=None), **kw)


def _small_graphs(seed, B, top, **kw):
    r = _rng(seed)
    sizes = r.integers(0, top + 1, B)
    off = _offsets(sizes)
    return dict(dict(score=_scores(r, int(off[-1]), distinct=5), offsets=off, k=3, ratio=None, min_score=None), **kw)


def _mixed(seed, **kw):
    """wave and sort graphs side by side, odd sizes, an empty one"""
    r = _rng(seed)
    sizes = [7, 0, 131, 33, 65, 1, 64, 99]
    off = _offsets(sizes)
    return dict(dict(score=_scores(r, int(off[-1]), distinct=11), offsets=off, k=None, ratio=None, min_score=None), **kw)


def _min_score_case(which):
    c = _mixed(31)
    s, off = c["score"], c["offsets"]
    sizes = np.diff(off)
    if which == "above":                                              # above every score of graph 3 (131 vertices), not of the others
        s = s.copy()
        g = 2
        s[off[g]:off[g + 1]] = np.minimum(s[off[g]:off[g + 1]], np.float32(-0.5))
        s[off[3]] = np.float32(0.75)
        return dict(c, score=s, k=sizes.astype(np.int32), min_score=0.0)
    if which == "equal":
        return dict(c, k=sizes.astype(np.int32), min_score=float(np.sort(np.unique(s))[3]))
    if which == "nans":
        s = s.copy()
        s[::5] = _bits([0x7FC00000])[0]
        s[1::7] = _bits([0xFFC00123])[0]
        return dict(c, score=s, k=sizes.astype(np.int32), min_score=-10.0)
    raise KeyError(which)


_CASES = {
    "sizes 0 1 2 63 64 65 128 129": lambda: _sizes_case(11, SIZES),
    "the same sizes reversed": lambda: _sizes_case(12, SIZES[::-1]),
    "B = 1": lambda: dict(score=_scores(_rng(13), 200, distinct=20), offsets=_offsets([200]), k=17, ratio=None, min_score=None),
    "B = 1, wave": lambda: dict(score=_scores(_rng(14), 37, distinct=6), offsets=_offsets([37]), k=9, ratio=None, min_score=None),
    "300 small graphs": lambda: _small_graphs(15, 300, 40),
    "three tiles, three values": lambda: _three_tiles(16, 3),
    "three tiles, all equal": lambda: _three_tiles(17, 1),
    "special values, wave": lambda: _specials_case(18, 64),
    "special values, sort": lambda: _specials_case(19, 150),
    "special values, sort, k small": lambda: _specials_case(20, 150, k=11),
    "special values, wave, min_score -0": lambda: _specials_case(21, 60, min_score=-0.0),
    "special values, sort, min_score -inf": lambda: _specials_case(22, 97, min_score=float("-inf")),
    "special values, sort, min_score NaN": lambda: _specials_case(23, 97, min_score=float("nan")),
    "k = 0": lambda: _mixed(24, k=0),
    "k = 1": lambda: _mixed(25, k=1),
    "k = n_g": lambda: (lambda c: dict(c, k=np.diff(c["offsets"]).astype(np.int32)))(_mixed(26)),
    "k beyond n_g": lambda: _mixed(27, k=1000),
    "k per graph": lambda: _mixed(28, k=np.array([3, 5, 70, 0, 65, 2, 1, 200], np.int32)),
    "ratio 0.5 on odd sizes": lambda: _mixed(29, ratio=0.5),
    "ratio 1": lambda: _mixed(30, ratio=1.0),
    "min_score above a graph's scores": lambda: _min_score_case("above"),
    "min_score equal to a score": lambda: _min_score_case("equal"),
    "min_score with NaNs": lambda: _min_score_case("nans"),
    "NaNs kept last": lambda: (lambda c: dict(c, min_score=None))(_min_score_case("nans")),
    "every graph at most 64": lambda: _small_graphs(32, 40, 64, k=None, ratio=0.5),
    "three tiles and small graphs": lambda: (lambda a, b: dict(score=np.concatenate([b["score"][:b["offsets"][5]], a["score"],
                                                                                    b["score"][b["offsets"][5]:]]),
                                                               offsets=_offsets(np.concatenate([np.diff(b["offsets"])[:5], [a["score"].size],
                                                                                                np.diff(b["offsets"])[5:]])),
                                                               k=None, ratio=0.5, min_score=None))(_three_tiles(33, 3), _small_graphs(34, 12, 90)),
    "n = 0, B = 3": lambda: dict(score=np.zeros(0, np.float32), offsets=np.zeros(4, np.int32), k=2, ratio=None, min_score=None),
    "B = 0": lambda: dict(score=np.zeros(0, np.float32), offsets=np.zeros(1, np.int32), k=2, ratio=None, min_score=None),
}
NAMES = tuple(_CASES)


@functools.lru_cache(None)
def _case(name):
    c = _CASES[name]()
    for a in (c["score"], c["offsets"]):
        a.setflags(write=False)
    return c


def case(name):
    """the named input: dict(score, offsets, k, ratio, min_score), exactly one of k and ratio given; the arrays are read-only"""
    return dict(_case(name))


def counts_of(c):
    """k as the library takes it: an int, or int32 [B]"""
    if c["ratio"] is not None:
        return ratio_counts(np.diff(c["offsets"].astype(np.int64)), c["ratio"])
    return c["k"]


@functools.lru_cache(None)
def expected(name):
    """select() on the named case, computed once"""
    c = case(name)
    return select(c["score"], c["offsets"], counts_of(c), c["min_score"])


def rows_case(seed, n, m_drop, F, gated=True, special=False):
    """(cluster, selected, x, gate, dy): a selection of n vertices that drops m_drop of them, features F wide; special: x and the
    gate hold -0, infinities, subnormals and NaNs with payloads"""
    r = _rng(seed)
    keep = np.sort(r.permutation(n)[:n - m_drop])
    m = keep.size
    cluster = np.zeros(n, np.int32)
    cluster[keep] = np.arange(1, m + 1)
    x = r.standard_normal((n, F)).astype(np.float32)
    gate = r.standard_normal(n).astype(np.float32) if gated else None
    dy = r.standard_normal((m, F)).astype(np.float32)
    if special:
        odd = _bits([0x80000000, 0x7F800000, 0xFF800000, 0x00000003, 0x80000400, 0x7FC01234, 0xFFC00001, 0x7F800055])
        flat = x.reshape(-1)
        at = r.permutation(flat.size)[:4 * odd.size]
        flat.view(np.uint32)[at] = np.tile(odd.view(np.uint32), 4)
        if gated:
            godd = _bits([0x80000000, 0x7F800000, 0x00000007, 0x80000009, 0x00000000])
            gate.view(np.uint32)[r.permutation(n)[:godd.size]] = godd.view(np.uint32)
    return cluster, (keep + 1).astype(np.int32), x, gate, dy
