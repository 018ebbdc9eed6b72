"""The yardstick of the periodic-structure graph builder (athena_amd/csrc/periodic_graph.hip): the definition of
include/athena_mp.h, term by term in numpy float32 (numpy's fp32 sqrt and divide are correctly rounded), over EVERY atom pair
i <= j and every shift of a range that is `extra` (default three) wider per axis than the bound requires:

    every kept shift has |a| <= floor(h_a + 1/2),   h_a = cutoff_max * |L_b x L_c| / |det L|      (float64 here)

reference_bounds_edges transcribes the loop bounds of the reference itself (get_graph_from_basis,
example/example_library/src/mod_read_chemical_graphs.f90:230-251: -amax .. amax+1 with amax = ceiling(cutoff_max / |L_a|)),
which are not sufficient for skewed cells."""
import numpy as np

F32 = np.float32
CHUNK = 1 << 21                      # candidates evaluated at a time


def half_ranges(lat, cutoff_max, pbc=(1, 1, 1)):
    """floor(h_a + 1/2) per axis, 0 on an open axis (float64 from the float32 lattice)"""
    L = np.asarray(lat, np.float32).astype(np.float64)
    out = [0, 0, 0]
    if not any(pbc):
        return out
    det = float(np.dot(L[0], np.cross(L[1], L[2])))
    for a in range(3):
        if pbc[a]:
            h = float(F32(cutoff_max)) * float(np.linalg.norm(np.cross(L[(a + 1) % 3], L[(a + 2) % 3]))) / abs(det)
            out[a] = int(np.floor(h + 0.5))
    return out


def _edges_over_shifts(frac, lat, cutoff_min, cutoff_max, pbc, lo, hi):
    """one structure, the shifts lo[k] .. hi[k] per axis -> (i, j, shift [E, 3], r [E], x [E, 3]), in (i, j, a, b, c) order"""
    frac = np.ascontiguousarray(frac, F32).reshape(-1, 3)
    L = np.ascontiguousarray(lat, F32).reshape(3, 3)
    cmin, cmax = F32(cutoff_min), F32(cutoff_max)
    m = frac.shape[0]
    i, j = np.triu_indices(m)                                             # i <= j, lexicographic
    axes = [np.arange(lo[k], hi[k] + 1, dtype=np.int32) for k in range(3)]
    sh = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)     # (a, b, c) lexicographic
    shf = sh.astype(F32)
    S = sh.shape[0]
    got = []
    step = max(1, CHUNK // S)
    with np.errstate(over="ignore", invalid="ignore"):
        for p0 in range(0, i.size, step):
            ii, jj = i[p0:p0 + step], j[p0:p0 + step]
            f = frac[ii] - frac[jj]
            w = f.copy()
            for k in range(3):
                if pbc[k]:
                    w[:, k] = f[:, k] - np.ceil(f[:, k] - F32(0.5))
            v = w[:, None, :] + shf[None, :, :]                             # [P, S, 3] float32
            x = np.empty_like(v)
            for c in range(3):
                x[..., c] = ((v[..., 0] * L[0, c]) + v[..., 1] * L[1, c]) + v[..., 2] * L[2, c]
            s = ((x[..., 0] * x[..., 0]) + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2]
            r = np.sqrt(s)
            assert r.dtype == F32
            pk, sk = np.nonzero((r > cmin) & (r < cmax))                    # row-major: pair, then shift
            got.append((ii[pk], jj[pk], sh[sk], r[pk, sk], x[pk, sk]))
    if not got:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros((0, 3), np.int32), np.zeros(0, F32), np.zeros((0, 3), F32)
    return tuple(np.concatenate([g[k] for g in got]) for k in range(5))


def structure_edges(frac, lat, cutoff_min, cutoff_max, pbc=(1, 1, 1), extra=3):
    """the definition on one structure over the bound's range widened by `extra` on every periodic axis"""
    R = half_ranges(lat, cutoff_max, pbc)
    hi = [R[k] + extra if pbc[k] else 0 for k in range(3)]
    return _edges_over_shifts(frac, lat, cutoff_min, cutoff_max, pbc, [-h for h in hi], hi)


def reference_bounds_edges(frac, lat, cutoff_min, cutoff_max):
    """the same predicate over the REFERENCE's loop bounds: -amax .. amax + 1, amax = ceiling(cutoff_max / |L_a|) in real32"""
    L = np.ascontiguousarray(lat, F32).reshape(3, 3)
    amax = []
    for a in range(3):
        modu = np.sqrt(((L[a, 0] * L[a, 0]) + L[a, 1] * L[a, 1]) + L[a, 2] * L[a, 2])
        amax.append(int(np.ceil(F32(cutoff_max) / modu)))
    return _edges_over_shifts(frac, lat, cutoff_min, cutoff_max, (1, 1, 1), [-a for a in amax], [a + 1 for a in amax])


def assemble(per_structure, offsets, cutoff_max):
    """per-structure results of structure_edges -> the arrays of athena_mp_periodic_pairs for the batch:
    dict(pairs [2, E] int32 1-based global, feature [E], vec [E, 3], shift [E, 3], first_count [n], edge_offsets [B + 1])"""
    offsets = np.asarray(offsets, np.int64)
    B = offsets.size - 1
    assert len(per_structure) == B
    eoff = np.zeros(B + 1, np.int64)
    eoff[1:] = np.cumsum([e[0].size for e in per_structure])
    E, n = int(eoff[-1]), int(offsets[-1])
    pairs = np.zeros((2, E), np.int32, order="F")
    feature, vec, shift = np.zeros(E, F32), np.zeros((E, 3), F32), np.zeros((E, 3), np.int32)
    first = np.zeros(n, np.int32)
    for s, (i, j, sh, r, x) in enumerate(per_structure):
        e = slice(eoff[s], eoff[s + 1])
        pairs[0, e] = i + offsets[s] + 1
        pairs[1, e] = j + offsets[s] + 1
        feature[e] = r / F32(cutoff_max)
        vec[e], shift[e] = x, sh
        first[offsets[s]:offsets[s + 1]] = np.bincount(i, minlength=int(offsets[s + 1] - offsets[s]))
    assert feature.dtype == F32
    return {"pairs": pairs, "feature": feature, "vec": vec, "shift": shift, "first_count": first, "edge_offsets": eoff}


def reference_edges(frac, lat, offsets, cutoff_min, cutoff_max, pbc=(1, 1, 1), extra=3):
    """the whole batch: every structure through structure_edges, assembled"""
    frac = np.ascontiguousarray(frac, F32).reshape(-1, 3)
    lat = np.ascontiguousarray(lat, F32).reshape(-1, 3, 3)
    per = [structure_edges(frac[offsets[s]:offsets[s + 1]], lat[s], cutoff_min, cutoff_max, pbc, extra) for s in range(lat.shape[0])]
    return assemble(per, offsets, cutoff_max)


def random_cell(rng, kind, max_range=12):
    """a float32 lattice: 'cubic' (edge 4.5 - 8), 'skewed' (strongly sheared, volume >= 3: half-ranges from 5 to max_range at
    cutoff 3) or 'small' (edges 1.2 - 2.4, below the cutoff: self images, several edges per pair)"""
    if kind == "cubic":
        return (np.eye(3) * rng.uniform(4.5, 8.0)).astype(F32)
    if kind == "small":
        L = np.diag(rng.uniform(1.2, 2.4, 3)) + rng.uniform(-0.15, 0.15, (3, 3))
        return L.astype(F32)
    assert kind == "skewed"
    while True:
        L = np.diag(rng.uniform(1.5, 3.0, 3))
        L[1] += rng.uniform(2.0, 4.0) * L[0] * rng.choice([-1, 1])
        L[2] += rng.uniform(2.0, 4.0) * L[1] * rng.choice([-1, 1]) + rng.uniform(-1, 1) * L[0]
        L = L.astype(F32)
        if abs(np.linalg.det(L.astype(np.float64))) >= 3.0 and 5 <= max(half_ranges(L, 3.0)) <= max_range:
            return L
