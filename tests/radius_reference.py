"""The yardstick of the radius-graph builder (athena_amd/csrc/radius_graph.hip): the definition of include/athena_mp.h,
term by term in float32, over the candidates of a float64 k-d tree.

The candidate radius is safe: the fp32 sum of at most three squares is within a few 2^-24 (relative) of the exact one, so
a pair the predicate keeps has an exact distance below radius * (1 + 2^-20).  test_radius_graph.py pins reference_pairs to
an all-pairs evaluation of fp32_keep."""
import numpy as np


def fp32_keep(p, i, j, r):
    """the definition: every multiply and add rounded to float32 on its own, left to right"""
    r2 = np.float32(r) * np.float32(r)
    d = p[i] - p[j]
    s = d[:, 0] * d[:, 0]
    for a in range(1, p.shape[1]):
        s = s + d[:, a] * d[:, a]
    return s <= r2


def reference_pairs(p, r):
    """p float32 [n, dim] -> (i, j, coords): 0-based pairs i < j in lexicographic order, coords = p[i] - p[j]"""
    from scipy.spatial import cKDTree

    assert p.dtype == np.float32 and p.ndim == 2
    if p.shape[0] < 2:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros((0, p.shape[1]), np.float32)
    cand = cKDTree(p.astype(np.float64)).query_pairs(float(np.float32(r)) * (1 + 2.0 ** -20), output_type="ndarray")
    i, j = cand.min(1).astype(np.int64), cand.max(1).astype(np.int64)
    k = fp32_keep(p, i, j, r)
    i, j = i[k], j[k]
    o = np.lexsort((j, i))
    i, j = i[o], j[o]
    return i, j, p[i] - p[j]


def all_pairs(p, r):
    """every i < j evaluated with fp32_keep (small n only)"""
    i, j = np.triu_indices(p.shape[0], 1)
    k = fp32_keep(p, i, j, r)
    i, j = i[k].astype(np.int64), j[k].astype(np.int64)
    return i, j, p[i] - p[j]


def degree_radius(n, mean_degree, dim):
    """radius for which a uniform cloud of n points in the unit box has about this mean degree"""
    vol = {1: 2.0, 2: np.pi, 3: 4.0 / 3.0 * np.pi}[dim]
    return float((mean_degree / (n * vol)) ** (1.0 / dim))
