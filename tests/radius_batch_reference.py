"""The yardstick of the batched radius-graph builder (athena_mp_radius_pairs_batched, athena_amd/csrc/radius_graph.hip): the
sentence of include/athena_mp.h -- the concatenation, in cloud order, of what the single-cloud definition gives for each slice
points[offsets[b] : offsets[b+1]], with offsets[b] added to both indices.  radius_reference.reference_pairs per slice; nothing of
its own decides a pair.  test_radius_batch.py pins it to an all-pairs evaluation of fp32_keep under a same-cloud mask."""
import numpy as np

from radius_reference import fp32_keep, reference_pairs


def reference_pairs_batched(p, offsets, r):
    """p float32 [n, dim], offsets [B + 1] -> (i, j, coords, edge_offsets): 0-based global pairs i < j of one cloud in
    lexicographic order, coords = p[i] - p[j], edge_offsets int64 [B + 1] = where each cloud's pairs start"""
    assert p.dtype == np.float32 and p.ndim == 2
    off = np.asarray(offsets, np.int64)
    assert off.ndim == 1 and off.size >= 1 and off[0] == 0 and off[-1] == p.shape[0] and np.all(np.diff(off) >= 0)
    ii, jj, cc = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros((0, p.shape[1]), np.float32)]
    eoff = np.zeros(off.size, np.int64)
    for b in range(off.size - 1):
        i, j, c = reference_pairs(np.ascontiguousarray(p[off[b]:off[b + 1]]), r)
        ii.append(i + off[b])
        jj.append(j + off[b])
        cc.append(c)
        eoff[b + 1] = eoff[b] + i.size
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(cc), eoff


def all_pairs_batched(p, offsets, r):
    """every i < j of the whole batch evaluated with fp32_keep, kept only where both ends lie in one cloud (small n only)"""
    off = np.asarray(offsets, np.int64)
    cloud = np.searchsorted(off, np.arange(p.shape[0]), side="right") - 1           # the last b with off[b] <= i
    i, j = np.triu_indices(p.shape[0], 1)
    k = fp32_keep(p, i, j, r) & (cloud[i] == cloud[j])
    i, j = i[k].astype(np.int64), j[k].astype(np.int64)
    return i, j, p[i] - p[j]


def edge_offsets_of(i, offsets):
    """edge_offsets[b] = the number of pairs whose first index is below offsets[b]"""
    return np.searchsorted(np.asarray(i, np.int64), np.asarray(offsets, np.int64), side="left").astype(np.int64)


def cloud_sizes(rng, B, mean=18.0, sd=3.0, lo=4, hi=29):
    """clip(round(N(mean, sd)), lo, hi): the sizes of a dataset of small clouds"""
    return np.clip(np.rint(rng.normal(mean, sd, B)), lo, hi).astype(np.int64)
