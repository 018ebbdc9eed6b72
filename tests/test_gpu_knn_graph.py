"""GPU: k-nearest-neighbour graphs of point clouds on the device (athena_amd/csrc/knn_graph.hip; athena_mp_knn_pairs_batched,
athena_mp_knn_pairs, athena_mp_knn_graph_batched_host, athena_mp_knn_stats and their Python / Fortran mirrors) against the
yardstick of tests/knn_reference.py: brute force where the cloud is small, the large form (pinned to brute force by
test_knn_graph.py) otherwise.  Integers and single fp32 subtractions: every comparison of nbr, pair lists, coords, edge_offsets and
handle arrays is np.array_equal / torch.equal on whole arrays.  The only tolerance is the project's 1e-5 where the GNO layer is held
to oracle/layers.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import batch_reference as br
import geometry_reference as gr
import knn_reference as kr
import oracle_layers as ol
from helpers import assert_close, csr_from_index_list
from radius_reference import reference_pairs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "knn_graph_run")
INF = float("inf")


def _call(pts, off, k, r=None, mode=0, nbr=None, pairs=None, coords=None, capacity=0, n=None, dim=None, B=None):
    """athena_mp_knn_pairs_batched on a device tensor -> (E, edge_offsets)"""
    from athena_amd import _capi

    off = np.ascontiguousarray(off, np.int32)
    B = off.size - 1 if B is None else B
    _capi.use_torch_stream()
    E = C.c_int64(-1)
    eoff = np.full(max(B, 0) + 1, -9, np.int64)
    ptr = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
    _capi.call("athena_mp_knn_pairs_batched", int(B), int(pts.shape[0] if n is None else n), off.ctypes.data_as(C.c_void_p),
               int(pts.shape[1] if dim is None else dim), ptr(pts), int(k), INF if r is None else float(r), int(mode), ptr(nbr),
               ptr(pairs), ptr(coords), int(capacity), eoff.ctypes.data_as(C.c_void_p), C.byref(E))
    return E.value, eoff


def _stats():
    from athena_amd import _capi

    out = np.zeros(4, np.int64)
    _capi.call("athena_mp_knn_stats", out.ctypes.data_as(C.c_void_p))
    return out


def _gpu(dev, p, off, k, r=None, mode=0):
    """size query, then fill -> (nbr, i, j, coords, edge_offsets) 0-based numpy (nbr as the library writes it), plus the raw tensors"""
    import torch

    pts = torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dev)
    q, eoff_q = _call(pts, off, k, r, mode)
    nbr = torch.full((pts.shape[0], k), -7, dtype=torch.int32, device=dev)
    pairs = torch.full((q, 2), -7, dtype=torch.int32, device=dev)
    coords = torch.full((q, pts.shape[1]), np.nan, dtype=torch.float32, device=dev)
    E, eoff = _call(pts, off, k, r, mode, nbr, pairs, coords, q)
    torch.cuda.synchronize()
    assert E == q and np.array_equal(eoff, eoff_q), "the size query and the fill disagree"
    pr = pairs.cpu().numpy().astype(np.int64)
    return nbr.cpu().numpy(), pr[:, 0] - 1, pr[:, 1] - 1, coords.cpu().numpy(), eoff, (nbr, pairs, coords)


def _check(dev, p, off, k, r, want_nbr, modes=(0, 1)):
    """both modes against the graph the yardstick's neighbour lists define; returns the pair counts"""
    p = np.ascontiguousarray(p, np.float32)
    counts = []
    for mode in modes:
        ri, rj, rc, reoff = kr.graph_of(want_nbr, p, off, mode)
        nbr, gi, gj, gc, geoff, _ = _gpu(dev, p, off, k, r, mode)
        print(f"B = {len(off) - 1}, n = {p.shape[0]}, dim = {p.shape[1]}, k = {k}, radius = {r}, mode = {mode}: {ri.size} reference "
              f"pairs, {gi.size} device pairs; stats {_stats().tolist()}")
        assert nbr.dtype == want_nbr.dtype and np.array_equal(nbr, want_nbr), "nbr differs from the yardstick"
        assert np.array_equal(gi, ri) and np.array_equal(gj, rj), "pair list differs from the yardstick"
        assert gc.dtype == rc.dtype and np.array_equal(gc, rc), "coords differ from the yardstick"
        assert geoff.dtype == reoff.dtype and np.array_equal(geoff, reoff), "edge_offsets differ from the yardstick"
        counts.append(int(ri.size))
    return counts


CASES = {c[0]: c[1:] for c in kr.shape_cases()}


@functools.lru_cache(None)
def _brute(name):
    p, off, k, r = CASES[name]
    return kr.brute_force_neighbours(p, off, k, r)


# ---- edges of the definition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_no_point_one_point_two_points(dev, dim):
    import torch

    none = torch.zeros((0, dim), dtype=torch.float32, device=dev)
    assert _call(none, [0], 3)[0] == 0 and _call(none, [0], 3)[1].tolist() == [0]
    E0, e0 = _call(none, [0, 0, 0], 3)
    assert E0 == 0 and e0.tolist() == [0, 0, 0]
    p = kr._rng(dim).random((2, dim)).astype(np.float32)
    assert _check(dev, p[:1], [0, 1], 3, None, np.zeros((1, 3), np.int32)) == [0, 0]
    want = np.array([[2, 0, 0], [1, 0, 0]], np.int32)
    assert _check(dev, p, [0, 2], 3, None, want) == [1, 1]
    assert _check(dev, np.repeat(p[:1], 2, 0), [0, 2], 1, None, want[:, :1]) == [1, 1]      # coincident: s = 0, joined
    assert _check(dev, p, [0, 1, 2], 3, None, np.zeros((2, 3), np.int32)) == [0, 0]           # two clouds of one point


def test_fewer_candidates_than_k_pads_nbr(dev):
    p, off, k, r = CASES["k >= n"]
    want = _brute("k >= n")
    assert np.all(want[:, :4] > 0) and np.all(want[:, 4:] == 0)
    assert _check(dev, p, off, k, r, want) == [10, 10]


@pytest.mark.parametrize("k", [1, 64])
def test_smallest_and_largest_k(dev, k):
    p = kr._rng(9).random((200, 3)).astype(np.float32)
    union, mutual = _check(dev, p, [0, 200], k, None, kr.brute_force_neighbours(p, [0, 200], k))
    assert mutual < union


def test_refuses_bad_input_and_stays_usable(dev):
    import torch
    from athena_amd import DeviceGraph, _capi

    rng = kr._rng(14)
    off = kr.offsets_of([700, 0, 900, 5, 1400])
    p = rng.random((int(off[-1]), 3)).astype(np.float32)
    want = kr.large_form_neighbours(p, off, 6)
    good = kr.graph_of(want, p, off, 0)[0].size
    pts = torch.from_numpy(p).to(dev)
    assert _call(pts, off, 6)[0] == good
    err = _capi.AthenaMPError
    for k in (65, 0, -1):
        with pytest.raises(err, match=r"k = %d outside \[1,64\]" % k):
            _call(pts, off, k)
    with pytest.raises(err, match=r"k = 65 outside \[1,64\]"):
        DeviceGraph.from_point_clouds_knn(pts, off, 65)
    for bad in (0.0, -1.0, float("nan"), -INF):
        with pytest.raises(err, match=r"radius = .* is not a positive number"):
            _call(pts, off, 6, bad)
    for bad in (2, -1):
        with pytest.raises(err, match=r"mode = %d is neither 0 \(union\) nor 1 \(mutual\)" % bad):
            _call(pts, off, 6, mode=bad)
    with pytest.raises(err, match=r"dim = 4 outside \[1,3\]"):
        _call(torch.zeros((10, 4), device=dev), [0, 10], 6)
    with pytest.raises(err, match=r"dim = 0 outside \[1,3\]"):
        _call(pts, off, 6, dim=0)
    # bad offsets: the wording of the batched radius builder
    with pytest.raises(err, match=r"n_clouds = -1 is negative"):
        _call(pts, off, 6, B=-1)
    with pytest.raises(err, match=r"offsets\(1\) = 2, not 0"):
        _call(pts, np.concatenate([[2], off[1:]]), 6)
    down = off.copy(); down[3] = down[2] - 1
    with pytest.raises(err, match=r"cloud 3: offsets descend from %d to %d" % (down[2], down[3])):
        _call(pts, down, 6)
    with pytest.raises(err, match=r"offsets end at %d, the batch has %d points" % (off[-1], off[-1] - 1)):
        _call(pts, off, 6, n=int(off[-1]) - 1)
    pairs = torch.empty((good, 2), dtype=torch.int32, device=dev)
    coords = torch.empty((good, 3), dtype=torch.float32, device=dev)
    with pytest.raises(err, match=r"buffers hold %d pairs, the graph has %d" % (good - 1, good)):
        _call(pts, off, 6, pairs=pairs, coords=coords, capacity=good - 1)
    for value, where, cloud in ((np.nan, (1234, 1), 3), (np.inf, (7, 2), 1), (-np.inf, (1601, 0), 4)):
        q = p.copy()
        q[where] = value
        q[3004, 0] = np.nan                                                # a later one
        text = "-?nan" if np.isnan(value) else "-inf" if value < 0 else "inf"
        with pytest.raises(err, match=r"cloud %d: points\(%d,%d\) = %s is not finite" % (cloud, where[1] + 1, where[0] + 1, text)):
            _call(torch.from_numpy(q).to(dev), off, 6)
    # n * k >= 2^31 is refused before anything is read: the pointer is never followed
    with pytest.raises(err, match=r"n \* k = %d: more than 2\^31 neighbour entries" % (40_000_000 * 64)):
        _call(pts, [0, 40_000_000], 64, n=40_000_000)
    _check(dev, p, off, 6, None, want)                                     # the library is usable afterwards


# ---- ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice 1-D 64", "lattice 12 x 12", "lattice 6 x 6 x 6, k = 6", "lattice 6 x 6 x 6, k = 7",
                                  "40 coincident among 200", "1e6 + lattice 12 x 12", "1e6 + 1-D 200", "1e6 + uniform, spacing 1"])
def test_ties_are_broken_by_index(dev, name):
    p, off, k, r = CASES[name]
    want = _brute(name)
    union, mutual = _check(dev, p, off, k, r, want)
    assert mutual <= union
    if name == "lattice 6 x 6 x 6, k = 7":
        # an inner vertex has six neighbours at s = 1 and twelve at s = 2: the seventh is the smallest index among the twelve
        i = 2 * 36 + 2 * 6 + 2
        s = kr.sq_dist(p[i], p[want[i] - 1])
        assert s.tolist() == [1] * 6 + [2] and want[i, 6] - 1 == min(j for j in range(216) if kr.sq_dist(p[i], p[j]) == 2)


# ---- a range that is not known in advance ---------------------------------------------------------------------------------------
def test_the_smaller_cluster_crosses_the_gap(dev):
    p, off, k, r = CASES["two clusters"]
    want = _brute("two clusters")
    assert np.all((want[:20] > 20).sum(1) == 6) and np.all(want[20:] > 20)                    # 19 at home, 6 across; 30 stay home
    _check(dev, p, off, k, r, want)
    queries, cand, cells, shell = _stats()
    print(f"two clusters: {cand} candidates, {cells} cells, largest shell {shell}")
    assert queries == 50 and shell > 1


@pytest.mark.parametrize("name", ["planar in 3-D", "1000 : 1 : 1 box"] + [f"cell boundaries dim {d}" for d in (1, 2, 3)])
def test_degenerate_boxes_and_points_on_cell_boundaries(dev, name):
    p, off, k, r = CASES[name]
    _check(dev, p, off, k, r, _brute(name))


# ---- bulk ----------------------------------------------------------------------------------------------------------------------
N_BULK = 5000


@functools.lru_cache(None)
def _bulk(dim, k):
    p = kr._rng(100 + dim).random((N_BULK, dim)).astype(np.float32)
    return p, kr.large_form_neighbours(p, [0, N_BULK], k)


@pytest.mark.parametrize("k", [1, 8, 33, 64])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_uniform_cloud_against_the_large_form(dev, dim, k):
    p, want = _bulk(dim, k)
    union, mutual = _check(dev, p, [0, N_BULK], k, None, want)
    assert mutual < union                                                  # the two modes differ
    queries, cand, cells, shell = _stats()
    print(f"dim {dim}, k {k}: {cand / queries:.1f} candidates and {cells / queries:.1f} cells per query, largest shell {shell}")
    assert queries == N_BULK and 0 < cand < N_BULK * N_BULK / 8            # the search was pruned: brute force examines n * n


# ---- the cap -------------------------------------------------------------------------------------------------------------------
def test_cap_cuts_some_rows_and_k_cuts_others(dev):
    p, off, k, r = kr.cap_case()
    degree = (kr.large_form_neighbours(p, off, 64, r) > 0).sum(1)
    assert (degree > k).mean() >= 0.1 and (degree < k).mean() >= 0.1
    want = kr.large_form_neighbours(p, off, k, r)
    assert np.array_equal((want > 0).sum(1), np.minimum(degree, k))
    union, mutual = _check(dev, p, off, k, r, want)
    assert mutual < union


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_cap_with_a_k_no_row_reaches_is_the_radius_graph(dev, dim):
    """k = 64 and a radius whose largest degree is below 64: the union pair list and coords are athena_mp_radius_pairs', byte for byte"""
    import torch
    from athena_amd import _capi
    from radius_reference import degree_radius

    n = 3000
    p = kr._rng(200 + dim).random((n, dim)).astype(np.float32)
    r = degree_radius(n, 12.0, dim)
    ri, rj, rc = reference_pairs(p, r)
    assert np.bincount(np.concatenate([ri, rj]), minlength=n).max() < 64
    pts = torch.from_numpy(p).to(dev)
    _capi.use_torch_stream()
    E = C.c_int64()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    _capi.call("athena_mp_radius_pairs", n, dim, ptr(pts), float(r), None, None, 0, C.byref(E))
    rp = torch.empty((E.value, 2), dtype=torch.int32, device=dev)
    rco = torch.empty((E.value, dim), dtype=torch.float32, device=dev)
    _capi.call("athena_mp_radius_pairs", n, dim, ptr(pts), float(r), ptr(rp), ptr(rco), E.value, C.byref(E))
    _, _, _, _, _, (nbr, pairs, coords) = _gpu(dev, p, [0, n], 64, r, 0)
    assert E.value == ri.size > n and torch.equal(pairs, rp) and torch.equal(coords.view(torch.int32), rco.view(torch.int32))
    _, mi, mj, _, _, _ = _gpu(dev, p, [0, n], 64, r, 1)                    # nobody is cut by k: every choice is mutual
    assert np.array_equal(mi, ri) and np.array_equal(mj, rj)


# ---- batches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_batch_equals_the_single_cloud_entry_per_slice(dev, mode):
    import torch
    from athena_amd import _capi

    p, off, k, r = CASES["batch"]
    _check(dev, p, off, k, r, _brute("batch"), modes=(mode,))
    nbr, gi, gj, gc, geoff, _ = _gpu(dev, p, off, k, r, mode)
    parts, eoff = {"nbr": [], "i": [], "j": [], "c": []}, [0]
    _capi.use_torch_stream()
    for b in range(off.size - 1):
        m = int(off[b + 1] - off[b])
        pts = torch.from_numpy(np.ascontiguousarray(p[off[b]:off[b + 1]])).to(dev)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
        one_nbr = torch.full((m, k), -7, dtype=torch.int32, device=dev)
        pairs = torch.empty((m * k, 2), dtype=torch.int32, device=dev)
        coords = torch.empty((m * k, 3), dtype=torch.float32, device=dev)
        E = C.c_int64()
        _capi.call("athena_mp_knn_pairs", m, 3, ptr(pts), k, INF, mode, ptr(one_nbr), ptr(pairs), ptr(coords), m * k, C.byref(E))
        torch.cuda.synchronize()
        pr = pairs[:E.value].cpu().numpy().astype(np.int64)
        one = one_nbr.cpu().numpy()
        parts["nbr"].append(np.where(one > 0, one + off[b], 0))
        parts["i"].append(pr[:, 0] - 1 + off[b]); parts["j"].append(pr[:, 1] - 1 + off[b]); parts["c"].append(coords[:E.value].cpu().numpy())
        eoff.append(eoff[-1] + E.value)
    assert np.array_equal(np.concatenate(parts["nbr"]), nbr)
    assert np.array_equal(np.concatenate(parts["i"]), gi) and np.array_equal(np.concatenate(parts["j"]), gj)
    assert np.array_equal(np.concatenate(parts["c"]), gc) and np.array_equal(np.asarray(eoff, np.int64), geoff)
    assert geoff[-1] > 1000 and geoff[2] == geoff[3] and geoff[5] - geoff[4] == 1


@functools.lru_cache(None)
def _small_clouds(dim):
    """3 000 clouds of 4 .. 29 points in the unit box and the yardstick's neighbour lists at k = 8"""
    rng = kr._rng(50 + dim)
    off = kr.offsets_of(rng.integers(4, 30, 3000))
    p = rng.random((int(off[-1]), dim)).astype(np.float32)
    return p, off, kr.large_form_neighbours(p, off, 8)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_many_small_clouds(dev, dim):
    p, off, want = _small_clouds(dim)
    assert np.any((want > 0).sum(1) < 8) and np.any((want > 0).sum(1) == 8)                   # clouds below and above k + 1 points
    _check(dev, p, off, 8, None, want)


def test_two_builds_are_byte_identical(dev):
    import torch

    p, off, want = _small_clouds(3)
    for mode in (0, 1):
        a = _gpu(dev, p, off, 8, None, mode)
        b = _gpu(dev, p, off, 8, None, mode)
        assert np.array_equal(a[4], b[4])
        for x, y in zip(a[5], b[5]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # capacity n * k always suffices, and either output alone gives the same bytes
    nbr, pairs, coords = a[5]
    pts = torch.from_numpy(p).to(dev)
    E, T = pairs.shape[0], p.shape[0] * 8
    only_p = torch.full((T, 2), -7, dtype=torch.int32, device=dev)
    only_c = torch.full((T, 3), np.nan, dtype=torch.float32, device=dev)
    assert _call(pts, off, 8, None, 1, pairs=only_p, capacity=T)[0] == E and _call(pts, off, 8, None, 1, coords=only_c, capacity=T)[0] == E
    torch.cuda.synchronize()
    assert torch.equal(only_p[:E], pairs) and torch.equal(only_c[:E].view(torch.int32), coords.view(torch.int32))
    assert torch.all(only_p[E:] == -7) and torch.all(torch.isnan(only_c[E:]))


# ---- downstream ----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    for n in br.NAMES:
        x, y = a.export(n), b.export(n)
        assert x.shape == y.shape, n
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), f"{n} differs"


@pytest.mark.parametrize("dim,loops,mode,r", [(3, True, "union", None), (3, False, "mutual", None), (2, True, "union", 0.08), (1, False, "union", None)])
def test_handle_from_point_clouds_knn_and_mini_batches_of_it(dev, dim, loops, mode, r):
    import torch
    from athena_amd import DeviceDataset, DeviceGraph
    from athena_amd.graph import graph_type

    rng = kr._rng(90 + dim)
    sizes = [260, 1, 140, 0, 75, 310, 2]
    off = kr.offsets_of(sizes)
    n, k = int(off[-1]), 5
    p = rng.random((n, dim)).astype(np.float32)
    want_nbr = kr.brute_force_neighbours(p, off, k, r)
    ri, rj, rc, reoff = kr.graph_of(want_nbr, p, off, {"union": 0, "mutual": 1}[mode])
    idx = np.asfortranarray(np.stack([ri + 1, rj + 1]).astype(np.int32))
    ref = DeviceGraph.from_edges(n, idx, add_self_loops=loops)
    host = csr_from_index_list(n, idx, self_loops=loops)
    one, coords, voff, eoff, ia, ja, nbr = DeviceGraph.from_point_clouds_knn(p, off, k, r, mode, add_self_loops=loops, want_adjacency=True,
                                                                           want_neighbours=True)
    lean, coords2, voff2, eoff2 = DeviceGraph.from_point_clouds_knn(torch.from_numpy(p).to(dev), off, k, r, mode, add_self_loops=loops)
    assert nbr.is_cuda and nbr.dtype == torch.int32 and np.array_equal(nbr.cpu().numpy(), want_nbr)
    assert coords.is_cuda and coords.shape == (ri.size, dim) and coords.dtype == torch.float32
    assert np.array_equal(coords.cpu().numpy(), rc) and torch.equal(coords, coords2)
    assert voff.dtype == np.int32 and np.array_equal(voff, off) and np.array_equal(voff2, off)
    assert eoff.dtype == np.int64 and np.array_equal(eoff, reoff) and np.array_equal(eoff2, reoff)
    assert np.array_equal(ia, host.adj_ia) and np.array_equal(ja, host.adj_ja)
    assert (one.n_rows, one.nnz, one.n_edge_cols) == (ref.n_rows, ref.nnz, ref.n_edge_cols) == (n, host.nnz, ri.size)
    _same(one, ref)                                                        # all thirteen arrays
    _same(lean, ref)
    # one cloud through from_points_knn
    b0 = slice(0, sizes[0])
    w0 = kr.graph_of(want_nbr[b0], p[b0], [0, sizes[0]], {"union": 0, "mutual": 1}[mode])
    g0, c0, nbr0 = DeviceGraph.from_points_knn(p[b0], k, r, mode, add_self_loops=loops, want_neighbours=True)
    assert np.array_equal(nbr0.cpu().numpy(), want_nbr[b0]) and np.array_equal(c0.cpu().numpy(), w0[2]) and g0.n_edge_cols == w0[0].size
    # the host-array siblings
    d = graph_type(); d.set_num_vertices(n, 1)
    c3, eoff3 = d.generate_knn_batch_adjacency_device(p, off, k, r, mode, add_self_loops=loops)
    assert d.num_edges == ri.size and np.array_equal(c3, rc) and np.array_equal(eoff3, reoff)
    assert np.array_equal(d.adj_ia, host.adj_ia) and np.array_equal(d.adj_ja, host.adj_ja)
    d1 = graph_type(); d1.set_num_vertices(sizes[0], 1)
    assert np.array_equal(d1.generate_knn_adjacency_device(p[b0], k, r, mode, add_self_loops=loops), w0[2])
    # the dataset machinery takes the handle as it is: a selection equals the yardstick of tests/batch_reference.py
    ds = DeviceDataset(one, voff, eoff)
    sel = [5, 2, 2, 0, 3]
    b = ds.select(sel)
    want, cvoff, ceoff, vmap, emap = br.select_reference({name: one.export(name) for name in br.NAMES}, off, reoff, sel)
    assert np.array_equal(b.vertex_offsets, cvoff) and np.array_equal(b.edge_offsets, ceoff)
    for name in br.NAMES:
        assert np.array_equal(b.handle.export(name).view(np.int32), want[name].view(np.int32)), f"{name} differs from the yardstick"
    assert torch.equal(b.take_edges(coords).view(torch.int32), coords[torch.from_numpy(emap).to(dev).long()].view(torch.int32))
    assert ceoff[-1] > 100
    b.close()
    ds.close()
    for g in (one, lean, ref, g0):
        g.close()


@pytest.mark.parametrize("Fi,Fo,d,H,act", [(64, 64, 3, 64, "relu"), (5, 3, 2, 7, "tanh")])
def test_gno_layer_on_the_knn_handle_and_its_coords(dev, Fi, Fo, d, H, act):
    """graph_nop_layer_type through set_graph_handle(handle, vertex_offsets) on from_point_clouds_knn: forward and reverse within
    1e-5 of oracle/layers.py on the yardstick's graph, and points_grad of its dcoords == tests/geometry_reference.py"""
    import torch
    from athena_amd import DeviceGraph, points_grad
    from athena_amd.layers import graph_nop_layer_type

    rng = kr._rng(Fi + d)
    sizes = [60, 1, 35, 48]
    off = kr.offsets_of(sizes)
    n, k = int(off[-1]), 4
    p = rng.random((n, d)).astype(np.float32)
    ri, rj, rc, reoff = kr.graph_of(kr.brute_force_neighbours(p, off, k), p, off, 0)
    assert ri.size > n
    got, coords, voff, eoff = DeviceGraph.from_point_clouds_knn(torch.from_numpy(p).to(dev), off, k)
    assert np.array_equal(coords.cpu().numpy(), rc) and np.array_equal(eoff, reoff)
    x = rng.uniform(-1, 1, (n, Fi)).astype(np.float32)
    up = rng.uniform(-1, 1, (n, Fo)).astype(np.float32)
    xd, upd = torch.from_numpy(x).to(dev), torch.from_numpy(up).to(dev)
    layer = graph_nop_layer_type(num_outputs=Fo, coord_dim=d, kernel_hidden=H, num_inputs=Fi, use_bias=True, activation=act, seed=5)
    params = layer.get_params() + kr._rng(1).standard_normal(layer.get_num_params()).astype(np.float32) * 0.05
    layer.set_params(params)
    layer.set_graph_handle(got, voff)
    out = layer.forward(xd, coords).clone()
    dx, dc = layer.backward(upd, need_coord_grad=True)
    out, dx, dc_t, dparams = out.cpu().numpy(), dx.cpu().numpy(), dc.clone(), layer.get_gradients()
    dc = dc_t.cpu().numpy()
    assert np.isfinite(out).all() and np.abs(out).max() > 0
    gs, xs, cs, ups = [], [], [], []
    for b in range(len(sizes)):
        e = slice(int(reoff[b]), int(reoff[b + 1]))
        gs.append(csr_from_index_list(sizes[b], np.stack([ri[e] - off[b] + 1, rj[e] - off[b] + 1]).reshape(2, -1)))
        gs[-1].num_edges = int(reoff[b + 1] - reoff[b])
        xs.append(x[off[b]:off[b + 1]]); cs.append(rc[e]); ups.append(up[off[b]:off[b + 1]])
    F = Fo * Fi
    plist, o_ = [], 0
    for m in (H * d + H + F * H + F, F, Fo):
        plist.append(params[o_:o_ + m]); o_ += m
    outs, tapes = ol.gno_forward(gs, xs, cs, plist, Fi, Fo, d, H, True, act)
    dxs, dcs, grads = ol.gno_backward(gs, xs, cs, tapes, plist, Fi, Fo, d, H, True, act, ups)

    @functools.lru_cache(None)
    def hi():
        with ol.double_precision():
            _, t64 = ol.gno_forward(gs, xs, cs, plist, Fi, Fo, d, H, True, act)
            a, b, c = ol.gno_backward(gs, xs, cs, t64, plist, Fi, Fo, d, H, True, act, ups)
        return np.concatenate(a), np.concatenate(b), np.concatenate(c)
    assert_close(out, np.concatenate(outs), 1e-5, "gno forward on the knn handle")
    assert_close(dx, np.concatenate(dxs), 1e-5, "gno dx on the knn handle", f64=lambda: hi()[0])
    assert_close(dc, np.concatenate(dcs), 1e-5, "gno dcoords on the knn handle", f64=lambda: hi()[1])
    assert_close(dparams, np.concatenate(grads), 1e-5, "gno dparams on the knn handle", f64=lambda: hi()[2])
    want, _ = gr.points_grad(got.export("rowptr"), got.export("col"), got.export("eid"), dc, np.float32)
    dp = points_grad(got, dc_t.contiguous())
    assert dp.shape == (n, d) and np.array_equal(dp.cpu().numpy(), want) and np.abs(want).max() > 0
    got.close()


# ---- Fortran -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,loops,capped", [(0, 1, False), (1, 0, False), (0, 0, True)])
def test_fortran_program_writes_the_arrays_of_the_yardstick(dev, tmp_path, mode, loops, capped):
    if not os.path.exists(RUNNER):
        pytest.fail("knn_graph_run is not built: __graft_entry__.build() compiles the Fortran host side")
    p, off, k, _ = CASES["batch"]
    r = 0.15 if capped else INF
    n, B, dim = int(off[-1]), off.size - 1, 3
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(case, "wb") as f:
        f.write(np.asarray([B, n, dim, k, mode, loops], np.int32).tobytes() + np.asarray([r], np.float32).tobytes() + off.tobytes() + p.tobytes())
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"knn_graph_run failed ({out.returncode}): {out.stderr[-2000:]}"
    ri, rj, rc, reoff = kr.graph_of(kr.brute_force_neighbours(p, off, k, r), p, off, mode)
    host = csr_from_index_list(n, np.stack([ri + 1, rj + 1]).astype(np.int32), self_loops=bool(loops))
    b = open(res, "rb").read()
    hB, hn, hdim, nnz, E = np.frombuffer(b, np.int32, 5)
    assert (hB, hn, hdim, nnz, E) == (B, n, dim, host.nnz, ri.size) and E > n
    o = 20
    ia = np.frombuffer(b, np.int32, n + 1, o); o += 4 * (n + 1)
    ja = np.frombuffer(b, np.int32, 2 * nnz, o).reshape((2, nnz), order="F"); o += 8 * nnz
    cf = np.frombuffer(b, np.float32, dim * E, o).reshape(E, dim); o += 4 * dim * E
    eo = np.frombuffer(b, np.int64, B + 1, o); o += 8 * (B + 1)
    st = np.frombuffer(b, np.int64, 4, o); o += 32
    assert o == len(b)
    assert np.array_equal(ia, host.adj_ia) and np.array_equal(ja, host.adj_ja) and np.array_equal(cf, rc) and np.array_equal(eo, reoff)
    assert st[0] == n and 0 < st[1] < n * n
