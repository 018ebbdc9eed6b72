"""GPU: a batch of point clouds -> one block-diagonal radius graph on the device (athena_amd/csrc/radius_graph.hip;
athena_mp_radius_pairs_batched, athena_mp_radius_graph_batched_host and their Python / Fortran mirrors) against the yardstick of
tests/radius_batch_reference.py: the single-cloud definition per slice, rebased and concatenated.  Integers and single fp32
subtractions: every comparison of pair lists, coords, edge_offsets and handle arrays is np.array_equal / torch.equal on whole
arrays.  The only tolerance is the project's 1e-5 where the GNO layer is held to oracle/layers.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import geometry_reference as gr
import oracle_layers as ol
from helpers import assert_close, csr_from_index_list, placed, placed_out, unwritten
from radius_batch_reference import cloud_sizes, edge_offsets_of, reference_pairs_batched
from radius_reference import degree_radius, reference_pairs
from test_gpu_graph_build import NAMES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "radius_batch_run")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _call(pts, off, r, pairs=None, coords=None, capacity=0, n=None, dim=None, B=None):
    """athena_mp_radius_pairs_batched on a device tensor -> (E, edge_offsets)"""
    from athena_amd import _capi

    off = np.ascontiguousarray(off, np.int32)
    B = off.size - 1 if B is None else B
    _capi.use_torch_stream()
    E = C.c_int64(-1)
    eoff = np.full(max(B, 0) + 1, -9, np.int64)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    _capi.call("athena_mp_radius_pairs_batched", int(B), int(pts.shape[0] if n is None else n), off.ctypes.data_as(C.c_void_p),
               int(pts.shape[1] if dim is None else dim), ptr(pts), float(r), ptr(pairs), ptr(coords), int(capacity),
               eoff.ctypes.data_as(C.c_void_p), C.byref(E))
    return E.value, eoff


def _gpu_pairs(dev, p, off, r):
    """size query, then fill -> (i, j, coords, edge_offsets) 0-based numpy, plus the raw device tensors"""
    import torch

    pts = torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dev)
    q, eoff_q = _call(pts, off, r)
    pairs = torch.full((q, 2), -7, dtype=torch.int32, device=dev)
    coords = torch.full((q, pts.shape[1]), np.nan, dtype=torch.float32, device=dev)
    E, eoff = _call(pts, off, r, pairs, coords, q)
    torch.cuda.synchronize()
    assert E == q and np.array_equal(eoff, eoff_q), "the size query and the fill disagree"
    pr = pairs.cpu().numpy().astype(np.int64)
    return pr[:, 0] - 1, pr[:, 1] - 1, coords.cpu().numpy(), eoff, pairs, coords


def _check(dev, p, off, r, min_pairs=None):
    p = np.ascontiguousarray(p, np.float32)
    ri, rj, rc, reoff = reference_pairs_batched(p, off, r)
    gi, gj, gc, geoff, _, _ = _gpu_pairs(dev, p, off, r)
    print(f"B = {len(off) - 1}, n = {p.shape[0]}, dim = {p.shape[1]}, radius = {r:.6g}: {ri.size} reference pairs, {gi.size} device pairs")
    if min_pairs is not None:
        assert ri.size >= min_pairs
    assert np.array_equal(gi, ri) and np.array_equal(gj, rj), "pair list differs from the yardstick"
    assert gc.dtype == rc.dtype and np.array_equal(gc, rc), "coords differ from the yardstick"
    assert geoff.dtype == reoff.dtype and np.array_equal(geoff, reoff), "edge_offsets differ from the yardstick"
    return ri.size


@functools.lru_cache(None)
def _small_clouds(dim):
    """3 000 clouds of clip(round(N(18, 3)), 4, 29) points in the unit box, radius for a mean degree of about 4, and the yardstick"""
    rng = _rng(50 + dim)
    off = _offsets(cloud_sizes(rng, 3000))
    p = rng.random((int(off[-1]), dim)).astype(np.float32)
    r = degree_radius(18, 4.0, dim)
    return p, off, r, reference_pairs_batched(p, off, r)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_yardstick_equals_the_single_cloud_entry_called_per_cloud(dev, dim):
    import torch
    from athena_amd import _capi

    rng = _rng(dim)
    off = _offsets([300, 0, 1, 450, 2, 120])
    p = rng.random((int(off[-1]), dim)).astype(np.float32)
    r = degree_radius(300, 8.0, dim)
    ri, rj, rc, reoff = reference_pairs_batched(p, off, r)
    got_i, got_j, got_c = [], [], []
    _capi.use_torch_stream()
    for b in range(off.size - 1):
        m = int(off[b + 1] - off[b])
        pts = torch.from_numpy(np.ascontiguousarray(p[off[b]:off[b + 1]])).to(dev)
        E = C.c_int64()
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
        _capi.call("athena_mp_radius_pairs", m, dim, ptr(pts), float(r), None, None, 0, C.byref(E))
        pairs = torch.empty((E.value, 2), dtype=torch.int32, device=dev)
        coords = torch.empty((E.value, dim), dtype=torch.float32, device=dev)
        _capi.call("athena_mp_radius_pairs", m, dim, ptr(pts), float(r), ptr(pairs), ptr(coords), E.value, C.byref(E))
        assert E.value == reoff[b + 1] - reoff[b]
        pr = pairs.cpu().numpy().astype(np.int64)
        got_i.append(pr[:, 0] - 1 + off[b]); got_j.append(pr[:, 1] - 1 + off[b]); got_c.append(coords.cpu().numpy())
    assert ri.size > 1000
    assert np.array_equal(np.concatenate(got_i), ri) and np.array_equal(np.concatenate(got_j), rj)
    assert np.array_equal(np.concatenate(got_c), rc)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_clouds_that_overlap_in_space(dev, dim):
    """8 clouds of 500 points, all uniform in the same unit box: a builder with one grid for all would see the other clouds' points"""
    B, m = 8, 500
    p = _rng(20 + dim).random((B * m, dim)).astype(np.float32)
    off = _offsets([m] * B)
    r = degree_radius(m, 10.0, dim)
    bi, bj, _ = reference_pairs(p, r)                                      # cloud-blind
    cross = int((bi // m != bj // m).sum())
    print(f"dim {dim}: {cross} of the {bi.size} cloud-blind pairs join two clouds")
    assert cross > 0
    _check(dev, p, off, r, min_pairs=B * m)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_empty_and_tiny_clouds(dev, dim):
    import torch

    rng = _rng(30 + dim)
    off = np.array([0, 0, 1, 1, 3, 3, 40, 40], np.int32)                   # empty first, middle, last; one point; two points
    p = rng.random((40, dim)).astype(np.float32)
    p[2] = p[1]                                                            # the two-point cloud: coincident points, joined
    r = degree_radius(37, 5.0, dim)
    E = _check(dev, p, off, r, min_pairs=20)
    gi, gj, gc, eoff, _, _ = _gpu_pairs(dev, p, off, r)
    assert (gi[0], gj[0]) == (1, 2) and np.all(gc[0] == 0)
    assert eoff.tolist() == [0, 0, 0, 0, 1, 1, E, E]
    assert np.array_equal(eoff, edge_offsets_of(gi, off))
    # no cloud at all; clouds without a point
    none = torch.zeros((0, dim), dtype=torch.float32, device=dev)
    E0, e0 = _call(none, [0], r)
    assert E0 == 0 and e0.tolist() == [0]
    E0, e0 = _call(none, [0, 0, 0, 0], r)
    assert E0 == 0 and e0.tolist() == [0, 0, 0, 0]
    # one point in all, among empty clouds
    assert _check(dev, p[:1], np.array([0, 0, 1, 1], np.int32), r) == 0


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_clouds_at_the_work_item_edges(dev, dim):
    """exactly one work item of 4 096 points, one point more (a second item of one point), beside a cloud of 3"""
    sizes = [4096, 3, 4097]
    rng = _rng(40 + dim)
    p = rng.random((sum(sizes), dim)).astype(np.float32)
    p[4097] = p[4096]
    _check(dev, p, _offsets(sizes), degree_radius(4096, 8.0, dim), min_pairs=8000)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_grids_that_differ_per_cloud(dev, dim):
    rng = _rng(60 + dim)
    r = 0.1
    h = r * (1.0 + 2.0 ** -10)                                             # the smallest cell width
    clouds = [rng.random((800, dim)),                                      # [0, 1]^dim
              100.0 + 0.01 * rng.random((300, dim)),                       # [100, 100.01]^dim: one cell, fp32 spacing 8e-6
              rng.random((400, dim)) * ([1.0] * (dim - 1) + [0.0]) + 0.25,   # flat on the last axis (zero extent)
              np.tile(rng.random((1, dim)) - 3.0, (50, 1))]                # all points coincident
    strung = np.zeros((10, dim)); strung[:, 0] = np.array([0, 0.5, 1000, 2000, 3000, 5000, 7000, 9000, 9999.5, 10000]) * r
    clouds.append(strung)                                                  # 10 points over 10 000 radii: the 2 m cell cap halves the axis
    for f in (1.0 - 1e-4, 1.0 + 1e-4):                                     # extent just below / just above two cell widths
        c = rng.random((200, dim)) * 2.0 * h * f
        c[0], c[1] = 0.0, 2.0 * h * f
        clouds.append(c - 7.0)
    p = np.concatenate(clouds).astype(np.float32)
    off = _offsets([c.shape[0] for c in clouds])
    h32 = float(np.float32(r)) * (1.0 + 2.0 ** -10)                        # as the builder sees it: the fp32 radius, the fp32 points
    cells = [int((float(p[off[b]:off[b + 1], 0].max()) - float(p[off[b]:off[b + 1], 0].min())) / h32) for b in (5, 6)]
    assert cells == [1, 2], cells                                          # one cell and two cells on every axis
    ri, rj, rc, reoff = reference_pairs_batched(p, off, r)
    assert np.all(np.diff(reoff) > 0)                                      # every cloud has pairs
    assert reoff[4] - reoff[3] == 50 * 49 // 2 and reoff[5] - reoff[4] == 2
    _check(dev, p, off, r)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_many_small_clouds(dev, dim):
    p, off, r, ref = _small_clouds(dim)
    gi, gj, gc, geoff, _, _ = _gpu_pairs(dev, p, off, r)
    deg = 2.0 * ref[0].size / p.shape[0]
    print(f"dim {dim}: {p.shape[0]} points in 3000 clouds, {ref[0].size} pairs, mean degree {deg:.2f}")
    assert 2.0 < deg < 6.0
    assert np.array_equal(gi, ref[0]) and np.array_equal(gj, ref[1]) and np.array_equal(gc, ref[2]) and np.array_equal(geoff, ref[3])


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_pair_counts_on_both_sides_of_the_radix_tiles(dev, dim):
    """pair counts around one and two 4 096-entry tiles of the radix passes (radix_sort.h) on a two-cloud input, chosen from the
    sorted fp32 squared distances inside the clouds"""
    sizes = [450, 250]
    p = _rng(70 + dim).random((sum(sizes), dim)).astype(np.float32)
    off = _offsets(sizes)
    s = []
    for b in range(2):
        q = p[off[b]:off[b + 1]]
        i, j = np.triu_indices(q.shape[0], 1)
        d = q[i] - q[j]
        t = d[:, 0] * d[:, 0]
        for a in range(1, dim):
            t = t + d[:, a] * d[:, a]
        s.append(t)
    s = np.sort(np.concatenate(s))
    counts = []
    for target in (4090, 4095, 4096, 4097, 4100, 8191, 8192, 8193):
        r = float(np.sqrt(np.float32(0.5) * (s[target - 1] + s[target])))
        counts.append(_check(dev, p, off, r))
    assert min(counts) <= 4096 < max(counts) and min(c for c in counts if c > 4100) <= 8192 < max(counts), counts


def test_two_builds_are_byte_identical_and_the_count_only_call_agrees(dev):
    import torch

    p, off, r, ref = _small_clouds(3)
    _, _, _, eoff1, pairs1, coords1 = _gpu_pairs(dev, p, off, r)
    _, _, _, eoff2, pairs2, coords2 = _gpu_pairs(dev, p, off, r)
    assert torch.equal(pairs1, pairs2) and torch.equal(coords1.view(torch.int32), coords2.view(torch.int32))
    assert np.array_equal(eoff1, eoff2)
    E, eoff = _call(torch.from_numpy(p).to(dev), off, r)                   # count only
    assert E == pairs1.shape[0] == ref[0].size and np.array_equal(eoff, eoff1)
    # either output alone
    pts = torch.from_numpy(p).to(dev)
    only_p = torch.full_like(pairs1, -7)
    only_c = torch.full_like(coords1, np.nan)
    assert _call(pts, off, r, pairs=only_p, capacity=E)[0] == E and _call(pts, off, r, coords=only_c, capacity=E)[0] == E
    torch.cuda.synchronize()
    assert torch.equal(only_p, pairs1) and torch.equal(only_c.view(torch.int32), coords1.view(torch.int32))


def test_refuses_bad_input_and_stays_usable(dev):
    import torch
    from athena_amd import DeviceGraph, _capi

    rng = _rng(14)
    sizes = [700, 0, 900, 5, 1400]
    off = _offsets(sizes)
    p = rng.random((int(off[-1]), 3)).astype(np.float32)
    r = 0.12
    good = reference_pairs_batched(p, off, r)[0].size
    pts = torch.from_numpy(p).to(dev)
    assert _call(pts, off, r)[0] == good
    err = _capi.AthenaMPError
    with pytest.raises(err, match=r"dim = 4 outside \[1,3\]"):
        _call(torch.zeros((10, 4), device=dev), [0, 10], r)
    with pytest.raises(err, match=r"dim = 0 outside \[1,3\]"):
        _call(pts, off, r, dim=0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(err, match=r"radius = .* is not a positive finite number"):
            _call(pts, off, bad)
    with pytest.raises(err, match=r"radius = .* squared is not finite in fp32"):
        _call(pts, off, 3e19)
    with pytest.raises(err, match=r"n_clouds = -1 is negative"):
        _call(pts, off, r, B=-1)
    with pytest.raises(err, match=r"offsets\(1\) = 2, not 0"):
        _call(pts, np.concatenate([[2], off[1:]]), r)
    down = off.copy(); down[3] = down[2] - 1                               # cloud 3 (1-based) runs backwards
    with pytest.raises(err, match=r"cloud 3: offsets descend from %d to %d" % (down[2], down[3])):
        _call(pts, down, r)
    with pytest.raises(err, match=r"offsets end at %d, the batch has %d points" % (off[-1] - 5, off[-1])):
        _call(pts, np.concatenate([off[:-1], [off[-1] - 5]]), r)
    with pytest.raises(err, match=r"offsets end at %d, the batch has %d points" % (off[-1], off[-1] - 1)):
        _call(pts, off, r, n=int(off[-1]) - 1)
    pairs = torch.empty((good, 2), dtype=torch.int32, device=dev)
    coords = torch.empty((good, 3), dtype=torch.float32, device=dev)
    with pytest.raises(err, match=r"buffers hold %d pairs, the batch has %d" % (good - 1, good)):
        _call(pts, off, r, pairs, coords, good - 1)
    # the FIRST non-finite point is named with its cloud, component and global index, 1-based (cloud 2 is empty)
    for value, where, cloud in ((np.nan, (1234, 1), 3), (np.inf, (7, 2), 1), (-np.inf, (1601, 0), 4), (np.nan, (3004, 2), 5)):
        q = p.copy()
        q[where] = value
        if where[0] < 3004:
            q[3004, 0] = np.nan                                            # a later one
        text = "-?nan" if np.isnan(value) else "-inf" if value < 0 else "inf"
        with pytest.raises(err, match=r"cloud %d: points\(%d,%d\) = %s is not finite" % (cloud, where[1] + 1, where[0] + 1, text)):
            _call(torch.from_numpy(q).to(dev), off, r)
    # too many entries: a cloud of 10 and one of 50 000 points inside one radius, 1.25e9 pairs; found by the count pass
    crowd = torch.from_numpy((rng.random((50_010, 3)) * 1e-3).astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(err, match=r"1249975045 pairs among 50010 points: more than 2\^31 CSR entries"):
        _call(crowd, [0, 10, 50_010], 1.0)
    with pytest.raises(err, match=r"more than 2\^31 CSR entries"):
        DeviceGraph.from_point_clouds(crowd, [0, 10, 50_010], 1.0)
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 8 << 20
    _check(dev, p, off, r)                                                 # the library is usable afterwards


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_operands_at_four_byte_addresses_between_guards(dev, dim):
    """points, pairs and coords one element past a 512-byte boundary: 4-byte but not 8-byte aligned"""
    import torch

    rng = _rng(80 + dim)
    off = _offsets([700, 0, 333, 1, 501])
    p = rng.random((int(off[-1]), dim)).astype(np.float32)
    r = degree_radius(500, 9.0, dim)
    ri, rj, rc, reoff = reference_pairs_batched(p, off, r)
    E = ri.size
    pts = placed(p, dev, 1)
    before = pts.clone()
    pairs, check_p = placed_out((E, 2), torch.int32, dev, 1)
    coords, check_c = placed_out((E, dim), torch.float32, dev, 1)
    assert pts.data_ptr() % 8 == 4 and pairs.data_ptr() % 8 == 4 and coords.data_ptr() % 8 == 4
    got, eoff = _call(pts, off, r, pairs, coords, E)
    torch.cuda.synchronize()
    check_p("pairs at a 4-byte address")
    check_c("coords at a 4-byte address")
    assert got == E and np.array_equal(eoff, reoff) and unwritten(pairs) == 0 and unwritten(coords) == 0
    assert np.array_equal(pairs.cpu().numpy().astype(np.int64), np.stack([ri + 1, rj + 1], axis=1))
    assert np.array_equal(coords.cpu().numpy(), rc)
    assert torch.equal(pts.view(torch.int32), before.view(torch.int32))


def _same(a, b):
    for n in NAMES:
        x, y = a.export(n), b.export(n)
        assert x.shape == y.shape, n
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), f"{n} differs"


@pytest.mark.parametrize("dim,loops", [(3, True), (3, False), (2, True), (1, False)])
def test_handle_from_point_clouds_and_mini_batches_of_it(dev, dim, loops):
    import torch
    from athena_amd import DeviceDataset, DeviceGraph
    from athena_amd.graph import graph_type

    rng = _rng(90 + dim)
    sizes = [260, 1, 140, 0, 75, 310, 2]
    off = _offsets(sizes)
    n = int(off[-1])
    p = rng.random((n, dim)).astype(np.float32)
    r = degree_radius(200, 9.0, dim)
    ri, rj, rc, reoff = reference_pairs_batched(p, off, r)
    idx = np.asfortranarray(np.stack([ri + 1, rj + 1]).astype(np.int32))
    ref = DeviceGraph.from_edges(n, idx, add_self_loops=loops)
    host = csr_from_index_list(n, idx, self_loops=loops)
    one, coords, voff, eoff, ia, ja = DeviceGraph.from_point_clouds(p, off, r, add_self_loops=loops, want_adjacency=True)
    lean, coords2, voff2, eoff2 = DeviceGraph.from_point_clouds(torch.from_numpy(p).to(dev), off, r, add_self_loops=loops)
    assert coords.is_cuda and coords.shape == (ri.size, dim) and coords.dtype == torch.float32
    assert np.array_equal(coords.cpu().numpy(), rc) and torch.equal(coords, coords2)
    assert voff.dtype == np.int32 and np.array_equal(voff, off) and np.array_equal(voff2, off)
    assert eoff.dtype == np.int64 and np.array_equal(eoff, reoff) and np.array_equal(eoff2, reoff)
    assert np.array_equal(ia, host.adj_ia) and np.array_equal(ja, host.adj_ja)
    assert (one.n_rows, one.nnz, one.n_edge_cols) == (ref.n_rows, ref.nnz, ref.n_edge_cols) == (n, host.nnz, ri.size)
    _same(one, ref)
    _same(lean, ref)
    # the host-array sibling
    d = graph_type(); d.set_num_vertices(n, 1)
    c3, eoff3 = d.generate_radius_batch_adjacency_device(p, off, r, add_self_loops=loops)
    assert d.num_edges == ri.size and np.array_equal(c3, rc) and np.array_equal(eoff3, reoff)
    assert np.array_equal(d.adj_ia, host.adj_ia) and np.array_equal(d.adj_ja, host.adj_ja)
    # the dataset machinery takes the handle as it is
    ds = DeviceDataset(one, voff, eoff)
    sel = [5, 2, 2, 0]
    b = ds.select(sel)
    child_p = np.concatenate([p[off[s]:off[s + 1]] for s in sel])
    child_off = _offsets([sizes[s] for s in sel])
    scratch, scoords, svoff, seoff = DeviceGraph.from_point_clouds(child_p, child_off, r, add_self_loops=loops)
    assert np.array_equal(b.vertex_offsets, svoff) and np.array_equal(b.edge_offsets, seoff)
    _same(b.handle, scratch)
    assert torch.equal(b.take_edges(coords).view(torch.int32), scoords.view(torch.int32)) and scoords.shape[0] > 100
    b.close()
    ds.close()
    for g in (one, lean, ref, scratch):
        g.close()


@pytest.mark.parametrize("Fi,Fo,d,H,act", [(64, 64, 3, 64, "relu"), (5, 3, 2, 7, "tanh")])
def test_gno_layer_on_the_batched_handle_and_its_coords(dev, Fi, Fo, d, H, act):
    """graph_nop_layer_type through set_graph_handle(handle, vertex_offsets) on from_point_clouds: bit for bit the layer on the
    from_edges handle of the yardstick's list, within 1e-5 of oracle/layers.py, and points_grad of its dcoords == the yardstick"""
    import torch
    from athena_amd import DeviceGraph, points_grad
    from athena_amd.layers import graph_nop_layer_type

    rng = _rng(Fi + d)
    sizes = [60, 1, 35, 48]
    off = _offsets(sizes)
    n = int(off[-1])
    p = rng.random((n, d)).astype(np.float32)
    r = degree_radius(48, 6.0, d)
    ri, rj, rc, reoff = reference_pairs_batched(p, off, r)
    assert ri.size > n
    ref = DeviceGraph.from_edges(n, np.stack([ri + 1, rj + 1]).astype(np.int32))
    got, coords, voff, eoff = DeviceGraph.from_point_clouds(torch.from_numpy(p).to(dev), off, r)
    x = rng.uniform(-1, 1, (n, Fi)).astype(np.float32)
    up = rng.uniform(-1, 1, (n, Fo)).astype(np.float32)
    xd, upd = torch.from_numpy(x).to(dev), torch.from_numpy(up).to(dev)
    res = []
    for handle, c in ((got, coords), (ref, torch.from_numpy(rc).to(dev))):
        layer = graph_nop_layer_type(num_outputs=Fo, coord_dim=d, kernel_hidden=H, num_inputs=Fi, use_bias=True, activation=act, seed=5)
        params = layer.get_params() + _rng(1).standard_normal(layer.get_num_params()).astype(np.float32) * 0.05
        layer.set_params(params)
        layer.set_graph_handle(handle, voff)
        out = layer.forward(xd, c).clone()
        dx, dc = layer.backward(upd, need_coord_grad=True)
        res.append((out, dx.clone(), dc.clone(), torch.from_numpy(layer.get_gradients())))
    assert torch.isfinite(res[0][0]).all() and res[0][0].abs().max() > 0
    for a, b, what in zip(res[0], res[1], ("output", "dx", "dcoords", "dparams")):
        assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), what
    # the oracle's layer on the clouds one by one
    gs, xs, cs, ups = [], [], [], []
    for b in range(len(sizes)):
        k = slice(int(reoff[b]), int(reoff[b + 1]))
        gs.append(csr_from_index_list(sizes[b], np.stack([ri[k] - off[b] + 1, rj[k] - off[b] + 1]).reshape(2, -1)))
        gs[-1].num_edges = int(reoff[b + 1] - reoff[b])
        xs.append(x[off[b]:off[b + 1]]); cs.append(rc[k]); ups.append(up[off[b]:off[b + 1]])
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
    out, dx, dc, dparams = (t.cpu().numpy() for t in res[0])
    assert_close(out, np.concatenate(outs), 1e-5, "gno forward on the batched handle")
    assert_close(dx, np.concatenate(dxs), 1e-5, "gno dx on the batched handle", f64=lambda: hi()[0])
    assert_close(dc, np.concatenate(dcs), 1e-5, "gno dcoords on the batched handle", f64=lambda: hi()[1])
    assert_close(dparams, np.concatenate(grads), 1e-5, "gno dparams on the batched handle", f64=lambda: hi()[2])
    # dcoords back to the points
    want, _ = gr.points_grad(got.export("rowptr"), got.export("col"), got.export("eid"), dc, np.float32)
    dp = points_grad(got, res[0][2].contiguous())
    assert dp.shape == (n, d) and np.array_equal(dp.cpu().numpy(), want) and np.abs(want).max() > 0
    got.close(); ref.close()


@pytest.mark.parametrize("dim,loops", [(3, 1), (3, 0), (2, 1), (2, 0)])
def test_fortran_program_writes_the_arrays_of_the_python_mirror(dev, tmp_path, dim, loops):
    from athena_amd.graph import graph_type

    if not os.path.exists(RUNNER):
        pytest.fail("radius_batch_run is not built: __graft_entry__.build() compiles the Fortran host side")
    rng = _rng(dim + loops)
    off = _offsets([900, 0, 1, 1300, 4, 600])
    n, B = int(off[-1]), off.size - 1
    p = (rng.random((n, dim)) - 0.5).astype(np.float32)
    r = degree_radius(900, 10.0, dim)
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(case, "wb") as f:
        f.write(np.asarray([B, n, dim, loops], np.int32).tobytes() + np.asarray([r], np.float32).tobytes() + off.tobytes() + p.tobytes())
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"radius_batch_run failed ({out.returncode}): {out.stderr[-2000:]}"
    g = graph_type(); g.set_num_vertices(n, 1)
    coords, eoff = g.generate_radius_batch_adjacency_device(p, off, r, add_self_loops=bool(loops))
    b = open(res, "rb").read()
    hB, hn, hdim, nnz, E = np.frombuffer(b, np.int32, 5)
    assert (hB, hn, hdim, nnz, E) == (B, n, dim, g.nnz, g.num_edges) and E > n
    o = 20
    ia = np.frombuffer(b, np.int32, n + 1, o); o += 4 * (n + 1)
    ja = np.frombuffer(b, np.int32, 2 * nnz, o).reshape((2, nnz), order="F"); o += 8 * nnz
    cf = np.frombuffer(b, np.float32, dim * E, o).reshape(E, dim); o += 4 * dim * E
    eo = np.frombuffer(b, np.int64, B + 1, o); o += 8 * (B + 1)
    assert o == len(b)
    assert np.array_equal(ia, g.adj_ia) and np.array_equal(ja, g.adj_ja) and np.array_equal(cf, coords) and np.array_equal(eo, eoff)
    ri, rj, rc, reoff = reference_pairs_batched(p, off, r)
    assert np.array_equal(cf, rc) and np.array_equal(eo, reoff)


def test_builds_from_point_clouds_do_not_leak_device_memory(dev):
    import torch
    from athena_amd import DeviceGraph

    rng = _rng(21)
    off = _offsets(cloud_sizes(rng, 1500))
    n = int(off[-1])
    pts = torch.from_numpy(rng.random((n, 3)).astype(np.float32)).to(dev)
    r = degree_radius(18, 4.0, 3)

    def cycle():
        g, coords, _, _ = DeviceGraph.from_point_clouds(pts, off, r, add_self_loops=True)
        assert coords.shape[0] > n
        g.close()
        del coords

    cycle()                                                            # warm: workspaces, pools
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(50):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 8 << 20, f"{(free0 - free1) >> 20} MiB of device memory lost over 50 builds from point clouds"
