"""GPU: points -> radius graph on the device (athena_amd/csrc/radius_graph.hip; athena_mp_radius_pairs,
athena_mp_graph_create_from_edges_dev, athena_mp_radius_graph_host and their Python / Fortran mirrors) against the
yardstick of tests/radius_reference.py.  Integers and single fp32 subtractions: every comparison is np.array_equal /
torch.equal, no tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from radius_reference import degree_radius, reference_pairs
from test_gpu_graph_build import NAMES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "radius_graph_run")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _query(pts, r):
    from athena_amd import _capi

    _capi.use_torch_stream()
    E = C.c_int64(-1)
    _capi.call("athena_mp_radius_pairs", int(pts.shape[0]), int(pts.shape[1]), C.c_void_p(pts.data_ptr()), float(r), None, None, 0,
               C.byref(E))
    return E.value


def _gpu_pairs(dev, p, r, capacity=None):
    """athena_mp_radius_pairs: size query, then fill -> (i, j, coords) 0-based numpy, plus the raw device tensors"""
    import torch
    from athena_amd import _capi

    pts = torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dev)
    n, dim = pts.shape
    q = _query(pts, r)
    cap = q if capacity is None else capacity
    pairs = torch.full((max(cap, 0), 2), -7, dtype=torch.int32, device=dev)
    coords = torch.full((max(cap, 0), dim), np.nan, dtype=torch.float32, device=dev)
    E = C.c_int64(-1)
    _capi.call("athena_mp_radius_pairs", int(n), int(dim), C.c_void_p(pts.data_ptr()), float(r), C.c_void_p(pairs.data_ptr()),
               C.c_void_p(coords.data_ptr()), cap, C.byref(E))
    torch.cuda.synchronize()
    assert E.value == q, "the size query and the fill disagree"
    pr = pairs.cpu().numpy()[:q].astype(np.int64)
    return pr[:, 0] - 1, pr[:, 1] - 1, coords.cpu().numpy()[:q], pairs, coords


def _check(dev, p, r, min_pairs=None):
    p = np.ascontiguousarray(p, np.float32)
    ri, rj, rc = reference_pairs(p, r)
    gi, gj, gc, _, _ = _gpu_pairs(dev, p, r)
    print(f"n = {p.shape[0]}, dim = {p.shape[1]}, radius = {r:.6g}: {ri.size} reference pairs, {gi.size} device pairs")
    if min_pairs is not None:
        assert ri.size >= min_pairs
    assert np.array_equal(gi, ri) and np.array_equal(gj, rj), "pair list differs from the reference"
    assert gc.dtype == rc.dtype and np.array_equal(gc, rc), "coords differ from the reference"
    return ri.size


@pytest.mark.parametrize("n,dim,deg", [(3000, 1, 6.0), (5000, 2, 9.0), (4000, 3, 15.0), (300_000, 1, 10.0), (200_000, 2, 12.0),
                                       (250_000, 3, 15.0)])
def test_radius_pairs_uniform_clouds(dev, n, dim, deg):
    p = _rng(n + dim).random((n, dim)).astype(np.float32)
    _check(dev, p, degree_radius(n, deg, dim), min_pairs=n)


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8192, 8193])
def test_radius_pairs_at_the_work_item_edges(dev, n, dim):
    """one cloud is a batch of one; its cell keys are written by one wave per work item of 4 096 points (cell_grid.h): one item
    less a point, exactly one, one and a point, exactly two, two and a point.  _gpu_pairs holds the count-only call against the
    fill."""
    p = _rng(7 * n + dim).random((n, dim)).astype(np.float32)
    _check(dev, p, degree_radius(n, 6.0, dim), min_pairs=n)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_radius_pairs_counts_on_both_sides_of_the_radix_tiles(dev, dim):
    """pair counts around one and two 4 096-entry tiles of the radix passes (radix_sort.h), chosen from the sorted fp32
    squared distances of the cloud"""
    n = 700
    p = _rng(40 + dim).random((n, dim)).astype(np.float32)
    i, j = np.triu_indices(n, 1)
    d = p[i] - p[j]
    s = d[:, 0] * d[:, 0]
    for a in range(1, dim):
        s = s + d[:, a] * d[:, a]
    s = np.sort(s)
    counts = []
    for target in (4090, 4095, 4096, 4097, 4100, 8191, 8192, 8193):
        r = float(np.sqrt(np.float32(0.5) * (s[target - 1] + s[target])))
        counts.append(_check(dev, p, r))
    assert min(counts) <= 4096 < max(counts) and min(c for c in counts if c > 4100) <= 8192 < max(counts), counts


def test_radius_pairs_special_clouds(dev):
    rng = _rng(11)
    # one point; two points apart; no pair at all
    assert _check(dev, np.array([[0.5, 0.25, 0.125]], np.float32), 0.3) == 0
    assert _check(dev, np.array([[0.0], [1.0]], np.float32), 0.5) == 0
    p = rng.random((2000, 3)).astype(np.float32)
    assert _check(dev, p, 1e-6) == 0
    # radius beyond the diameter: complete graph, one cell
    p = rng.random((1500, 3)).astype(np.float32)
    assert _check(dev, p, 2.0) == 1500 * 1499 // 2
    assert _check(dev, rng.random((300, 2)).astype(np.float32), 1.5) == 300 * 299 // 2
    # identical points: one crowded cell, complete graph, every difference zero
    p = np.tile(np.array([[0.3, -1.7, 2.5]], np.float32), (200, 1))
    assert _check(dev, p, 0.01) == 200 * 199 // 2
    # identical points inside a sparse background
    p = rng.random((3000, 3)).astype(np.float32)
    p[100:300] = p[5]
    _check(dev, p, 0.05, min_pairs=200 * 199 // 2)


def test_radius_pairs_degenerate_extents_and_coarse_spacing(dev):
    rng = _rng(12)
    n = 6000
    # a line and a plane inside 3-D: one or two axes of zero extent
    line = np.zeros((n, 3), np.float32); line[:, 1] = rng.random(n)
    _check(dev, line, 0.002, min_pairs=n)
    plane = rng.random((n, 3)).astype(np.float32); plane[:, 2] = 0.75
    _check(dev, plane, 0.03, min_pairs=n)
    # an axis whose extent is below the radius
    thin = rng.random((n, 3)).astype(np.float32); thin[:, 0] *= 0.01
    _check(dev, thin, 0.03, min_pairs=n)
    # negative coordinates
    # (a cube of side 2: about n^2 / 2 * (4/3 pi r^3) / 8 = 16 000 pairs at r = 0.12)
    _check(dev, (rng.random((n, 3)) * 2 - 1.5).astype(np.float32), 0.12, min_pairs=n)
    _check(dev, (-rng.random((n, 2)) * 40).astype(np.float32), 0.9, min_pairs=n)
    # a cloud around 1 000: fp32 spacing 6e-5, many borderline cell assignments and borderline distances
    for dim, r in ((1, 0.002), (2, 0.02), (3, 0.06)):
        p = (rng.random((n, dim)) + 1000.0).astype(np.float32)
        _check(dev, p, r, min_pairs=n)
    p = (rng.random((20000, 3)) * 0.25 + np.array([1000.0, -1000.0, 512.0])).astype(np.float32)
    _check(dev, p, 0.0125, min_pairs=20000)
    # points ON a lattice whose pitch is the radius: every axis neighbour sits exactly on the bound
    g = np.stack(np.meshgrid(*[np.arange(24)] * 3, indexing="ij"), -1).reshape(-1, 3)
    for pitch in (0.1, 0.3, 1.0 / 3.0):
        p = (g * np.float32(pitch)).astype(np.float32)[rng.permutation(g.shape[0])]
        _check(dev, p, float(np.float32(pitch)), min_pairs=1000)


def test_radius_pairs_clustered_cloud(dev):
    rng = _rng(13)
    blobs = [c + 0.004 * rng.standard_normal((m, 3)) for c, m in ((np.array([0.2, 0.2, 0.2]), 1500), (np.array([0.7, 0.4, 0.9]), 900),
                                                                   (np.array([0.71, 0.41, 0.9]), 600))]
    p = np.concatenate(blobs + [rng.random((20000, 3))]).astype(np.float32)
    p = p[rng.permutation(p.shape[0])]
    _check(dev, p, 0.02, min_pairs=100_000)


def test_radius_pairs_refuses_bad_input_and_stays_usable(dev):
    import torch
    from athena_amd import _capi

    rng = _rng(14)
    p = rng.random((4000, 3)).astype(np.float32)
    r = 0.06
    good = reference_pairs(p, r)[0].size
    pts = torch.from_numpy(p).to(dev)
    assert _query(pts, r) == good
    with pytest.raises(_capi.AthenaMPError, match=r"buffers hold %d pairs, the graph has %d" % (good - 1, good)):
        _gpu_pairs(dev, p, r, capacity=good - 1)
    with pytest.raises(_capi.AthenaMPError, match=r"dim = 4 outside \[1,3\]"):
        _query(torch.zeros((10, 4), device=dev), r)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_capi.AthenaMPError, match=r"radius = .* is not a positive finite number"):
            _query(pts, bad)
    for value, where in ((np.nan, (1234, 1)), (np.inf, (7, 2)), (-np.inf, (3999, 0))):
        q = p.copy()
        q[where] = value
        if where[0] < 3999:
            q[3999, 0] = np.nan                                            # a later one: the FIRST offending point is named
        text = "-?nan" if np.isnan(value) else "-inf" if value < 0 else "inf"
        with pytest.raises(_capi.AthenaMPError, match=r"points\(%d,%d\) = %s is not finite" % (where[1] + 1, where[0] + 1, text)):
            _query(torch.from_numpy(q).to(dev), r)
    # some 50 000 points inside one radius: 1.25e9 pairs; the count pass finds it, nothing of that size is allocated
    crowd = torch.from_numpy((rng.random((50_000, 3)) * 1e-3).astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(_capi.AthenaMPError, match=r"1249975000 pairs among 50000 points: more than 2\^31 CSR entries"):
        _query(crowd, 1.0)
    with pytest.raises(_capi.AthenaMPError, match=r"more than 2\^31 CSR entries"):
        from athena_amd import DeviceGraph
        DeviceGraph.from_points(crowd, 1.0)
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 8 << 20
    _check(dev, p, r)                                                      # the library is usable afterwards


@pytest.mark.parametrize("bad,first", [({8500: (0, np.nan), 4096: (1, np.inf)}, (4096, 1, "inf")),
                                       ({4096: (0, np.nan), 4095: (2, -np.inf)}, (4095, 2, "-inf"))])
def test_radius_pairs_names_the_first_non_finite_point_across_work_items(dev, bad, first):
    """bad points 4 400 apart, and on both sides of index 4 096.  One cloud alone takes its box and validity from block partials
    (rg_box_kernel: a block strides over the cloud, so the bad points fall to different threads and blocks; 4 096 is where a
    batch of more clouds would cut its work items), and the pipeline behind it is the batched one.  The message is the
    single-cloud one: the smallest index and its first bad component, 1-based, and no cloud."""
    import re

    import torch
    from athena_amd import _capi

    p = _rng(15).random((9000, 3)).astype(np.float32)
    r = degree_radius(9000, 6.0, 3)
    q = p.copy()
    for i, (a, v) in bad.items():
        q[i, a] = v
        q[i, 2] = v if a < 2 else q[i, 2]                                 # a later component of the same point: the FIRST is named
    i, a, text = first
    with pytest.raises(_capi.AthenaMPError) as err:
        _query(torch.from_numpy(q).to(dev), r)
    msg = str(err.value).split(": ", 1)[1]
    assert re.fullmatch(r"radius_pairs: points\(%d,%d\) = .* is not finite" % (a + 1, i + 1), msg), msg
    assert msg == "radius_pairs: points(%d,%d) = %s is not finite" % (a + 1, i + 1, text) and "cloud" not in str(err.value)
    _check(dev, p, r, min_pairs=9000)                                      # a valid call afterwards succeeds


def test_radius_pairs_of_no_points_and_a_radius_whose_square_overflows(dev):
    """n = 0 returns before the square of the radius is looked at in the single-cloud entry; the batched entry checks its
    arguments first and refuses"""
    import torch
    from athena_amd import _capi

    none = torch.zeros((0, 3), dtype=torch.float32, device=dev)
    assert _query(none, 1e30) == 0
    E, off = C.c_int64(-1), np.zeros(2, np.int32)
    with pytest.raises(_capi.AthenaMPError, match=r"radius_pairs_batched: radius = .* squared is not finite in fp32"):
        _capi.call("athena_mp_radius_pairs_batched", 1, 0, off.ctypes.data_as(C.c_void_p), 3, None, 1e30, None, None, 0, None, C.byref(E))
    assert E.value == 0


def _same(a, b):
    for n in NAMES:
        x, y = a.export(n), b.export(n)
        assert x.shape == y.shape, n
        assert np.array_equal(x, y), f"{n} differs"


@pytest.mark.parametrize("n,dim,deg,loops", [(1, 3, 1.0, True), (40, 2, 3.0, False), (6000, 3, 15.0, True), (6000, 3, 15.0, False),
                                             (150_000, 2, 8.0, True), (120_000, 3, 15.0, False)])
def test_handle_from_points_equals_handle_from_the_reference_pairs(dev, n, dim, deg, loops):
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.graph import graph_type

    p = _rng(n + 17 * dim).random((n, dim)).astype(np.float32)
    r = degree_radius(n, deg, dim)
    ri, rj, rc = reference_pairs(p, r)
    idx = np.asfortranarray(np.stack([ri + 1, rj + 1]).astype(np.int32))
    ref = DeviceGraph.from_edges(n, idx, add_self_loops=loops)
    host = graph_type(); host.set_num_vertices(n, 1); host.generate_adjacency(idx)
    if loops:
        host.add_self_loops()
    one, coords, ia, ja = DeviceGraph.from_points(p, r, add_self_loops=loops, want_adjacency=True)
    lean, coords2 = DeviceGraph.from_points(torch.from_numpy(p).to(dev), r, add_self_loops=loops)       # points already in HBM
    assert coords.is_cuda and coords.shape == (ri.size, dim) and coords.dtype == torch.float32
    assert np.array_equal(coords.cpu().numpy(), rc) and torch.equal(coords, coords2)
    assert np.array_equal(ia, host.adj_ia) and np.array_equal(ja, host.adj_ja)
    assert (one.n_rows, one.nnz, one.n_edge_cols) == (ref.n_rows, ref.nnz, ref.n_edge_cols) == (n, host.nnz, ri.size)
    _same(one, ref)
    _same(lean, ref)
    # with lexicographic edge ids the neighbours of every row ascend (an added self loop, id 0, comes first)
    rows = np.repeat(np.arange(n), np.diff(ia))
    nb = ja[0].astype(np.int64)
    inner = (rows[1:] == rows[:-1]) & (ja[1, :-1] != 0)
    assert np.all(nb[1:][inner] > nb[:-1][inner])
    # the host-array sibling
    d = graph_type(); d.set_num_vertices(n, 1)
    c3 = d.generate_radius_adjacency_device(p, r, add_self_loops=loops)
    assert d.num_edges == ri.size and np.array_equal(c3, rc)
    assert np.array_equal(d.adj_ia, host.adj_ia) and np.array_equal(d.adj_ja, host.adj_ja)
    for g in (one, lean, ref):
        g.close()


@pytest.mark.parametrize("n,pairs,loops,edge_ids", [(60, 150, True, True), (5000, 40000, False, True), (40000, 150000, True, False),
                                                    (5, 0, True, True)])
def test_handle_from_a_device_edge_list_equals_the_host_list_route(dev, n, pairs, loops, edge_ids):
    """athena_mp_graph_create_from_edges_dev == athena_mp_graph_create_from_edges: self pairs, duplicate pairs, the
    adjacency handed back, and the message for a bad pair"""
    import torch
    from athena_amd import DeviceGraph, _capi

    rng = _rng(n + pairs)
    idx = np.asfortranarray(rng.integers(1, n + 1, (2, pairs)).astype(np.int32))
    if pairs >= 5:
        idx[:, 0] = [3, 3]
        idx[:, 1] = idx[:, 2]

    def from_dev(index):
        t = torch.from_numpy(np.ascontiguousarray(index.T)).to(dev)        # [E, 2] row-major = [2, E] column-major
        ia = np.empty(n + 1, np.int32)
        ja = np.empty((2, 2 * pairs + n), np.int32, order="F")
        nnz, h = C.c_int64(), C.c_void_p()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _capi.call("athena_mp_graph_create_from_edges_dev", n, pairs, C.c_void_p(t.data_ptr()), int(loops), int(edge_ids), vp(ia), vp(ja),
                   ja.shape[1], C.byref(nnz), C.byref(h))
        return DeviceGraph.borrow(h), h, ia, np.asfortranarray(ja[:, :nnz.value])

    ref, ria, rja = DeviceGraph.from_edges(n, idx, add_self_loops=loops, with_edge_ids=edge_ids, want_adjacency=True)
    got, h, ia, ja = from_dev(idx)
    try:
        assert np.array_equal(ia, ria) and np.array_equal(ja, rja)
        assert (got.n_rows, got.nnz, got.n_edge_cols) == (ref.n_rows, ref.nnz, ref.n_edge_cols)
        _same(got, ref)
    finally:
        _capi.call("athena_mp_graph_destroy", h)
    if pairs:
        bad = idx.copy()
        bad[1, pairs // 2] = n + 5
        msgs = []
        for build in (lambda: DeviceGraph.from_edges(n, bad, add_self_loops=loops), lambda: from_dev(bad)):
            with pytest.raises(_capi.AthenaMPError, match=r"index_list\(:,%d\) = \(%d, %d\) outside \[1,%d\]"
                               % (pairs // 2 + 1, bad[0, pairs // 2], n + 5, n)) as err:
                build()
            msgs.append(str(err.value).split("failed", 1)[1])
        assert msgs[0] == msgs[1]


@pytest.mark.parametrize("n,Fi,Fo,d,H,act", [(20000, 64, 64, 3, 64, "relu"), (700, 5, 3, 2, 7, "tanh")])
def test_gno_layer_on_the_handle_and_coords_from_points(dev, n, Fi, Fo, d, H, act):
    """graph_nop_layer_type forward and backward on (handle, coords) of from_points == the same layer on the handle built
    from the reference pairs with the reference's coords"""
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.layers import graph_nop_layer_type

    rng = _rng(n + Fi)
    p = rng.random((n, d)).astype(np.float32)
    r = degree_radius(n, 12.0, d)
    ri, rj, rc = reference_pairs(p, r)
    ref = DeviceGraph.from_edges(n, np.stack([ri + 1, rj + 1]).astype(np.int32))
    got, coords = DeviceGraph.from_points(torch.from_numpy(p).to(dev), r)
    x = torch.from_numpy(rng.uniform(-1, 1, (n, Fi)).astype(np.float32)).to(dev)
    up = torch.from_numpy(rng.uniform(-1, 1, (n, Fo)).astype(np.float32)).to(dev)
    res = []
    for handle, c in ((got, coords), (ref, torch.from_numpy(rc).to(dev))):
        layer = graph_nop_layer_type(num_outputs=Fo, coord_dim=d, kernel_hidden=H, num_inputs=Fi, use_bias=True, activation=act, seed=5)
        layer.set_params(layer.get_params() + _rng(1).standard_normal(layer.get_num_params()).astype(np.float32) * 0.05)
        layer.set_graph_handle(handle)
        out = layer.forward(x, c).clone()
        dx, dc = layer.backward(up, need_coord_grad=True)
        res.append((out, dx.clone(), dc.clone(), torch.from_numpy(layer.get_gradients())))
    assert torch.isfinite(res[0][0]).all() and res[0][0].abs().max() > 0
    for a, b, what in zip(res[0], res[1], ("output", "dx", "dcoords", "dparams")):
        assert a.shape == b.shape and torch.equal(a, b), what
    got.close(); ref.close()


def test_full_size_cloud_equals_the_reference_and_builds_are_byte_identical(dev):
    """BASELINE configs[3]'s cloud: 2 M points uniform in the unit cube (PCG64(4), cast to fp32), radius for mean degree 15"""
    import time

    import torch

    n = 2_000_000
    p = _rng(4).random((n, 3)).astype(np.float32)
    r = (15.0 / (n * 4.0 / 3.0 * np.pi)) ** (1.0 / 3.0)
    t0 = time.time()
    gi, gj, gc, pairs1, coords1 = _gpu_pairs(dev, p, r)
    t1 = time.time()
    _, _, _, pairs2, coords2 = _gpu_pairs(dev, p, r)
    assert torch.equal(pairs1, pairs2) and torch.equal(coords1.view(torch.int32), coords2.view(torch.int32))
    del pairs2, coords2
    ri, rj, rc = reference_pairs(p, r)
    print(f"2 M points: {ri.size} pairs; device query + fill + copies {t1 - t0:.2f} s, host reference {time.time() - t1:.1f} s")
    assert ri.size > 14_000_000
    assert np.array_equal(gi, ri) and np.array_equal(gj, rj)
    assert np.array_equal(gc, rc)


@pytest.mark.parametrize("dim,loops", [(3, 1), (3, 0), (2, 1), (1, 0)])
def test_fortran_program_writes_the_arrays_of_the_python_mirror(dev, tmp_path, dim, loops):
    from athena_amd.graph import graph_type

    if not os.path.exists(RUNNER):
        pytest.fail("radius_graph_run is not built: __graft_entry__.build() compiles the Fortran host side")
    n = 5000
    p = (_rng(dim + loops).random((n, dim)) - 0.5).astype(np.float32)
    r = degree_radius(n, 10.0, dim)
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(case, "wb") as f:
        f.write(np.asarray([n, dim, loops], np.int32).tobytes() + np.asarray([r], np.float32).tobytes() + p.tobytes())
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"radius_graph_run failed ({out.returncode}): {out.stderr[-2000:]}"
    g = graph_type(); g.set_num_vertices(n, 1)
    coords = g.generate_radius_adjacency_device(p, r, add_self_loops=bool(loops))
    b = open(res, "rb").read()
    hn, hdim, nnz, E = np.frombuffer(b, np.int32, 4)
    assert (hn, hdim, nnz, E) == (n, dim, g.nnz, g.num_edges) and E > n
    o = 16
    ia = np.frombuffer(b, np.int32, n + 1, o); o += 4 * (n + 1)
    ja = np.frombuffer(b, np.int32, 2 * nnz, o).reshape((2, nnz), order="F"); o += 8 * nnz
    cf = np.frombuffer(b, np.float32, dim * E, o).reshape(E, dim); o += 4 * dim * E
    assert o == len(b)
    assert np.array_equal(ia, g.adj_ia) and np.array_equal(ja, g.adj_ja) and np.array_equal(cf, coords)
    ri, rj, rc = reference_pairs(p, r)
    assert np.array_equal(cf, rc)


def test_builds_from_points_do_not_leak_device_memory(dev):
    import torch
    from athena_amd import DeviceGraph

    n = 30000
    pts = torch.from_numpy(_rng(21).random((n, 3)).astype(np.float32)).to(dev)
    r = degree_radius(n, 15.0, 3)

    def cycle():
        g, coords = DeviceGraph.from_points(pts, r, add_self_loops=True)
        assert coords.shape[0] > n
        g.close()
        del coords

    cycle()                                                            # warm: workspaces, pools
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(40):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 8 << 20, f"{(free0 - free1) >> 20} MiB of device memory lost over 40 builds from points"
