"""GPU: periodic structures -> neighbour graphs on the device (athena_amd/csrc/periodic_graph.hip; athena_mp_periodic_pairs,
athena_mp_periodic_graph_host and their Python / Fortran mirrors) against the yardstick of tests/periodic_reference.py.  The
definition leaves no freedom: integers and fp32 arrays are compared with np.array_equal / torch.equal, no tolerance.

The yardstick evaluates every candidate of a range three wider than the bound, so a large batch is built from a few hundred
DISTINCT structures repeated (the expected arrays of a repeated structure are those of the first, shifted), and the structures
in strongly skewed cells are kept to 1 - 8 atoms."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import periodic_reference as pr
from test_gpu_graph_build import NAMES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "periodic_graph_run")
FIXTURE = os.path.join(ROOT, "tests", "golden", "msgpass_chemical_head.xyz")
FIXTURE_EDGES = 1849
LDS_ATOMS = 128                       # kLdsAtoms of periodic_graph.hip: larger structures are read from global memory
KEYS = ("pairs", "feature", "vec", "shift", "first_count", "edge_offsets")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _pairs_call(dev, frac, lat, off, cmin, cmax, pbc=(1, 1, 1), capacity=None, fill=True):
    """athena_mp_periodic_pairs: size query, then (fill) every output into sentinel-filled buffers -> dict of numpy arrays cut to
    the edge count, plus the raw tensors under 'raw'"""
    import torch
    from athena_amd import _capi

    frac = np.ascontiguousarray(frac, np.float32).reshape(-1, 3)
    lat = np.ascontiguousarray(lat, np.float32).reshape(-1, 3, 3)
    off = np.ascontiguousarray(off, np.int32)
    pbc3 = np.asarray(pbc, np.int32)
    B, n = lat.shape[0], frac.shape[0]
    fd, ld = torch.from_numpy(frac).to(dev), torch.from_numpy(lat).to(dev)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    head = (B, n, vp(off), ptr(fd), ptr(ld), vp(pbc3), float(cmin), float(cmax))
    _capi.use_torch_stream()
    E = C.c_int64(-1)
    _capi.call("athena_mp_periodic_pairs", *head, None, None, None, None, None, 0, C.byref(E), None)
    q = E.value
    if not fill:
        return q
    cap = q if capacity is None else capacity
    pairs = torch.full((max(cap, 0), 2), -7, dtype=torch.int32, device=dev)
    feature = torch.full((max(cap, 0),), np.nan, dtype=torch.float32, device=dev)
    vec = torch.full((max(cap, 0), 3), np.nan, dtype=torch.float32, device=dev)
    shift = torch.full((max(cap, 0), 3), -99, dtype=torch.int32, device=dev)
    first = torch.full((n,), -5, dtype=torch.int32, device=dev)
    eoff = np.full(B + 1, -1, np.int64)
    E2 = C.c_int64(-1)
    _capi.call("athena_mp_periodic_pairs", *head, ptr(pairs), ptr(feature), ptr(vec), ptr(shift), ptr(first), cap, C.byref(E2), vp(eoff))
    torch.cuda.synchronize()
    assert E2.value == q, "the size query and the fill disagree"
    return {"pairs": np.asfortranarray(pairs.cpu().numpy()[:q].T), "feature": feature.cpu().numpy()[:q], "vec": vec.cpu().numpy()[:q],
            "shift": shift.cpu().numpy()[:q], "first_count": first.cpu().numpy(), "edge_offsets": eoff,
            "raw": (pairs, feature, vec, shift, first)}


def _equal(got, want, what=""):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs from the yardstick"


def _structures(rng, kind, sizes, max_range=12):
    """distinct random structures: [(frac rows, lattice)]"""
    out = []
    for m in sizes:
        k = kind if isinstance(kind, str) else kind[len(out) % len(kind)]
        if k == "skewed":
            m = min(m, 1 + m % 8)
        out.append((rng.random((m, 3)).astype(np.float32), pr.random_cell(rng, k, max_range)))
    return out


def _batch(distinct, order):
    """the batch that holds distinct[k] for k in order (None: an empty structure, lattice of the first) -> frac, lat, offsets"""
    rows = [distinct[k][0] if k is not None else np.zeros((0, 3), np.float32) for k in order]
    lat = np.array([distinct[k if k is not None else 0][1] for k in order], np.float32).reshape(-1, 3, 3)
    off = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int32)
    return np.concatenate(rows + [np.zeros((0, 3), np.float32)]).astype(np.float32), lat, off


def _expected(distinct, order, off, cmin, cmax, pbc=(1, 1, 1)):
    per = [pr.structure_edges(f, L, cmin, cmax, pbc) for f, L in distinct]
    empty = pr.structure_edges(np.zeros((0, 3), np.float32), distinct[0][1], cmin, cmax, pbc)
    return pr.assemble([per[k] if k is not None else empty for k in order], off, cmax)


def _sizes(rng, count):
    """1, 2 and 8 - 30 atoms"""
    s = [1, 2] + list(rng.integers(8, 31, max(count - 2, 0)))
    return [int(v) for v in s[:count]]


def _fixture():
    from athena_amd import io

    return io.structures_from_frames(io.read_extxyz(FIXTURE))


def test_fixture_equals_the_yardstick(dev):
    frac, lat, off = _fixture()
    want = pr.reference_edges(frac, lat, off, 0.5, 3.0)
    got = _pairs_call(dev, frac, lat, off, 0.5, 3.0)
    assert got["pairs"].shape == (2, FIXTURE_EDGES)
    _equal(got, want, "fixture")
    assert np.all(got["pairs"][0] <= got["pairs"][1])


@pytest.mark.parametrize("kind", ["cubic", "skewed", "small"])
@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_random_batches_equal_the_yardstick(dev, kind, B):
    rng = _rng(B * 7 + len(kind))
    distinct = _structures(rng, kind, _sizes(rng, B) if B > 1 else [int(rng.integers(8, 31))])
    order = list(range(B))
    if B > 1:
        order[B // 2] = None                                               # an empty structure in the middle
        order[-1] = None                                                   # ... and one at the end
    frac, lat, off = _batch(distinct, order)
    cmin = 0.5 if kind != "small" else 0.0
    want = _expected(distinct, order, off, cmin, 3.0)
    got = _pairs_call(dev, frac, lat, off, cmin, 3.0)
    print(f"{kind}, {B} structures, {off[-1]} atoms: {want['pairs'].shape[1]} edges")
    _equal(got, want, f"{kind} x {B}")
    assert want["pairs"].shape[1] > 0
    if kind == "skewed":
        assert max(max(pr.half_ranges(L, 3.0)) for _, L in distinct) >= 5
    if kind == "small":
        own = want["pairs"][0] == want["pairs"][1]
        assert own.any() and not np.any(np.all(want["shift"][own] == 0, axis=1))          # self images, never the zero shift
        key = want["pairs"][0].astype(np.int64) * (off[-1] + 1) + want["pairs"][1]
        assert np.bincount(np.unique(key, return_inverse=True)[1]).max() > 1              # several edges on one pair


def test_twenty_thousand_structures_equal_the_yardstick(dev):
    rng = _rng(77)
    D, B = 400, 20_000
    distinct = _structures(rng, ("cubic", "small", "cubic", "skewed"), _sizes(rng, D), max_range=8)
    order = [int(k) for k in rng.integers(0, D, B)]
    for k in (5, B // 3, B // 3 + 1, B - 2, B - 1):
        order[k] = None
    frac, lat, off = _batch(distinct, order)
    want = _expected(distinct, order, off, 0.5, 3.0)
    got = _pairs_call(dev, frac, lat, off, 0.5, 3.0)
    print(f"{B} structures, {off[-1]} atoms: {want['pairs'].shape[1]} edges")
    assert want["pairs"].shape[1] > 10 * B
    _equal(got, want, "20 000 structures")


def test_structures_above_the_lds_switch_and_above_one_work_item(dev):
    """150 atoms (read from global memory, rows cut into several work items) and 600 atoms (one row is a work item of its own)
    between small structures"""
    rng = _rng(31)
    distinct = _structures(rng, "cubic", [12, 9])
    distinct.insert(1, (rng.random((LDS_ATOMS + 22, 3)).astype(np.float32), (np.eye(3) * 12.0).astype(np.float32)))
    distinct.append((rng.random((600, 3)).astype(np.float32), (np.eye(3) * 20.0).astype(np.float32)))
    distinct.append((rng.random((LDS_ATOMS, 3)).astype(np.float32), (np.eye(3) * 11.0).astype(np.float32)))   # the last size in LDS
    order = [0, 1, 2, None, 3, 4]
    frac, lat, off = _batch(distinct, order)
    want = _expected(distinct, order, off, 0.5, 3.0)
    got = _pairs_call(dev, frac, lat, off, 0.5, 3.0)
    assert want["pairs"].shape[1] > 3000
    _equal(got, want, "large structures")


@pytest.mark.parametrize("pbc", [(0, 1, 1), (1, 0, 1), (1, 1, 0)])
def test_one_open_axis(dev, pbc):
    rng = _rng(41 + pbc.index(0))
    distinct = _structures(rng, ("small", "cubic", "skewed"), _sizes(rng, 12), max_range=8)
    order = list(range(12))
    frac, lat, off = _batch(distinct, order)
    want = _expected(distinct, order, off, 0.0, 3.0, pbc)
    got = _pairs_call(dev, frac, lat, off, 0.0, 3.0, pbc)
    _equal(got, want, f"pbc {pbc}")
    assert want["pairs"].shape[1] > 0 and np.all(got["shift"][:, pbc.index(0)] == 0) and np.any(got["shift"] != 0)


def test_open_box_with_identity_lattice_equals_the_radius_graph(dev):
    """pbc = (0,0,0), lat = identity, cutoff_min = 0, no coincident points: x = p_i - p_j and s is the radius builder's sum.  That
    one keeps s <= fl(r * r), this one sqrt(s) < r: the radius is put between two neighbouring distances of the cloud, so no pair
    sits on the boundary"""
    import torch

    n = 1500
    p = _rng(51).random((n, 3)).astype(np.float32)
    i, j = np.triu_indices(n, 1)
    d = p[i] - p[j]
    s = np.sort((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    k = 20_000
    while not (s[k + 1] > s[k] * np.float32(1.0001)):                       # a gap far wider than any rounding of sqrt or r * r
        k += 1
    r = float(np.sqrt(0.5 * (float(s[k]) + float(s[k + 1]))))
    assert s[0] > 0
    got = _pairs_call(dev, p, np.eye(3, dtype=np.float32)[None], [0, n], 0.0, r, (0, 0, 0))
    from athena_amd import _capi

    pts = torch.from_numpy(p).to(dev)
    E = C.c_int64()
    _capi.call("athena_mp_radius_pairs", n, 3, C.c_void_p(pts.data_ptr()), r, None, None, 0, C.byref(E))
    assert E.value == k + 1 == got["pairs"].shape[1]
    pairs = torch.empty((E.value, 2), dtype=torch.int32, device=dev)
    coords = torch.empty((E.value, 3), dtype=torch.float32, device=dev)
    _capi.call("athena_mp_radius_pairs", n, 3, C.c_void_p(pts.data_ptr()), r, C.c_void_p(pairs.data_ptr()), C.c_void_p(coords.data_ptr()),
               E.value, C.byref(E))
    assert torch.equal(pairs, got["raw"][0]) and np.array_equal(coords.cpu().numpy(), got["vec"])
    assert np.all(got["shift"] == 0)


def test_size_query_untouched_capacity_and_byte_identical_builds(dev):
    import torch

    rng = _rng(61)
    distinct = _structures(rng, ("small", "cubic"), _sizes(rng, 40))
    order = list(range(40))
    frac, lat, off = _batch(distinct, order)
    q = _pairs_call(dev, frac, lat, off, 0.5, 3.0, fill=False)
    a = _pairs_call(dev, frac, lat, off, 0.5, 3.0, capacity=q + 9)          # asserts query == fill count
    b = _pairs_call(dev, frac, lat, off, 0.5, 3.0, capacity=q + 9)
    assert q == a["pairs"].shape[1] > 0
    pairs, feature, vec, shift, first = a["raw"]
    assert torch.all(pairs[q:] == -7) and torch.all(shift[q:] == -99)
    assert torch.isnan(feature[q:]).all() and torch.isnan(vec[q:]).all()
    assert not torch.isnan(feature[:q]).any() and torch.all(first >= 0)
    for x, y in zip(a["raw"], b["raw"]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert np.array_equal(a["edge_offsets"], b["edge_offsets"])


def test_refusals_name_the_structure_and_leave_the_library_usable(dev):
    import torch
    from athena_amd import _capi

    rng = _rng(71)
    distinct = _structures(rng, "cubic", _sizes(rng, 10))
    order = list(range(10))
    frac, lat, off = _batch(distinct, order)
    want = _expected(distinct, order, off, 0.5, 3.0)
    E = want["pairs"].shape[1]
    call = lambda **kw: _pairs_call(dev, kw.get("frac", frac), kw.get("lat", lat), kw.get("off", off), kw.get("cmin", 0.5),
                                    kw.get("cmax", 3.0), kw.get("pbc", (1, 1, 1)), kw.get("capacity"), kw.get("fill", False))
    bad = off.copy(); bad[4] = bad[3] - 1
    with pytest.raises(_capi.AthenaMPError, match=r"structure 4: offsets descend from %d to %d" % (bad[3], bad[4])):
        call(off=bad)
    bad = off.copy(); bad[0] = 1
    with pytest.raises(_capi.AthenaMPError, match=r"offsets\(1\) = 1, not 0"):
        call(off=bad)
    bad = off.copy(); bad[-1] -= 1
    with pytest.raises(_capi.AthenaMPError, match=r"offsets end at %d, the batch has %d atoms" % (bad[-1], off[-1])):
        call(off=bad)
    for value, text in ((np.nan, "-?nan"), (np.inf, "inf")):
        f = frac.copy(); f[off[6] + 1, 2] = value; f[off[8], 0] = np.nan          # a later one: the FIRST is named
        with pytest.raises(_capi.AthenaMPError, match=r"structure 7: frac\(3,%d\) = %s is not finite" % (off[6] + 2, text)):
            call(frac=f)
        L = lat.copy(); L[3, 1, 2] = value; L[9, 0, 0] = np.inf
        with pytest.raises(_capi.AthenaMPError, match=r"structure 4: lat\(2,3\) = %s is not finite" % text):
            call(lat=L)
    L = lat.copy(); L[5, 2] = L[5, 0] + L[5, 1]; L[5, 1] = 2 * L[5, 0]            # coplanar: no volume
    with pytest.raises(_capi.AthenaMPError, match=r"structure 6: det\(lat\) is zero or not finite"):
        call(lat=L)
    assert call(lat=L, pbc=(0, 0, 0)) >= 0                                       # ... which an open box does not need
    for cmin, cmax in ((0.5, np.inf), (np.nan, 3.0)):
        with pytest.raises(_capi.AthenaMPError, match=r"cutoffs \(.*\) are not finite"):
            call(cmin=cmin, cmax=cmax)
    for cmin, cmax in ((-0.1, 3.0), (3.0, 3.0), (3.0, 0.5)):
        with pytest.raises(_capi.AthenaMPError, match=r"need 0 <= cutoff_min < cutoff_max"):
            call(cmin=cmin, cmax=cmax)
    L = lat.copy(); L[2] = np.eye(3, dtype=np.float32) * np.float32(0.09)       # 3 / 0.09 = 33.3: above 31
    with pytest.raises(_capi.AthenaMPError, match=r"structure 3: half-range 33 on axis 1 is above 31: the cell is too small"):
        call(lat=L)
    with pytest.raises(_capi.AthenaMPError, match=r"buffers hold %d edges, the batch has %d" % (E - 1, E)):
        call(capacity=E - 1, fill=True)
    # 200 structures of 10 atoms in cells of edge 0.1: some 113 000 images per pair, 1.2e9 edges; the count pass finds it and
    # nothing of that size is allocated
    crowd_f = rng.random((2000, 3)).astype(np.float32)
    crowd_L = np.tile((np.eye(3) * 0.1).astype(np.float32), (200, 1, 1))
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(_capi.AthenaMPError, match=r"1\d{9} edges among 2000 atoms: more than 2\^31 CSR entries"):
        call(frac=crowd_f, lat=crowd_L, off=np.arange(201) * 10)
    with pytest.raises(_capi.AthenaMPError, match=r"more than 2\^31 CSR entries"):
        from athena_amd import DeviceGraph
        DeviceGraph.from_structures(crowd_f, crowd_L, np.arange(201) * 10, 0.5, 3.0)
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 8 << 20
    _equal(call(fill=True), want, "after the refusals")                          # the library is usable afterwards


def _same(a, b):
    for n in NAMES:
        x, y = a.export(n), b.export(n)
        assert x.shape == y.shape, n
        assert np.array_equal(x, y), f"{n} differs"


@pytest.mark.parametrize("loops", [False, True])
def test_handle_from_structures_equals_handle_from_the_yardstick_pairs(dev, loops):
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.graph import graph_type

    rng = _rng(81)
    distinct = _structures(rng, ("cubic", "small", "skewed"), _sizes(rng, 60), max_range=8)
    order = [int(k) for k in rng.integers(0, 60, 300)]
    order[100] = order[-1] = None
    frac, lat, off = _batch(distinct, order)
    want = _expected(distinct, order, off, 0.5, 3.0)
    n, E = int(off[-1]), want["pairs"].shape[1]
    assert np.any(want["pairs"][0] == want["pairs"][1])                          # self-image edges: one CSR entry each
    ref = DeviceGraph.from_edges(n, want["pairs"], add_self_loops=loops)
    host = graph_type(); host.set_num_vertices(n, 1); host.generate_adjacency(want["pairs"])
    if loops:
        host.add_self_loops()
    one, feature, vec, voff, eoff, ia, ja = DeviceGraph.from_structures(frac, lat, off, 0.5, 3.0, add_self_loops=loops, want_adjacency=True)
    lean, feature2, vec2, _, _ = DeviceGraph.from_structures(torch.from_numpy(frac).to(dev), torch.from_numpy(lat).to(dev), off, 0.5, 3.0,
                                                             add_self_loops=loops)
    assert feature.is_cuda and feature.shape == (E,) and vec.shape == (E, 3)
    assert np.array_equal(feature.cpu().numpy(), want["feature"]) and np.array_equal(vec.cpu().numpy(), want["vec"])
    assert torch.equal(feature, feature2) and torch.equal(vec, vec2)
    assert voff.dtype == np.int32 and np.array_equal(voff, off) and eoff.dtype == np.int64 and np.array_equal(eoff, want["edge_offsets"])
    assert np.array_equal(ia, host.adj_ia) and np.array_equal(ja, host.adj_ja)
    assert (one.n_rows, one.nnz, one.n_edge_cols) == (ref.n_rows, ref.nnz, ref.n_edge_cols) == (n, host.nnz, E)
    _same(one, ref)
    _same(lean, ref)
    # the host-array sibling
    d = graph_type(); d.set_num_vertices(n, 1)
    f3, v3, first, e3 = d.generate_periodic_adjacency_device(frac, lat, off, 0.5, 3.0, add_self_loops=loops)
    assert d.num_edges == E and np.array_equal(f3, want["feature"]) and np.array_equal(v3, want["vec"])
    assert np.array_equal(first, want["first_count"]) and np.array_equal(e3, want["edge_offsets"])
    assert np.array_equal(d.adj_ia, host.adj_ia) and np.array_equal(d.adj_ja, host.adj_ja)
    for g in (one, lean, ref):
        g.close()


@pytest.mark.parametrize("Fv,Fe,T,O,MX", [(64, 8, 2, 16, 10), (6, 1, 4, 10, 10)])
def test_duvenaud_layer_on_the_handle_from_structures(dev, Fv, Fe, T, O, MX):
    """duvenaud_msgpass_layer_type on 2 000 structures through set_graph_handle(handle, vertex_offsets) == the same layer through
    set_graph_batched on the host-assembled graph of the yardstick's pairs: outputs and every gradient, bit for bit.  (64 / 8 with
    the edge feature tiled, and msgpass_chemical's widths: 6 vertex features, 1 edge feature, 4 steps, 10 outputs, degree 10.)"""
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.graph import graph_type
    from athena_amd.layers import duvenaud_msgpass_layer_type

    rng = _rng(91)
    D, B = 200, 2000
    distinct = _structures(rng, ("cubic", "cubic", "small"), _sizes(rng, D))
    order = [int(k) for k in rng.integers(0, D, B)]
    order[B // 2] = None
    frac, lat, off = _batch(distinct, order)
    want = _expected(distinct, order, off, 0.5, 3.0)
    n, E = int(off[-1]), want["pairs"].shape[1]
    host = graph_type(); host.set_num_vertices(n, Fv); host.generate_adjacency(want["pairs"]); host.num_edges = E
    handle, feature, vec, voff, eoff = DeviceGraph.from_structures(frac, lat, off, 0.5, 3.0)
    assert np.array_equal(feature.cpu().numpy(), want["feature"])
    x = torch.from_numpy(rng.uniform(-1, 1, (n, Fv)).astype(np.float32)).to(dev)
    up = torch.from_numpy(rng.uniform(-1, 1, (B, O)).astype(np.float32)).to(dev)
    res = []
    for route in ("handle", "host"):
        layer = duvenaud_msgpass_layer_type(num_vertex_features=[Fv], num_edge_features=[Fe], num_time_steps=T, max_vertex_degree=MX,
                                            num_outputs=O, min_vertex_degree=1, seed=3)
        if route == "handle":
            layer.set_graph_handle(handle, voff)
            e = feature[:, None].repeat(1, Fe).contiguous()
        else:
            layer.set_graph_batched(host, off)
            e = torch.from_numpy(np.tile(want["feature"][:, None], (1, Fe))).to(dev)
        assert layer.graph.batch == B
        out = layer.forward(x, e).clone()
        dx, de = layer.backward(up, need_input_grad=True, need_edge_grad=True)
        res.append((out, dx.clone(), de.clone(), torch.from_numpy(layer.get_gradients())))
    assert res[0][0].shape == (B, O) and torch.isfinite(res[0][0]).all() and res[0][0].abs().max() > 0
    for a, b, what in zip(res[0], res[1], ("output", "dx", "de", "dparams")):
        assert a.shape == b.shape and torch.equal(a, b), what
    handle.close()


@pytest.mark.parametrize("loops,pbc", [(1, (1, 1, 1)), (0, (1, 1, 0))])
def test_fortran_program_writes_the_arrays_of_the_python_mirror(dev, tmp_path, loops, pbc):
    from athena_amd.graph import graph_type

    if not os.path.exists(RUNNER):
        pytest.fail("periodic_graph_run is not built: __graft_entry__.build() compiles the Fortran host side")
    rng = _rng(101 + loops)
    distinct = _structures(rng, ("cubic", "small", "skewed"), _sizes(rng, 50), max_range=8)
    order = list(range(50)); order[20] = None
    frac, lat, off = _batch(distinct, order)
    B, n = lat.shape[0], frac.shape[0]
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(case, "wb") as f:
        f.write(np.asarray([B, n, loops, *pbc], np.int32).tobytes() + np.asarray([0.5, 3.0], np.float32).tobytes() + off.tobytes()
                + frac.tobytes() + lat.tobytes())
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"periodic_graph_run failed ({out.returncode}): {out.stderr[-2000:]}"
    g = graph_type(); g.set_num_vertices(n, 1)
    feature, vec, first, eoff = g.generate_periodic_adjacency_device(frac, lat, off, 0.5, 3.0, pbc=pbc, add_self_loops=bool(loops))
    b = open(res, "rb").read()
    hB, hn, nnz, E = np.frombuffer(b, np.int32, 4)
    assert (hB, hn, nnz, E) == (B, n, g.nnz, g.num_edges) and E > n
    o = 16
    ia = np.frombuffer(b, np.int32, n + 1, o); o += 4 * (n + 1)
    ja = np.frombuffer(b, np.int32, 2 * nnz, o).reshape((2, nnz), order="F"); o += 8 * nnz
    ff = np.frombuffer(b, np.float32, E, o); o += 4 * E
    vf = np.frombuffer(b, np.float32, 3 * E, o).reshape(E, 3); o += 12 * E
    fc = np.frombuffer(b, np.int32, n, o); o += 4 * n
    eo = np.frombuffer(b, np.int64, B + 1, o); o += 8 * (B + 1)
    assert o == len(b)
    assert np.array_equal(ia, g.adj_ia) and np.array_equal(ja, g.adj_ja)
    assert np.array_equal(ff, feature) and np.array_equal(vf, vec) and np.array_equal(fc, first) and np.array_equal(eo, eoff)
    want = _expected(distinct, order, off, 0.5, 3.0, pbc)
    assert np.array_equal(ff, want["feature"]) and np.array_equal(vf, want["vec"]) and np.array_equal(fc, want["first_count"])


def test_builds_from_structures_do_not_leak_device_memory(dev):
    import torch
    from athena_amd import DeviceGraph

    rng = _rng(111)
    distinct = _structures(rng, "cubic", _sizes(rng, 100))
    frac, lat, off = _batch(distinct, [int(k) for k in rng.integers(0, 100, 3000)])
    fd, ld = torch.from_numpy(frac).to(dev), torch.from_numpy(lat).to(dev)

    def cycle():
        g, feature, vec, _, _ = DeviceGraph.from_structures(fd, ld, off, 0.5, 3.0, add_self_loops=True)
        assert feature.shape[0] > off[-1]
        g.close()
        del feature, vec

    cycle()                                                            # warm: workspaces, pools
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(40):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 8 << 20, f"{(free0 - free1) >> 20} MiB of device memory lost over 40 builds from structures"
