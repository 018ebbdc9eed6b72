"""GPU: athena_mp_grid_clusters (athena_amd/csrc/grid_clusters.hip) against the transcription of the definition
(tests/grid_clusters_reference.py).  Every output is compared with np.array_equal, the floats by their int32 view, on every shape
class of tests/test_grid_clusters.py, into buffers of exactly m clusters pre-filled with -1 / NaN so that an unwritten entry shows;
then the refusals, the handle and what runs on it, the reverse step, the host entries and the Fortran program."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import grid_clusters_reference as gr
import interp_reference as ir
import knn_bipartite_reference as kb
import pool_reference as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "grid_clusters_run")
vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


def _longest_row_cases():
    """exactly m clusters, m round one block of the longest-row reduction and one past its 512 blocks of 256 rows (the grid-stride
    loop wraps), all of one point but one of three: the first, the last, and 1-based row 131 072, the last of the first sweep.
    One cloud on a line, cell i at i + 1/4 (exact in float32), the cloud's corner at 0"""
    cases = []
    for m in (1, 255, 256, 257, 131073):
        line = np.arange(m, dtype=np.float64) + 0.25
        line[0] = 0.0
        for where, row in (("first", 0), ("last", m - 1), ("row 131072", 131071)):
            if row >= m or (where != "first" and row == 0):
                continue
            p = np.concatenate([line, [row + 0.5, row + 0.75]]).astype(np.float32)[:, None]
            cases.append((f"longest row {where} of {m}", np.ascontiguousarray(p), gr.offsets_of([m + 2]), 1.0, None))
    return cases


CASES = gr.shape_cases() + _longest_row_cases()
NAMES = [c[0] for c in CASES]
DEVICE_KEYS = ("cluster", "pairs", "rowptr", "weights", "centroid", "nearest", "cell")


@functools.lru_cache(None)
def _want(c):
    name, p, off, size, origin = CASES[c]
    return gr.clusters(p, off, size, origin)


def _buffers(dev, n, dim, cap):
    import torch

    i32 = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    return dict(cluster=i32(n), pairs=i32(n, 2), rowptr=i32(cap + 1), weights=f32(n), centroid=f32(cap, dim), nearest=i32(cap), cell=i32(cap, dim))


def _device(dev, p, off, size, origin=None, cap=None, keep=DEVICE_KEYS):
    """the arrays of the device as the yardstick names them, into buffers of `cap` clusters (None: the yardstick's m)"""
    import torch
    from athena_amd import _capi

    _capi.use_torch_stream()
    B, n, dim = off.size - 1, p.shape[0], p.shape[1]
    cap = gr.clusters(p, off, size, origin)["m"] if cap is None else cap
    pd = torch.from_numpy(p).to(dev)
    buf = _buffers(dev, n, dim, cap)
    coff, org = np.full(B + 1, -1, np.int32), np.full((B, dim), np.nan, np.float32)
    o = None if origin is None else np.ascontiguousarray(origin, np.float32)
    m = C.c_int64(-1)
    _capi.call("athena_mp_grid_clusters", B, n, vp(off), dim, ptr(pd), float(size), vp(o), cap,
               *(ptr(buf[k]) if k in keep else None for k in DEVICE_KEYS), vp(coff), vp(org), C.byref(m))
    torch.cuda.synchronize()
    out = {k: buf[k].cpu().numpy() for k in keep}
    out.update(cluster_offsets=coff, origin_out=org, m=int(m.value))
    return out


def _stats():
    from athena_amd import _capi

    out = np.zeros(4, np.int64)
    _capi.call("athena_mp_grid_clusters_stats", vp(out))
    return out.tolist()


@pytest.mark.parametrize("c", range(len(CASES)), ids=NAMES)
def test_the_shape_classes_of_the_cpu_tests(dev, c):
    name, p, off, size, origin = CASES[c]
    want = _want(c)
    got = _device(dev, p, off, size, origin)
    assert got["m"] == want["m"]
    assert gr.same(got, want) == [], name
    assert _stats() == [want["m"], want["bits"] if p.shape[0] and off.size > 1 else 0, want["passes"] if p.shape[0] and off.size > 1 else 0,
                        want["largest"]]
    if name == "wide key":
        assert _stats()[1] > 32 and _stats()[2] == 5


def test_two_runs_are_byte_identical_and_each_output_may_be_null_alone(dev):
    c = NAMES.index("mixed batch")
    name, p, off, size, origin = CASES[c]
    want = _want(c)
    first, again = _device(dev, p, off, size), _device(dev, p, off, size)
    for k in gr.KEYS:
        assert first[k].tobytes() == again[k].tobytes(), k
    for k in DEVICE_KEYS:
        one = _device(dev, p, off, size, keep=(k,))
        assert gr.same(one, want, (k, "cluster_offsets", "origin_out")) == [] and one["m"] == want["m"], k
    query = _device(dev, p, off, size, cap=0, keep=())
    assert query["m"] == want["m"] and gr.same(query, want, ("cluster_offsets", "origin_out")) == []
    assert _stats() == [want["m"], want["bits"], want["passes"], 0]
    roomy = _device(dev, p, off, size, cap=p.shape[0])                 # capacity n always suffices; rows beyond m stay untouched
    m = want["m"]
    assert gr.same({k: (roomy[k][:m + 1] if k == "rowptr" else roomy[k][:m] if k in ("centroid", "nearest", "cell") else roomy[k]) for k in gr.KEYS},
                   want) == []
    assert (roomy["nearest"][m:] == -1).all() and np.isnan(roomy["centroid"][m:]).all() and (roomy["rowptr"][m + 1:] == -1).all()


def test_each_cloud_alone_is_its_slice_of_the_batch(dev):
    c = NAMES.index("mixed batch")
    name, p, off, size, origin = CASES[c]
    batch = _device(dev, p, off, size)
    coff = batch["cluster_offsets"]
    for b in range(off.size - 1):
        if off[b + 1] == off[b]:
            assert coff[b + 1] == coff[b]
            continue
        one = _device(dev, np.ascontiguousarray(p[off[b]:off[b + 1]]), gr.offsets_of([off[b + 1] - off[b]]), size)
        rows, pts = slice(coff[b], coff[b + 1]), slice(off[b], off[b + 1])
        assert one["m"] == coff[b + 1] - coff[b]
        assert np.array_equal(one["cluster"] + coff[b], batch["cluster"][pts])
        assert np.array_equal(one["pairs"] + [coff[b], off[b]], batch["pairs"][pts])
        assert np.array_equal(one["rowptr"] + off[b], batch["rowptr"][coff[b]:coff[b + 1] + 1])
        assert np.array_equal(one["nearest"] + off[b], batch["nearest"][rows]) and np.array_equal(one["cell"], batch["cell"][rows])
        assert np.array_equal(one["weights"].view(np.int32), batch["weights"][pts].view(np.int32))
        assert np.array_equal(one["centroid"].view(np.int32), batch["centroid"][rows].view(np.int32))
        assert np.array_equal(one["origin_out"][0].view(np.int32), batch["origin_out"][b].view(np.int32))


def test_refusals_leave_the_library_usable(dev):
    import torch
    from athena_amd import _capi
    from athena_amd._capi import AthenaMPError

    _capi.use_torch_stream()
    c = NAMES.index("mixed batch")
    name, p, off, size, origin = CASES[c]
    want = _want(c)
    B, n = off.size - 1, p.shape[0]
    pd = torch.from_numpy(p).to(dev)
    cluster = torch.empty((n,), dtype=torch.int32, device=dev)
    m = C.c_int64()

    def call(B=B, n=n, off=off, dim=3, pd=pd, size=size, origin=None, cap=n):
        _capi.call("athena_mp_grid_clusters", B, n, vp(off), dim, ptr(pd), float(size), vp(origin), cap, ptr(cluster), None, None, None,
                   None, None, None, None, None, C.byref(m))

    def refused(match, **kw):
        with pytest.raises(AthenaMPError, match=match):
            call(**kw)
        cluster.fill_(-1)
        call()                                             # the library stays usable
        assert np.array_equal(cluster.cpu().numpy(), want["cluster"]) and m.value == want["m"]

    refused(r"dim = 4 outside \[1,3\]", dim=4)
    refused(r"dim = 0 outside \[1,3\]", dim=0)
    refused(r"size = 0 is not finite and positive", size=0.0)
    refused(r"size = -1 is not finite and positive", size=-1.0)
    refused(r"size = inf is not finite and positive", size=float("inf"))
    refused(r"size = nan is not finite and positive", size=float("nan"))
    refused(r"1 / size = inf is not finite", size=1e-45)
    refused(r"n_clouds = -1 is negative", B=-1)
    bad = off.copy(); bad[0] = 1
    refused(r"offsets\(1\) = 1, not 0", off=bad)
    bad = off.copy(); bad[5] = bad[4] - 1
    refused(rf"cloud 5: offsets descend from {off[4]} to {off[4] - 1}", off=bad)
    refused(rf"offsets end at {n}, the batch has {n + 1} points", n=n + 1)
    i = int(off[6]) + 2
    bad_p = p.copy(); bad_p[i, 1] = np.nan
    refused(rf"cloud 7: points\(2,{i + 1}\) = nan is not finite", pd=torch.from_numpy(bad_p).to(dev))
    j = int(off[8])
    bad_p = p.copy(); bad_p[j, 2] = -np.inf
    refused(rf"cloud 9: points\(3,{j + 1}\) = -inf is not finite", pd=torch.from_numpy(bad_p).to(dev))
    bad_p = p.copy(); bad_p[off[1], 0], bad_p[off[1] + 1, 0] = -3e38, 3e38
    refused(r"cloud 2: axis 1: the extent 3e\+38 - -3e\+38 is not finite", pd=torch.from_numpy(bad_p).to(dev))
    refused(r"origin\(2\) = inf is not finite", origin=np.array([0, np.inf, 0], np.float32))
    # the first cloud with points is cloud 2; on axis 3 the origin lies above some of its points: the first of them is named
    lo2 = p[off[1]:off[2]].min(axis=0)
    org = np.array([lo2[0] - 1, lo2[1] - 1, 0.5], np.float32)
    k = int(np.nonzero(p[off[1]:off[2], 2] < org[2])[0][0]) + int(off[1])
    refused(rf"cloud 2: origin\(3\) = 0\.5 is above points\(3,{k + 1}\) = ", origin=org)
    refused(r"cloud 2: axis \d: \S+ cells of size \S+, more than 2\^21", size=2.0 ** -22)
    # 2^21 cells on each axis is allowed per axis, and is 63 cell bits
    edge = np.array([[0, 0, 0], [1 - 2.0 ** -24] * 3], np.float32)
    refused(r"the keys need 1 \+ 63 bits for 1 clouds and 9223372036854775808 cells, more than 62", B=1, n=2, off=gr.offsets_of([2]),
            pd=torch.from_numpy(edge).to(dev), size=2.0 ** -21)
    refused(rf"the buffers hold {want['m'] - 1} clusters, the batch has {want['m']}", cap=want["m"] - 1)


@functools.lru_cache(None)
def _handle_case():
    c = NAMES.index("uniform and graded clouds")
    name, p, off, size, origin = CASES[c]
    return p, off, size, _want(c)


def test_the_handle_is_the_host_built_rectangular_handle(dev):
    from athena_amd import DeviceGraph

    p, off, size, want = _handle_case()
    n, m = p.shape[0], want["m"]
    i, j = want["pairs"][:, 0].astype(np.int64) - 1, want["pairs"][:, 1].astype(np.int64) - 1
    ia = (want["rowptr"] + 1).astype(np.int32)
    ja = np.asfortranarray(np.stack([j + 1, np.arange(1, n + 1)]).astype(np.int32))
    host = DeviceGraph(ia, ja, n_cols=n, n_edge_cols=n, row_deg=np.diff(want["rowptr"]), col_deg=np.ones(n, np.int64))
    got, centroid, coff, cluster, weights, nearest, cells = DeviceGraph.from_grid_clusters(p, size, off, want_nearest=True, want_cells=True)
    assert (got.n_rows, got.n_cols, got.nnz, got.n_edge_cols) == (m, n, n, n)
    for name in DeviceGraph._ARRAYS:
        a, b = got.export(name), host.export(name)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), name
    have = dict(centroid=centroid.cpu().numpy(), cluster_offsets=coff, cluster=cluster.cpu().numpy(), weights=weights.cpu().numpy(),
                nearest=nearest.cpu().numpy(), cell=cells.cpu().numpy(), rowptr=got.cluster_rowptr.cpu().numpy())
    assert gr.same(have, want, tuple(have)) == []
    short = DeviceGraph.from_grid_clusters(p[:off[1]], size)
    assert len(short) == 5 and short[0].n_rows == coff[1] and np.array_equal(short[2], [0, coff[1]])
    with_origin = DeviceGraph.from_grid_clusters(p, size, off, origin=[-2.0, -1.03, -3.5])
    assert with_origin[0].n_rows == _want(NAMES.index("uniform and graded clouds, origin below"))["m"]


def test_pooling_and_the_two_level_chain_on_the_handle(dev):
    """pool_max(handle, x=x) and interpolate(handle, weights, x) against their yardsticks; then the two-level chain from_grid_clusters
    -> from_point_sets_knn(points, centroid, k = 3) -> interp_weights -> interpolate against its numpy transcription, on integer-valued
    features (the pooled maxima are then integers too, and every yardstick here is bit-defined)"""
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.geometry import interp_weights, interpolate, pool_max

    c = NAMES.index("mixed batch")
    name, p, off, size, origin = CASES[c]
    want = _want(c)
    n, m = p.shape[0], want["m"]
    A = ir.arrays_of(want["pairs"][:, 0].astype(np.int64) - 1, want["pairs"][:, 1].astype(np.int64) - 1, m, n)
    x = gr._rng(81).integers(-50, 50, (n, 5)).astype(np.float32)
    handle, centroid, coff, cluster, weights = DeviceGraph.from_grid_clusters(p, size, off)
    xd = torch.from_numpy(x).to(dev)
    y, arg = pool_max(handle, x=xd)
    wy, warg = pr.fwd(A, x)
    assert np.array_equal(y.cpu().numpy().view(np.int32), wy.view(np.int32)) and np.array_equal(arg.cpu().numpy(), warg)
    mean = interpolate(handle, weights, xd)
    assert np.array_equal(mean.cpu().numpy().view(np.int32), ir.fwd(A, want["weights"], x).view(np.int32))
    # the way up: every point from the 3 nearest centroids of its cloud
    up, coords, eoff = DeviceGraph.from_point_sets_knn(p, centroid, k=3, query_offsets=off, source_offsets=coff)
    w, wsum = interp_weights(up, coords)
    z = interpolate(up, w, y)
    nbr, _ = kb.brute_force(p, want["centroid"], 3, None, off, want["cluster_offsets"])
    ui, uj, ucoords, _, _ = kb.graph_of(nbr, p, want["centroid"], off)
    U = ir.arrays_of(ui, uj, n, m)
    uw, _ = ir.weights(U, ucoords, 1e-16)
    assert np.array_equal(coords.cpu().numpy().view(np.int32), ucoords.view(np.int32))
    assert np.array_equal(z.cpu().numpy().view(np.int32), ir.fwd(U, uw, wy).view(np.int32))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_the_reverse_step_is_the_yardstick_bit_for_bit(dev, dim):
    import torch
    from athena_amd import DeviceGraph, _capi
    from athena_amd._capi import AthenaMPError
    from athena_amd.geometry import grid_clusters_grad

    c = NAMES.index(f"sizes 1..65 and a hub, dim {dim}")
    name, p, off, size, origin = CASES[c]
    want = _want(c)
    n, m = p.shape[0], want["m"]
    G = gr._rng(90 + dim).standard_normal((m, dim)).astype(np.float32)
    ref = gr.grad(want["cluster"], want["rowptr"], G)
    handle, centroid, coff, cluster, weights = DeviceGraph.from_grid_clusters(p, size, off)
    Gd = torch.from_numpy(G).to(dev)
    out = torch.full((n, dim), float("nan"), dtype=torch.float32, device=dev)
    got = grid_clusters_grad(cluster, handle, Gd, out=out)
    assert got is out and np.array_equal(out.cpu().numpy().view(np.int32), ref.view(np.int32))
    again = grid_clusters_grad(cluster, handle.cluster_rowptr, Gd)
    assert np.array_equal(again.cpu().numpy().view(np.int32), ref.view(np.int32))
    host = np.full((n, dim), np.nan, np.float32)
    _capi.call("athena_mp_grid_clusters_grad_host", n, dim, m, vp(want["cluster"]), vp((want["rowptr"] + 1).astype(np.int32)), vp(G), vp(host))
    assert np.array_equal(host.view(np.int32), ref.view(np.int32))
    bad = cluster.clone()
    bad[7], bad[11] = m + 1, 0
    with pytest.raises(AthenaMPError, match=rf"cluster\(8\) = {m + 1} outside \[1,{m}\]"):
        grid_clusters_grad(bad, handle, Gd)
    assert np.array_equal(grid_clusters_grad(cluster, handle, Gd).cpu().numpy().view(np.int32), ref.view(np.int32))


def _host(p, off, size, origin, want):
    from athena_amd import _capi

    B, n, dim, m = off.size - 1, p.shape[0], p.shape[1], want["m"]
    o = None if origin is None else np.ascontiguousarray(origin, np.float32)
    coff, org, count = np.full(B + 1, -1, np.int32), np.full((B, dim), np.nan, np.float32), C.c_int64(-1)
    _capi.call("athena_mp_grid_clusters_host", B, n, vp(off), dim, vp(p), float(size), vp(o), 0, None, None, None, None, None, None, None,
               vp(coff), vp(org), C.byref(count))
    assert count.value == m and np.array_equal(coff, want["cluster_offsets"])
    out = dict(cluster=np.full(n, -1, np.int32), adj_ia=np.full(m + 1, -1, np.int32), adj_ja=np.full((n, 2), -1, np.int32),
               weights=np.full(n, np.nan, np.float32), centroid=np.full((m, dim), np.nan, np.float32), nearest=np.full(m, -1, np.int32),
               cell=np.full((m, dim), -1, np.int32))
    _capi.call("athena_mp_grid_clusters_host", B, n, vp(off), dim, vp(p), float(size), vp(o), m, *(vp(a) for a in out.values()), vp(coff),
               vp(org), C.byref(count))
    out.update(cluster_offsets=coff, origin_out=org, m=int(count.value))
    return out


def _assert_host_arrays(got, want):
    n = want["cluster"].size
    assert got["m"] == want["m"]
    assert gr.same(got, want, ("cluster", "weights", "centroid", "nearest", "cell", "cluster_offsets", "origin_out")) == []
    assert np.array_equal(got["adj_ia"], want["rowptr"] + 1)
    assert np.array_equal(got["adj_ja"][:, 0], want["pairs"][:, 1]) and np.array_equal(got["adj_ja"][:, 1], np.arange(1, n + 1))


@pytest.mark.parametrize("name", ["mixed batch", "uniform and graded clouds, origin below", "n = 0"])
def test_the_host_form_agrees_with_the_yardstick(dev, name):
    from athena_amd import _capi
    from athena_amd._capi import AthenaMPError

    c = NAMES.index(name)
    _, p, off, size, origin = CASES[c]
    want = _want(c)
    _assert_host_arrays(_host(p, off, size, origin, want), want)
    if want["m"] > 0:
        with pytest.raises(AthenaMPError, match=rf"the buffers hold {want['m'] - 1} clusters, the batch has {want['m']}"):
            n, dim, m = p.shape[0], p.shape[1], C.c_int64()
            ia, ja = np.zeros(want["m"] + 1, np.int32), np.zeros((n, 2), np.int32)
            o = None if origin is None else np.ascontiguousarray(origin, np.float32)
            _capi.call("athena_mp_grid_clusters_host", off.size - 1, n, vp(off), dim, vp(p), float(size), vp(o), want["m"] - 1, None, vp(ia),
                       vp(ja), None, None, None, None, None, None, C.byref(m))


@pytest.mark.parametrize("has_origin", [0, 1])
def test_fortran_program_writes_the_arrays_of_the_yardstick(dev, tmp_path, has_origin):
    if not os.path.exists(RUNNER):
        pytest.fail("grid_clusters_run is not built: __graft_entry__.build() compiles the Fortran host side")
    c = NAMES.index("uniform and graded clouds, origin below" if has_origin else "mixed batch")
    name, p, off, size, origin = CASES[c]
    want = _want(c)
    B, n, dim, m = off.size - 1, p.shape[0], p.shape[1], want["m"]
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        np.array([B, n, dim, has_origin], np.int32).tofile(f)
        np.array([size, *(origin if has_origin else (0, 0, 0))], np.float32).tofile(f)
        off.tofile(f); p.tofile(f)
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"grid_clusters_run failed ({out.returncode}): {out.stdout[-1000:]} {out.stderr[-2000:]}"
    raw = open(res, "rb").read()
    at = 0

    def take(dtype, *shape):
        nonlocal at
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at).reshape(shape)
        at += a.nbytes
        return a

    assert take(np.int64, 1)[0] == m
    got = dict(cluster=take(np.int32, n), adj_ia=take(np.int32, m + 1), adj_ja=take(np.int32, n, 2), weights=take(np.float32, n),
               centroid=take(np.float32, m, dim), nearest=take(np.int32, m), cell=take(np.int32, m, dim), cluster_offsets=take(np.int32, B + 1),
               origin_out=take(np.float32, B, dim), m=m)
    _assert_host_arrays(got, want)
    dcentroid = (np.arange(1, m + 1)[:, None] + np.arange(1, dim + 1)[None, :]).astype(np.float32)
    assert np.array_equal(take(np.float32, n, dim).view(np.int32), gr.grad(want["cluster"], want["rowptr"], dcentroid).view(np.int32))
    assert take(np.int64, 4).tolist() == [m, want["bits"], want["passes"], want["largest"]] and at == len(raw)
