"""GPU: athena_mp_contract_pairs, athena_mp_graph_pairs and athena_mp_cell_pairs (athena_amd/csrc/contract.hip) against the
transcription of the definition (tests/contract_reference.py).  Every output is compared with np.array_equal, the floats by their
int32 view, on every shape class of tests/test_contract.py, into buffers of exactly P coarse pairs and M members pre-filled with
-1 / NaN so that an unwritten entry shows; then the refusals, the two small entries, the chain from points to a pooled graph with
what runs on its handles, the host entry and the Fortran program."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import contract_reference as cr
import interp_reference as ir
import pool_reference as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "contract_run")
vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


def _longest_row_cases():
    """exactly P coarse pairs, P round one block of the longest-row reduction and one past its 512 blocks of 256 rows (the grid-stride
    loop wraps), all of one member but one of three: the first, the last, and 1-based row 131 072, the last of the first sweep.
    The chain i -- i + 1 under the identity map; P = 0 is "every edge dropped" of the shared cases"""
    cases = []
    for P in (1, 255, 256, 257, 131073):
        chain = np.stack([np.arange(1, P + 1), np.arange(2, P + 2)], axis=1)
        for where, row in (("first", 0), ("last", P - 1), ("row 131072", 131071)):
            if row >= P or (where != "first" and row == 0):
                continue
            pairs = np.concatenate([chain, chain[[row, row]][:, ::-1]]).astype(np.int32)          # twice more, given high-low
            cases.append((f"longest row {where} of {P}", dict(pairs=pairs, n_rows=P + 1, n_cols=P + 1, row_cluster=None, col_cluster=None,
                                                               m_rows=P + 1, m_cols=P + 1, mode=0, row_points=None, col_points=None)))
    return tuple(cases)


CASES = cr.shape_cases() + _longest_row_cases()
NAMES = [c[0] for c in CASES]


@functools.lru_cache(None)
def _want(c):
    return cr.contract(*cr.args_of(CASES[c][1]))


def _buffers(dev, E, P, M, dim):
    import torch

    i32 = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    return dict(coarse_pairs=i32(P, 2), rowptr=i32(P + 1), members=i32(M, 2), weights=f32(M), edge_pair=i32(E), coords=f32(P, max(dim, 1)))


def _device(dev, kw, keep=None, cap=None, mcap=None, **change):
    """the arrays of the device as the yardstick names them, into buffers of cap coarse pairs and mcap members (None: the yardstick's)"""
    import torch
    from athena_amd import _capi

    _capi.use_torch_stream()
    kw = dict(kw, **change)
    want = cr.contract(*cr.args_of(kw)) if cap is None or mcap is None else None
    cap = want["P"] if cap is None else cap
    mcap = want["M"] if mcap is None else mcap
    E = kw["pairs"].shape[0]
    dim = kw["row_points"].shape[1] if kw["row_points"] is not None else 0
    keep = tuple(k for k in cr.KEYS if dim or k != "coords") if keep is None else keep
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pd, rc, rp = up(kw["pairs"]), up(kw["row_cluster"]), up(kw["row_points"])
    cc = rc if kw["col_cluster"] is kw["row_cluster"] else up(kw["col_cluster"])
    cp = rp if kw["col_points"] is kw["row_points"] else up(kw["col_points"])
    buf = _buffers(dev, E, cap, mcap, dim)
    P, M = C.c_int64(-1), C.c_int64(-1)
    _capi.call("athena_mp_contract_pairs", E, ptr(pd), kw["n_rows"], kw["n_cols"], ptr(rc), ptr(cc), kw["m_rows"], kw["m_cols"], kw["mode"], dim,
               ptr(rp), ptr(cp), cap, mcap, *(ptr(buf[k]) if k in keep else None for k in cr.KEYS), C.byref(P), C.byref(M))
    torch.cuda.synchronize()
    out = {k: buf[k].cpu().numpy() for k in keep}
    out.update(P=int(P.value), M=int(M.value))
    assert torch.equal(pd, torch.from_numpy(kw["pairs"]).to(dev))
    return out


def _stats():
    from athena_amd import _capi

    out = np.zeros(4, np.int64)
    _capi.call("athena_mp_contract_stats", vp(out))
    return out.tolist()


@pytest.mark.parametrize("c", range(len(CASES)), ids=NAMES)
def test_the_shape_classes_of_the_cpu_tests(dev, c):
    name, kw = CASES[c]
    want = _want(c)
    got = _device(dev, kw)
    assert (got["P"], got["M"]) == (want["P"], want["M"])
    assert cr.same(got, want, tuple(k for k in cr.KEYS if k in got)) == [], name
    assert _stats() == [want["P"], want["M"], want["bits"], want["largest"]]


def test_two_runs_are_byte_identical_and_each_output_may_be_null_alone(dev):
    c = NAMES.index("three tiles, 300 clusters, mode 0")
    name, kw = CASES[c]
    want = _want(c)
    first, again = _device(dev, kw), _device(dev, kw)
    for k in cr.KEYS:
        assert first[k].tobytes() == again[k].tobytes(), k
    for k in cr.KEYS:
        one = _device(dev, kw, keep=(k,))
        assert cr.same(one, want, (k,)) == [] and (one["P"], one["M"]) == (want["P"], want["M"]), k
    query = _device(dev, kw, keep=(), cap=0, mcap=0)
    assert (query["P"], query["M"]) == (want["P"], want["M"])
    assert _stats() == [want["P"], want["M"], want["bits"], 0]
    E = kw["pairs"].shape[0]
    roomy = _device(dev, kw, cap=E, mcap=E)                            # n_pairs always suffices; rows beyond P and M stay untouched
    P, M = want["P"], want["M"]
    cut = dict(coarse_pairs=P, rowptr=P + 1, members=M, weights=M, edge_pair=E, coords=P)
    assert cr.same({k: roomy[k][:cut[k]] for k in cr.KEYS}, want) == []
    assert (roomy["coarse_pairs"][P:] == -1).all() and (roomy["rowptr"][P + 1:] == -1).all() and (roomy["members"][M:] == -1).all()
    assert np.isnan(roomy["weights"][M:]).all() and np.isnan(roomy["coords"][P:]).all()


def test_refusals_leave_the_library_usable(dev):
    from athena_amd._capi import AthenaMPError

    c = NAMES.index("mode 1, dim 2")
    name, kw = CASES[c]
    want = _want(c)
    P, M, E = want["P"], want["M"], kw["pairs"].shape[0]

    def refused(match, cap=P, mcap=M, keep=None, **change):
        with pytest.raises(AthenaMPError, match=match):
            _device(dev, kw, keep=keep, cap=cap, mcap=mcap, **change)
        got = _device(dev, kw)                                       # the library stays usable
        assert cr.same(got, want) == [] and (got["P"], got["M"]) == (P, M)

    refused(r"mode = 2 outside \[0,1\]", mode=2)
    refused(r"mode = -1 outside \[0,1\]", mode=-1)
    refused(r"n_rows = -1, n_cols = \d+, m_rows = \d+, m_cols = \d+: negative", n_rows=-1)
    refused(r"mode 0 is one set: n_rows = 333, n_cols = 211", mode=0)
    refused(r"no row map \(the identity\), but m_rows = 40 is not n_rows = 333", row_cluster=None)
    refused(r"no column map \(the identity\), but m_cols = 23 is not n_cols = 211", col_cluster=None)
    refused(r"only one of row_points and col_points is given", col_points=None, keep=("edge_pair",))
    refused(r"dim = 4 outside \[1,3\]", row_points=np.zeros((40, 4), np.float32), col_points=np.zeros((23, 4), np.float32), keep=("edge_pair",))
    refused(r"coords asked for without points", row_points=None, col_points=None, keep=("coords",))
    p = kw["pairs"].copy(); p[5, 1] = kw["n_cols"] + 1; p[9, 0] = -1
    refused(rf"pairs\(:,6\) = \({p[5, 0]}, 212\) outside \[0,333\] x \[0,211\]", pairs=p)
    p = kw["pairs"].copy(); p[E - 1, 0] = -7
    refused(rf"pairs\(:,{E}\) = \(-7, {p[E - 1, 1]}\) outside", pairs=p)
    rc = kw["row_cluster"].copy(); rc[3] = 41; rc[200] = -1
    refused(r"row_cluster\(4\) = 41 outside \[0,40\]", row_cluster=rc)
    cc = kw["col_cluster"].copy(); cc[8] = -1
    refused(r"col_cluster\(9\) = -1 outside \[0,23\]", col_cluster=cc)
    refused(rf"the buffers hold {P - 1} coarse pairs, the list has {P}", cap=P - 1)
    refused(rf"the buffers hold {M - 1} members, the list has {M}", mcap=M - 1)
    # a list of 2^31 pairs is refused before anything of that size is touched
    import torch
    from athena_amd import _capi

    n1, n2 = C.c_int64(), C.c_int64()
    pd = torch.zeros((4, 2), dtype=torch.int32, device=dev)
    for E_bad, match in ((2 ** 31, r"n_pairs = 2147483648, 2\^31 or more"), (-1, r"n_pairs = -1 is negative")):
        with pytest.raises(AthenaMPError, match=match):
            _capi.call("athena_mp_contract_pairs", E_bad, ptr(pd), 5, 5, None, None, 5, 5, 0, 0, None, None, 0, 0, None, None, None, None, None, None,
                       C.byref(n1), C.byref(n2))
    assert cr.same(_device(dev, kw), want) == []


def test_graph_pairs_is_the_list_a_handle_was_built_from(dev):
    import torch
    from athena_amd import DeviceGraph, _capi
    from athena_amd._capi import AthenaMPError

    r = cr._rng(50)
    n, E = 700, 4096 + 55
    idx = np.stack([r.integers(1, n + 1, E), r.integers(1, n + 1, E)]).astype(np.int32)
    idx[:, 100:140] = idx[:, 200:240]                                        # duplicated pairs
    idx[1, 300:320] = idx[0, 300:320]                                        # self pairs
    g = DeviceGraph.from_edges(n, idx)
    got = g.pair_list().cpu().numpy()
    assert np.array_equal(got, np.stack([idx.min(axis=0), idx.max(axis=0)], axis=1))
    assert np.array_equal(got, cr.graph_pairs(g.export("e_rowptr"), g.export("e_row"), g.export("e_entry"), g.export("col")))
    with pytest.raises(AthenaMPError, match=rf"the buffer holds {E - 1} pairs, the handle has {E} edge columns"):
        _capi.call("athena_mp_graph_pairs", g.handle, ptr(torch.empty((E, 2), dtype=torch.int32, device=dev)), E - 1)
    # a rectangular handle: the list itself
    k = np.unique(r.integers(0, 300 * 170, 2500))
    pairs = np.stack([k // 170 + 1, k % 170 + 1], axis=1).astype(np.int32)
    pd = torch.from_numpy(pairs).to(dev)
    b = DeviceGraph.__new__(DeviceGraph)
    h, ia = C.c_void_p(), np.empty(301, np.int32)
    _capi.use_torch_stream()
    _capi.call("athena_mp_graph_create_bipartite_dev", 300, 170, pairs.shape[0], ptr(pd), vp(ia), None, 0, C.byref(h))
    b.handle, b.n_rows, b.n_cols, b.nnz, b.n_edge_cols = h, 300, 170, pairs.shape[0], pairs.shape[0]
    assert np.array_equal(b.pair_list().cpu().numpy(), pairs)
    # edge columns that no entry carries give (0, 0)
    ia, ja = np.array([1, 3, 4, 6], np.int32), np.asfortranarray(np.array([[3, 3, 2, 1, 1], [1, 4, 2, 1, 4]], np.int32))
    host = DeviceGraph(ia, ja, n_edge_cols=6)
    assert host.pair_list().cpu().numpy().tolist() == [[1, 3], [2, 2], [0, 0], [1, 3], [0, 0], [0, 0]]


@pytest.mark.parametrize("cell_type,shape", [(1, (60, 40)), (2, (40, 30)), (3, (40, 30)), (4, (7, 6, 5))])
def test_cell_pairs_and_the_edge_graph_of_a_structured_mesh(dev, cell_type, shape):
    import torch
    from athena_amd import DeviceGraph, _capi
    from athena_amd._capi import AthenaMPError

    cells, nvert, edges, boundary, pts = cr.grid_mesh(cell_type, *shape)
    ne = len(cr.LOCAL[cell_type])
    total = cells.shape[0] * ne
    assert total > 4096
    want_pairs = cr.cell_pairs(cells, cell_type)
    cd = torch.from_numpy(cells).to(dev)
    out = torch.full((total, 2), -1, dtype=torch.int32, device=dev)
    count = C.c_int64(-1)
    _capi.use_torch_stream()
    _capi.call("athena_mp_cell_pairs", nvert, cells.shape[0], cell_type, ptr(cd), ptr(out), total, C.byref(count))
    torch.cuda.synchronize()
    assert count.value == total and np.array_equal(out.cpu().numpy(), want_pairs)
    want = cr.contract(want_pairs, nvert, nvert, None, None, nvert, nvert, 0, pts, pts)
    handle, mesh_edges, pool, weights, edge_pair, coords = DeviceGraph.from_mesh(cells, nvert, cell_type, points=pts)
    got = dict(coarse_pairs=mesh_edges.cpu().numpy(), weights=weights.cpu().numpy(), edge_pair=edge_pair.cpu().numpy(), coords=coords.cpu().numpy())
    assert cr.same(got, want, tuple(got)) == []
    assert (handle.n_rows, handle.n_cols, handle.n_edge_cols, handle.nnz) == (nvert, nvert, edges, 2 * edges)
    assert (pool.n_rows, pool.n_cols, pool.nnz) == (edges, total, want["M"])
    elements = np.bincount(got["edge_pair"][got["edge_pair"] > 0] - 1, minlength=edges)       # elements on each edge
    if boundary is not None:
        assert (elements == 1).sum() == boundary
    assert np.array_equal(pool.export("rowptr"), want["rowptr"]) and np.array_equal(pool.export("col"), want["members"][:, 1] - 1)
    # the refusals: the type, a vertex id outside 1 .. n_vertices (the first such cell is named), the capacity
    call = lambda nv=nvert, ct=cell_type, c=cd, cap=total: _capi.call("athena_mp_cell_pairs", nv, c.shape[0], ct, ptr(c), ptr(out), cap, C.byref(count))
    for ct in (0, 5):
        with pytest.raises(AthenaMPError, match=rf"cell_type = {ct} outside \[1,4\]"):
            call(ct=ct)
    bad = cells.copy(); bad[11, cells.shape[1] - 1] = 0; bad[3, 1] = nvert + 1
    with pytest.raises(AthenaMPError, match=rf"cells\(2,4\) = {nvert + 1} outside \[1,{nvert}\]"):
        call(c=torch.from_numpy(bad).to(dev))
    with pytest.raises(AthenaMPError, match=rf"the buffer holds {total - 1} pairs, the cells have {total}"):
        call(cap=total - 1)
    out.fill_(-1)
    call()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want_pairs)


@functools.lru_cache(None)
def _chain_points():
    r = cr._rng(60)
    sizes = [900, 0, 700, 350]
    p = np.concatenate([r.random((s, 3)).astype(np.float32) + np.float32(3 * b) for b, s in enumerate(sizes)])
    return p, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def test_the_chain_from_points_to_a_pooled_graph(dev):
    """from_point_clouds -> from_grid_clusters -> from_contraction(handle, cluster, m, points=centroid) against numpy: the coarse
    handle is from_edges of the yardstick's coarse list, the pool handle the host-built rectangular handle, and max and mean pooling
    of integer-valued fine edge features run on it (every yardstick here is then bit-defined)"""
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.geometry import interpolate, pool_max

    p, off = _chain_points()
    n = p.shape[0]
    fine, fine_coords, voff, eoff = DeviceGraph.from_point_clouds(p, off, 0.15)
    grid, centroid, coff, cluster, _ = DeviceGraph.from_grid_clusters(p, 0.25, off)
    m = grid.n_rows
    pairs = fine.pair_list().cpu().numpy()
    E = pairs.shape[0]
    assert E == fine.n_edge_cols and E > 4096 and (pairs[:, 0] < pairs[:, 1]).all()
    cl, cen = cluster.cpu().numpy(), centroid.cpu().numpy()
    want = cr.contract(pairs, n, n, cl, cl, m, m, 0, cen, cen)
    P, M = want["P"], want["M"]
    assert 0 < P < M < E
    coarse, coarse_pairs, pool, weights, edge_pair, coords = DeviceGraph.from_contraction(fine, cluster, m, points=centroid)
    got = dict(coarse_pairs=coarse_pairs.cpu().numpy(), weights=weights.cpu().numpy(), edge_pair=edge_pair.cpu().numpy(), coords=coords.cpu().numpy())
    assert cr.same(got, want, tuple(got)) == []
    host = DeviceGraph.from_edges(m, np.asfortranarray(want["coarse_pairs"].T))
    assert (coarse.n_rows, coarse.n_cols, coarse.nnz, coarse.n_edge_cols) == (m, m, host.nnz, P)
    for name in DeviceGraph._ARRAYS:
        a, b = coarse.export(name), host.export(name)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), name
    i, j = want["members"][:, 0].astype(np.int64) - 1, want["members"][:, 1].astype(np.int64) - 1
    ia = (want["rowptr"] + 1).astype(np.int32)
    ja = np.asfortranarray(np.stack([j + 1, np.arange(1, M + 1)]).astype(np.int32))
    host_pool = DeviceGraph(ia, ja, n_cols=E, n_edge_cols=M, row_deg=np.diff(want["rowptr"]), col_deg=np.bincount(j, minlength=E))
    assert (pool.n_rows, pool.n_cols, pool.nnz, pool.n_edge_cols) == (P, E, M, M)
    for name in DeviceGraph._ARRAYS:
        a, b = pool.export(name), host_pool.export(name)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), name
    A = ir.arrays_of(i, j, P, E)
    h = cr._rng(61).integers(-50, 50, (E, 5)).astype(np.float32)
    hd = torch.from_numpy(h).to(dev)
    y, arg = pool_max(pool, x=hd)
    wy, warg = pr.fwd(A, h)
    assert np.array_equal(y.cpu().numpy().view(np.int32), wy.view(np.int32)) and np.array_equal(arg.cpu().numpy(), warg)
    mean = interpolate(pool, weights, hd)
    assert np.array_equal(mean.cpu().numpy().view(np.int32), ir.fwd(A, want["weights"], h).view(np.int32))
    # the same from the pair list as a tensor, without the pool; and a two-set contraction through the Python layer
    short = DeviceGraph.from_contraction(fine.pair_list(), cluster, m, n_vertices=n, want_pool=False)
    assert len(short) == 5 and short[2] is None and np.array_equal(short[1].cpu().numpy(), want["coarse_pairs"])
    kw = cr.case("three tiles, 300 x 200 clusters, mode 1")
    two = cr.contract(*cr.args_of(kw))
    res = DeviceGraph.from_contraction(torch.from_numpy(kw["pairs"]).to(dev), kw["row_cluster"], kw["m_rows"], col_cluster=kw["col_cluster"],
                                       n_col_clusters=kw["m_cols"], points=kw["row_points"], col_points=kw["col_points"],
                                       n_vertices=kw["n_rows"], n_col_vertices=kw["n_cols"])
    have = dict(coarse_pairs=res[1].cpu().numpy(), weights=res[3].cpu().numpy(), edge_pair=res[4].cpu().numpy(), coords=res[5].cpu().numpy())
    assert cr.same(have, two, tuple(have)) == []
    assert (res[0].n_rows, res[0].n_cols, res[0].nnz) == (kw["m_rows"], kw["m_cols"], two["P"])
    assert np.array_equal(res[0].pair_list().cpu().numpy(), two["coarse_pairs"])


def _host(kw, want):
    from athena_amd import _capi

    E = kw["pairs"].shape[0]
    dim = kw["row_points"].shape[1] if kw["row_points"] is not None else 0
    head = (E, vp(kw["pairs"]), kw["n_rows"], kw["n_cols"], vp(kw["row_cluster"]), vp(kw["col_cluster"]), kw["m_rows"], kw["m_cols"], kw["mode"],
            dim, vp(kw["row_points"]), vp(kw["col_points"]))
    P, M = C.c_int64(-1), C.c_int64(-1)
    _capi.call("athena_mp_contract_pairs_host", *head, 0, 0, None, None, None, None, None, None, C.byref(P), C.byref(M))
    assert (P.value, M.value) == (want["P"], want["M"])
    P, M = P.value, M.value
    out = dict(coarse_pairs=np.full((P, 2), -1, np.int32), rowptr=np.full(P + 1, -1, np.int32), members=np.full((M, 2), -1, np.int32),
               weights=np.full(M, np.nan, np.float32), edge_pair=np.full(E, -1, np.int32),
               coords=np.full((P, dim), np.nan, np.float32) if dim else None)
    P2, M2 = C.c_int64(-1), C.c_int64(-1)
    _capi.call("athena_mp_contract_pairs_host", *head, P, M, *(vp(out[k]) for k in cr.KEYS), C.byref(P2), C.byref(M2))
    out.update(P=int(P2.value), M=int(M2.value))
    return out


@pytest.mark.parametrize("name", ["three tiles, 300 clusters, mode 0", "mode 1, dim 2", "identity over 2^17 + 3 vertices", "E = 0",
                                  "every edge dropped"])
def test_the_host_form_agrees_with_the_yardstick(dev, name):
    from athena_amd import _capi
    from athena_amd._capi import AthenaMPError

    c = NAMES.index(name)
    kw, want = CASES[c][1], _want(c)
    got = _host(kw, want)
    assert (got["P"], got["M"]) == (want["P"], want["M"]) and cr.same(got, want) == []
    if want["P"] > 0:
        with pytest.raises(AthenaMPError, match=rf"the buffers hold {want['P'] - 1} coarse pairs, the list has {want['P']}"):
            n1, n2 = C.c_int64(), C.c_int64()
            cp = np.zeros((want["P"], 2), np.int32)
            dim = kw["row_points"].shape[1] if kw["row_points"] is not None else 0
            _capi.call("athena_mp_contract_pairs_host", kw["pairs"].shape[0], vp(kw["pairs"]), kw["n_rows"], kw["n_cols"], vp(kw["row_cluster"]),
                       vp(kw["col_cluster"]), kw["m_rows"], kw["m_cols"], kw["mode"], dim, vp(kw["row_points"]), vp(kw["col_points"]),
                       want["P"] - 1, want["M"], vp(cp), None, None, None, None, None, C.byref(n1), C.byref(n2))


@pytest.mark.parametrize("name", ["three tiles, 300 clusters, mode 0", "mode 1, dim 2", "identity over 2^17 + 3 vertices"])
def test_fortran_program_writes_the_arrays_of_the_yardstick(dev, tmp_path, name):
    if not os.path.exists(RUNNER):
        pytest.fail("contract_run is not built: __graft_entry__.build() compiles the Fortran host side")
    c = NAMES.index(name)
    kw, want = CASES[c][1], _want(c)
    E, P, M = kw["pairs"].shape[0], want["P"], want["M"]
    has_maps, has_points = int(kw["row_cluster"] is not None), int(kw["row_points"] is not None)
    dim = kw["row_points"].shape[1] if has_points else 0
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        np.array([E, kw["n_rows"], kw["n_cols"], kw["m_rows"], kw["m_cols"], kw["mode"], dim, has_maps, has_points], np.int32).tofile(f)
        kw["pairs"].tofile(f)
        if has_maps:
            kw["row_cluster"].tofile(f)
            if kw["mode"] == 1:
                kw["col_cluster"].tofile(f)
        if has_points:
            kw["row_points"].tofile(f)
            if kw["mode"] == 1:
                kw["col_points"].tofile(f)
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"contract_run failed ({out.returncode}): {out.stdout[-1000:]} {out.stderr[-2000:]}"
    raw = open(res, "rb").read()
    at = 0

    def take(dtype, *shape):
        nonlocal at
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at).reshape(shape)
        at += a.nbytes
        return a

    assert take(np.int64, 2).tolist() == [P, M]
    got = dict(coarse_pairs=take(np.int32, P, 2), rowptr=take(np.int32, P + 1), members=take(np.int32, M, 2), weights=take(np.float32, M),
               edge_pair=take(np.int32, E), coords=take(np.float32, P, dim) if has_points else None)
    assert cr.same(got, want) == []
    assert take(np.int64, 4).tolist() == [P, M, want["bits"], want["largest"]] and at == len(raw)
