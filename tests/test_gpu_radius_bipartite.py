"""GPU: radius graphs between two point sets (athena_mp_radius_pairs_bipartite), their handle
(athena_mp_graph_create_bipartite_dev), the reverse step (athena_mp_edge_grad_to_point_sets), graph_nop_layer_type(local_term=False)
on such a handle, and the Fortran host form -- against tests/bipartite_reference.py (brute force, fp32 term by term) and, for the
layer, against the unchanged oracle on a square embedding.  Integer arrays and single fp32 subtractions are compared whole with
np.array_equal; the layer is held to 1e-5 through helpers.assert_close.  Every case first asserts that the yardstick itself finds
pairs, so an empty answer cannot pass."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bipartite_reference as br
import radius_reference as rr
from helpers import assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "radius_bipartite_run")
vp = lambda a: a.ctypes.data_as(C.c_void_p)
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


def _rng(seed):
    return np.random.default_rng(51000 + seed)


def _device_pairs(dev, q, s, qoff, soff, r):
    """size query, then the fill with rowptr: (i, j, coords, rowptr, edge_offsets) of the device, the size query's answers checked
    against the fill's on the way"""
    import torch
    from athena_amd import _capi

    _capi.use_torch_stream()
    qoff = br.offsets_of([q.shape[0]]) if qoff is None else qoff
    soff = br.offsets_of([s.shape[0]]) if soff is None else soff
    B, dim = qoff.size - 1, q.shape[1]
    qd, sd = torch.from_numpy(q).to(dev), torch.from_numpy(s).to(dev)
    head = (B, q.shape[0], vp(qoff), s.shape[0], vp(soff), dim, ptr(qd), ptr(sd), float(r))
    E0, eoff0 = C.c_int64(-1), np.full(B + 1, -7, np.int64)
    _capi.call("athena_mp_radius_pairs_bipartite", *head, None, None, 0, None, vp(eoff0), C.byref(E0))
    E = E0.value
    pairs = torch.full((E, 2), -1, dtype=torch.int32, device=dev)
    coords = torch.full((E, dim), float("nan"), dtype=torch.float32, device=dev)
    rowptr = torch.full((q.shape[0] + 1,), -1, dtype=torch.int32, device=dev)
    E1, eoff = C.c_int64(-1), np.full(B + 1, -7, np.int64)
    _capi.call("athena_mp_radius_pairs_bipartite", *head, ptr(pairs), ptr(coords), E, ptr(rowptr), vp(eoff), C.byref(E1))
    torch.cuda.synchronize()
    assert E1.value == E and np.array_equal(eoff0, eoff), "the size query and the fill disagree"
    p = pairs.cpu().numpy().astype(np.int64)
    return p[:, 0] - 1, p[:, 1] - 1, coords.cpu().numpy(), rowptr.cpu().numpy(), eoff


def _compare(dev, q, s, r, qoff=None, soff=None, at_least=None):
    """device == yardstick on all five arrays; the yardstick finds at least one pair in every cloud that has both sets (or
    at_least pairs in all)"""
    wi, wj, wc, wrow, weoff = br.reference_pairs(q, s, r, qoff, soff)
    if qoff is not None:
        both = (np.diff(qoff) > 0) & (np.diff(soff) > 0)
        assert both.any() and np.all(np.diff(weoff)[both] >= 1), "the yardstick finds no pair in some cloud: the case checks nothing"
    assert wi.size >= (at_least or 1)
    i, j, c, row, eoff = _device_pairs(dev, q, s, qoff, soff, r)
    assert np.array_equal(i, wi) and np.array_equal(j, wj), "pairs"
    assert np.array_equal(c.view(np.int32), wc.view(np.int32)), "coords"
    assert np.array_equal(row, wrow), "rowptr"
    assert np.array_equal(eoff, weoff), "edge_offsets"
    return wi, wj, wc


# ---- the search ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,ns", [(300, 200), (200, 300)])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_one_cloud(dev, dim, nq, ns):
    rng = _rng(dim)
    q, s = rng.random((nq, dim)).astype(np.float32), rng.random((ns, dim)).astype(np.float32)
    _compare(dev, q, s, rr.degree_radius(ns, 6, dim), at_least=nq)


def _small_clouds(seed, dim):
    rng = _rng(seed)
    nq, ns = rng.integers(4, 30, 200), rng.integers(4, 30, 200)
    nq[[0, 97, 199]] = 0               # no queries: at the front, in the middle, at the end
    ns[[1, 98, 198]] = 0               # no sources
    nq[[2, 99, 197]] = 0               # neither
    ns[[2, 99, 197]] = 0
    qoff, soff = br.offsets_of(nq), br.offsets_of(ns)
    shift = rng.uniform(-50, 50, (200, dim))          # the clouds lie anywhere, also on top of each other
    q = (rng.random((int(qoff[-1]), dim)) + np.repeat(shift, nq, axis=0)).astype(np.float32)
    s = (rng.random((int(soff[-1]), dim)) + np.repeat(shift, ns, axis=0)).astype(np.float32)
    return q, s, qoff, soff


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_a_batch_of_small_clouds_with_empty_slices(dev, dim):
    q, s, qoff, soff = _small_clouds(dim, dim)
    _compare(dev, q, s, 0.6, qoff, soff)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_queries_outside_the_source_box(dev, dim):
    rng = _rng(10 + dim)
    s = rng.random((200, dim)).astype(np.float32)
    r = np.float32(rr.degree_radius(200, 6, dim))            # about six partners for a query inside the box
    lo, hi, ext = s.min(0), s.max(0), s.max(0) - s.min(0)
    near, far = [], []
    for a in range(dim):
        for side, k in ((-1.0, int(s[:, a].argmin())), (1.0, int(s[:, a].argmax()))):
            p = s[k].copy()
            p[a] += np.float32(side * 0.5) * r                    # just outside the box on this axis, inside the radius of s[k]
            assert p[a] < lo[a] or p[a] > hi[a]
            near.append(p)
            for dist in (np.float32(1e6) * ext[a], np.float32(3e38)):
                p = s[k].copy()
                p[a] = side * dist if dist > 1e38 else p[a] + side * dist
                far.append(p)
    far.append(np.full(dim, 3e38, np.float32))
    far.append(np.full(dim, -3e38, np.float32))
    q = np.concatenate([rng.random((60, dim)).astype(np.float32), np.array(near, np.float32), np.array(far, np.float32)])
    q = q[rng.permutation(q.shape[0])]
    wi, _, _ = _compare(dev, q, s, r, at_least=60)
    deg = np.bincount(wi, minlength=q.shape[0])
    is_near = (q[:, None, :] == np.array(near, np.float32)[None]).all(2).any(1)
    is_far = (q[:, None, :] == np.array(far, np.float32)[None]).all(2).any(1)
    assert is_near.sum() == 2 * dim and np.all(deg[is_near] >= 1), "a query just outside the box must keep its partner"
    assert is_far.sum() == 4 * dim + 2 and not deg[is_far].any(), "a query far outside the box has no partner"
    # the same with the far queries in a cloud that has no sources at all, and a cloud of ordinary ones beside it
    qoff, soff = br.offsets_of([int(is_far.sum()), q.shape[0]]), br.offsets_of([0, 200])
    _compare(dev, np.concatenate([q[is_far], q]), s, r, qoff, soff)


@pytest.mark.parametrize("radius", [1.0, 5.0])
def test_integer_lattice_where_s_equals_r2_exactly(dev, radius):
    g = np.arange(8, dtype=np.float32)
    s = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.float32(1e6)     # fp32 spacing there: 1/16
    h = np.arange(6, dtype=np.float32) + 1
    q = np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3) + np.float32(1e6)
    q = q[_rng(3).permutation(q.shape[0])]
    wi, wj, wc = _compare(dev, q, s, radius, at_least=7 * 216)
    on_sphere = (wc.astype(np.float64) ** 2).sum(1) == radius * radius
    assert on_sphere.sum() >= 6 * 216, "the case must have many pairs with s == r^2"


def test_a_query_that_coincides_with_a_source(dev):
    rng = _rng(4)
    s = rng.random((40, 3)).astype(np.float32)
    q = rng.random((30, 3)).astype(np.float32)
    q[0], q[1], q[7] = s[0], s[5], s[39]                    # at an equal index and at unequal ones
    wi, wj, wc = _compare(dev, q, s, 0.05, at_least=3)
    for i, j in ((0, 0), (1, 5), (7, 39)):
        e = np.nonzero((wi == i) & (wj == j))[0]
        assert e.size == 1 and not wc[e[0]].any()


def test_one_source_is_a_one_cell_grid(dev):
    rng = _rng(5)
    s = np.array([[0.5, 0.5, 0.5]], np.float32)
    q = rng.random((500, 3)).astype(np.float32)
    _compare(dev, q, s, 0.3, at_least=20)


@pytest.mark.parametrize("dim", [2, 3])
def test_sources_on_a_line_reach_the_cell_caps(dev, dim):
    # a diagonal line: extent / radius = 10^4 on every axis, so every axis is capped at 2048 cells and the product at 2 m
    rng = _rng(6)
    t = np.sort(rng.random(3000)).astype(np.float32)
    s = np.repeat(t[:, None], dim, axis=1).copy()
    q = s[rng.integers(0, 3000, 400)] + rng.uniform(-5e-5, 5e-5, (400, dim)).astype(np.float32)
    _compare(dev, q.astype(np.float32), s, 1e-4, at_least=400)


def test_a_cloud_of_more_than_one_work_item(dev):
    rng = _rng(7)
    s = rng.random((5000, 3)).astype(np.float32)
    q = rng.random((4500, 3)).astype(np.float32)
    qoff, soff = br.offsets_of([300, 4200]), br.offsets_of([5000 - 64, 64])
    _compare(dev, q, s, 0.05, qoff, soff)


def _hub_case():
    rng = _rng(8)
    s = np.concatenate([0.5 + 0.02 * rng.standard_normal((700, 3)), rng.random((100, 3))]).astype(np.float32)
    q = np.concatenate([[[0.5, 0.5, 0.5]], rng.random((49, 3)), rng.random((30, 3))]).astype(np.float32)
    return q, s, br.offsets_of([50, 30]), br.offsets_of([700, 100]), 0.2


def test_a_hub_query(dev):
    q, s, qoff, soff, r = _hub_case()
    wi, _, _ = _compare(dev, q, s, r, qoff, soff)
    assert np.bincount(wi)[0] == 700, "query 0 must be within the radius of all 700 sources of its cloud"


def test_capacity_determinism_and_refusals(dev):
    import torch
    from athena_amd import _capi
    from athena_amd._capi import AthenaMPError

    _capi.use_torch_stream()
    q, s, qoff, soff = _small_clouds(9, 3)
    r = 0.6
    first = _device_pairs(dev, q, s, qoff, soff, r)
    again = _device_pairs(dev, q, s, qoff, soff, r)
    assert first[0].size > 0
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes(), "two builds of the same input differ"
    E, B, nq, ns = first[0].size, qoff.size - 1, q.shape[0], s.shape[0]
    qd, sd = torch.from_numpy(q).to(dev), torch.from_numpy(s).to(dev)
    pairs = torch.empty((E, 2), dtype=torch.int32, device=dev)
    coords = torch.empty((E, 3), dtype=torch.float32, device=dev)
    got = C.c_int64()

    def call(B=B, nq=nq, qoff=qoff, ns=ns, soff=soff, dim=3, qd=qd, sd=sd, r=r, cap=E):
        _capi.call("athena_mp_radius_pairs_bipartite", B, nq, vp(qoff), ns, vp(soff), dim, ptr(qd), ptr(sd), float(r), ptr(pairs),
                   ptr(coords), cap, None, None, C.byref(got))

    def refused(match, **kw):
        with pytest.raises(AthenaMPError, match=match):
            call(**kw)
        call()                                             # the library stays usable
        assert got.value == E

    refused(rf"the output buffers hold {E - 1} pairs, the batch has {E}", cap=E - 1)
    refused(r"dim = 4 outside \[1,3\]", dim=4)
    refused(r"dim = 0 outside \[1,3\]", dim=0)
    refused(r"radius = -1 is not a positive finite number", r=-1.0)
    refused(r"radius = nan is not a positive finite number", r=float("nan"))
    refused(r"radius = 1e\+30 squared is not finite in fp32", r=1e30)
    refused(r"n_clouds = -1 is negative", B=-1)
    bad = qoff.copy(); bad[0] = 1
    refused(r"query_offsets\(1\) = 1, not 0", qoff=bad)
    bad = soff.copy(); bad[5] = bad[4] - 1
    refused(rf"cloud 5: source_offsets descend from {soff[4]} to {soff[4] - 1}", soff=bad)
    refused(rf"query_offsets end at {nq}, the batch has {nq + 1} queries", nq=nq + 1)
    refused(rf"source_offsets end at {ns}, the batch has {ns - 1} sources", ns=ns - 1)
    b, k = 40, int(qoff[40]) + 2
    nan_q = q.copy(); nan_q[k, 1] = np.nan
    refused(rf"cloud {b + 1}: queries\(2,{k + 1}\) = nan is not finite", qd=torch.from_numpy(nan_q).to(dev))
    k = int(soff[150])
    inf_s = s.copy(); inf_s[k, 2] = -np.inf
    refused(rf"cloud 151: sources\(3,{k + 1}\) = -inf is not finite", sd=torch.from_numpy(inf_s).to(dev))
    # an empty set on either side succeeds with no pairs
    zero = br.offsets_of([0] * B)
    call(nq=0, qoff=zero)
    assert got.value == 0
    call(ns=0, soff=zero)
    assert got.value == 0


def test_more_than_2_to_31_pairs_is_refused_by_the_count_pass(dev):
    import torch
    from athena_amd import _capi
    from athena_amd._capi import AthenaMPError

    _capi.use_torch_stream()
    n = 46400                                              # n^2 = 2 152 960 000 > 2^31: every query reaches every source
    p = torch.zeros((n, 1), dtype=torch.float32, device=dev)
    off, got = br.offsets_of([n]), C.c_int64()
    with pytest.raises(AthenaMPError, match=rf"{n * n} pairs between {n} queries and {n} sources: more than 2\^31 CSR entries"):
        _capi.call("athena_mp_radius_pairs_bipartite", 1, n, vp(off), n, vp(off), 1, ptr(p), ptr(p), 1.0, None, None, 0, None, None,
                   C.byref(got))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_a_set_against_itself_holds_the_pairs_of_the_one_set_builder(dev, dim):
    import torch
    from athena_amd import _capi

    _capi.use_torch_stream()
    rng = _rng(20 + dim)
    sizes = [250, 0, 1, 120, 37]
    off = br.offsets_of(sizes)
    p = (rng.random((int(off[-1]), dim)) + np.repeat(rng.uniform(-3, 3, (len(sizes), dim)), sizes, axis=0)).astype(np.float32)
    r = rr.degree_radius(120, 6, dim)
    i, j, c, _, _ = _device_pairs(dev, p, p, off, off, r)
    pd = torch.from_numpy(p).to(dev)
    E = C.c_int64()
    head = (off.size - 1, p.shape[0], vp(off), dim, ptr(pd), float(r))
    _capi.call("athena_mp_radius_pairs_batched", *head, None, None, 0, None, C.byref(E))
    pairs = torch.empty((E.value, 2), dtype=torch.int32, device=dev)
    coords = torch.empty((E.value, dim), dtype=torch.float32, device=dev)
    _capi.call("athena_mp_radius_pairs_batched", *head, ptr(pairs), ptr(coords), E.value, None, C.byref(E))
    torch.cuda.synchronize()
    up = i < j
    assert E.value >= 100 and up.sum() == E.value
    assert np.array_equal(np.stack([i[up] + 1, j[up] + 1], 1), pairs.cpu().numpy())
    assert np.array_equal(c[up], coords.cpu().numpy())
    assert (i == j).sum() == p.shape[0]


# ---- the handle ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _handle_case():
    q, s, qoff, soff, r = _hub_case()
    i, j, c, rowptr, eoff = br.reference_pairs(q, s, r, qoff, soff)
    assert i.size > 700
    return q, s, qoff, soff, r, i, j, c


def _env(mode):
    class ctx:
        def __enter__(self):
            self.old = os.environ.get("ATHENA_MP_GRAPH_BUILD")
            os.environ["ATHENA_MP_GRAPH_BUILD"] = mode

        def __exit__(self, *a):
            if self.old is None:
                del os.environ["ATHENA_MP_GRAPH_BUILD"]
            else:
                os.environ["ATHENA_MP_GRAPH_BUILD"] = self.old
    return ctx()


@pytest.mark.parametrize("mode", ["host", "device"])
def test_the_handle_is_the_host_built_rectangular_handle(dev, mode):
    from athena_amd import DeviceGraph

    q, s, qoff, soff, r, i, j, c = _handle_case()
    nq, ns, E = q.shape[0], s.shape[0], i.size
    ia, ja = br.csr_of(i, j, nq)
    with _env(mode):
        want = DeviceGraph(ia, ja, n_cols=ns, n_edge_cols=E, row_deg=np.bincount(i, minlength=nq), col_deg=np.bincount(j, minlength=ns))
        got, coords, eoff, gia, gja = DeviceGraph.from_point_sets(q, s, r, qoff, soff, want_adjacency=True)
    assert (got.n_rows, got.n_cols, got.nnz, got.n_edge_cols) == (nq, ns, E, E)
    assert np.array_equal(gia, ia) and np.array_equal(gja, ja) and np.array_equal(coords.cpu().numpy(), c)
    for name in DeviceGraph._ARRAYS:
        a, b = got.export(name), want.export(name)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), name
    assert np.array_equal(got.export("deg_row"), np.bincount(i, minlength=nq)) and got.export("eid").tolist() == list(range(E))


def test_the_handle_refuses_a_list_that_is_not_ascending_or_out_of_range(dev):
    import torch
    from athena_amd import _capi
    from athena_amd._capi import AthenaMPError

    _capi.use_torch_stream()
    good = np.array([[1, 1], [1, 3], [2, 2], [4, 1], [4, 4]], np.int32)
    ia, h = np.empty(6, np.int32), C.c_void_p()

    def create(pairs, n_rows=5, n_cols=4):
        t = torch.from_numpy(np.ascontiguousarray(pairs)).to(dev)
        _capi.call("athena_mp_graph_create_bipartite_dev", n_rows, n_cols, len(pairs), ptr(t), vp(ia), None, 0, C.byref(h))

    with pytest.raises(AthenaMPError, match=r"pairs\(:,3\) = \(1, 3\) does not ascend from pairs\(:,2\) = \(2, 2\)"):
        create(good[[0, 2, 1, 3, 4]])
    with pytest.raises(AthenaMPError, match=r"pairs\(:,4\) = \(2, 2\) does not ascend from pairs\(:,3\) = \(2, 2\)"):
        create(good[[0, 1, 2, 2, 3, 4]])
    with pytest.raises(AthenaMPError, match=r"pairs\(:,5\) = \(4, 4\) outside \[1,5\] x \[1,3\]"):
        create(good, n_cols=3)
    with pytest.raises(AthenaMPError, match=r"pairs\(:,1\) = \(0, 1\) outside \[1,5\] x \[1,4\]"):
        create(np.array([[0, 1], [1, 1]], np.int32))
    create(good)
    assert ia.tolist() == [1, 3, 4, 4, 6, 6]
    _capi.call("athena_mp_graph_destroy", h)


# ---- the reverse step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_the_reverse_step_is_the_sequential_sum(dev, dim):
    import torch
    from athena_amd import DeviceGraph, geometry

    q, s, qoff, soff, r = _hub_case()
    q, s = np.ascontiguousarray(q[:, :dim]), np.ascontiguousarray(s[:, :dim])
    i, j, _, _, _ = br.reference_pairs(q, s, r, qoff, soff)
    assert np.bincount(i).max() >= 700 and np.bincount(j).max() >= 2
    g, coords, _ = DeviceGraph.from_point_sets(q, s, r, qoff, soff)
    d = (_rng(30 + dim).standard_normal((i.size, dim)) * 10.0 ** _rng(31).integers(-3, 4, (i.size, 1))).astype(np.float32)
    wq, ws = br.reference_grad(i, j, d, q.shape[0], s.shape[0])
    dd = torch.from_numpy(d).to(dev)
    both = geometry.point_sets_grad(g, dd)
    only_q = geometry.point_sets_grad(g, dd, want=("queries",))
    only_s = geometry.point_sets_grad(g, dd, want=("sources",))
    assert set(only_q) == {"queries"} and set(only_s) == {"sources"}
    for got in (both["queries"], only_q["queries"]):
        assert np.array_equal(got.cpu().numpy().view(np.int32), wq.view(np.int32))
    for got in (both["sources"], only_s["sources"]):
        assert np.array_equal(got.cpu().numpy().view(np.int32), ws.view(np.int32))


def test_the_reverse_step_refuses_what_it_cannot_mean(dev):
    import torch
    from athena_amd import DeviceGraph, _capi
    from athena_amd._capi import AthenaMPError
    from helpers import random_graph

    g, coords, _ = DeviceGraph.from_point_sets(np.zeros((3, 2), np.float32), np.zeros((2, 2), np.float32), 1.0)
    d = torch.zeros((6, 2), device=dev)
    out = torch.empty((3, 2), device=dev)
    with pytest.raises(AthenaMPError, match=r"dim = 4 is outside 1..3"):
        _capi.call("athena_mp_edge_grad_to_point_sets", g.handle, 4, ptr(d), ptr(out), None)
    with pytest.raises(AthenaMPError, match=r"dqueries and dsources are both null"):
        _capi.call("athena_mp_edge_grad_to_point_sets", g.handle, 2, ptr(d), None, None)
    ia, ja = random_graph(20, 40, 1, self_loops=True)
    kipf = DeviceGraph(ia, ja, n_edge_cols=0)
    with pytest.raises(AthenaMPError, match=r"the handle has no edge columns"):
        _capi.call("athena_mp_edge_grad_to_point_sets", kipf.handle, 2, ptr(d), ptr(out), None)
    loops = DeviceGraph(ia, ja)                              # self-loop entries carry no edge id
    with pytest.raises(AthenaMPError, match=r"\d+ of the handle's \d+ entries carry no edge id"):
        _capi.call("athena_mp_edge_grad_to_point_sets", loops.handle, 2, ptr(d), ptr(out), None)


# ---- the layer -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _layer_points(nq, ns):
    rng = _rng(40 + nq)
    q, s = rng.random((nq, 2)).astype(np.float32), rng.random((ns, 2)).astype(np.float32)
    i, j, c, _, _ = br.reference_pairs(q, s, 0.15)
    assert i.size >= 4 * nq
    return q, s, i, j, c


@pytest.mark.parametrize("nq,ns", [(150, 100), (100, 150)])
@pytest.mark.parametrize("Fi,Fo,Hh,keep_s", [(64, 64, 64, True), (64, 64, 64, False), (5, 7, 16, None)])
def test_the_layer_without_its_local_term_on_a_rectangular_handle(dev, oracle, nq, ns, Fi, Fo, Hh, keep_s):
    """forward, dx, dtheta, db and dcoords at 1e-5 against the unchanged oracle on the square embedding [queries | sources];
    dtheta and dcoords with the float64 anchor of helpers.assert_close, as the square layer's own tests hold them"""
    import torch
    from athena_amd import DeviceGraph, geometry
    from athena_amd.layers import graph_nop_layer_type
    from oracle import oracle64 as o64

    q, s, i, j, c = _layer_points(nq, ns)
    E, N, d = i.size, nq + ns, 2
    rng = _rng(41 + Fi)
    g, coords, _ = DeviceGraph.from_point_sets(q, s, 0.15)
    assert np.array_equal(coords.cpu().numpy(), c)
    layer = graph_nop_layer_type(num_outputs=Fo, coord_dim=d, kernel_hidden=Hh, num_inputs=Fi, activation="tanh", device=str(dev),
                                 keep_s=keep_s, local_term=False)
    assert len(layer.params) == 2
    # the layer's own initialisation, perturbed as the square layer's tests perturb it: the pre-activation stays O(1).  (1e-5 is
    # relative to the tensor's scale; behind a saturated tanh the output's scale is 1 whatever |z| is, and the check would hold
    # the aggregate to 1e-5 / max|z| instead.)
    layer.set_params(layer.get_params() + rng.standard_normal(layer.get_num_params()).astype(np.float32) * 0.05)
    theta, b = layer.params[0].cpu().numpy(), layer.params[1].cpu().numpy()
    x = rng.uniform(-1, 1, (ns, Fi)).astype(np.float32)
    up = rng.uniform(-1, 1, (nq, Fo)).astype(np.float32)
    layer.set_graph_handle(g)
    out = layer.forward(torch.from_numpy(x).to(dev), coords)
    dx, dc = layer.backward(torch.from_numpy(up).to(dev), need_coord_grad=True)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (nq, Fo) and tuple(dx.shape) == (ns, Fi) and tuple(dc.shape) == (E, d)

    # the square embedding: vertices [queries | sources], features [0 ; x], columns shifted by nq, empty rows for the sources
    ia = np.concatenate([1 + np.concatenate([[0], np.cumsum(np.bincount(i, minlength=nq))]), np.full(ns, E + 1)]).astype(np.int32)
    ja = np.asfortranarray(np.stack([j + nq + 1, np.arange(1, E + 1)]).astype(np.int32))
    xs = np.concatenate([np.zeros((nq, Fi), np.float32), x])
    kap = oracle.gno_kernel_eval(c, theta, Hh, Fo * Fi)
    z = oracle.gno_aggregate(xs, kap, ia, ja, Fo)[:nq] + b
    assert 0.5 < np.abs(z).max() < 8, "the case must neither vanish nor saturate the activation everywhere"
    want = np.tanh(z)
    assert_close(out.cpu().numpy(), want, 1e-5, "forward")
    dz = (up * (np.float32(1) - want * want)).astype(np.float32)
    dzs = np.concatenate([dz, np.zeros((ns, Fo), np.float32)])
    assert_close(dx.cpu().numpy(), oracle.gno_aggregate_bwd_x(dzs, kap, ia, ja, Fi)[nq:], 1e-5, "dx")
    dk = oracle.gno_aggregate_bwd_k(dzs, xs, E, ia, ja)
    dk64 = lambda: o64.gno_aggregate_bwd_k(dzs, xs, E, ia, ja)
    assert_close(layer.grads[0].cpu().numpy(), oracle.gno_kernel_bwd_theta(c, theta, dk, Hh), 1e-5, "dtheta",
                 f64=lambda: o64.gno_kernel_bwd_theta(c, theta, dk64(), Hh))
    assert_close(layer.grads[1].cpu().numpy(), dz.sum(0, dtype=np.float64).astype(np.float32), 1e-5, "db")
    assert_close(dc.cpu().numpy(), oracle.gno_kernel_bwd_coords(c, theta, dk, Hh), 1e-5, "dcoords",
                 f64=lambda: o64.gno_kernel_bwd_coords(c, theta, dk64(), Hh))
    # and the gradient carried back to the two point sets, bit for bit the sequential sums of that dcoords
    wq, ws = br.reference_grad(i, j, dc.cpu().numpy(), nq, ns)
    got = geometry.point_sets_grad(g, dc)
    assert np.array_equal(got["queries"].cpu().numpy().view(np.int32), wq.view(np.int32))
    assert np.array_equal(got["sources"].cpu().numpy().view(np.int32), ws.view(np.int32))


def test_a_rectangular_handle_needs_local_term_false(dev):
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.layers import graph_nop_layer_type

    q, s, i, j, c = _layer_points(150, 100)
    g, coords, _ = DeviceGraph.from_point_sets(q, s, 0.15)
    layer = graph_nop_layer_type(num_outputs=4, coord_dim=2, kernel_hidden=8, num_inputs=3, device=str(dev))
    layer.set_graph_handle(g)
    with pytest.raises(ValueError, match="local term W x has no meaning when the output points are not the input points"):
        layer.forward(torch.zeros((100, 3), device=dev), coords)


@pytest.mark.parametrize("shape", [(64, 64, 64), (5, 7, 16)])
def test_a_square_handle_with_the_default_arguments_gives_the_same_bits(dev, shape):
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.layers import graph_nop_layer_type

    Fi, Fo, Hh = shape
    rng = _rng(60)
    p = rng.random((200, 2)).astype(np.float32)
    g, coords = DeviceGraph.from_points(p, 0.12, add_self_loops=True)
    assert g.n_edge_cols >= 400
    x = torch.from_numpy(rng.uniform(-1, 1, (200, Fi)).astype(np.float32)).to(dev)
    up = torch.from_numpy(rng.uniform(-1, 1, (200, Fo)).astype(np.float32)).to(dev)
    res = []
    for kw in ({}, {"local_term": True}):
        layer = graph_nop_layer_type(num_outputs=Fo, coord_dim=2, kernel_hidden=Hh, num_inputs=Fi, activation="tanh", device=str(dev),
                                     seed=3, **kw)
        layer.set_graph_handle(g)
        out = layer.forward(x, coords)
        dx, dc = layer.backward(up, need_coord_grad=True)
        res.append([layer.get_params(), out.cpu().numpy(), dx.cpu().numpy(), dc.cpu().numpy(), layer.get_gradients()])
    assert len(layer.params) == 3
    for a, b in zip(*res):
        assert a.tobytes() == b.tobytes()


# ---- Fortran -------------------------------------------------------------------------------------------------------------------
def test_fortran_program_writes_the_arrays_of_the_yardstick(dev, tmp_path):
    if not os.path.exists(RUNNER):
        pytest.fail("radius_bipartite_run is not built: __graft_entry__.build() compiles the Fortran host side")
    q, s, qoff, soff = _small_clouds(70, 3)
    r = np.float32(0.6)
    i, j, c, rowptr, eoff = br.reference_pairs(q, s, r, qoff, soff)
    E, nq, ns, B = i.size, q.shape[0], s.shape[0], qoff.size - 1
    assert E > 1000
    d = _rng(71).standard_normal((E, 3)).astype(np.float32)
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        np.array([B, nq, ns, 3], np.int32).tofile(f)
        np.array([r], np.float32).tofile(f)
        qoff.tofile(f); soff.tofile(f); q.tofile(f); s.tofile(f)
        np.array([E], np.int64).tofile(f)
        d.tofile(f)
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"radius_bipartite_run failed ({out.returncode}): {out.stdout[-1000:]} {out.stderr[-2000:]}"
    raw = open(res, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a

    assert take(np.int64, 1)[0] == E
    ia, ja = br.csr_of(i, j, nq)
    assert np.array_equal(take(np.int32, nq + 1), ia)
    assert np.array_equal(take(np.int32, 2 * E).reshape(E, 2).T, ja)
    assert np.array_equal(take(np.float32, 3 * E).reshape(E, 3).view(np.int32), c.view(np.int32))
    assert np.array_equal(take(np.int64, B + 1), eoff)
    wq, ws = br.reference_grad(i, j, d, nq, ns)
    assert np.array_equal(take(np.float32, 3 * nq).reshape(nq, 3).view(np.int32), wq.view(np.int32))
    assert np.array_equal(take(np.float32, 3 * ns).reshape(ns, 3).view(np.int32), ws.view(np.int32))
    assert at == len(raw)
