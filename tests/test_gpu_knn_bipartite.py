"""GPU: k-nearest-neighbour graphs between two point sets (athena_mp_knn_pairs_bipartite), their handle, the reverse step and
graph_nop_layer_type(local_term=False) on such a handle, and the Fortran host form -- against tests/knn_bipartite_reference.py
(brute force, fp32 term by term).  nbr, sqdist, pairs, coords, rowptr and edge_offsets are compared whole with np.array_equal; the
layer is held to 1e-5 through helpers.assert_close against the unchanged oracle on a square embedding."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bipartite_reference as br
import knn_bipartite_reference as kb
from helpers import assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "knn_bipartite_run")
INF = float("inf")
vp = lambda a: a.ctypes.data_as(C.c_void_p)
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
CASES = kb.shape_cases()


def _rng(seed):
    return np.random.default_rng(52000 + seed)


def _radius(r):
    return INF if r is None else float(r)


def _device(dev, q, s, k, r=None, qoff=None, soff=None):
    """size query, then ONE search into buffers of n_queries * k: (nbr, sqdist, i, j, coords, rowptr, edge_offsets) of the device,
    the size query's answers checked against the fill's and the buffers beyond the pairs still unwritten"""
    import torch
    from athena_amd import _capi

    _capi.use_torch_stream()
    qoff = kb.offsets_of([q.shape[0]]) if qoff is None else qoff
    soff = kb.offsets_of([s.shape[0]]) if soff is None else soff
    B, nq, dim = qoff.size - 1, q.shape[0], q.shape[1]
    qd, sd = torch.from_numpy(q).to(dev), torch.from_numpy(s).to(dev)
    head = (B, nq, vp(qoff), s.shape[0], vp(soff), dim, ptr(qd), ptr(sd), k, _radius(r))
    E0, eoff0 = C.c_int64(-1), np.full(B + 1, -7, np.int64)
    _capi.call("athena_mp_knn_pairs_bipartite", *head, None, None, None, None, 0, None, vp(eoff0), C.byref(E0))
    T = nq * k
    nbr = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    sqd = torch.full((nq, k), float("nan"), dtype=torch.float32, device=dev)
    pairs = torch.full((T, 2), -1, dtype=torch.int32, device=dev)
    coords = torch.full((T, dim), float("nan"), dtype=torch.float32, device=dev)
    rowptr = torch.full((nq + 1,), -1, dtype=torch.int32, device=dev)
    E1, eoff = C.c_int64(-1), np.full(B + 1, -7, np.int64)
    _capi.call("athena_mp_knn_pairs_bipartite", *head, ptr(nbr), ptr(sqd), ptr(pairs), ptr(coords), T, ptr(rowptr), vp(eoff), C.byref(E1))
    torch.cuda.synchronize()
    E = E1.value
    assert E0.value == E and np.array_equal(eoff0, eoff), "the size query and the fill disagree"
    assert bool((pairs[E:] == -1).all()) and bool(torch.isnan(coords[E:]).all()), "entries beyond the pairs were written"
    p = pairs[:E].cpu().numpy().astype(np.int64)
    return nbr.cpu().numpy(), sqd.cpu().numpy(), p[:, 0] - 1, p[:, 1] - 1, coords[:E].cpu().numpy(), rowptr.cpu().numpy(), eoff


def _compare(dev, q, s, k, r=None, qoff=None, soff=None, at_least=1):
    """device == yardstick on all six arrays; returns the yardstick's (nbr, sqdist, i, j, coords)"""
    want_nbr, want_s = kb.brute_force(q, s, k, r, qoff, soff)
    wi, wj, wc, wrow, weoff = kb.graph_of(want_nbr, q, s, qoff)
    assert wi.size >= at_least, "the yardstick finds too few pairs: the case checks nothing"
    nbr, sqd, i, j, c, row, eoff = _device(dev, q, s, k, r, qoff, soff)
    assert np.array_equal(nbr, want_nbr), "nbr"
    assert np.array_equal(sqd.view(np.int32), want_s.view(np.int32)), "sqdist"
    assert np.array_equal(i, wi) and np.array_equal(j, wj), "pairs"
    assert np.array_equal(c.view(np.int32), wc.view(np.int32)), "coords"
    assert np.array_equal(row, wrow), "rowptr"
    assert np.array_equal(eoff, weoff), "edge_offsets"
    return want_nbr, want_s, wi, wj, wc


# ---- the search ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,ns", [(300, 200), (200, 300)])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_one_cloud(dev, dim, nq, ns):
    rng = _rng(dim)
    q, s = rng.random((nq, dim)).astype(np.float32), rng.random((ns, dim)).astype(np.float32)
    _compare(dev, q, s, 8, at_least=8 * nq)


@pytest.mark.parametrize("c", range(len(CASES)), ids=[c[0] for c in CASES])
def test_the_shape_classes_of_the_cpu_tests(dev, c):
    """queries outside the box, on the cell boundaries, at +-3e38, around 1e6, lattices where the tie rule decides, coincident
    sources, k = 1, k = 64, k above the number of sources, capped and not"""
    name, q, s, qoff, soff, k, r = CASES[c]
    _compare(dev, q, s, k, r, qoff, soff)


@pytest.mark.parametrize("k", [8, 64])
@pytest.mark.parametrize("m", [64, 65, 200])
def test_coincident_sources(dev, m, k):
    """one step of 64 candidates, two steps, and ties across steps: every key has the same s, the index decides"""
    q, s = kb.coincident_sources(m)
    want_nbr, _, _, _, _ = _compare(dev, q, s, k)
    assert np.array_equal(want_nbr, np.tile(np.arange(1, k + 1, dtype=np.int32), (q.shape[0], 1)))


def test_fewer_sources_than_k_is_padded(dev):
    q, s = kb.uniform_with_outside(3, 100, 5)
    want_nbr, want_s, _, _, _ = _compare(dev, q, s, 9)
    assert (want_nbr[:, :5] > 0).all() and not want_nbr[:, 5:].any() and np.isinf(want_s[:, 5:]).all()


def test_the_margin_probe(dev):
    q, s, k, a, b = kb.margin_probe()
    want_nbr, _, _, _, _ = _compare(dev, q, s, k)
    assert want_nbr[0, 0] == b + 1


def test_a_batch_equals_the_single_calls(dev):
    q, s, qoff, soff = kb.batch()
    want_nbr, want_s, wi, wj, wc = _compare(dev, q, s, 8, None, qoff, soff)
    assert not want_nbr[qoff[2]:qoff[3]].any(), "the cloud without sources has empty rows"
    for b in range(qoff.size - 1):
        q0, q1, s0, s1 = int(qoff[b]), int(qoff[b + 1]), int(soff[b]), int(soff[b + 1])
        nbr, sqd, i, j, c, row, _ = _device(dev, q[q0:q1], s[s0:s1], 8)
        assert np.array_equal(np.where(nbr > 0, nbr + s0, 0), want_nbr[q0:q1])
        assert np.array_equal(sqd.view(np.int32), want_s[q0:q1].view(np.int32))
        mine = (wi >= q0) & (wi < q1)
        assert np.array_equal(i + q0, wi[mine]) and np.array_equal(j + s0, wj[mine])
        assert np.array_equal(c.view(np.int32), wc[mine].view(np.int32))


def test_empty_sets(dev):
    rng = _rng(4)
    q, s = rng.random((30, 3)).astype(np.float32), rng.random((20, 3)).astype(np.float32)
    none = np.zeros((0, 3), np.float32)
    for qq, ss in ((q, none), (none, s), (none, none)):
        nbr, sqd, i, j, c, row, eoff = _device(dev, qq, ss, 4)
        assert i.size == 0 and not nbr.any() and np.isinf(sqd).all() and not row.any() and not eoff.any()
        assert nbr.shape == (qq.shape[0], 4)
    # in a batch: a cloud without queries and one without sources, at either end
    _compare(dev, q, s, 4, None, kb.offsets_of([0, 18, 12, 0]), kb.offsets_of([7, 13, 0, 0]), at_least=18 * 4)


def test_a_cloud_of_more_than_one_work_item(dev):
    rng = _rng(7)
    s = rng.random((5000, 3)).astype(np.float32)
    q = (rng.random((4500, 3)) * 1.2 - 0.1).astype(np.float32)
    _compare(dev, q, s, 8, None, kb.offsets_of([300, 4200]), kb.offsets_of([5000 - 64, 64]), at_least=8 * 4500)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_a_set_against_itself_holds_the_rows_of_the_one_set_builder(dev, dim):
    """k + 1 against itself: each row with the query's own index removed -- or without its last entry where the index is absent
    (coincident points) -- is the nbr row of athena_mp_knn_pairs_batched at k"""
    import torch
    from athena_amd import _capi

    k = 6
    off = kb.offsets_of([250, 0, 1, 120, 37])
    p = _rng(20 + dim).random((int(off[-1]), dim)).astype(np.float32)
    p[260:270] = p[260]                                       # ten coincident points: more than k + 1 keys at s = 0
    nbr2, _, _, _, _, _, _ = _device(dev, p, p, k + 1, None, off, off)
    pd = torch.from_numpy(p).to(dev)
    one = torch.full((p.shape[0], k), -1, dtype=torch.int32, device=dev)
    E = C.c_int64()
    _capi.call("athena_mp_knn_pairs_batched", off.size - 1, p.shape[0], vp(off), dim, ptr(pd), k, INF, 0, ptr(one), None, None, 0, None,
               C.byref(E))
    torch.cuda.synchronize()
    own = nbr2 == np.arange(1, p.shape[0] + 1, dtype=np.int32)[:, None]
    assert own.sum(1).max() == 1 and (own.sum(1) == 0).sum() >= 1, "the case must hold rows with and without their own index"
    own[own.sum(1) == 0, -1] = True
    rest = nbr2[~own].reshape(p.shape[0], k)
    assert np.array_equal(rest, one.cpu().numpy())


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_a_cap_cuts_some_rows_and_k_the_others(dev, dim):
    q, s, r = kb.cap_case(dim)
    want_nbr, _, _, _, _ = _compare(dev, q, s, 8, r)
    inside = (kb.brute_force(q, s, 64, r)[0] > 0).sum(1)
    assert (inside < 8).any() and (inside > 8).any(), "both kinds of rows must occur"
    assert np.array_equal((want_nbr > 0).sum(1), np.minimum(inside, 8))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_k_64_under_a_cap_is_the_radius_graph(dev, dim):
    """no row holds 64 sources inside the cap: pairs, coords, rowptr and edge_offsets are byte for byte those of
    athena_mp_radius_pairs_bipartite"""
    import torch
    from athena_amd import _capi

    q, s, r = kb.cap_case(dim)
    nbr, sqd, i, j, c, row, eoff = _device(dev, q, s, 64, r)
    assert 16 <= (nbr > 0).sum(1).max() <= 18
    qd, sd = torch.from_numpy(q).to(dev), torch.from_numpy(s).to(dev)
    off_q, off_s = kb.offsets_of([300]), kb.offsets_of([200])
    head = (1, 300, vp(off_q), 200, vp(off_s), dim, ptr(qd), ptr(sd), float(r))
    E, reoff = C.c_int64(), np.zeros(2, np.int64)
    _capi.call("athena_mp_radius_pairs_bipartite", *head, None, None, 0, None, None, C.byref(E))
    pairs = torch.empty((E.value, 2), dtype=torch.int32, device=dev)
    coords = torch.empty((E.value, dim), dtype=torch.float32, device=dev)
    rowptr = torch.empty((301,), dtype=torch.int32, device=dev)
    _capi.call("athena_mp_radius_pairs_bipartite", *head, ptr(pairs), ptr(coords), E.value, ptr(rowptr), vp(reoff), C.byref(E))
    torch.cuda.synchronize()
    assert E.value == i.size > 300
    assert np.stack([i + 1, j + 1], 1).astype(np.int32).tobytes() == pairs.cpu().numpy().tobytes()
    assert c.tobytes() == coords.cpu().numpy().tobytes() and row.tobytes() == rowptr.cpu().numpy().tobytes()
    assert eoff.tobytes() == reoff.tobytes()


def test_each_output_may_be_null_alone(dev):
    import torch
    from athena_amd import _capi

    q, s, qoff, soff = kb.batch()
    k, r = 5, 0.4
    full = _device(dev, q, s, k, r, qoff, soff)
    nq, T, B = q.shape[0], q.shape[0] * k, qoff.size - 1
    qd, sd = torch.from_numpy(q).to(dev), torch.from_numpy(s).to(dev)
    for only in range(5):
        bufs = [torch.full((nq, k), -1, dtype=torch.int32, device=dev), torch.full((nq, k), float("nan"), device=dev),
                torch.full((T, 2), -1, dtype=torch.int32, device=dev), torch.full((T, 3), float("nan"), device=dev),
                torch.full((nq + 1,), -1, dtype=torch.int32, device=dev)]
        a = [b if t == only else None for t, b in enumerate(bufs)]
        E, eoff = C.c_int64(-1), np.full(B + 1, -7, np.int64)
        _capi.call("athena_mp_knn_pairs_bipartite", B, nq, vp(qoff), s.shape[0], vp(soff), 3, ptr(qd), ptr(sd), k, r, ptr(a[0]), ptr(a[1]),
                   ptr(a[2]), ptr(a[3]), T, ptr(a[4]), vp(eoff), C.byref(E))
        torch.cuda.synchronize()
        assert E.value == full[2].size and np.array_equal(eoff, full[6])
        got = bufs[only].cpu().numpy()
        if only == 0:
            assert np.array_equal(got, full[0])
        elif only == 1:
            assert np.array_equal(got.view(np.int32), full[1].view(np.int32))
        elif only == 2:
            assert np.array_equal(got[:E.value], np.stack([full[2] + 1, full[3] + 1], 1))
        elif only == 3:
            assert np.array_equal(got[:E.value].view(np.int32), full[4].view(np.int32))
        else:
            assert np.array_equal(got, full[5])


def test_capacity_determinism_and_refusals(dev):
    import torch
    from athena_amd import _capi
    from athena_amd._capi import AthenaMPError

    _capi.use_torch_stream()
    q, s, qoff, soff = kb.batch()
    k, r = 8, 0.35
    first = _device(dev, q, s, k, r, qoff, soff)
    again = _device(dev, q, s, k, r, qoff, soff)
    E = first[2].size
    assert 0 < E < q.shape[0] * k
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes(), "two builds of the same input differ"
    B, nq, ns = qoff.size - 1, q.shape[0], s.shape[0]
    qd, sd = torch.from_numpy(q).to(dev), torch.from_numpy(s).to(dev)
    pairs = torch.empty((E, 2), dtype=torch.int32, device=dev)
    coords = torch.empty((E, 3), dtype=torch.float32, device=dev)
    got = C.c_int64()

    def call(B=B, nq=nq, qoff=qoff, ns=ns, soff=soff, dim=3, qd=qd, sd=sd, k=k, r=r, cap=E):
        _capi.call("athena_mp_knn_pairs_bipartite", B, nq, vp(qoff), ns, vp(soff), dim, ptr(qd), ptr(sd), k, float(r), None, None,
                   ptr(pairs), ptr(coords), cap, None, None, C.byref(got))

    def refused(match, **kw):
        with pytest.raises(AthenaMPError, match=match):
            call(**kw)
        call()                                             # the library stays usable
        assert got.value == E
        assert np.array_equal(pairs.cpu().numpy(), np.stack([first[2] + 1, first[3] + 1], 1))

    refused(rf"the output buffers hold {E - 1} pairs, the graph has {E}", cap=E - 1)
    refused(r"dim = 4 outside \[1,3\]", dim=4)
    refused(r"dim = 0 outside \[1,3\]", dim=0)
    refused(r"k = 0 outside \[1,64\]", k=0)
    refused(r"k = 65 outside \[1,64\]", k=65)
    refused(r"radius = -1 is not a positive number", r=-1.0)
    refused(r"radius = 0 is not a positive number", r=0.0)
    refused(r"radius = nan is not a positive number", r=float("nan"))
    refused(r"n_clouds = -1 is negative", B=-1)
    bad = qoff.copy(); bad[0] = 1
    refused(r"query_offsets\(1\) = 1, not 0", qoff=bad)
    bad = soff.copy(); bad[5] = bad[4] - 1
    refused(rf"cloud 5: source_offsets descend from {soff[4]} to {soff[4] - 1}", soff=bad)
    refused(rf"query_offsets end at {nq}, the batch has {nq + 1} queries", nq=nq + 1)
    refused(rf"source_offsets end at {ns}, the batch has {ns - 1} sources", ns=ns - 1)
    i = int(qoff[3]) + 2
    nan_q = q.copy(); nan_q[i, 1] = np.nan
    refused(rf"cloud 4: queries\(2,{i + 1}\) = nan is not finite", qd=torch.from_numpy(nan_q).to(dev))
    j = int(soff[4])
    inf_s = s.copy(); inf_s[j, 2] = -np.inf
    refused(rf"cloud 5: sources\(3,{j + 1}\) = -inf is not finite", sd=torch.from_numpy(inf_s).to(dev))
    both = torch.from_numpy(nan_q).to(dev)                 # the queries are looked at first
    refused(rf"cloud 4: queries\(2,{i + 1}\) = nan is not finite", qd=both, sd=torch.from_numpy(inf_s).to(dev))
    # the size query refuses the same inputs, with and without a cap
    for radius in (r, INF):
        with pytest.raises(AthenaMPError, match=rf"cloud 5: sources\(3,{j + 1}\) = -inf is not finite"):
            _capi.call("athena_mp_knn_pairs_bipartite", B, nq, vp(qoff), ns, vp(soff), 3, ptr(qd), ptr(torch.from_numpy(inf_s).to(dev)), k,
                       radius, None, None, None, None, 0, None, None, C.byref(got))
    # n_queries * k >= 2^31, refused before anything of that size is touched: the offsets are all the entry reads
    n_big = 2 ** 31 // 64
    with pytest.raises(AthenaMPError, match=rf"n_queries \* k = {n_big * 64}: more than 2\^31 neighbour entries"):
        _capi.call("athena_mp_knn_pairs_bipartite", 1, n_big, vp(kb.offsets_of([n_big])), 0, vp(kb.offsets_of([0])), 3, ptr(qd), ptr(sd), 64,
                   INF, None, None, None, None, 0, None, None, C.byref(got))
    call()
    assert got.value == E
    # the size query without a cap needs no search: min(k, sources of the cloud) per query
    eoff = np.zeros(B + 1, np.int64)
    _capi.call("athena_mp_knn_pairs_bipartite", B, nq, vp(qoff), ns, vp(soff), 3, ptr(qd), ptr(sd), k, INF, None, None, None, None, 0, None,
               vp(eoff), C.byref(got))
    rows = np.diff(qoff).astype(np.int64) * np.minimum(k, np.diff(soff))
    assert got.value == rows.sum() and np.array_equal(eoff, np.concatenate([[0], np.cumsum(rows)]))


def test_the_stats_are_the_counts_of_the_transcription(dev):
    from athena_amd import _capi

    name, q, s, qoff, soff, k, r = CASES[2]
    assert name.startswith("uniform") and q.shape[1] == 3
    _, _, want = kb.grid_search(q, s, k, r)
    _device(dev, q, s, k, r)
    out = (C.c_int64 * 4)()
    _capi.call("athena_mp_knn_stats", out)
    assert [int(v) for v in out] == [int(v) for v in want]
    assert 0 < want[1] < q.shape[0] * s.shape[0], "the search examines fewer candidates than brute force, even at 200 sources"


# ---- the handle, the reverse step, the layer -----------------------------------------------------------------------------------
@functools.lru_cache(None)
def _handle_case():
    q, s, qoff, soff = kb.batch()
    nbr, sqd = kb.brute_force(q, s, 8, 0.5, qoff, soff)
    i, j, c, rowptr, eoff = kb.graph_of(nbr, q, s, qoff)
    assert i.size > 2000 and ((nbr > 0).sum(1) < 8).any()
    return q, s, qoff, soff, 8, 0.5, nbr, sqd, i, j, c, eoff


def test_the_handle_is_the_host_built_rectangular_handle(dev):
    from athena_amd import DeviceGraph

    q, s, qoff, soff, k, r, nbr, sqd, i, j, c, weoff = _handle_case()
    nq, ns, E = q.shape[0], s.shape[0], i.size
    ia, ja = br.csr_of(i, j, nq)
    want = DeviceGraph(ia, ja, n_cols=ns, n_edge_cols=E, row_deg=np.bincount(i, minlength=nq), col_deg=np.bincount(j, minlength=ns))
    got, coords, eoff, gia, gja, gnbr, gsqd = DeviceGraph.from_point_sets_knn(q, s, k, r, qoff, soff, want_adjacency=True,
                                                                              want_neighbours=True)
    assert (got.n_rows, got.n_cols, got.nnz, got.n_edge_cols) == (nq, ns, E, E)
    assert np.array_equal(gia, ia) and np.array_equal(gja, ja) and np.array_equal(coords.cpu().numpy(), c) and np.array_equal(eoff, weoff)
    assert np.array_equal(gnbr.cpu().numpy(), nbr) and np.array_equal(gsqd.cpu().numpy().view(np.int32), sqd.view(np.int32))
    for name in DeviceGraph._ARRAYS:
        a, b = got.export(name), want.export(name)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), name
    short = DeviceGraph.from_point_sets_knn(q[:qoff[1]], s[:soff[1]], k)
    assert len(short) == 3 and short[0].nnz == k * int(qoff[1])


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_the_reverse_step_is_the_sequential_sum(dev, dim):
    import torch
    from athena_amd import DeviceGraph, geometry

    q, s, qoff, soff = kb.batch()
    q, s = np.ascontiguousarray(q[:, :dim]), np.ascontiguousarray(s[:, :dim])
    nbr, _ = kb.brute_force(q, s, 8, None, qoff, soff)
    i, j, _, _, _ = kb.graph_of(nbr, q, s, qoff)
    g, coords, _ = DeviceGraph.from_point_sets_knn(q, s, 8, None, qoff, soff)
    assert g.nnz == i.size
    d = (_rng(30 + dim).standard_normal((i.size, dim)) * 10.0 ** _rng(31).integers(-3, 4, (i.size, 1))).astype(np.float32)
    wq, ws = br.reference_grad(i, j, d, q.shape[0], s.shape[0])
    got = geometry.point_sets_grad(g, torch.from_numpy(d).to(dev))
    assert np.array_equal(got["queries"].cpu().numpy().view(np.int32), wq.view(np.int32))
    assert np.array_equal(got["sources"].cpu().numpy().view(np.int32), ws.view(np.int32))


@functools.lru_cache(None)
def _layer_points(nq, ns):
    rng = _rng(40 + nq)
    q, s = (rng.random((nq, 2)) * 1.2 - 0.1).astype(np.float32), rng.random((ns, 2)).astype(np.float32)
    nbr, _ = kb.brute_force(q, s, 8)
    i, j, c, _, _ = kb.graph_of(nbr, q, s)
    assert i.size == 8 * nq
    return q, s, i, j, c


@pytest.mark.parametrize("nq,ns", [(150, 100), (100, 150)])
@pytest.mark.parametrize("Fi,Fo,Hh,keep_s", [(64, 64, 64, True), (64, 64, 64, False), (5, 7, 16, None)])
def test_the_layer_without_its_local_term_on_a_knn_handle(dev, oracle, nq, ns, Fi, Fo, Hh, keep_s):
    """forward, dx, dtheta, db and dcoords at 1e-5 against the unchanged oracle on the square embedding [queries | sources], as
    test_gpu_radius_bipartite.py holds the layer on a radius handle; every query has exactly 8 partners, those outside the
    source box included"""
    import torch
    from athena_amd import DeviceGraph, geometry
    from athena_amd.layers import graph_nop_layer_type
    from oracle import oracle64 as o64

    q, s, i, j, c = _layer_points(nq, ns)
    E, d = i.size, 2
    rng = _rng(41 + Fi)
    g, coords, _ = DeviceGraph.from_point_sets_knn(q, s, 8)
    assert np.array_equal(coords.cpu().numpy(), c)
    layer = graph_nop_layer_type(num_outputs=Fo, coord_dim=d, kernel_hidden=Hh, num_inputs=Fi, activation="tanh", device=str(dev),
                                 keep_s=keep_s, local_term=False)
    assert len(layer.params) == 2
    # the layer's own initialisation, perturbed by 0.05: the pre-activation stays O(1)
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
    print(f"max|z| = {np.abs(z).max():.3f}")
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
    wq, ws = br.reference_grad(i, j, dc.cpu().numpy(), nq, ns)
    got = geometry.point_sets_grad(g, dc)
    assert np.array_equal(got["queries"].cpu().numpy().view(np.int32), wq.view(np.int32))
    assert np.array_equal(got["sources"].cpu().numpy().view(np.int32), ws.view(np.int32))


# ---- Fortran -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [None, 0.5])
def test_fortran_program_writes_the_arrays_of_the_yardstick(dev, tmp_path, radius):
    if not os.path.exists(RUNNER):
        pytest.fail("knn_bipartite_run is not built: __graft_entry__.build() compiles the Fortran host side")
    q, s, qoff, soff = kb.batch()
    k = 8
    nbr, sqd = kb.brute_force(q, s, k, radius, qoff, soff)
    i, j, c, rowptr, eoff = kb.graph_of(nbr, q, s, qoff)
    E, nq, ns, B = i.size, q.shape[0], s.shape[0], qoff.size - 1
    assert E > 2000
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        np.array([B, nq, ns, 3, k], np.int32).tofile(f)
        np.array([_radius(radius)], np.float32).tofile(f)
        qoff.tofile(f); soff.tofile(f); q.tofile(f); s.tofile(f)
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"knn_bipartite_run failed ({out.returncode}): {out.stdout[-1000:]} {out.stderr[-2000:]}"
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
    assert np.array_equal(take(np.int32, nq * k).reshape(nq, k), nbr)
    assert np.array_equal(take(np.float32, nq * k).reshape(nq, k).view(np.int32), sqd.view(np.int32))
    assert at == len(raw)
