"""GPU: the device entries of the two-set radius graph -- athena_mp_radius_pairs_bipartite, athena_mp_graph_create_bipartite_dev,
athena_mp_edge_grad_to_point_sets, athena_mp_add_row_bias -- with each pointer operand in turn placed 1 and 2 elements past a
512-byte boundary (4- and 8-byte aligned addresses) between guard words and the others on torch's own 256-byte alignment, the way
test_gpu_knn_unaligned.py places the operands of its entries.  The results equal the yardstick's (tests/bipartite_reference.py),
no guard word is written, every output element is, and no input changes."""
import ctypes as C
import functools

import numpy as np
import pytest

import bipartite_reference as br
from helpers import placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

vp = lambda a: a.ctypes.data_as(C.c_void_p)
ptr = lambda t: C.c_void_p(t.data_ptr())


@functools.lru_cache(None)
def _case():
    rng = np.random.default_rng(52001)
    nq, ns = [130, 0, 77, 5, 1], [90, 40, 111, 0, 300]
    qoff, soff = br.offsets_of(nq), br.offsets_of(ns)
    q = rng.random((int(qoff[-1]), 3)).astype(np.float32)
    s = rng.random((int(soff[-1]), 3)).astype(np.float32)
    r = 0.2
    i, j, c, rowptr, eoff = br.reference_pairs(q, s, r, qoff, soff)
    assert np.all(np.diff(eoff)[[0, 2, 4]] >= 1) and i.size >= 300
    d = rng.standard_normal((i.size, 3)).astype(np.float32)
    return q, s, qoff, soff, r, i, j, c, rowptr, eoff, d


def _in(array, dev, here, at):
    import torch

    return placed(array, dev, at) if here else torch.from_numpy(np.ascontiguousarray(array)).to(dev)


def _out(shape, dtype, dev, here, at):
    return placed_out(shape, dtype, dev, at if here else 0)


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("which", ["queries", "sources", "pairs", "coords", "rowptr"])
def test_the_search_between_guards(dev, which, at):
    import torch
    from athena_amd import _capi

    q, s, qoff, soff, r, i, j, c, rowptr, eoff, _ = _case()
    E, nq = i.size, q.shape[0]
    qd, sd = _in(q, dev, which == "queries", at), _in(s, dev, which == "sources", at)
    before = (qd.clone(), sd.clone())
    pairs, check_p = _out((E, 2), torch.int32, dev, which == "pairs", at)
    coords, check_c = _out((E, 3), torch.float32, dev, which == "coords", at)
    row, check_r = _out((nq + 1,), torch.int32, dev, which == "rowptr", at)
    moved = {"queries": qd, "sources": sd, "pairs": pairs, "coords": coords, "rowptr": row}[which]
    assert moved.data_ptr() % 16 == 4 * at
    got, geoff = C.c_int64(-1), np.full(eoff.size, -9, np.int64)
    _capi.use_torch_stream()
    _capi.call("athena_mp_radius_pairs_bipartite", qoff.size - 1, nq, vp(qoff), s.shape[0], vp(soff), 3, ptr(qd), ptr(sd), r, ptr(pairs),
               ptr(coords), E, ptr(row), vp(geoff), C.byref(got))
    torch.cuda.synchronize()
    check_p("pairs"); check_c("coords"); check_r("rowptr")
    assert got.value == E and np.array_equal(geoff, eoff)
    assert unwritten(pairs) == 0 and unwritten(coords) == 0 and unwritten(row) == 0
    assert np.array_equal(pairs.cpu().numpy().astype(np.int64), np.stack([i + 1, j + 1], axis=1))
    assert np.array_equal(coords.cpu().numpy(), c) and np.array_equal(row.cpu().numpy(), rowptr)
    assert torch.equal(qd.view(torch.int32), before[0].view(torch.int32)) and torch.equal(sd.view(torch.int32), before[1].view(torch.int32))


@pytest.mark.parametrize("at", [1, 2])
def test_the_handle_from_a_pair_list_between_guards(dev, at):
    import torch
    from athena_amd import DeviceGraph, _capi

    q, s, qoff, soff, r, i, j, c, rowptr, eoff, _ = _case()
    E, nq, ns = i.size, q.shape[0], s.shape[0]
    pairs = placed(np.stack([i + 1, j + 1], axis=1).astype(np.int32), dev, at)
    before = pairs.clone()
    ia, ja, h = np.empty(nq + 1, np.int32), np.empty((2, E), np.int32, order="F"), C.c_void_p()
    _capi.use_torch_stream()
    _capi.call("athena_mp_graph_create_bipartite_dev", nq, ns, E, ptr(pairs), vp(ia), vp(ja), E, C.byref(h))
    torch.cuda.synchronize()
    wia, wja = br.csr_of(i, j, nq)
    assert np.array_equal(ia, wia) and np.array_equal(ja, wja) and torch.equal(pairs, before)
    got = DeviceGraph.__new__(DeviceGraph)
    got.handle = h
    want = DeviceGraph(wia, wja, n_cols=ns, n_edge_cols=E, row_deg=np.bincount(i, minlength=nq), col_deg=np.bincount(j, minlength=ns))
    for name in DeviceGraph._ARRAYS:
        assert np.array_equal(got.export(name).view(np.int32), want.export(name).view(np.int32)), name
    got.close(); want.close()                              # got owns h: nothing else may destroy it


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("which", ["dcoords", "dqueries", "dsources"])
def test_the_reverse_step_between_guards(dev, which, at):
    import torch
    from athena_amd import DeviceGraph, _capi

    q, s, qoff, soff, r, i, j, c, rowptr, eoff, d = _case()
    nq, ns = q.shape[0], s.shape[0]
    g, _, _ = DeviceGraph.from_point_sets(q, s, r, qoff, soff)
    dd = _in(d, dev, which == "dcoords", at)
    before = dd.clone()
    dq, check_q = _out((nq, 3), torch.float32, dev, which == "dqueries", at)
    ds, check_s = _out((ns, 3), torch.float32, dev, which == "dsources", at)
    assert {"dcoords": dd, "dqueries": dq, "dsources": ds}[which].data_ptr() % 16 == 4 * at
    _capi.use_torch_stream()
    _capi.call("athena_mp_edge_grad_to_point_sets", g.handle, 3, ptr(dd), ptr(dq), ptr(ds))
    torch.cuda.synchronize()
    check_q("dqueries"); check_s("dsources")
    wq, ws = br.reference_grad(i, j, d, nq, ns)
    assert unwritten(dq) == 0 and unwritten(ds) == 0
    assert np.array_equal(dq.cpu().numpy().view(np.int32), wq.view(np.int32))
    assert np.array_equal(ds.cpu().numpy().view(np.int32), ws.view(np.int32))
    assert torch.equal(dd.view(torch.int32), before.view(torch.int32))


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("which", ["b", "y"])
def test_the_row_bias_between_guards(dev, which, at):
    import torch
    from athena_amd import _capi

    rng = np.random.default_rng(52002)
    y0, b0 = rng.standard_normal((37, 7)).astype(np.float32), rng.standard_normal(7).astype(np.float32)
    b = _in(b0, dev, which == "b", at)
    y, check = placed_out((37, 7), torch.float32, dev, at if which == "y" else 0, init=y0)
    _capi.use_torch_stream()
    _capi.call("athena_mp_add_row_bias", 37, 7, ptr(b), ptr(y))
    check("y")
    assert np.array_equal(y.cpu().numpy(), y0 + b0[None, :]) and np.array_equal(b.cpu().numpy(), b0)
