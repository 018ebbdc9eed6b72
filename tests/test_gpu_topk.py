"""GPU: athena_mp_topk_vertices and athena_mp_select_rows_fwd / _bwd against their numpy yardstick (tests/topk_reference.py).
Every array of the selection equals the yardstick's word for word on every named case -- both routes side by side, three radix
tiles decided by stability, every special value inside a graph of each route, every way of giving k, min_score --, the inputs are
unchanged and two runs are byte-identical; the test switch pins the routes and the statistics report them; the gated rows equal the
fp32 transcription word for word and the gate's gradient stays inside its bound; the chain from a batch of graphs through the
selection to the induced subgraph equals the contraction yardstick; the host forms and the Fortran program write the same bytes;
refusals carry their messages and leave the library usable."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contract_reference as cr
import topk_reference as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "topk_run")
WIDTHS = (1, 3, 4, 64, 67, 128, 130)
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None


def _run(dev, c, want_order=True):
    """the named case through the Python wrapper -> (dict of numpy arrays, the device score tensor)"""
    import torch
    from athena_amd.geometry import topk_vertices

    score = torch.from_numpy(np.array(c["score"])).to(dev)
    k = c["k"] if c["ratio"] is None else None
    out = topk_vertices(score, c["offsets"], k=k, ratio=c["ratio"], min_score=c["min_score"], want_order=want_order)
    got = dict(cluster=out[0].cpu().numpy(), selected=out[1].cpu().numpy(), sel_offsets=out[2], m=int(out[1].shape[0]))
    got["order"] = out[3].cpu().numpy() if want_order else None
    return got, score


def same_f32(a, b):
    """word for word, but a NaN that arithmetic made equals any NaN (its payload is the hardware's)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("name", tr.NAMES)
def test_every_array_equals_the_yardstick(dev, name):
    from athena_amd.geometry import topk_stats

    c, want = tr.case(name), tr.expected(name)
    got, score = _run(dev, c)
    assert tr.same(got, want) == []
    assert got["sel_offsets"].dtype == np.int32 and got["cluster"].dtype == np.int32
    assert topk_stats() == tr.stats(c["offsets"])
    assert np.array_equal(score.cpu().numpy().view(np.int32), c["score"].view(np.int32))          # the input is unchanged
    again, _ = _run(dev, c)
    assert tr.same(again, got) == []                                                             # two runs: the same bytes
    short, _ = _run(dev, c, want_order=False)
    assert short["order"] is None and all(np.array_equal(short[k], want[k]) for k in ("cluster", "selected", "sel_offsets"))


def test_numpy_scores_one_graph_and_each_output_alone(dev):
    import torch
    from athena_amd import _capi
    from athena_amd.geometry import topk_vertices

    c, want = tr.case("B = 1"), tr.expected("B = 1")
    cluster, selected, soff = topk_vertices(np.array(c["score"]), k=c["k"])                       # numpy in, offsets None: one graph
    assert np.array_equal(cluster.cpu().numpy(), want["cluster"]) and np.array_equal(selected.cpu().numpy(), want["selected"])
    assert soff.tolist() == [0, want["m"]]
    c, want = tr.case("sizes 0 1 2 63 64 65 128 129"), tr.expected("sizes 0 1 2 63 64 65 128 129")
    n, B, m = c["score"].size, c["offsets"].size - 1, want["m"]
    score = torch.from_numpy(np.array(c["score"])).to(dev)
    kk = tr.counts_of(c)
    _capi.use_torch_stream()
    for key in ("cluster", "selected", "order", None):
        outs = {k: torch.full((n if k == "cluster" else m,), -7, dtype=torch.int32, device=dev) if k == key else None
                for k in ("cluster", "selected", "order")}
        soff, count = np.full(B + 1, -1, np.int32), C.c_int64(-1)
        _capi.call("athena_mp_topk_vertices", B, n, vp(c["offsets"]), ptr(score), 0, vp(kk), 0, 0.0, ptr(outs["cluster"]), ptr(outs["selected"]),
                   ptr(outs["order"]), vp(soff) if key is not None else None, C.byref(count))
        assert count.value == m
        if key is not None:
            assert np.array_equal(outs[key].cpu().numpy(), want[key]) and np.array_equal(soff, want["sel_offsets"])


def test_the_switch_pins_the_route_and_the_statistics_report_it(dev, monkeypatch):
    from athena_amd._capi import AthenaMPError
    from athena_amd.geometry import topk_stats

    name = "every graph at most 64"
    c, want = tr.case(name), tr.expected(name)
    B = c["offsets"].size - 1
    runs = {}
    for route in ("auto", "wave", "sort"):
        monkeypatch.setenv("ATHENA_MP_TOPK_ROUTE", route)
        runs[route], _ = _run(dev, c)
        assert tr.same(runs[route], want) == []
        assert topk_stats() == tr.stats(c["offsets"], route), route
    assert topk_stats() == (0, B, 32 + tr.bits_for(B - 1), 5)
    # a batch of both kinds through the sort alone
    c, want = tr.case("sizes 0 1 2 63 64 65 128 129"), tr.expected("sizes 0 1 2 63 64 65 128 129")
    got, _ = _run(dev, c)
    assert tr.same(got, want) == [] and topk_stats() == (0, 8, 35, 5)
    monkeypatch.setenv("ATHENA_MP_TOPK_ROUTE", "wave")
    with pytest.raises(AthenaMPError, match=r"ATHENA_MP_TOPK_ROUTE = wave, but graph 6 has 65 vertices, more than 64"):
        _run(dev, c)
    monkeypatch.setenv("ATHENA_MP_TOPK_ROUTE", "lds")
    with pytest.raises(AthenaMPError, match="ATHENA_MP_TOPK_ROUTE = lds is none of auto, wave, sort"):
        _run(dev, c)
    monkeypatch.delenv("ATHENA_MP_TOPK_ROUTE")
    got, _ = _run(dev, c)                                                                        # the next call is correct
    assert tr.same(got, want) == [] and topk_stats() == (5, 3, 35, 5)
    c = tr.case("300 small graphs")
    monkeypatch.setenv("ATHENA_MP_TOPK_ROUTE", "sort")
    got, _ = _run(dev, c)
    assert tr.same(got, tr.expected("300 small graphs")) == [] and topk_stats() == (0, 300, 41, 6)


def test_refusals_carry_their_messages_and_leave_the_library_usable(dev):
    import torch
    from athena_amd import _capi
    from athena_amd._capi import AthenaMPError

    c, want = tr.case("k per graph"), tr.expected("k per graph")
    s, off, k = c["score"], c["offsets"], c["k"]
    n, B = s.size, off.size - 1
    score = torch.from_numpy(np.array(s)).to(dev)
    cluster = torch.full((n,), -7, dtype=torch.int32, device=dev)
    count, soff = C.c_int64(-1), np.zeros(B + 1, np.int32)

    def call(B_=B, n_=n, off_=off, k_=0, kk_=k):
        _capi.call("athena_mp_topk_vertices", B_, n_, vp(off_), ptr(score), k_, vp(kk_), 0, 0.0, ptr(cluster), None, None, vp(soff), C.byref(count))

    down = off.copy(); down[3] = off[2] - 1
    short = off.copy(); short[-1] -= 1
    first = off.copy(); first[0] = 1
    kneg = k.copy(); kneg[4] = -2
    _capi.use_torch_stream()
    for kw, match in ((dict(B_=-1), r"n_graphs = -1, n = \d+: negative"), (dict(n_=-1), r"n = -1: negative"),
                      (dict(off_=down), rf"offsets\(4\) = {down[3]} is below offsets\(3\) = {down[2]}: not ascending"),
                      (dict(off_=short), rf"the offsets end at {n - 1}, not at n = {n}"), (dict(off_=first), r"offsets\(1\) = 1, not 0"),
                      (dict(k_=-3, kk_=None), "k = -3 is negative"), (dict(kk_=kneg), r"k\(5\) = -2 is negative"),
                      (dict(B_=0, off_=np.zeros(1, np.int32)), rf"the offsets end at 0, not at n = {n}")):
        with pytest.raises(AthenaMPError, match=match):
            call(**kw)
        assert count.value == 0
        call()
        assert count.value == want["m"] and np.array_equal(cluster.cpu().numpy(), want["cluster"]) and np.array_equal(soff, want["sel_offsets"])
    with pytest.raises(AthenaMPError, match="null n_selected_out"):
        _capi.call("athena_mp_topk_vertices", B, n, vp(off), ptr(score), 0, vp(k), 0, 0.0, None, None, None, None, None)


# ---- the gated rows -----------------------------------------------------------------------------------------------------------------
def _rows(dev, cluster, selected, x, gate, dy):
    import torch

    t = lambda a: torch.from_numpy(np.array(a)).to(dev) if a is not None else None
    return t(cluster), t(selected), t(x), t(gate), t(dy)


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("gated", [True, False], ids=["gate", "no gate"])
def test_the_gated_rows_equal_the_transcription(dev, F, gated):
    from athena_amd.geometry import select_rows, select_rows_grad, unpool

    cluster, selected, x, gate, dy = tr.rows_case(60 + F, 777, 300, F, gated=gated, special=True)
    n, m = cluster.size, selected.size
    assert 0 < m < n and (cluster == 0).sum() == 300
    cd, sd, xd, gd, dyd = _rows(dev, cluster, selected, x, gate, dy)
    before = [t.clone() for t in (cd, sd, xd, dyd)]
    y = select_rows(sd, xd, gd)
    want = tr.rows_fwd(selected, x, gate)
    if gated:
        assert same_f32(y.cpu().numpy(), want)
    else:
        assert np.array_equal(y.cpu().numpy().view(np.int32), want.view(np.int32))               # NaN payloads and -0 survive
    g = select_rows_grad(cd, dyd, x=xd, gate=gd)
    dx, dgate = g["x"].cpu().numpy(), g["gate"].cpu().numpy()
    assert np.array_equal(dx.view(np.int32), tr.rows_bwd_x(cluster, dy, gate).view(np.int32))
    assert (dx.view(np.int32)[cluster == 0] == 0).all()
    # the gate's gradient: the one free order.  x holds non-finite values in a few rows: there the sum is what IEEE makes of them
    ref, scale = tr.rows_bwd_gate(cluster, dy, x)
    finite = np.isfinite(ref)
    assert finite.sum() > n - 40
    err = np.abs(dgate[finite].astype(np.float64) - ref[finite])
    worst = err - 1e-5 * scale[finite]
    print(f"F = {F}: dgate worst excess over 1e-5 * sum|dy x| = {worst.max():.3e}, worst |dev - f64| / scale = "
          f"{(err / np.maximum(scale[finite], 1e-300)).max():.3e}")
    assert (worst <= 0).all()
    assert (np.isnan(dgate[~finite]) == np.isnan(ref[~finite])).all() and np.array_equal(dgate[~finite & ~np.isnan(ref)], ref[~finite & ~np.isnan(ref)])
    assert (dgate.view(np.int32)[cluster == 0] == 0).all()                                        # exactly +0 where dropped
    again = select_rows_grad(cd, dyd, x=xd, gate=gd)
    assert np.array_equal(again["gate"].cpu().numpy().view(np.int32), dgate.view(np.int32)) and \
        np.array_equal(again["x"].cpu().numpy().view(np.int32), dx.view(np.int32))
    assert np.array_equal(select_rows(sd, xd, gd).cpu().numpy().view(np.int32), y.cpu().numpy().view(np.int32))
    # un-pooling after pooling: x on the kept rows, +0 elsewhere
    back = unpool(cd, select_rows(sd, xd)).cpu().numpy().view(np.int32)
    assert np.array_equal(back[selected - 1], x.view(np.int32)[selected - 1]) and (back[cluster == 0] == 0).all()
    for t, b in zip((cd, sd, xd, dyd), before):
        assert np.array_equal(t.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))


def test_the_gate_with_special_values_gives_numpys_products(dev):
    from athena_amd.geometry import select_rows, select_rows_grad

    # finite x and dy against a gate of -0, +0, inf, -inf and subnormals: every product is defined bit for bit
    r = tr._rng(70)
    n, F = 96, 6
    cluster = np.arange(1, n + 1, dtype=np.int32)
    selected = cluster.copy()
    x = r.standard_normal((n, F)).astype(np.float32)
    x[::7, 1] = np.float32(-0.0)
    x[3::11, 2] = tr._bits([0x00000005])[0]
    dy = r.standard_normal((n, F)).astype(np.float32)
    gate = np.tile(tr._bits([0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000007, 0x80000009, 0x3F800000, 0x00800000]), n // 8)
    keep = x != 0                                                     # 0 * inf is the one product whose NaN the hardware names
    cd, sd, xd, gd, dyd = _rows(dev, cluster, selected, x, gate, dy)
    y = select_rows(sd, xd, gd).cpu().numpy()
    want = tr.rows_fwd(selected, x, gate)
    assert np.array_equal(y.view(np.int32)[keep], want.view(np.int32)[keep]) and same_f32(y, want)
    assert np.signbit(y[0, 0]) != np.signbit(x[0, 0]) and (y[0] == 0).all()                      # times -0
    dx = select_rows_grad(cd, dyd, gate=gd, want=("x",))["x"].cpu().numpy()
    assert np.array_equal(dx.view(np.int32), tr.rows_bwd_x(cluster, dy, gate).view(np.int32))


def test_the_gated_rows_at_m_zero_and_their_refusals(dev):
    import torch
    from athena_amd import _capi
    from athena_amd._capi import AthenaMPError
    from athena_amd.geometry import select_rows, select_rows_grad, unpool

    cluster, selected, x, gate, dy = tr.rows_case(71, 50, 50, 8)
    assert selected.size == 0
    cd, sd, xd, gd, dyd = _rows(dev, cluster, selected, x, gate, dy)
    assert tuple(select_rows(sd, xd, gd).shape) == (0, 8)
    g = select_rows_grad(cd, dyd, x=xd, gate=gd)
    assert (g["x"].cpu().numpy().view(np.int32) == 0).all() and (g["gate"].cpu().numpy().view(np.int32) == 0).all()
    assert tuple(unpool(cd, dyd).shape) == (50, 8)
    cluster, selected, x, gate, dy = tr.rows_case(72, 300, 100, 12)
    n, m, F = 300, 200, 12
    cd, sd, xd, gd, dyd = _rows(dev, cluster, selected, x, gate, dy)
    y = torch.empty((m, F), dtype=torch.float32, device=dev)
    dx, dgate = torch.empty((n, F), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev)
    fwd = lambda n_=n, m_=m, F_=F, s=sd: _capi.call("athena_mp_select_rows_fwd", n_, m_, F_, ptr(s), ptr(xd), ptr(gd), ptr(y))
    bwd = lambda n_=n, m_=m, F_=F, c=cd, a=dx, b=dgate: _capi.call("athena_mp_select_rows_bwd", n_, m_, F_, ptr(c), ptr(dyd), ptr(xd), ptr(gd),
                                                                   ptr(a), ptr(b))
    bad_sel = selected.copy(); bad_sel[150] = n + 1; bad_sel[170] = 0
    bad_low = selected.copy(); bad_low[9] = 0
    bad_cl = cluster.copy(); bad_cl[40] = m + 1; bad_cl[250] = -1
    bad_neg = cluster.copy(); bad_neg[7] = -5
    t = lambda a: torch.from_numpy(a).to(dev)
    _capi.use_torch_stream()
    for call, kw, match in ((fwd, dict(F_=0), "select_rows_fwd: F = 0: need at least one feature column"),
                            (fwd, dict(m_=-1), rf"select_rows_fwd: n = {n}, m = -1: negative"),
                            (fwd, dict(s=t(bad_sel)), rf"select_rows_fwd: selected\(151\) = {n + 1} outside \[1,{n}\]"),
                            (fwd, dict(s=t(bad_low)), rf"select_rows_fwd: selected\(10\) = 0 outside \[1,{n}\]"),
                            (bwd, dict(F_=-2), "select_rows_bwd: F = -2: need at least one feature column"),
                            (bwd, dict(n_=-1), rf"select_rows_bwd: n = -1, m = {m}: negative"),
                            (bwd, dict(c=t(bad_cl)), rf"select_rows_bwd: cluster\(41\) = {m + 1} outside \[0,{m}\]"),
                            (bwd, dict(c=t(bad_neg)), rf"select_rows_bwd: cluster\(8\) = -5 outside \[0,{m}\]"),
                            (bwd, dict(c=t(bad_neg), a=None), rf"select_rows_bwd: cluster\(8\) = -5 outside \[0,{m}\]"),
                            (bwd, dict(a=None, b=None), "select_rows_bwd: neither dx nor dgate is asked for")):
        with pytest.raises(AthenaMPError, match=match):
            call(**kw)
        fwd()
        bwd()
        assert same_f32(y.cpu().numpy(), tr.rows_fwd(selected, x, gate))
        assert np.array_equal(dx.cpu().numpy().view(np.int32), tr.rows_bwd_x(cluster, dy, gate).view(np.int32))


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
def test_the_chain_from_a_batch_to_the_induced_subgraph(dev):
    """from_edges -> topk_vertices -> from_contraction(handle, cluster, m): the coarse list, edge_pair and weights of the
    contraction yardstick on the same map, and sel_offsets cut the pooled handle into its graphs"""
    import torch
    from athena_amd import DeviceDataset, DeviceGraph
    from athena_amd.geometry import select_rows, topk_vertices

    r = tr._rng(80)
    sizes = np.array([9, 70, 1, 33, 0, 140])
    off = tr._offsets(sizes)
    n = int(off[-1])
    pairs = []
    for g, ng in enumerate(sizes):                                    # a ring and some chords inside every graph: block-diagonal
        if ng < 2:
            continue
        a = np.arange(ng)
        ring = np.stack([a, (a + 1) % ng], axis=1)
        chords = r.integers(0, ng, (2 * ng, 2))
        e = np.concatenate([ring, chords[chords[:, 0] != chords[:, 1]]])
        pairs.append(np.unique(np.sort(e, axis=1), axis=0) + off[g] + 1)
    pairs = np.concatenate(pairs).astype(np.int32)
    fine = DeviceGraph.from_edges(n, np.asfortranarray(pairs.T))
    score = r.standard_normal(n).astype(np.float32)
    cluster, selected, soff = topk_vertices(torch.from_numpy(score).to(dev), off, ratio=0.5)
    want_sel = tr.select(score, off, tr.ratio_counts(sizes, 0.5))
    m = want_sel["m"]
    assert np.array_equal(cluster.cpu().numpy(), want_sel["cluster"]) and np.array_equal(soff, want_sel["sel_offsets"]) and m == int(selected.shape[0])
    list_of_handle = fine.pair_list().cpu().numpy()
    want = cr.contract(list_of_handle, n, n, want_sel["cluster"], want_sel["cluster"], m, m, 0)
    assert 0 < want["P"] < pairs.shape[0]
    coarse, coarse_pairs, pool, weights, edge_pair = DeviceGraph.from_contraction(fine, cluster, m)
    got = dict(coarse_pairs=coarse_pairs.cpu().numpy(), weights=weights.cpu().numpy(), edge_pair=edge_pair.cpu().numpy())
    assert cr.same(got, want, tuple(got)) == []
    host = DeviceGraph.from_edges(m, np.asfortranarray(want["coarse_pairs"].T))
    assert (coarse.n_rows, coarse.n_cols, coarse.nnz, coarse.n_edge_cols) == (m, m, host.nnz, want["P"])
    for name in DeviceGraph._ARRAYS:
        a, b = coarse.export(name), host.export(name)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), name
    # every kept edge joins two kept vertices of one graph: the pooled batch is block-diagonal under sel_offsets
    cp = want["coarse_pairs"]
    eoff = np.searchsorted(cp[:, 0], soff.astype(np.int64) + 1, side="left").astype(np.int64)
    ds = DeviceDataset(coarse, soff, eoff)
    assert len(ds) == sizes.size
    voff, eo = ds.sizes([5, 1])
    assert voff.tolist() == [0, soff[6] - soff[5], soff[6] - soff[5] + soff[2] - soff[1]] and eo[-1] == (eoff[6] - eoff[5]) + (eoff[2] - eoff[1])
    x = torch.from_numpy(r.standard_normal((n, 4)).astype(np.float32)).to(dev)
    assert np.array_equal(select_rows(selected, x).cpu().numpy(), x.cpu().numpy()[want_sel["selected"] - 1])


# ---- the other forms ----------------------------------------------------------------------------------------------------------------
HOST_CASES = ("three tiles and small graphs", "special values, sort", "k per graph", "min_score with NaNs", "n = 0, B = 3")


def _device_rows(dev, want, x, gate, dy):
    """the device entries on a selection: (y, dx, dgate) as numpy"""
    import torch
    from athena_amd.geometry import select_rows, select_rows_grad

    t = lambda a: torch.from_numpy(np.array(a)).to(dev) if a is not None else None
    cd, sd, xd, gd, dyd = t(want["cluster"]), t(want["selected"]), t(x), t(gate), t(dy)
    y = select_rows(sd, xd, gd)
    g = select_rows_grad(cd, dyd, x=xd, gate=gd)
    return y.cpu().numpy(), g["x"].cpu().numpy(), g["gate"].cpu().numpy()


def _features(name, want, n, F=5):
    r = tr._rng(len(name))
    x = r.standard_normal((n, F)).astype(np.float32)
    gate = r.standard_normal(n).astype(np.float32)
    dy = r.standard_normal((want["m"], F)).astype(np.float32)
    return x, gate, dy


@pytest.mark.parametrize("name", HOST_CASES)
def test_the_host_forms_write_the_bytes_of_the_device_entries(dev, name):
    from athena_amd import _capi

    c, want = tr.case(name), tr.expected(name)
    s, off = np.array(c["score"]), c["offsets"]
    n, B, m = s.size, off.size - 1, want["m"]
    kk = np.ascontiguousarray(np.broadcast_to(np.asarray(tr.counts_of(c), np.int32), (B,)))
    room = int(np.minimum(kk.astype(np.int64), np.diff(off.astype(np.int64))).sum())
    out = dict(cluster=np.full(n, -7, np.int32), selected=np.full(room, -7, np.int32), order=np.full(room, -7, np.int32),
               sel_offsets=np.full(B + 1, -7, np.int32))
    count = C.c_int64(-1)
    has_min = int(c["min_score"] is not None)
    _capi.call("athena_mp_topk_vertices_host", B, n, vp(off), vp(s), 0, vp(kk), has_min, float(c["min_score"]) if has_min else 0.0,
               vp(out["cluster"]), vp(out["selected"]), vp(out["order"]), vp(out["sel_offsets"]), C.byref(count))
    assert count.value == m and (out["selected"][m:] == -7).all() and (out["order"][m:] == -7).all()       # exactly m are written
    got = dict(out, selected=out["selected"][:m], order=out["order"][:m], m=m)
    assert tr.same(got, want) == []
    x, gate, dy = _features(name, want, n)
    F = x.shape[1]
    y, dx, dgate = np.full((m, F), np.nan, np.float32), np.full((n, F), np.nan, np.float32), np.full(n, np.nan, np.float32)
    _capi.call("athena_mp_select_rows_host", n, m, F, vp(want["selected"]), vp(x), vp(gate), vp(y))
    _capi.call("athena_mp_select_rows_bwd_host", n, m, F, vp(want["cluster"]), vp(dy), vp(x), vp(gate), vp(dx), vp(dgate))
    dev_y, dev_dx, dev_dgate = _device_rows(dev, want, x, gate, dy)
    for a, b in ((y, dev_y), (dx, dev_dx), (dgate, dev_dgate)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    if n:
        assert np.array_equal(y.view(np.int32), tr.rows_fwd(want["selected"], x, gate).view(np.int32))


@pytest.mark.parametrize("name", ["three tiles and small graphs", "k per graph", "min_score with NaNs"])
def test_fortran_program_writes_the_bytes_of_the_device_entries(dev, tmp_path, name):
    if not os.path.exists(RUNNER):
        pytest.fail("topk_run is not built: __graft_entry__.build() compiles the Fortran host side")
    c, want = tr.case(name), tr.expected(name)
    s, off = np.array(c["score"]), c["offsets"]
    n, B, m = s.size, off.size - 1, want["m"]
    k = tr.counts_of(c)
    each = np.ndim(k) > 0
    has_min = int(c["min_score"] is not None)
    x, gate, dy = _features(name, want, n)
    F = x.shape[1]
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        np.array([B, n, int(each), 0 if each else int(k), has_min, F, 1], np.int32).tofile(f)
        np.array([c["min_score"] if has_min else 0.0], np.float32).tofile(f)
        off.tofile(f)
        s.tofile(f)
        if each:
            np.asarray(k, np.int32).tofile(f)
        x.tofile(f)
        gate.tofile(f)
        dy.tofile(f)
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"topk_run failed ({out.returncode}): {out.stdout[-1000:]} {out.stderr[-2000:]}"
    raw = open(res, "rb").read()
    at = 0

    def take(dtype, *shape):
        nonlocal at
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), at).reshape(shape)
        at += a.nbytes
        return a

    assert take(np.int64, 1).tolist() == [m]
    got = dict(cluster=take(np.int32, n), selected=take(np.int32, m), order=take(np.int32, m), sel_offsets=take(np.int32, B + 1), m=m)
    assert tr.same(got, want) == []
    y, dx, dgate = take(np.float32, m, F), take(np.float32, n, F), take(np.float32, n)
    assert take(np.int64, 4).tolist() == list(tr.stats(off)) and at == len(raw)
    dev_y, dev_dx, dev_dgate = _device_rows(dev, want, x, gate, dy)
    for a, b in ((y, dev_y), (dx, dev_dx), (dgate, dev_dgate)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
