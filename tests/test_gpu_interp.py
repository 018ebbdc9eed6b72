"""GPU: inverse-distance interpolation over two-set handles (athena_amd/csrc/interp.hip) against the transcription of the definition
(tests/interp_reference.py).  Handles come from DeviceGraph.from_point_sets_knn and from_point_sets on clouds of 300 queries
and 200 sources in all, one of them without sources: k = 1, 3, 64; a radius handle with a hub row of 150 entries beside empty rows; a query
on a source (s = 0, the clamp); coordinates whose squared distances overflow (w = 0, a row with W = 0); coordinates at 1e19
(subnormal w).  weights, wsum, y and dx equal the yardstick word for word; dcoords is exactly +0 where the definition says so and
elsewhere inside the derived bound around the float64 twin; refusals, the host forms, the Fortran runner and the Python chain down to
both point sets are covered."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bipartite_reference as br
import interp_reference as ir
import knn_bipartite_reference as kb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "interp_run")
EPS = 1e-16
ALL_F = (1, 3, 4, 7, 64, 66, 128, 256, 260)        # both load routes, every group width (4 .. 64), two passes beyond 256 columns
CASES = ("knn1", "knn3", "knn64", "hub", "overflow", "subnormal", "wide")

vp = lambda a: a.ctypes.data_as(C.c_void_p)
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def _rng(seed):
    return np.random.default_rng(seed)


@functools.lru_cache(None)
def points(name):
    """(queries, sources, query_offsets, source_offsets, k or None, radius or None): three clouds, the middle one without
    sources, so its queries' rows are empty"""
    rng = _rng(7000 + CASES.index(name))
    qoff, soff = br.offsets_of([170, 30, 100]), br.offsets_of([120, 0, 80])
    q, s = rng.random((300, 3)).astype(np.float32), rng.random((200, 3)).astype(np.float32)
    if name.startswith("knn"):
        q[5], q[250] = s[7], s[160]                          # queries on sources of their own clouds: s = 0
        return q, s, qoff, soff, int(name[3:]), None
    if name == "hub":
        centre = np.array([0.5, 0.5, 0.5], np.float32)
        soff = br.offsets_of([160, 0, 40])
        s[:150] = centre + (rng.random((150, 3)).astype(np.float32) - 0.5) * np.float32(0.02)   # 150 sources inside one radius
        s[150:] = rng.random((50, 3)).astype(np.float32) * np.float32(0.25)                      # the rest in a corner
        q[0] = centre
        q[1:60] = centre + (rng.random((59, 3)).astype(np.float32) - 0.5) * np.float32(0.12)    # around the hub: part of it in reach
        q[60:170] = rng.random((110, 3)).astype(np.float32) * np.float32(0.3)                    # short rows and empty ones
        q[200:] = rng.random((100, 3)).astype(np.float32) * np.float32(0.6)
        q[201] = s[175]
        return q, s, qoff, soff, None, 0.05
    if name == "overflow":
        q, s = q * np.float32(2e19), s * np.float32(2e19)    # far pairs: s = +inf beside finite ones
        q[3] = np.float32(3e38)                              # every s of this row overflows: W = 0
        return q, s, qoff, soff, 64, None
    if name == "subnormal":
        return q * np.float32(1e19), s * np.float32(1e19), qoff, soff, 64, None
    draw = lambda n: (2.0 ** rng.uniform(-10, 10, (n, 3))).astype(np.float32)            # "wide": the clouds of the dcoords bound
    q, s = draw(300), draw(200)
    q[9] = s[11]
    return q, s, qoff, soff, 8, None


@functools.lru_cache(None)
def yardstick(name):
    """(i, j, coords, A) of the case from the builders' yardsticks"""
    q, s, qoff, soff, k, radius = points(name)
    if k is not None:
        nbr, _ = kb.brute_force(q, s, k, None, qoff, soff)
        i, j, coords, _, _ = kb.graph_of(nbr, q, s, qoff)
    else:
        i, j, coords, _, _ = br.reference_pairs(q, s, radius, qoff, soff)
    return i, j, coords, ir.arrays_of(i, j, q.shape[0], s.shape[0])


@functools.lru_cache(None)
def handle(name):
    """(DeviceGraph, coords on the device) from the device builders, checked against the yardstick's pairs once"""
    from athena_amd import DeviceGraph

    q, s, qoff, soff, k, radius = points(name)
    if k is not None:
        g, coords, _ = DeviceGraph.from_point_sets_knn(q, s, k, query_offsets=qoff, source_offsets=soff)
    else:
        g, coords, _ = DeviceGraph.from_point_sets(q, s, radius, qoff, soff)
    i, j, want, A = yardstick(name)
    assert np.array_equal(bits(coords.cpu().numpy()), bits(want)), "the builder's coords are not the yardstick's"
    for key, arr in A.items():
        assert np.array_equal(g.export(key), arr), f"the handle's {key} is not the one derived from the pair list"
    return g, coords


@functools.lru_cache(None)
def features(name, F):
    """x [n_sources, F], dy [n_queries, F]; the "wide" case in +-[2^-10, 2^10] so that nothing under- or overflows on the way"""
    rng = _rng(7100 + 17 * CASES.index(name) + F)
    if name == "wide":
        draw = lambda n: ((2.0 ** rng.uniform(-10, 10, (n, F))) * rng.choice([-1.0, 1.0], (n, F))).astype(np.float32)
        return draw(200), draw(300)
    x, dy = rng.standard_normal((200, F)).astype(np.float32), rng.standard_normal((300, F)).astype(np.float32)
    x[::7, 0], dy[::5, F - 1] = -0.0, -0.0
    return x, dy


@functools.lru_cache(None)
def reference(name, F):
    """the yardstick's (weights, wsum, y, dx), computed once per case"""
    _, _, coords, A = yardstick(name)
    x, dy = features(name, F)
    w, W = ir.weights(A, coords, EPS)
    return w, W, ir.fwd(A, w, x), ir.bwd_x(A, w, dy)


def up(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def device_weights(g, coords, dev, eps=EPS, dim=3):
    import torch
    from athena_amd import _capi

    w = torch.full((g.n_edge_cols,), np.nan, dtype=torch.float32, device=dev)
    W = torch.full((g.n_rows,), np.nan, dtype=torch.float32, device=dev)
    _capi.use_torch_stream()
    _capi.call("athena_mp_interp_weights", g.handle, dim, ptr(coords), eps, ptr(w), ptr(W))
    return w, W


def device_gather(entry, g, w, x, rows, dev):
    import torch
    from athena_amd import _capi

    out = torch.full((rows, x.shape[1]), np.nan, dtype=torch.float32, device=dev)
    _capi.use_torch_stream()
    _capi.call(entry, g.handle, int(x.shape[1]), ptr(w), ptr(x), ptr(out))
    return out


def device_dcoords(g, coords, w, x, y, dy, dev, eps=EPS):
    import torch
    from athena_amd import _capi

    out = torch.full((g.n_edge_cols, 3), np.nan, dtype=torch.float32, device=dev)
    _capi.use_torch_stream()
    _capi.call("athena_mp_interp_bwd_coords", g.handle, 3, int(x.shape[1]), ptr(coords), eps, ptr(w), ptr(x), ptr(y), ptr(dy), ptr(out))
    return out


# ---- weights -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_weights_and_their_row_sums_equal_the_yardstick(dev, name):
    g, coords = handle(name)
    i, j, cnp, A = yardstick(name)
    lens = np.diff(A["rowptr"])
    want_w, want_W = ir.weights(A, cnp, EPS)
    raw, s = ir.raw_weight(cnp, EPS)
    if name.startswith("knn") or name == "wide":
        assert (s == 0).sum() >= 1, "the case must hold a query on a source"
    if name == "hub":
        assert lens[0] > 64 and lens[0] % 8 != 0 and (lens == 0).sum() >= 10 and (s == 0).any()
    if name == "overflow":
        assert np.isinf(s).any() and (want_W == 0).sum() >= 1 and ((want_W > 0) & (lens > 0)).any()
        assert any(np.isinf(s[a:b]).any() and np.isfinite(s[a:b]).any() for a, b in zip(A["rowptr"][:-1], A["rowptr"][1:]))
    if name == "subnormal":
        assert ((raw > 0) & (raw < np.finfo(np.float32).tiny)).any(), "the case must hold a subnormal w"
    assert (lens == 0).any(), "an empty slice gives empty rows"
    w, W = device_weights(g, coords, dev)
    assert np.array_equal(bits(w.cpu().numpy()), bits(want_w))
    assert np.array_equal(bits(W.cpu().numpy()), bits(want_W))
    w2, W2 = device_weights(g, coords, dev)
    assert w2.cpu().numpy().tobytes() == w.cpu().numpy().tobytes() and W2.cpu().numpy().tobytes() == W.cpu().numpy().tobytes()
    import torch
    from athena_amd import _capi

    only = torch.full((g.n_edge_cols,), np.nan, dtype=torch.float32, device=dev)          # wsum may be NULL
    _capi.call("athena_mp_interp_weights", g.handle, 3, ptr(coords), EPS, ptr(only), None)
    assert np.array_equal(bits(only.cpu().numpy()), bits(want_w))


# ---- the weighted gather, forward and transposed -------------------------------------------------------------------------------
GATHER = [(n, F) for n in ("knn3", "hub") for F in ALL_F] + [(n, F) for n in ("knn1", "knn64", "overflow", "subnormal") for F in (4, 7)]


@pytest.mark.parametrize("name,F", GATHER)
def test_y_and_dx_equal_the_yardstick(dev, name, F):
    g, _ = handle(name)
    x, dy = features(name, F)
    want_w, _, want_y, want_dx = reference(name, F)
    w, xd, dyd = up(want_w, dev), up(x, dev), up(dy, dev)
    y = device_gather("athena_mp_interp_fwd", g, w, xd, g.n_rows, dev)
    dx = device_gather("athena_mp_interp_bwd_x", g, w, dyd, g.n_cols, dev)
    assert np.array_equal(bits(y.cpu().numpy()), bits(want_y))
    assert np.array_equal(bits(dx.cpu().numpy()), bits(want_dx))
    again = device_gather("athena_mp_interp_fwd", g, w, xd, g.n_rows, dev)
    assert again.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert np.array_equal(bits(xd.cpu().numpy()), bits(x)) and np.array_equal(bits(w.cpu().numpy()), bits(want_w))


def test_unit_weights_give_the_plain_column_sum(dev):
    g, _ = handle("hub")
    _, _, _, A = yardstick("hub")
    _, dy = features("hub", 7)
    want = np.zeros((g.n_cols, 7), np.float32)
    for j in range(g.n_cols):
        acc = np.zeros(7, np.float32)
        for k in range(A["t_rowptr"][j], A["t_rowptr"][j + 1]):
            acc = acc + dy[A["t_src"][k]]
        want[j] = acc
    dx = device_gather("athena_mp_interp_bwd_x", g, up(np.ones(g.n_edge_cols, np.float32), dev), up(dy, dev), g.n_cols, dev)
    assert np.array_equal(bits(dx.cpu().numpy()), bits(want))


# ---- the coordinate gradient ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", ALL_F)
def test_dcoords_stays_inside_the_derived_bound(dev, F):
    """|device - f64| <= (F + 8) 2^-24 * 2 |d_c| * weights[e] * w_e * sum_f |dy| (|x| + |y|), the twin evaluated from the same fp32
    weights, y and coords; exactly +0 on the clamped edge"""
    g, coords = handle("wide")
    _, _, cnp, A = yardstick("wide")
    x, dy = features("wide", F)
    w, _, y, _ = reference("wide", F)
    got = device_dcoords(g, coords, up(w, dev), up(x, dev), up(y, dev), up(dy, dev), dev).cpu().numpy()
    zero = ir.zero_by_definition(cnp, EPS)
    assert zero.sum() >= 1 and not bits(got[zero]).any(), "a clamped edge must have dcoords = +0 exactly"
    twin = ir.bwd_coords(A, cnp, EPS, w, x, y, dy, np.float64)
    bound = ir.dcoords_bound(cnp, EPS, w, x, y, dy, A)
    err = np.abs(got.astype(np.float64) - twin)
    print(f"F = {F}: worst |device - f64| / bound = {(err[~zero] / bound[~zero]).max():.3f}")
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    assert (err[~zero] <= bound[~zero]).all()


@pytest.mark.parametrize("name", ["knn64", "hub", "overflow"])
def test_dcoords_is_zero_where_the_definition_says_so(dev, name):
    g, coords = handle(name)
    _, _, cnp, A = yardstick(name)
    x, dy = features(name, 7)
    w, _, y, _ = reference(name, 7)
    got = device_dcoords(g, coords, up(w, dev), up(x, dev), up(y, dev), up(dy, dev), dev).cpu().numpy()
    zero = ir.zero_by_definition(cnp, EPS)
    assert zero.any() and not bits(got[zero]).any()
    want = ir.bwd_coords(A, cnp, EPS, w, x, y, dy)
    live = ~zero & np.isfinite(want).all(axis=1)
    scale = np.abs(want[live]).max()
    assert live.any() and np.abs(got[live] - want[live]).max() <= 1e-4 * scale      # a gross check; the bound is held on "wide"


# ---- refusals, empty sets ------------------------------------------------------------------------------------------------------
def test_refusals_arrive_with_their_messages_and_the_library_goes_on(dev):
    import torch
    from athena_amd import DeviceGraph, _capi
    from athena_amd._capi import AthenaMPError
    from helpers import random_graph

    g, coords = handle("knn3")
    x, dy = features("knn3", 4)
    want_w, _, want_y, _ = reference("knn3", 4)
    w, xd, dyd, y = up(want_w, dev), up(x, dev), up(dy, dev), torch.empty((300, 4), device=dev)
    dc = torch.empty((g.n_edge_cols, 3), device=dev)
    with pytest.raises(AthenaMPError, match=r"interp_weights: dim = 4 is outside 1..3"):
        _capi.call("athena_mp_interp_weights", g.handle, 4, ptr(coords), EPS, ptr(w), None)
    with pytest.raises(AthenaMPError, match=r"interp_bwd_coords: dim = 0 is outside 1..3"):
        _capi.call("athena_mp_interp_bwd_coords", g.handle, 0, 4, ptr(coords), EPS, ptr(w), ptr(xd), ptr(y), ptr(dyd), ptr(dc))
    for entry, a, b in (("athena_mp_interp_fwd", xd, y), ("athena_mp_interp_bwd_x", dyd, xd)):
        with pytest.raises(AthenaMPError, match=r"F = 0: need at least one feature column"):
            _capi.call(entry, g.handle, 0, ptr(w), ptr(a), ptr(b))
    for eps in (0.0, 2.0 ** -61, float("inf"), float("nan"), -1.0):
        with pytest.raises(AthenaMPError, match=r"eps = .*: need a finite value of at least 2\^-60"):
            _capi.call("athena_mp_interp_weights", g.handle, 3, ptr(coords), eps, ptr(w), None)
    with pytest.raises(AthenaMPError, match=r"need a finite value of at least 2\^-60"):
        _capi.call("athena_mp_interp_bwd_coords", g.handle, 3, 4, ptr(coords), 0.0, ptr(w), ptr(xd), ptr(y), ptr(dyd), ptr(dc))
    ia, ja = random_graph(20, 40, 1, self_loops=True)
    kipf = DeviceGraph(ia, ja, n_edge_cols=0)
    with pytest.raises(AthenaMPError, match=r"interp_fwd: the handle has no edge columns"):
        _capi.call("athena_mp_interp_fwd", kipf.handle, 4, ptr(w), ptr(xd), ptr(y))
    loops = DeviceGraph(ia, ja)                              # self-loop entries carry no edge id
    with pytest.raises(AthenaMPError, match=r"interp_weights: \d+ of the handle's \d+ entries carry no edge id"):
        _capi.call("athena_mp_interp_weights", loops.handle, 3, ptr(coords), EPS, ptr(w), None)
    ia2, ja2 = random_graph(20, 40, 1, self_loops=False)
    square = DeviceGraph(ia2, ja2)                           # an undirected pair is two entries of one edge column
    with pytest.raises(AthenaMPError, match=r"interp_fwd: \d+ entries over \d+ edge columns: need one entry per edge column"):
        _capi.call("athena_mp_interp_fwd", square.handle, 4, ptr(w), ptr(xd), ptr(y))
    with pytest.raises(AthenaMPError, match=r"interp_host: dim = 7 is outside 1..3"):
        _capi.call("athena_mp_interp_host", g.handle, 7, 4, None, EPS, None, None, None)
    with pytest.raises(AthenaMPError, match=r"interp_bwd_host: F = -1"):
        _capi.call("athena_mp_interp_bwd_host", g.handle, 3, -1, None, EPS, None, None, None, None)
    _capi.call("athena_mp_interp_weights", g.handle, 3, ptr(coords), 2.0 ** -60, ptr(w), None)      # the smallest eps is taken
    w = up(want_w, dev)
    _capi.call("athena_mp_interp_fwd", g.handle, 4, ptr(w), ptr(xd), ptr(y))
    assert np.array_equal(bits(y.cpu().numpy()), bits(want_y))
    kipf.close(); loops.close(); square.close()


def test_empty_sets_succeed_and_write_zeros(dev):
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.geometry import interp_weights, interpolate, interpolate_grad

    some, none = _rng(7300).random((5, 2)).astype(np.float32), np.zeros((0, 2), np.float32)
    for q, s in ((some, none), (none, some), (none, none)):
        g, coords, _ = DeviceGraph.from_point_sets(q, s, 1.0)
        assert g.n_edge_cols == 0
        w, W = interp_weights(g, coords)
        y = interpolate(g, w, torch.ones((s.shape[0], 3), device=dev), out=torch.full((q.shape[0], 3), np.nan, device=dev))
        res = interpolate_grad(g, coords, w, torch.ones((s.shape[0], 3), device=dev), y, torch.ones((q.shape[0], 3), device=dev))
        for t, shape in ((w, (0,)), (W, (q.shape[0],)), (y, (q.shape[0], 3)), (res["x"], (s.shape[0], 3)), (res["coords"], (0, 2))):
            assert tuple(t.shape) == shape and not bits(t.cpu().numpy()).any()
        g.close()


# ---- host forms, Fortran, the Python chain -------------------------------------------------------------------------------------
def _device_chain(name, F, dev):
    """(weights, y, dx, dcoords, dqueries, dsources) of the device entries as numpy"""
    from athena_amd.geometry import interp_weights, interpolate, interpolate_grad, point_sets_grad

    g, coords = handle(name)
    x, dy = features(name, F)
    w, _ = interp_weights(g, coords, EPS)
    y = interpolate(g, w, up(x, dev))
    res = interpolate_grad(g, coords, w, up(x, dev), y, up(dy, dev), EPS)
    p = point_sets_grad(g, res["coords"])
    return tuple(t.cpu().numpy() for t in (w, y, res["x"], res["coords"], p["queries"], p["sources"]))


@pytest.mark.parametrize("name,F", [("knn3", 7), ("hub", 64)])
def test_the_chain_down_to_both_point_sets_equals_the_yardstick_chain(dev, name, F):
    """weights, y and dx word for word; dcoords (not bit-defined) inside the bound; the point gradients are the sequential sums of
    the device's own dcoords word for word"""
    import torch
    from athena_amd.geometry import interpolate, interpolate_grad

    i, j, cnp, A = yardstick(name)
    x, dy = features(name, F)
    want_w, _, want_y, want_dx = reference(name, F)
    w, y, dx, dc, dq, ds = _device_chain(name, F, dev)
    assert np.array_equal(bits(w), bits(want_w)) and np.array_equal(bits(y), bits(want_y)) and np.array_equal(bits(dx), bits(want_dx))
    zero = ir.zero_by_definition(cnp, EPS)
    assert not bits(dc[zero]).any()
    twin = ir.bwd_coords(A, cnp, EPS, w, x, y, dy, np.float64)
    assert (np.abs(dc.astype(np.float64) - twin)[~zero] <= ir.dcoords_bound(cnp, EPS, w, x, y, dy, A)[~zero]).all()
    wq, ws = br.reference_grad(i, j, dc, 300, 200)
    assert np.array_equal(bits(dq), bits(wq)) and np.array_equal(bits(ds), bits(ws))
    g, coords = handle(name)
    with pytest.raises(ValueError, match="weights must be a contiguous float32 device tensor"):
        interpolate(g, torch.zeros(3, device=dev), up(x, dev))
    with pytest.raises(ValueError, match="want must name"):
        interpolate_grad(g, coords, up(w, dev), up(x, dev), up(y, dev), up(dy, dev), want=("y",))
    only_x = interpolate_grad(g, None, up(w, dev), None, None, up(dy, dev), want=("x",))
    assert list(only_x) == ["x"] and np.array_equal(bits(only_x["x"].cpu().numpy()), bits(want_dx))


@pytest.mark.parametrize("name,F", [("knn3", 7), ("hub", 64)])
def test_host_forms_give_the_device_entries_bytes(dev, name, F):
    from athena_amd import _capi

    g, _ = handle(name)
    _, _, cnp, _ = yardstick(name)
    x, dy = features(name, F)
    w, y, dx, dc, _, _ = _device_chain(name, F, dev)
    E = g.n_edge_cols
    hy, hw = np.full((300, F), np.nan, np.float32), np.full(E, np.nan, np.float32)
    _capi.call("athena_mp_interp_host", g.handle, 3, F, vp(cnp), EPS, vp(x), vp(hy), vp(hw))
    assert hy.tobytes() == y.tobytes() and hw.tobytes() == w.tobytes()
    hy2 = np.full((300, F), np.nan, np.float32)
    _capi.call("athena_mp_interp_host", g.handle, 3, F, vp(cnp), EPS, vp(x), vp(hy2), None)
    assert hy2.tobytes() == y.tobytes()
    hdx, hdc = np.full((200, F), np.nan, np.float32), np.full((E, 3), np.nan, np.float32)
    _capi.call("athena_mp_interp_bwd_host", g.handle, 3, F, vp(cnp), EPS, vp(x), vp(dy), vp(hdx), vp(hdc))
    assert hdx.tobytes() == dx.tobytes() and hdc.tobytes() == dc.tobytes()
    hdx2, hdc2 = np.full((200, F), np.nan, np.float32), np.full((E, 3), np.nan, np.float32)
    _capi.call("athena_mp_interp_bwd_host", g.handle, 3, F, vp(cnp), EPS, vp(x), vp(dy), vp(hdx2), None)
    _capi.call("athena_mp_interp_bwd_host", g.handle, 3, F, vp(cnp), EPS, vp(x), vp(dy), None, vp(hdc2))
    assert hdx2.tobytes() == dx.tobytes() and hdc2.tobytes() == dc.tobytes()
    with pytest.raises(_capi.AthenaMPError, match="dx and dcoords are both null"):
        _capi.call("athena_mp_interp_bwd_host", g.handle, 3, F, vp(cnp), EPS, vp(x), vp(dy), None, None)


def test_fortran_program_writes_the_device_entries_bytes(dev, tmp_path):
    if not os.path.exists(RUNNER):
        pytest.fail("interp_run is not built: __graft_entry__.build() compiles the Fortran host side")
    from athena_amd import DeviceGraph
    from athena_amd.geometry import interp_weights, interpolate, interpolate_grad, point_sets_grad

    rng = _rng(7400)
    nq, ns, k, F = 90, 40, 3, 6
    q, s = rng.random((nq, 3)).astype(np.float32), rng.random((ns, 3)).astype(np.float32)
    q[4] = s[9]
    x, dy = rng.standard_normal((ns, F)).astype(np.float32), rng.standard_normal((nq, F)).astype(np.float32)
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        np.array([nq, ns, 3, k, F], np.int32).tofile(f)
        np.array([np.inf, EPS], np.float32).tofile(f)
        q.tofile(f); s.tofile(f); x.tofile(f); dy.tofile(f)
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"interp_run failed ({out.returncode}): {out.stdout[-1000:]} {out.stderr[-2000:]}"
    g, coords, _ = DeviceGraph.from_point_sets_knn(q, s, k)
    E = g.n_edge_cols
    w, _ = interp_weights(g, coords, EPS)
    y = interpolate(g, w, up(x, dev))
    grad = interpolate_grad(g, coords, w, up(x, dev), y, up(dy, dev), EPS)
    p = point_sets_grad(g, grad["coords"])
    raw = open(res, "rb").read()
    assert np.frombuffer(raw, np.int64, 1)[0] == E
    at = 8
    for what, t in (("coords", coords), ("weights", w), ("y", y), ("dx", grad["x"]), ("dcoords", grad["coords"]),
                    ("dqueries", p["queries"]), ("dsources", p["sources"])):
        a = t.cpu().numpy()
        assert raw[at:at + a.nbytes] == a.tobytes(), what
        at += a.nbytes
    assert at == len(raw)
    g.close()
