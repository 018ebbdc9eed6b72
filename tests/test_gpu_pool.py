"""GPU: max pooling over a handle's rows with its arg-max and both reverse steps (athena_amd/csrc/pool.hip) against the transcription
of the definition (tests/pool_reference.py).  The two-set handles are those of tests/test_gpu_interp.py -- 300 queries and 200
sources in three clouds, the middle one without sources, so its rows are empty: k = 1, 3, 64, and a radius handle with a hub row
of 150 entries beside empty rows (more rounds than a lane group is wide, and lanes past a row's end) --, and one square handle from
DeviceGraph.from_points_knn for the vertex forms.  Two kinds of features: standard normal with -0.0 planted, and small integers in
-2 .. 2 with signed zeros, infinities and NaNs planted, so that the tie rule decides most rows.  Every comparison is word for word,
values and arg alike; every output is pre-filled with NaN or a poison integer, so an element that was not written shows.

The integers are drawn with weights that favour the top value.  Drawn uniformly, three entries over five values attain their
maximum more than once in only 1 - 3 (0 + 1 + 4 + 9 + 16) / 125 = 28 % of the rows; with the weights below the top value alone
ties in 3 p^2 (1 - p) + p^3 = 97 % of them (p = 0.9), less the rows whose maximum is a single planted NaN or infinity.  Every
third feature column holds only -1, -0 and +0, so that zeros of both signs win rows and the first one must stay.  A row with one
entry cannot tie: knn1 has no other rows, and of the hub handle's 65 non-empty rows 20 hold one entry and 6 two, which caps its
share near one half whatever the values.  So the share -- more than half of the (i, f) attain their maximum more than once -- is
asserted over the rows that hold three entries or more: all non-empty rows of knn3 and knn64, 39 rows of the hub handle."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import fps_reference as fr
import knn_bipartite_reference as kb
import pool_reference as pr
import test_gpu_interp as ti

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "pool_run")
ALL_F = (1, 3, 4, 7, 64, 66, 128, 256, 260)        # both load routes, every group width (4 .. 64), two passes beyond 256 columns
CASES = ("knn1", "knn3", "knn64", "hub")
KINDS = ("normal", "ties")
VALUES, WEIGHTS = (-2.0, -1.0, 0.0, 1.0, 2.0), (0.02, 0.02, 0.02, 0.04, 0.9)
POISON = 0x5A5A5A5A

vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
bits = lambda a: np.ascontiguousarray(a).view(np.int32)
points, yardstick, handle, up = ti.points, ti.yardstick, ti.handle, ti.up


def _rng(seed):
    return np.random.default_rng(seed)


def draw(rng, kind, shape):
    """float32 values of one kind"""
    if kind == "normal":
        a = rng.standard_normal(shape).astype(np.float32)
        a[rng.random(shape) < 0.02] = -0.0
        return a
    a = rng.choice(np.array(VALUES, np.float32), shape, p=WEIGHTS)
    a[(a == 0) & (rng.random(shape) < 0.5)] = -0.0
    u = rng.random(shape)
    a[u < 0.02], a[(u >= 0.02) & (u < 0.04)], a[(u >= 0.04) & (u < 0.06)] = np.nan, np.inf, -np.inf
    zeros = rng.choice(np.array([-1.0, -0.0, 0.0], np.float32), shape, p=(0.2, 0.4, 0.4))
    a[:, 2::3] = zeros[:, 2::3]                               # every third column: the maximum is a zero, of either sign
    return a


@functools.lru_cache(None)
def features(name, kind, F, n_cols=200, n_rows=300):
    """x [n_cols, F], h [E, F], dy [n_rows, F]; dy without zeros but for a planted -0.0 per fifth row"""
    E = yardstick(name)[0].size if name in CASES else 0
    rng = _rng(8100 + 97 * (CASES + ("square",)).index(name) + 7 * KINDS.index(kind) + F)
    x, h = draw(rng, kind, (n_cols, F)), draw(rng, kind, (E, F))
    dy = rng.standard_normal((n_rows, F)).astype(np.float32)
    dy[::5, F - 1] = -0.0
    return x, h, dy


@functools.lru_cache(None)
def reference(name, kind, F):
    """the yardstick's results, computed once per case"""
    A = yardstick(name)[3]
    x, h, dy = features(name, kind, F)
    yx, ax = pr.fwd(A, x)
    yh, ah = pr.edges_fwd(A, h)
    return {"yx": yx, "ax": ax, "yh": yh, "ah": ah, "dx": pr.bwd_x(A, ax, dy), "dh": pr.bwd_edges(A, ah, dy, h.shape[0])}


def device_fwd(entry, g, values, dev, want_arg=True):
    import torch
    from athena_amd import _capi

    F = int(values.shape[1])
    y = torch.full((g.n_rows, F), np.nan, dtype=torch.float32, device=dev)
    arg = torch.full((g.n_rows, F), POISON, dtype=torch.int32, device=dev) if want_arg else None
    _capi.use_torch_stream()
    _capi.call(entry, g.handle, F, ptr(values), ptr(y), ptr(arg))
    return y, arg


def device_bwd(entry, g, arg, dy, rows, dev):
    import torch
    from athena_amd import _capi

    out = torch.full((rows, dy.shape[1]), np.nan, dtype=torch.float32, device=dev)
    _capi.use_torch_stream()
    _capi.call(entry, g.handle, int(dy.shape[1]), ptr(arg), ptr(dy), ptr(out))
    return out


def same(t, want):
    return np.array_equal(bits(t.cpu().numpy()), bits(want))


def inputs_are_what_the_test_needs(name, F, kind):
    """on the yardstick alone (tests/test_pool.py runs this on the CPU for every case): empty rows, the hub row, and for the integer
    features the share of rows that the tie rule decides and the special values among the results"""
    A = yardstick(name)[3]
    x, h, dy = features(name, kind, F)
    want = reference(name, kind, F)
    lens = np.diff(A["rowptr"])
    assert (lens == 0).any(), "an empty slice gives empty rows"
    if name == "hub":
        assert lens[0] > 64 and lens[0] % 8 != 0
    if kind != "ties":
        return
    for values, source, y in ((x, A["col"], want["yx"]), (h, A["eid"], want["yh"])):
        if name != "knn1":
            share = pr.attained_more_than_once(A, values, source, y)[lens >= 3].mean()
            assert share > 0.5, f"the tie rule decides only {share:.2f} of the rows of three entries and more"
        got = y[lens > 0]
        assert np.isnan(got).any()
        if F >= 3:
            assert np.isinf(got).any()
            zero = bits(got) << 1 == 0
            assert (bits(got)[zero] < 0).any() and (bits(got)[zero] == 0).any(), "both zeros must win rows"


# ---- the four entries against the yardstick ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", ALL_F)
@pytest.mark.parametrize("name", CASES)
def test_all_four_entries_equal_the_yardstick(dev, name, F, kind):
    g, _ = handle(name)
    x, h, dy = features(name, kind, F)
    want = reference(name, kind, F)
    inputs_are_what_the_test_needs(name, F, kind)
    xd, hd, dyd = up(x, dev), up(h, dev), up(dy, dev)
    yx, ax = device_fwd("athena_mp_pool_max_fwd", g, xd, dev)
    yh, ah = device_fwd("athena_mp_pool_max_edges_fwd", g, hd, dev)
    assert same(yx, want["yx"]) and same(ax, want["ax"])
    assert same(yh, want["yh"]) and same(ah, want["ah"])
    dx = device_bwd("athena_mp_pool_max_bwd_x", g, up(want["ax"], dev), dyd, g.n_cols, dev)
    dh = device_bwd("athena_mp_pool_max_bwd_edges", g, up(want["ah"], dev), dyd, g.n_edge_cols, dev)
    assert same(dx, want["dx"]) and same(dh, want["dh"])
    assert same(xd, x) and same(hd, h) and same(dyd, dy), "an input changed"


@pytest.mark.parametrize("F", ALL_F)
@pytest.mark.parametrize("name", ["knn3", "hub"])
def test_without_arg_the_same_y_and_two_runs_the_same_bytes(dev, name, F):
    g, _ = handle(name)
    x, h, dy = features(name, "ties", F)
    want = reference(name, "ties", F)
    xd, hd, dyd, axd, ahd = (up(a, dev) for a in (x, h, dy, want["ax"], want["ah"]))
    for entry, values, y_want in (("athena_mp_pool_max_fwd", xd, want["yx"]), ("athena_mp_pool_max_edges_fwd", hd, want["yh"])):
        only_y, none = device_fwd(entry, g, values, dev, want_arg=False)
        assert none is None and same(only_y, y_want)
        first, second = device_fwd(entry, g, values, dev), device_fwd(entry, g, values, dev)
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(first, second))
    for entry, arg, rows in (("athena_mp_pool_max_bwd_x", axd, g.n_cols), ("athena_mp_pool_max_bwd_edges", ahd, g.n_edge_cols)):
        first, second = device_bwd(entry, g, arg, dyd, rows, dev), device_bwd(entry, g, arg, dyd, rows, dev)
        assert first.cpu().numpy().tobytes() == second.cpu().numpy().tobytes()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,F", [(n, F) for n in ("knn3", "knn64", "hub") for F in (3, 64, 260)])
def test_the_edge_form_on_gathered_rows_is_the_vertex_form(dev, name, F, kind):
    g, _ = handle(name)
    A = yardstick(name)[3]
    x = features(name, kind, F)[0]
    entry_of_edge = np.empty(A["col"].size, np.int64)
    entry_of_edge[A["eid"]] = np.arange(A["col"].size)
    yx, ax = device_fwd("athena_mp_pool_max_fwd", g, up(x, dev), dev)
    yh, ah = device_fwd("athena_mp_pool_max_edges_fwd", g, up(x[A["col"][entry_of_edge]], dev), dev)
    assert same(yh, yx.cpu().numpy()) and same(ah, ax.cpu().numpy())


# ---- a square handle: the vertex forms ---------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def square():
    """(handle, its six arrays): 301 points, k = 8, either end's choice keeps a pair; both directions of a pair share its edge column"""
    from athena_amd import DeviceGraph

    g, _ = DeviceGraph.from_points_knn(_rng(8200).random((301, 3)).astype(np.float32), 8, mode="union")
    A = {key: g.export(key) for key in ("rowptr", "col", "eid", "t_rowptr", "t_src", "t_eid")}
    assert g.n_rows == g.n_cols == 301 and g.nnz == 2 * g.n_edge_cols and np.diff(A["rowptr"]).min() >= 8
    for r in range(301):
        row = A["col"][A["rowptr"][r]:A["rowptr"][r + 1]]
        assert np.unique(row).size == row.size, "a row holds a column twice"
        assert (np.diff(A["t_src"][A["t_rowptr"][r]:A["t_rowptr"][r + 1]]) > 0).all(), "a column's rows do not ascend"
    return g, A


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", ALL_F)
def test_the_vertex_forms_on_a_square_handle(dev, F, kind):
    g, A = square()
    x, _, dy = features("square", kind, F, 301, 301)
    want_y, want_arg = pr.fwd(A, x)
    want_dx = pr.bwd_x(A, want_arg, dy)
    if kind == "ties":
        assert pr.attained_more_than_once(A, x, A["col"], want_y).mean() > 0.5
    y, arg = device_fwd("athena_mp_pool_max_fwd", g, up(x, dev), dev)
    assert same(y, want_y) and same(arg, want_arg)
    dx = device_bwd("athena_mp_pool_max_bwd_x", g, arg, up(dy, dev), 301, dev)
    assert same(dx, want_dx)


# ---- refusals, empty sets ----------------------------------------------------------------------------------------------------------
def test_refusals_arrive_with_their_messages_and_the_library_goes_on(dev):
    import torch
    from athena_amd import DeviceGraph, _capi
    from athena_amd._capi import AthenaMPError
    from helpers import random_graph

    g, _ = handle("knn3")
    x, h, dy = features("knn3", "normal", 4)
    want = reference("knn3", "normal", 4)
    xd, hd, dyd = up(x, dev), up(h, dev), up(dy, dev)
    y = torch.empty((300, 4), device=dev)
    arg = torch.empty((300, 4), dtype=torch.int32, device=dev)
    ia, ja = random_graph(20, 40, 1, self_loops=True)
    kipf = DeviceGraph(ia, ja, n_edge_cols=0)
    for entry, a, b, c in (("athena_mp_pool_max_edges_fwd", hd, y, arg), ("athena_mp_pool_max_bwd_edges", arg, dyd, hd)):
        with pytest.raises(AthenaMPError, match=entry[10:] + r": the handle has no edge columns"):
            _capi.call(entry, kipf.handle, 4, ptr(a), ptr(b), ptr(c))
    sq, _ = square()
    for entry, a, b, c in (("athena_mp_pool_max_edges_fwd", hd, y, arg), ("athena_mp_pool_max_bwd_edges", arg, dyd, hd)):
        with pytest.raises(AthenaMPError, match=entry[10:] + r": \d+ entries over \d+ edge columns: need one entry per edge column"):
            _capi.call(entry, sq.handle, 4, ptr(a), ptr(b), ptr(c))
    loops = DeviceGraph(ia, ja)                              # self-loop entries carry no edge id
    with pytest.raises(AthenaMPError, match=r"pool_max_edges_fwd: \d+ of the handle's \d+ entries carry no edge id"):
        _capi.call("athena_mp_pool_max_edges_fwd", loops.handle, 4, ptr(hd), ptr(y), ptr(arg))
    for entry, a, b, c in (("athena_mp_pool_max_fwd", xd, y, arg), ("athena_mp_pool_max_edges_fwd", hd, y, arg),
                           ("athena_mp_pool_max_bwd_x", arg, dyd, xd), ("athena_mp_pool_max_bwd_edges", arg, dyd, hd)):
        with pytest.raises(AthenaMPError, match=entry[10:] + r": F = 0: need at least one feature column"):
            _capi.call(entry, g.handle, 0, ptr(a), ptr(b), ptr(c))
    with pytest.raises(AthenaMPError, match=r"pool_max_host: F = -1"):
        _capi.call("athena_mp_pool_max_host", g.handle, -1, vp(x), None, None, None)
    with pytest.raises(AthenaMPError, match=r"pool_max_host: exactly one of x"):
        _capi.call("athena_mp_pool_max_host", g.handle, 4, vp(x), vp(h), None, None)
    with pytest.raises(AthenaMPError, match=r"pool_max_bwd_host: dx and dh are both null"):
        _capi.call("athena_mp_pool_max_bwd_host", g.handle, 4, vp(want["ax"]), vp(dy), None, None)
    with pytest.raises(AthenaMPError, match=r"pool_max_fwd: null array"):
        _capi.call("athena_mp_pool_max_fwd", g.handle, 4, None, ptr(y), ptr(arg))
    yx, ax = device_fwd("athena_mp_pool_max_fwd", g, xd, dev)                   # and the next call works
    assert same(yx, want["yx"]) and same(ax, want["ax"])
    yk, ak = device_fwd("athena_mp_pool_max_fwd", kipf, up(_rng(8300).random((20, 4)).astype(np.float32), dev), dev)
    assert not torch.isnan(yk).any() and int(ak.min()) >= 0 and int(ak.max()) < 20      # a handle without edge ids is taken
    kipf.close(); loops.close()


def test_empty_sets_succeed(dev):
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.geometry import pool_max, pool_max_grad

    some, none = _rng(8400).random((5, 2)).astype(np.float32), np.zeros((0, 2), np.float32)
    for q, s in ((some, none), (none, some), (none, none)):
        g, _, _ = DeviceGraph.from_point_sets(q, s, 1.0)
        nq, ns = q.shape[0], s.shape[0]
        assert g.n_edge_cols == 0
        for kw in ({"x": torch.ones((ns, 3), device=dev)}, {"edges": torch.ones((0, 3), device=dev)}):
            y, arg = pool_max(g, out=(torch.full((nq, 3), np.nan, device=dev), torch.full((nq, 3), POISON, dtype=torch.int32, device=dev)), **kw)
            assert tuple(y.shape) == (nq, 3) and not bits(y.cpu().numpy()).any() and (arg.cpu().numpy() == -1).all()
            to = "x" if "x" in kw else "edges"
            back = pool_max_grad(g, arg, torch.ones((nq, 3), device=dev), to=to,
                                 out=torch.full((ns if to == "x" else 0, 3), np.nan, device=dev))
            assert tuple(back.shape) == ((ns, 3) if to == "x" else (0, 3)) and not bits(back.cpu().numpy()).any()
        g.close()


# ---- the Python chain, host forms, Fortran -------------------------------------------------------------------------------------------
def test_the_set_abstraction_chain_equals_the_yardstick_chain(dev):
    """farthest_points -> from_point_sets_knn(coarse, points, k) -> pool_max(edges=...) -> pool_max_grad(to="edges"), and the same
    over per-vertex values"""
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.geometry import farthest_points, pool_max, pool_max_grad

    rng = _rng(8500)
    offsets = kb.offsets_of([90, 60])
    pts = rng.random((150, 3)).astype(np.float32)
    k, F = 6, 7
    sample, coarse, soff, _ = farthest_points(pts, offsets, ratio=0.2)
    want_sample, want_coarse, _, _ = fr.brute_force(pts, soff, offsets)
    assert np.array_equal(sample.cpu().numpy(), want_sample) and same(coarse, want_coarse)
    g, _, _ = DeviceGraph.from_point_sets_knn(coarse, pts, k, query_offsets=soff, source_offsets=offsets)
    nbr, _ = kb.brute_force(want_coarse, pts, k, None, soff, offsets)
    i, j, _, _, _ = kb.graph_of(nbr, want_coarse, pts, soff)
    nc, E = int(soff[-1]), i.size
    A = pr.arrays_of(i, j, nc, 150)
    assert g.n_rows == nc == 30 and g.n_edge_cols == E == nc * k
    for key, arr in A.items():
        assert np.array_equal(g.export(key), arr)
    h, x, dy = draw(rng, "ties", (E, F)), draw(rng, "ties", (150, F)), rng.standard_normal((nc, F)).astype(np.float32)
    y, arg = pool_max(g, edges=up(h, dev))
    dh = pool_max_grad(g, arg, up(dy, dev), to="edges")
    want_y, want_arg = pr.edges_fwd(A, h)
    assert same(y, want_y) and same(arg, want_arg) and same(dh, pr.bwd_edges(A, want_arg, dy, E))
    yx, ax = pool_max(g, x=up(x, dev))
    dx = pool_max_grad(g, ax, up(dy, dev), to="x")
    want_yx, want_ax = pr.fwd(A, x)
    assert same(yx, want_yx) and same(ax, want_ax) and same(dx, pr.bwd_x(A, want_ax, dy))
    only_y, no_arg = pool_max(g, x=up(x, dev), want_arg=False)
    assert no_arg is None and same(only_y, want_yx)
    with pytest.raises(ValueError, match="exactly one of x and edges"):
        pool_max(g, x=up(x, dev), edges=up(h, dev))
    with pytest.raises(ValueError, match="exactly one of x and edges"):
        pool_max(g)
    with pytest.raises(ValueError, match="edges must be a contiguous float32 device tensor"):
        pool_max(g, edges=up(x, dev))
    with pytest.raises(ValueError, match="arg must be a contiguous int32 device tensor"):
        pool_max_grad(g, y, up(dy, dev))
    with pytest.raises(ValueError, match='to must be "x" or "edges"'):
        pool_max_grad(g, arg, up(dy, dev), to="coords")
    g.close()


@pytest.mark.parametrize("name,F", [("knn3", 7), ("hub", 64)])
def test_host_forms_give_the_device_entries_bytes(dev, name, F):
    from athena_amd import _capi

    g, _ = handle(name)
    x, h, dy = features(name, "ties", F)
    want = reference(name, "ties", F)
    E = g.n_edge_cols
    for values, y_want, a_want in ((x, want["yx"], want["ax"]), (h, want["yh"], want["ah"])):
        hy, ha = np.full((300, F), np.nan, np.float32), np.full((300, F), POISON, np.int32)
        first, second = (vp(values), None) if values is x else (None, vp(values))
        _capi.call("athena_mp_pool_max_host", g.handle, F, first, second, vp(hy), vp(ha))
        assert hy.tobytes() == y_want.tobytes() and ha.tobytes() == a_want.tobytes()
        hy2 = np.full((300, F), np.nan, np.float32)
        _capi.call("athena_mp_pool_max_host", g.handle, F, first, second, vp(hy2), None)
        assert hy2.tobytes() == y_want.tobytes()
    hdx, hdh = np.full((200, F), np.nan, np.float32), np.full((E, F), np.nan, np.float32)
    _capi.call("athena_mp_pool_max_bwd_host", g.handle, F, vp(want["ax"]), vp(dy), vp(hdx), None)
    _capi.call("athena_mp_pool_max_bwd_host", g.handle, F, vp(want["ah"]), vp(dy), None, vp(hdh))
    assert hdx.tobytes() == want["dx"].tobytes() and hdh.tobytes() == want["dh"].tobytes()
    both_x, both_h = np.full((200, F), np.nan, np.float32), np.full((E, F), np.nan, np.float32)
    _capi.call("athena_mp_pool_max_bwd_host", g.handle, F, vp(want["ah"]), vp(dy), vp(both_x), vp(both_h))
    A = yardstick(name)[3]
    assert both_h.tobytes() == want["dh"].tobytes() and both_x.tobytes() == pr.bwd_x(A, want["ah"], dy).tobytes()


def test_fortran_program_writes_the_device_entries_bytes(dev, tmp_path):
    if not os.path.exists(RUNNER):
        pytest.fail("pool_run is not built: __graft_entry__.build() compiles the Fortran host side")
    from athena_amd import DeviceGraph
    from athena_amd.geometry import pool_max, pool_max_grad

    rng = _rng(8600)
    nq, ns, k, F = 40, 90, 3, 6
    q, s = rng.random((nq, 3)).astype(np.float32), rng.random((ns, 3)).astype(np.float32)
    x, h, dy = draw(rng, "ties", (ns, F)), draw(rng, "ties", (nq * k, F)), rng.standard_normal((nq, F)).astype(np.float32)
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        np.array([nq, ns, 3, k, F], np.int32).tofile(f)
        np.array([np.inf], np.float32).tofile(f)
        q.tofile(f); s.tofile(f); x.tofile(f); h.tofile(f); dy.tofile(f)
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"pool_run failed ({out.returncode}): {out.stdout[-1000:]} {out.stderr[-2000:]}"
    g, _, _ = DeviceGraph.from_point_sets_knn(q, s, k)
    E = g.n_edge_cols
    assert E == nq * k
    yx, ax = pool_max(g, x=up(x, dev))
    yh, ah = pool_max(g, edges=up(h, dev))
    dx, dh = pool_max_grad(g, ax, up(dy, dev), to="x"), pool_max_grad(g, ah, up(dy, dev), to="edges")
    raw = open(res, "rb").read()
    assert np.frombuffer(raw, np.int64, 1)[0] == E
    at = 8
    for what, t in (("y_x", yx), ("arg_x", ax), ("y_h", yh), ("arg_h", ah), ("dx", dx), ("dh", dh)):
        a = t.cpu().numpy()
        assert raw[at:at + a.nbytes] == a.tobytes(), what
        at += a.nbytes
    assert at == len(raw)
    g.close()
