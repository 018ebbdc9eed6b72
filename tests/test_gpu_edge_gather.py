"""GPU: the gather that makes the edge MLP's input over a two-set handle, and its reverse (athena_amd/csrc/edge_gather.hip), against
the transcription of the definition (tests/edge_gather_reference.py).  The handles are those of tests/test_gpu_interp.py -- 300
queries and 200 sources in three clouds, the middle one without sources, so its rows are empty: k = 1, 3, 64, and a radius handle
with a hub row of 150 entries beside empty rows.  The widths (Fs, Fq, dim, relative) cover every group width (4 .. 64, sized from
max(Fs, Fq)), both load routes, a second pass beyond 256 columns and every block absent in turn; each runs at the pitch ld = W and
at the next multiple of 4 strictly above W, where h's pad columns hold a poison word that must survive and dh's hold NaN, so that
a read of them poisons a sum.  Outputs are pre-filled with a NaN no computation makes.  Every comparison is word for word.

Copied blocks are standard normal with -0, +-inf, NaNs with a payload and a signalling NaN planted; with relative, xs and xq are
finite with subnormals and zeros of both signs planted (some differences are -0, some subnormal), coords keeps the specials."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bipartite_reference as br
import edge_gather_reference as er
import fps_reference as fr
import knn_bipartite_reference as kb
import pool_reference as pr
import test_gpu_interp as ti

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "edge_gather_run")
CASES = ("knn1", "knn3", "knn64", "hub")
WIDTHS = ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 3, 0), (3, 0, 3, 0), (4, 4, 0, 1), (64, 0, 3, 0), (64, 64, 3, 0), (64, 64, 3, 1),
          (66, 7, 2, 0), (128, 128, 3, 1), (260, 0, 1, 0), (256, 256, 4, 1))
POISON = 0x5A5A5A5A                                 # h's pad columns, as a word (a finite float)
UNWRITTEN = 0x7FC0ABCD                              # the pre-fill of every output: a quiet NaN with a payload nothing here makes
MINUS_ZERO, SNAN, QNAN, NEG_NAN = -0x80000000, 0x7F800001, 0x7FC12345, -0x3FF889                # NEG_NAN = 0xFFC00777
SPECIALS = (MINUS_ZERO, 0x7F800000, -0x800000, QNAN, SNAN, NEG_NAN)                             # -0, +inf, -inf, three NaNs

vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
bits = lambda a: np.ascontiguousarray(a).view(np.int32)
points, yardstick, handle, up = ti.points, ti.yardstick, ti.handle, ti.up


def _rng(seed):
    return np.random.default_rng(seed)


def ld_of(W, padded):
    """the pitch: W, or the next multiple of 4 strictly above W"""
    return 4 * (W // 4 + 1) if padded else W


def draw_copy(rng, shape):
    """standard normal float32 with the special words planted, each several times from 200 elements on"""
    a = rng.standard_normal(shape).astype(np.float32)
    flat = a.reshape(-1).view(np.int32)
    for s, word in enumerate(SPECIALS):
        flat[7 + s::53] = word
    return a


def draw_finite(rng, shape, zero):
    """finite float32 for the operands of the difference: column 0 holds `zero` in every second row and the other zero in rows
    1, 5, 9, ..; the last column holds subnormals of both signs in every second row"""
    a = rng.standard_normal(shape).astype(np.float32)
    a[::2, 0], a[1::4, 0] = zero, -zero
    n = a[::2].shape[0]
    sub = rng.integers(1, 1 << 23, n).astype(np.int32) | (rng.integers(0, 2, n).astype(np.int32) << 31)
    a[::2, -1] = sub.view(np.float32)
    return a


@functools.lru_cache(2)
def features(name, widths):
    """(xs, xq, coords): a block of width 0 is None"""
    Fs, Fq, dim, rel = widths
    E = yardstick(name)[0].size
    rng = _rng(9300 + 131 * CASES.index(name) + WIDTHS.index(widths))
    if rel:
        xs, xq = draw_finite(rng, (200, Fs), np.float32(-0.0)), draw_finite(rng, (300, Fq), np.float32(0.0))
    else:
        xs = draw_copy(rng, (200, Fs)) if Fs else None
        xq = draw_copy(rng, (300, Fq)) if Fq else None
    return xs, xq, draw_copy(rng, (E, dim)) if dim else None


def prefilled(E, W, ld, word=UNWRITTEN):
    """h as it is before the call: `word` in the defined columns, the poison word beyond"""
    h = np.full((E, ld), word, np.int32)
    h[:, W:] = POISON
    return h.view(np.float32)


@functools.lru_cache(2)
def reference(name, widths, padded):
    """(h [E, ld] as it must be after the call, dh [E, ld], dxs, dxq, dcoords), computed once per case"""
    Fs, Fq, dim, rel = widths
    A = yardstick(name)[3]
    xs, xq, coords = features(name, widths)
    E, W = A["col"].size, Fs + Fq + dim
    ld = ld_of(W, padded)
    h = er.fwd(A, xs, xq, coords, rel, prefilled(E, W, ld))
    dh = _rng(9400 + 131 * CASES.index(name) + WIDTHS.index(widths)).standard_normal((E, ld)).astype(np.float32)
    dh[:, W:] = np.nan
    return (h, dh) + er.bwd(A, dh, (Fs, Fq, dim), rel)


def device_fwd(g, widths, ld, xs, xq, coords, h):
    """xs, xq, coords, h: device tensors (None for a block of width 0); h [E, ld] is written in place"""
    from athena_amd import _capi

    Fs, Fq, dim, rel = widths
    _capi.use_torch_stream()
    _capi.call("athena_mp_edge_gather_fwd", g.handle, Fs, ptr(xs), Fq, ptr(xq), dim, ptr(coords), rel, ld, ptr(h))
    return h


def device_bwd(g, widths, ld, dh, dev, want=(True, True, True)):
    """(dxs, dxq, dcoords), pre-filled; None where the width is 0 or the output is not wanted"""
    import torch
    from athena_amd import _capi

    Fs, Fq, dim, rel = widths
    shapes = ((g.n_cols, Fs), (g.n_rows, Fq), (g.n_edge_cols, dim))
    outs = [torch.full(s, UNWRITTEN, dtype=torch.int32, device=dev).view(torch.float32) if s[1] and w else None for s, w in zip(shapes, want)]
    _capi.use_torch_stream()
    _capi.call("athena_mp_edge_gather_bwd", g.handle, Fs, Fq, dim, rel, ld, ptr(dh), *(ptr(t) for t in outs))
    return outs


def same(t, want):
    return np.array_equal(bits(t.cpu().numpy()), bits(want))


def inputs_are_what_the_test_needs(name, widths, padded):
    """on the yardstick alone (tests/test_edge_gather.py runs this on the CPU for every case): empty rows, the hub row, the special
    words among the copies, and in relative cases a -0 and a subnormal among the differences"""
    Fs, Fq, dim, rel = widths
    A = yardstick(name)[3]
    h, dh, dxs, dxq, dc = reference(name, widths, padded)
    W = Fs + Fq + dim
    lens = np.diff(A["rowptr"])
    assert (lens == 0).any(), "an empty slice gives empty rows"
    if name in ("knn1", "hub"):
        assert (np.diff(A["t_rowptr"]) == 0).any(), "every source has a query: no empty column"
    if name == "hub":
        assert lens[0] > 64 and lens[0] % 8 != 0
    words = bits(h)
    assert not (words[:, :W] == UNWRITTEN).any() and (words[:, W:] == POISON).all() and (h.shape[1] > W) == bool(padded)
    copied = words[:, Fs + Fq if rel else 0:W]                  # the blocks that draw_copy made
    if copied.size:
        for word in SPECIALS:
            assert (copied == word).any(), f"the special word {word & 0xFFFFFFFF:#x} is not among the copies"
    if rel:
        diff = words[:, :Fs]
        assert (diff == MINUS_ZERO).any(), "no difference is -0"
        mag = diff & 0x7FFFFFFF
        assert ((mag > 0) & (mag < 0x00800000)).any(), "no difference is subnormal"
        assert np.isfinite(h[:, :Fs]).all()
    for out in (dxs, dxq, dc):
        assert np.isfinite(out).all(), "a pad column of dh went into a result"


# ---- both entries against the yardstick --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [0, 1])
@pytest.mark.parametrize("widths", WIDTHS)
@pytest.mark.parametrize("name", CASES)
def test_both_entries_equal_the_yardstick(dev, name, widths, padded):
    g, _ = handle(name)
    Fs, Fq, dim, rel = widths
    E, W = g.n_edge_cols, Fs + Fq + dim
    ld = ld_of(W, padded)
    inputs_are_what_the_test_needs(name, widths, padded)
    xs, xq, coords = features(name, widths)
    want_h, dh, want_dxs, want_dxq, want_dc = reference(name, widths, padded)
    ins = [up(a, dev) if a is not None else None for a in (xs, xq, coords)]
    h = device_fwd(g, widths, ld, *ins, up(prefilled(E, W, ld), dev))
    assert same(h, want_h), "h: a defined word differs, was not written, or a pad word changed"
    dhd = up(dh, dev)
    dxs, dxq, dc = device_bwd(g, widths, ld, dhd, dev)
    for got, want, width in ((dxs, want_dxs, Fs), (dxq, want_dxq, Fq), (dc, want_dc, dim)):
        assert (got is None) == (width == 0) and (got is None or same(got, want))
    for t, a in zip(ins + [dhd], (xs, xq, coords, dh)):
        assert t is None or same(t, a), "an input changed"


@pytest.mark.parametrize("widths", [(64, 64, 3, 1), (66, 7, 2, 0), (256, 256, 4, 1)])
@pytest.mark.parametrize("name", ["knn3", "hub"])
def test_two_runs_the_same_bytes_and_one_output_alone(dev, name, widths):
    g, _ = handle(name)
    Fs, Fq, dim, rel = widths
    E, W = g.n_edge_cols, Fs + Fq + dim
    ld = ld_of(W, 1)
    xs, xq, coords = features(name, widths)
    want_h, dh, want_dxs, want_dxq, want_dc = reference(name, widths, 1)
    ins = [up(a, dev) for a in (xs, xq, coords)]
    first = device_fwd(g, widths, ld, *ins, up(prefilled(E, W, ld), dev))
    second = device_fwd(g, widths, ld, *ins, up(prefilled(E, W, ld), dev))
    assert first.cpu().numpy().tobytes() == second.cpu().numpy().tobytes()
    dhd = up(dh, dev)
    a, b = device_bwd(g, widths, ld, dhd, dev), device_bwd(g, widths, ld, dhd, dev)
    assert all(s.cpu().numpy().tobytes() == t.cpu().numpy().tobytes() for s, t in zip(a, b))
    for n, want in enumerate((want_dxs, want_dxq, want_dc)):
        only = device_bwd(g, widths, ld, dhd, dev, want=tuple(m == n for m in range(3)))
        assert [t is not None for t in only] == [m == n for m in range(3)] and same(only[n], want)


@pytest.mark.parametrize("padded", [0, 1])
@pytest.mark.parametrize("name", ["knn3", "hub"])
def test_relative_with_infinities_and_nans_gives_nans_where_the_definition_does(dev, name, padded):
    """inf and NaN among the operands of the difference: a NaN result's payload is open, so the NaN masks are equal and the other
    words are; the pre-fill is the finite poison word here, so that an element that was not written is not taken for a NaN"""
    widths = (64, 64, 3, 1)
    g, _ = handle(name)
    A = yardstick(name)[3]
    E, W, ld = g.n_edge_cols, 131, ld_of(131, padded)
    rng = _rng(9500 + CASES.index(name))
    xs, xq, coords = draw_copy(rng, (200, 64)), draw_copy(rng, (300, 64)), draw_copy(rng, (E, 3))
    want = er.fwd(A, xs, xq, coords, 1, prefilled(E, W, ld, POISON))
    h = device_fwd(g, widths, ld, up(xs, dev), up(xq, dev), up(coords, dev), up(prefilled(E, W, ld, POISON), dev)).cpu().numpy()
    nan = np.isnan(want)
    assert nan[:, :64].any() and np.isinf(want[:, :64]).any(), "the case holds no NaN or no infinite difference"
    assert np.array_equal(np.isnan(h), nan) and np.array_equal(bits(h)[~nan], bits(want)[~nan])
    assert np.array_equal(bits(h)[:, 64:], bits(want)[:, 64:]), "the copied blocks keep every bit, NaNs included"


# ---- refusals, empty sets ----------------------------------------------------------------------------------------------------------
def test_refusals_arrive_with_their_messages_and_the_library_goes_on(dev):
    import torch
    from athena_amd import DeviceGraph, _capi
    from athena_amd._capi import AthenaMPError
    from helpers import random_graph

    g, _ = handle("knn3")
    E = g.n_edge_cols
    t = lambda rows, cols: torch.zeros((rows, cols), device=dev)
    xs, xq, co, h, out = t(200, 4), t(300, 4), t(E, 3), t(E, 16), t(300, 4)
    fwd = lambda gr, Fs, a, Fq, b, dim, c, rel, ld, o: _capi.call("athena_mp_edge_gather_fwd", gr.handle, Fs, ptr(a), Fq, ptr(b), dim,
                                                                   ptr(c), rel, ld, ptr(o))
    bwd = lambda gr, Fs, Fq, dim, rel, ld: _capi.call("athena_mp_edge_gather_bwd", gr.handle, Fs, Fq, dim, rel, ld, ptr(h), ptr(xs),
                                                       ptr(out), ptr(co))
    for who, call in (("edge_gather_fwd", lambda *w: fwd(g, w[0], xs, w[1], xq, w[2], co, w[3], w[4], h)),
                      ("edge_gather_bwd", lambda *w: bwd(g, *w))):
        for w, message in (((4, 4, 3, 0, 10), r"ld = 10 is less than Fs \+ Fq \+ dim = 11"),
                           ((4, 3, 3, 1, 16), r"relative needs Fs == Fq: Fs = 4, Fq = 3"),
                           ((0, 0, 3, 1, 16), r"relative needs a source block: Fs = 0"),
                           ((0, 0, 0, 0, 16), r"Fs \+ Fq \+ dim = 0: need at least one column"),
                           ((4, -1, 3, 0, 16), r"Fs = 4, Fq = -1, dim = 3: a negative width"),
                           ((4, 4, 3, 2, 16), r"relative = 2 is neither 0 nor 1")):
            with pytest.raises(AthenaMPError, match=who + ": " + message):
                call(*w)
    for a, b, c, o, message in ((None, xq, co, h, "xs is null and Fs = 4"), (xs, None, co, h, "xq is null and Fq = 4"),
                                (xs, xq, None, h, "coords is null and dim = 3"), (xs, xq, co, None, "h is null")):
        with pytest.raises(AthenaMPError, match="edge_gather_fwd: " + message):
            fwd(g, 4, a, 4, b, 3, c, 0, 16, o)
    with pytest.raises(AthenaMPError, match="edge_gather_bwd: dh is null"):
        _capi.call("athena_mp_edge_gather_bwd", g.handle, 4, 4, 3, 0, 16, None, ptr(xs), ptr(out), ptr(co))
    ia, ja = random_graph(20, 40, 1, self_loops=True)
    kipf, loops = DeviceGraph(ia, ja, n_edge_cols=0), DeviceGraph(ia, ja)
    sq, _ = DeviceGraph.from_points_knn(_rng(9600).random((301, 3)).astype(np.float32), 8, mode="union")
    for gr, message in ((kipf, "the handle has no edge columns"), (loops, r"\d+ of the handle's \d+ entries carry no edge id"),
                        (sq, r"\d+ entries over \d+ edge columns: need one entry per edge column")):
        with pytest.raises(AthenaMPError, match="edge_gather_fwd: " + message):
            fwd(gr, 4, xs, 4, xq, 3, co, 0, 16, h)
        with pytest.raises(AthenaMPError, match="edge_gather_bwd: " + message):
            bwd(gr, 4, 4, 3, 0, 16)
    with pytest.raises(AthenaMPError, match="edge_gather_host: ld = 10 is less than"):
        _capi.call("athena_mp_edge_gather_host", g.handle, 4, None, 4, None, 3, None, 0, 10, None)
    with pytest.raises(AthenaMPError, match="edge_gather_bwd_host: dxs, dxq and dcoords are all null"):
        _capi.call("athena_mp_edge_gather_bwd_host", g.handle, 4, 4, 3, 0, 16, None, None, None, None)
    widths = (4, 4, 0, 1)                                      # and the next call works
    want = reference("knn3", widths, 0)[0]
    ins = [up(a, dev) if a is not None else None for a in features("knn3", widths)]
    assert same(device_fwd(g, widths, 8, *ins, up(prefilled(E, 8, 8), dev)), want)
    kipf.close(); loops.close(); sq.close()


def test_empty_sets_succeed(dev):
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.geometry import edge_features, edge_features_grad

    some, none = _rng(9700).random((5, 2)).astype(np.float32), np.zeros((0, 2), np.float32)
    for q, s in ((some, none), (none, some), (none, none)):
        g, coords, _ = DeviceGraph.from_point_sets(q, s, 1.0)
        nq, ns = q.shape[0], s.shape[0]
        assert g.n_edge_cols == 0
        h = edge_features(g, torch.ones((ns, 3), device=dev), torch.ones((nq, 3), device=dev), coords, relative=True, pad_to=4)
        assert tuple(h.shape) == (0, 8)
        back = edge_features_grad(g, h, (3, 3, 2), relative=True,
                                  out={"sources": torch.full((ns, 3), np.nan, device=dev), "queries": torch.full((nq, 3), np.nan, device=dev)})
        assert tuple(back["sources"].shape) == (ns, 3) and tuple(back["queries"].shape) == (nq, 3) and tuple(back["coords"].shape) == (0, 2)
        assert not bits(back["sources"].cpu().numpy()).any() and not bits(back["queries"].cpu().numpy()).any(), "empty rows give +0"
        g.close()


# ---- the Python functions, host forms, Fortran ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,widths", [("knn3", (66, 7, 2, 0)), ("hub", (64, 64, 3, 1)), ("knn3", (0, 0, 3, 0))])
def test_the_python_functions_equal_the_raw_entries(dev, name, widths):
    import torch
    from athena_amd.geometry import edge_features, edge_features_grad

    g, _ = handle(name)
    Fs, Fq, dim, rel = widths
    E, W = g.n_edge_cols, Fs + Fq + dim
    xs, xq, coords = features(name, widths)
    want_h, dh, want_dxs, want_dxq, want_dc = reference(name, widths, 1)
    ld = ld_of(W, 1)
    ins = [up(a, dev) if a is not None else None for a in (xs, xq, coords)]
    h = edge_features(g, *ins, relative=bool(rel), pad_to=4)
    assert tuple(h.shape) == (E, W) and h.stride(1) == 1 and h.stride(0) == -(-W // 4) * 4 and same(h, want_h[:, :W])
    plain = edge_features(g, *ins, relative=bool(rel))
    assert plain.is_contiguous() and same(plain, want_h[:, :W])
    buf = up(prefilled(E, W, ld), dev)
    into = edge_features(g, *ins, relative=bool(rel), out=buf[:, :W])
    assert into.data_ptr() == buf.data_ptr() and same(buf, want_h), "a strided out: the pad columns stay"
    dhd = up(dh, dev)
    res = edge_features_grad(g, dhd[:, :W], (Fs, Fq, dim), relative=bool(rel))
    assert list(res) == ["sources", "queries", "coords"]
    for key, want, width in (("sources", want_dxs, Fs), ("queries", want_dxq, Fq), ("coords", want_dc, dim)):
        assert tuple(res[key].shape) == want.shape and (width == 0 or same(res[key], want))
    if dim:
        mine = torch.full((E, dim), np.nan, device=dev)
        only = edge_features_grad(g, dhd[:, :W].contiguous(), (Fs, Fq, dim), relative=bool(rel), want=("coords",), out={"coords": mine})
        assert list(only) == ["coords"] and only["coords"] is mine and same(mine, want_dc)
    with pytest.raises(ValueError, match="want must name"):
        edge_features_grad(g, dhd[:, :W], (Fs, Fq, dim), want=("x",))
    with pytest.raises(ValueError, match="dh must be a float32 device tensor"):
        edge_features_grad(g, dhd[:, :W].t(), (Fs, Fq, dim))
    with pytest.raises(ValueError, match="at least one of x_sources, x_queries and coords"):
        edge_features(g)
    with pytest.raises(ValueError, match="out must be a float32 device tensor"):
        edge_features(g, *ins, out=buf)


@pytest.mark.parametrize("name,widths", [("knn3", (66, 7, 2, 0)), ("hub", (64, 64, 3, 1))])
def test_host_forms_give_the_device_entries_bytes(dev, name, widths):
    from athena_amd import _capi

    g, _ = handle(name)
    Fs, Fq, dim, rel = widths
    E, W = g.n_edge_cols, Fs + Fq + dim
    ld = ld_of(W, 1)
    xs, xq, coords = features(name, widths)
    want_h, dh, want_dxs, want_dxq, want_dc = reference(name, widths, 1)
    h = prefilled(E, W, ld).copy()
    _capi.call("athena_mp_edge_gather_host", g.handle, Fs, vp(xs), Fq, vp(xq), dim, vp(coords), rel, ld, vp(h))
    assert h.tobytes() == want_h.tobytes(), "the host form keeps the pad columns too"
    outs = [np.full(a.shape, np.nan, np.float32) for a in (want_dxs, want_dxq, want_dc)]
    _capi.call("athena_mp_edge_gather_bwd_host", g.handle, Fs, Fq, dim, rel, ld, vp(dh), *(vp(a) for a in outs))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, (want_dxs, want_dxq, want_dc)))
    alone = np.full(want_dxq.shape, np.nan, np.float32)
    _capi.call("athena_mp_edge_gather_bwd_host", g.handle, Fs, Fq, dim, rel, ld, vp(dh), None, vp(alone), None)
    assert alone.tobytes() == want_dxq.tobytes()


@pytest.mark.parametrize("rel", [0, 1])
def test_fortran_program_writes_the_device_entries_bytes(dev, tmp_path, rel):
    if not os.path.exists(RUNNER):
        pytest.fail("edge_gather_run is not built: __graft_entry__.build() compiles the Fortran host side")
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.geometry import edge_features, edge_features_grad

    rng = _rng(9800 + rel)
    nq, ns, k, Fs, Fq = 40, 90, 3, 6, 6 if rel else 5
    W = Fs + Fq + 3
    ld = W + 2
    q, s = rng.random((nq, 3)).astype(np.float32), rng.random((ns, 3)).astype(np.float32)
    xs, xq = (draw_finite(rng, (ns, Fs), np.float32(-0.0)), draw_finite(rng, (nq, Fq), np.float32(0.0))) if rel else \
        (draw_copy(rng, (ns, Fs)), draw_copy(rng, (nq, Fq)))
    h0 = prefilled(nq * k, W, ld)
    dh = rng.standard_normal((nq * k, ld)).astype(np.float32)
    dh[:, W:] = np.nan
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        np.array([nq, ns, 3, k, Fs, Fq, rel, ld], np.int32).tofile(f)
        np.array([np.inf], np.float32).tofile(f)
        q.tofile(f); s.tofile(f); xs.tofile(f); xq.tofile(f); h0.tofile(f); dh.tofile(f)
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"edge_gather_run failed ({out.returncode}): {out.stdout[-1000:]} {out.stderr[-2000:]}"
    g, coords, _ = DeviceGraph.from_point_sets_knn(q, s, k)
    E = g.n_edge_cols
    assert E == nq * k
    buf = up(h0, dev)
    edge_features(g, up(xs, dev), up(xq, dev), coords, relative=bool(rel), out=buf[:, :W])
    back = edge_features_grad(g, up(dh, dev)[:, :W], (Fs, Fq, 3), relative=bool(rel))
    raw = open(res, "rb").read()
    assert np.frombuffer(raw, np.int64, 1)[0] == E
    at = 8
    for what, t in (("h", buf), ("dxs", back["sources"]), ("dxq", back["queries"]), ("dcoords", back["coords"])):
        a = t.cpu().numpy()
        assert raw[at:at + a.nbytes] == a.tobytes(), what
        at += a.nbytes
    assert at == len(raw)
    g.close()


# ---- end to end: the set-abstraction step on exact integers ----------------------------------------------------------------------------
def test_the_set_abstraction_step_on_integers_equals_numpy_exactly(dev):
    """farthest_points -> from_point_sets_knn(coarse, points, k = 8) -> edge_features(x_sources, coords, pad_to = 4) -> a dense step
    -> ReLU -> pool_max(edges = ...), and back with an integer dy: pool_max_grad(to = "edges") -> the ReLU mask -> the transposed
    dense step -> edge_features_grad -> point_sets_grad.  Lattice points, features in -2 .. 2 and an integer weight matrix: every
    intermediate is an integer below 2^24 (asserted on the numpy side), so no sum rounds and every array is np.array_equal"""
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.geometry import edge_features, edge_features_grad, farthest_points, point_sets_grad, pool_max, pool_max_grad

    rng = _rng(9900)
    sizes, k, Fs, H = [60, 50, 40], 8, 6, 8
    offsets = kb.offsets_of(sizes)
    pts = np.concatenate([np.stack(np.unravel_index(rng.choice(512, n, replace=False), (8, 8, 8)), 1) for n in sizes]).astype(np.float32)
    x = rng.integers(-2, 3, (150, Fs)).astype(np.float32)
    Wt = rng.integers(-2, 3, (Fs + 3, H)).astype(np.float32)
    exact = lambda *arrays: all(np.abs(a.astype(np.float64)).max() < 2.0 ** 24 and np.array_equal(a, np.rint(a)) for a in arrays)

    # numpy fp32
    sample, coarse, soff, _ = farthest_points(pts, offsets, ratio=0.2)
    want_sample, want_coarse, _, _ = fr.brute_force(pts, soff, offsets)
    nc = int(soff[-1])
    nbr, _ = kb.brute_force(want_coarse, pts, k, None, soff, offsets)
    i, j, cnp, _, _ = kb.graph_of(nbr, want_coarse, pts, soff)
    E = i.size
    A = er.arrays_of(i, j, nc, 150)
    assert nc == 30 and E == nc * k
    W = Fs + 3
    m = er.fwd(A, x, None, cnp, 0, prefilled(E, W, 12))[:, :W]
    z = m @ Wt
    bound = np.abs(m.astype(np.float64)) @ np.abs(Wt.astype(np.float64))            # what any order of the sum stays below
    a = np.where(z > 0, z, np.float32(0))
    y, arg = pr.edges_fwd(A, a)
    dy = rng.integers(-3, 4, (nc, H)).astype(np.float32)
    da = pr.bwd_edges(A, arg, dy, E)
    dz = np.where(z > 0, da, np.float32(0))
    dm = dz @ Wt.T
    back_bound = np.abs(dz.astype(np.float64)) @ np.abs(Wt.T.astype(np.float64))
    dxs, _, dc = er.bwd(A, dm, (Fs, 0, 3), 0)
    col_len = np.diff(A["t_rowptr"]).max()
    dq, ds = br.reference_grad(i, j, dc, nc, 150)
    assert exact(m, z, bound, a, y, da, dz, dm, back_bound, dxs, dc, dq, ds) and back_bound.max() * max(col_len, k) < 2.0 ** 24

    # the device
    assert np.array_equal(sample.cpu().numpy(), want_sample) and same(coarse, want_coarse)
    g, coords, _ = DeviceGraph.from_point_sets_knn(coarse, pts, k, query_offsets=soff, source_offsets=offsets)
    for key, arr in A.items():
        assert np.array_equal(g.export(key), arr)
    md = edge_features(g, x_sources=up(x, dev), coords=coords, pad_to=4)
    assert md.stride(0) == 12 and np.array_equal(md.cpu().numpy(), m)
    Wd = up(Wt, dev)
    zd = torch.matmul(md, Wd)
    assert np.array_equal(zd.cpu().numpy(), z)
    yd, argd = pool_max(g, edges=torch.relu(zd).contiguous())
    assert np.array_equal(yd.cpu().numpy(), y) and np.array_equal(argd.cpu().numpy(), arg)
    dad = pool_max_grad(g, argd, up(dy, dev), to="edges")
    dmd = torch.full((E, 12), np.nan, device=dev)
    dmd[:, :W] = torch.matmul(dad * (zd > 0), Wd.t())
    assert np.array_equal(dmd[:, :W].cpu().numpy(), dm)
    res = edge_features_grad(g, dmd[:, :W], (Fs, 0, 3))
    p = point_sets_grad(g, res["coords"])
    assert np.array_equal(res["sources"].cpu().numpy(), dxs) and np.array_equal(res["coords"].cpu().numpy(), dc)
    assert tuple(res["queries"].shape) == (nc, 0)
    assert np.array_equal(p["queries"].cpu().numpy(), dq) and np.array_equal(p["sources"].cpu().numpy(), ds)
    g.close()
