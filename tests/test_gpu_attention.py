"""GPU: attention pooling over a handle's rows (athena_amd/csrc/attention.hip) against the transcription of the definition
(tests/attention_reference.py).  The two-set handles are those of tests/test_gpu_interp.py -- 300 queries and 200 sources in three
clouds, the middle one without sources, so its rows are empty: k = 1, 3, 64, and a radius handle with a hub row of 150 entries
beside empty rows.  Every output is pre-filled with NaN, so an element that was not written shows.

alpha is held to the per-element bound of tests/activation_reference.py around the float64 twin, with the fp32 transcription as
anchor, and to bits where the definition fixes them (NaN exactly where the twin has one, +0 for a -inf score, 1 for a row of one
entry).  The gathers, bwd_x, bwd_edges and softmax_bwd are compared word for word with the transcription fed with the device's own
alpha (and dalpha).  bwd_alpha is compared word for word on small integers and at C = 1, and elsewhere held to
|dev - f64| <= |seq32 - f64| + 1e-5 sum_c |dy v|.

The shapes (F, H) cover both load routes (F % 4), every group width (4 .. 64), a second pass (260), the three weight paths of the
16-byte route (C % 4 == 0; H == F; neither: (4, 2)), and the three routes of bwd_alpha: C = 1, the __shfl_xor tree (C = 4, 16, 64) and
the plain walk (C = 2, 3, 24, 66, 260)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import activation_reference as act
import attention_reference as ar
import test_gpu_interp as ti
import test_gpu_pool as tp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "attention_run")
SHAPES = ((1, 1), (3, 1), (3, 3), (4, 2), (4, 4), (7, 7), (64, 1), (64, 4), (64, 16), (64, 64), (66, 1), (66, 33), (96, 4), (128, 8),
          (260, 1), (260, 65), (260, 260))
HEADS = tuple(sorted({H for _, H in SHAPES}))
CASES = ("knn1", "knn3", "knn64", "hub")
KINDS = ("normal", "edges")
ONE = 0x3F800000

vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
bits = lambda a: np.ascontiguousarray(a).view(np.int32)
yardstick, handle, up = ti.yardstick, ti.handle, ti.up


def _rng(seed):
    return np.random.default_rng(seed)


def same(t, want):
    return np.array_equal(bits(t.cpu().numpy()), bits(want))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def planted(name, H):
    """the named (row, head) pairs of the "edges" scores: "nan" (the row's last entry is a NaN), "inf" (its first is +inf), "all_minf"
    (every entry is -inf), "minf" (its second entry is -inf beside finite ones; None on knn1, whose rows hold one entry)"""
    lens = np.diff(yardstick(name)[3]["rowptr"])
    rows = np.nonzero(lens >= 2)[0] if (lens >= 2).sum() >= 4 else np.nonzero(lens >= 1)[0]
    rows = [int(r) for r in rows[:4]]
    return {"nan": (rows[0], 0), "inf": (rows[1], H - 1), "all_minf": (rows[2], H // 2),
            "minf": (rows[3], (H - 1) // 2) if lens[rows[3]] >= 2 else None}


@functools.lru_cache(None)
def scores(name, H, kind):
    """[E, H] float32.  "normal": standard normal times 3.  "edges": the rows of activation_reference.softmax_rows (spreads 0 .. 1e4,
    offsets 0 and +-1e4, the maximum first / last / tied three times) laid along the handle's rows -- (row i, head h) takes row
    (i H + h) mod 70 of softmax_rows(its length) --, then the pairs of planted()"""
    A = yardstick(name)[3]
    rowptr, eid = A["rowptr"].astype(np.int64), A["eid"]
    E, lens = eid.size, np.diff(A["rowptr"])
    rng = _rng(9400 + 31 * CASES.index(name) + H)
    if kind == "normal":
        return (3.0 * rng.standard_normal((E, H))).astype(np.float32)
    s = np.zeros((E, H), np.float32)
    for L in np.unique(lens[lens > 0]):
        R = act.softmax_rows(int(L), seed=7)                              # [70, L]
        rows = np.nonzero(lens == L)[0]
        which = (rows[:, None] * H + np.arange(H)[None, :]) % R.shape[0]  # [rows, H]
        e = eid[rowptr[rows][:, None] + np.arange(L)[None, :]]            # [rows, L]
        s[e] = np.transpose(R[which], (0, 2, 1))                          # [rows, L, H]
    entries = lambda i: eid[rowptr[i]:rowptr[i + 1]]
    p = planted(name, H)
    s[entries(p["nan"][0])[-1], p["nan"][1]] = np.nan
    s[entries(p["inf"][0])[0], p["inf"][1]] = np.inf
    s[entries(p["all_minf"][0]), p["all_minf"][1]] = -np.inf
    if p["minf"] is not None:
        s[entries(p["minf"][0])[1], p["minf"][1]] = -np.inf
    return s


@functools.lru_cache(None)
def alpha_reference(name, H, kind):
    """(fp32 transcription, float64 twin, scale, a) of the case's scores, computed once"""
    A = yardstick(name)[3]
    s = scores(name, H, kind)
    f64, scale, a = ar.softmax64(A, s)
    return ar.softmax(A, s), f64, scale, a


@functools.lru_cache(None)
def integers(name, F):
    """x, h, dy in -2 .. 2 with signed zeros: every product and every sum of bwd_alpha is exact"""
    E = yardstick(name)[0].size
    rng = _rng(9500 + 13 * CASES.index(name) + F)
    draw = lambda n: rng.integers(-2, 3, (n, F)).astype(np.float32)
    x, h, dy = draw(200), draw(E), draw(300)
    x[::9, 0], h[::11, F - 1] = -0.0, -0.0
    return x, h, dy


@functools.lru_cache(None)
def reference(name, F, H):
    """every bit-defined result from the fp32 transcription's alpha on the normal features of tests/test_gpu_pool.py, computed once:
    what the tests of operand placement compare with"""
    A = yardstick(name)[3]
    E = A["col"].size
    x, h, dy = tp.features(name, "normal", F)
    alpha = alpha_reference(name, H, "normal")[0]
    dalpha = ar.bwd_alpha(A, E, x, None, dy, H)
    return {"alpha": alpha, "y": ar.fwd(A, alpha, x, H), "yh": ar.edges_fwd(A, alpha, h, H), "dx": ar.bwd_x(A, alpha, dy, H),
            "dh": ar.bwd_edges(A, alpha, dy, H), "dalpha": dalpha, "dscores": ar.softmax_bwd(A, alpha, dalpha)}


def inputs_are_what_the_test_needs(name, H):
    """on the yardstick alone (tests/test_attention.py runs this on the CPU for every case): empty rows, the hub row, and for the
    "edges" scores that the planted pairs, and only they, are NaN, that a -inf beside a finite maximum is there, and the spread"""
    A = yardstick(name)[3]
    lens = np.diff(A["rowptr"])
    assert (lens == 0).any(), "an empty slice gives empty rows"
    if name == "hub":
        assert lens[0] > 64 and lens[0] % 8 != 0
    s = scores(name, H, "edges")
    _, f64, _, a = alpha_reference(name, H, "edges")
    p = planted(name, H)
    want = np.zeros(s.shape, bool)
    for key in ("nan", "inf", "all_minf"):
        i, h = p[key]
        want[A["eid"][A["rowptr"][i]:A["rowptr"][i + 1]], h] = True
    assert len({p[k][0] for k in ("nan", "inf", "all_minf")}) == 3
    assert np.array_equal(np.isnan(f64), want), "the planted (row, head) pairs are NaN in all of their entries, and nothing else is"
    zero = np.isneginf(s) & ~want
    assert zero.sum() == (0 if p["minf"] is None else 1) and not f64[zero].any()
    if name != "knn1":
        with np.errstate(invalid="ignore"):
            assert (a[~want & ~zero] < -1e4).any() and (np.abs(s[np.isfinite(s)]) >= 1e4).any()
    assert not np.isnan(alpha_reference(name, H, "normal")[1]).any()


# ---- the device entries --------------------------------------------------------------------------------------------------------
def device(entry, g, ints, arrays, shape, dev):
    """one call of athena_mp_<entry>(g, *ints, *arrays, out): out [shape] pre-filled with NaN"""
    import torch
    from athena_amd import _capi

    out = torch.full(shape, np.nan, dtype=torch.float32, device=dev)
    _capi.use_torch_stream()
    _capi.call("athena_mp_" + entry, g.handle, *ints, *(ptr(a) for a in arrays), ptr(out))
    return out


def device_alpha(g, s, dev):
    return device("attn_softmax_fwd", g, (int(s.shape[1]),), (s,), tuple(s.shape), dev)


# ---- alpha ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("name", CASES)
def test_alpha_is_inside_its_bound_and_exact_where_the_definition_says(dev, name, H, kind):
    g, _ = handle(name)
    s = scores(name, H, kind)
    o32, f64, scale, a = alpha_reference(name, H, kind)
    inputs_are_what_the_test_needs(name, H)
    sd = up(s, dev)
    got = device_alpha(g, sd, dev).cpu().numpy()
    nan = np.isnan(f64)
    assert np.array_equal(np.isnan(got), nan), "NaN where the definition has one, and nowhere else"
    zero = np.isneginf(s) & ~nan
    assert not bits(got[zero]).any(), "-inf beside a finite maximum gives +0"
    if name == "knn1":
        assert (bits(got[~nan]) == ONE).all() and (~nan).any(), "a row of one finite entry gives exactly 1"
    ok = ~nan & ~zero
    act.assert_each(got[ok], o32[ok], f64[ok], scale[ok], a[ok], 0.0, f"alpha {name} H={H} {kind}")
    again = device_alpha(g, sd, dev).cpu().numpy()
    assert again.tobytes() == got.tobytes() and same(sd, s)


# ---- the gathers and the reverse steps -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,H", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_gathers_and_reverse_steps_equal_the_transcription(dev, name, F, H):
    g, _ = handle(name)
    A = yardstick(name)[3]
    E = g.n_edge_cols
    x, h, dy = tp.features(name, "normal", F)
    assert (bits(x) == bits(np.float32(-0.0))).any() and (bits(dy) == bits(np.float32(-0.0))).any()
    xd, hd, dyd = up(x, dev), up(h, dev), up(dy, dev)
    alpha_d = device_alpha(g, up(scores(name, H, "normal"), dev), dev)
    alpha = alpha_d.cpu().numpy()
    assert not np.isnan(alpha).any()
    y = device("attn_gather_fwd", g, (F, H), (alpha_d, xd), (300, F), dev)
    yh = device("attn_gather_edges_fwd", g, (F, H), (alpha_d, hd), (300, F), dev)
    dx = device("attn_gather_bwd_x", g, (F, H), (alpha_d, dyd), (200, F), dev)
    dh = device("attn_gather_bwd_edges", g, (F, H), (alpha_d, dyd), (E, F), dev)
    assert same(y, ar.fwd(A, alpha, x, H)) and same(yh, ar.edges_fwd(A, alpha, h, H))
    assert same(dx, ar.bwd_x(A, alpha, dy, H)) and same(dh, ar.bwd_edges(A, alpha, dy, H))
    if H == 1:
        w = alpha_d.reshape(-1)
        assert y.cpu().numpy().tobytes() == ti.device_gather("athena_mp_interp_fwd", g, w, xd, 300, dev).cpu().numpy().tobytes()
        assert dx.cpu().numpy().tobytes() == ti.device_gather("athena_mp_interp_bwd_x", g, w, dyd, 200, dev).cpu().numpy().tobytes()
    xi, hi, dyi = integers(name, F)
    for form, values, ivalues in (("x", xd, xi), ("h", hd, hi)):
        pick = lambda v: (v, None) if form == "x" else (None, v)
        exact = device("attn_gather_bwd_alpha", g, (F, H), (*pick(up(ivalues, dev)), up(dyi, dev)), (E, H), dev)
        assert same(exact, ar.bwd_alpha(A, E, *pick(ivalues), dyi, H)), f"bwd_alpha ({form}) on small integers"
        dalpha_d = device("attn_gather_bwd_alpha", g, (F, H), (*pick(values), dyd), (E, H), dev)
        dalpha = dalpha_d.cpu().numpy()
        f64, bnd = ar.alpha_bound(A, E, *pick(x if form == "x" else h), dy, H)
        share = np.abs(dalpha - f64) / np.where(bnd > 0, bnd, 1.0)
        print(f"bwd_alpha ({form}) {name} F={F} H={H}: worst share of the bound {float(share.max()) if share.size else 0.0:.3f}")
        assert not np.isnan(dalpha).any() and (np.abs(dalpha - f64) <= bnd).all()
        if F == H:
            assert same(dalpha_d, ar.bwd_alpha(A, E, *pick(x if form == "x" else h), dy, H)), "C = 1: the product itself"
        ds = device("attn_softmax_bwd", g, (H,), (alpha_d, dalpha_d), (E, H), dev)
        assert same(ds, ar.softmax_bwd(A, alpha, dalpha)), f"softmax_bwd ({form})"
    assert same(xd, x) and same(hd, h) and same(dyd, dy), "an input changed"


@pytest.mark.parametrize("F,H", [(4, 2), (64, 4), (64, 64), (96, 4), (260, 65)])
@pytest.mark.parametrize("name", ["knn3", "hub"])
def test_two_runs_write_the_same_bytes(dev, name, F, H):
    g, _ = handle(name)
    E = g.n_edge_cols
    x, h, dy = tp.features(name, "normal", F)
    xd, hd, dyd = up(x, dev), up(h, dev), up(dy, dev)
    ad = up(reference(name, F, H)["alpha"], dev)
    dad = up(reference(name, F, H)["dalpha"], dev)
    calls = (("attn_gather_fwd", (F, H), (ad, xd), (300, F)), ("attn_gather_edges_fwd", (F, H), (ad, hd), (300, F)),
             ("attn_gather_bwd_x", (F, H), (ad, dyd), (200, F)), ("attn_gather_bwd_edges", (F, H), (ad, dyd), (E, F)),
             ("attn_gather_bwd_alpha", (F, H), (xd, None, dyd), (E, H)), ("attn_gather_bwd_alpha", (F, H), (None, hd, dyd), (E, H)),
             ("attn_softmax_bwd", (H,), (ad, dad), (E, H)))
    for entry, ints, arrays, shape in calls:
        first, second = device(entry, g, ints, arrays, shape, dev), device(entry, g, ints, arrays, shape, dev)
        assert first.cpu().numpy().tobytes() == second.cpu().numpy().tobytes(), entry


# ---- the Python wrappers, refusals, empty sets ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,F,H", [("knn3", 7, 7), ("hub", 64, 4), ("knn64", 96, 4)])
def test_the_wrappers_return_the_entries_bytes(dev, name, F, H):
    from athena_amd.geometry import attend, attend_grad, attention_weights

    g, _ = handle(name)
    E = g.n_edge_cols
    x, h, dy = tp.features(name, "normal", F)
    xd, hd, dyd, sd = up(x, dev), up(h, dev), up(dy, dev), up(scores(name, H, "normal"), dev)
    eq = lambda a, b: a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    alpha = attention_weights(g, sd)
    assert tuple(alpha.shape) == (E, H) and eq(alpha, device_alpha(g, sd, dev))
    for kw, entry, values, back, rows in (({"x": xd}, "attn_gather_fwd", xd, "attn_gather_bwd_x", 200),
                                          ({"edges": hd}, "attn_gather_edges_fwd", hd, "attn_gather_bwd_edges", E)):
        y = attend(g, alpha, **kw)
        assert eq(y, device(entry, g, (F, H), (alpha, values), (300, F), dev))
        grads = attend_grad(g, alpha, dyd, **kw)
        assert sorted(grads) == ["scores", "values"]
        assert eq(grads["values"], device(back, g, (F, H), (alpha, dyd), (rows, F), dev))
        pick = (values, None) if "x" in kw else (None, values)
        dalpha = device("attn_gather_bwd_alpha", g, (F, H), (*pick, dyd), (E, H), dev)
        assert eq(grads["scores"], device("attn_softmax_bwd", g, (H,), (alpha, dalpha), (E, H), dev))
        only = attend_grad(g, alpha, dyd, want=("values",), out={"values": y.new_full((rows, F), np.nan)}, **kw)
        assert sorted(only) == ["values"] and eq(only["values"], grads["values"])


def test_refusals_arrive_with_their_messages_and_the_library_goes_on(dev):
    import torch
    from athena_amd import DeviceGraph, _capi
    from athena_amd._capi import AthenaMPError
    from athena_amd.geometry import attend, attend_grad, attention_weights
    from helpers import random_graph

    g, _ = handle("knn3")
    F, H = 4, 2
    E = g.n_edge_cols
    x, h, dy = tp.features("knn3", "normal", F)
    xd, hd, dyd, sd = up(x, dev), up(h, dev), up(dy, dev), up(scores("knn3", H, "normal"), dev)
    alpha = device_alpha(g, sd, dev)
    y = torch.empty((300, F), device=dev)
    ia, ja = random_graph(20, 40, 1, self_loops=True)
    kipf, loops = DeviceGraph(ia, ja, n_edge_cols=0), DeviceGraph(ia, ja)
    sq, _ = tp.square()
    three = (("attn_gather_fwd", (alpha, xd, y)), ("attn_gather_edges_fwd", (alpha, hd, y)), ("attn_gather_bwd_x", (alpha, dyd, xd)),
             ("attn_gather_bwd_edges", (alpha, dyd, hd)))
    every = three + (("attn_gather_bwd_alpha", (xd, None, dyd, alpha)),)
    for bad, message in ((kipf, r": the handle has no edge columns"), (loops, r": \d+ of the handle's \d+ entries carry no edge id"),
                         (sq, r": \d+ entries over \d+ edge columns: need one entry per edge column")):
        for entry, arrays in every:
            with pytest.raises(AthenaMPError, match=entry + message):
                _capi.call("athena_mp_" + entry, bad.handle, F, H, *(ptr(a) for a in arrays))
        with pytest.raises(AthenaMPError, match="attn_softmax_fwd" + message):
            _capi.call("athena_mp_attn_softmax_fwd", bad.handle, H, ptr(sd), ptr(alpha))
        with pytest.raises(AthenaMPError, match="attn_softmax_bwd" + message):
            _capi.call("athena_mp_attn_softmax_bwd", bad.handle, H, ptr(alpha), ptr(alpha), ptr(sd))
    for entry, arrays in every:
        with pytest.raises(AthenaMPError, match=entry + r": F = 6 is no multiple of H = 4"):
            _capi.call("athena_mp_" + entry, g.handle, 6, 4, *(ptr(a) for a in arrays))
        with pytest.raises(AthenaMPError, match=entry + r": H = 0: need at least one head"):
            _capi.call("athena_mp_" + entry, g.handle, F, 0, *(ptr(a) for a in arrays))
        with pytest.raises(AthenaMPError, match=entry + r": F = 0: need at least one feature column"):
            _capi.call("athena_mp_" + entry, g.handle, 0, 1, *(ptr(a) for a in arrays))
    with pytest.raises(AthenaMPError, match=r"attn_softmax_fwd: H = -1"):
        _capi.call("athena_mp_attn_softmax_fwd", g.handle, -1, ptr(sd), ptr(alpha))
    for both in ((xd, hd), (None, None)):
        with pytest.raises(AthenaMPError, match=r"attn_gather_bwd_alpha: exactly one of x"):
            _capi.call("athena_mp_attn_gather_bwd_alpha", g.handle, F, H, ptr(both[0]), ptr(both[1]), ptr(dyd), ptr(alpha))
    with pytest.raises(AthenaMPError, match=r"attn_gather_fwd: null array"):
        _capi.call("athena_mp_attn_gather_fwd", g.handle, F, H, ptr(alpha), None, ptr(y))
    with pytest.raises(AthenaMPError, match=r"attention_host: exactly one of x"):
        _capi.call("athena_mp_attention_host", g.handle, F, H, vp(scores("knn3", H, "normal")), vp(x), vp(h), None, vp(np.zeros((300, F), np.float32)))
    with pytest.raises(AthenaMPError, match=r"attention_bwd_host: dx, dh and dscores are all null"):
        _capi.call("athena_mp_attention_bwd_host", g.handle, F, H, vp(x), vp(x), None, vp(dy), None, None, None)
    with pytest.raises(ValueError, match="exactly one of x and edges"):
        attend(g, alpha, x=xd, edges=hd)
    with pytest.raises(ValueError, match="exactly one of x and edges"):
        attend_grad(g, alpha, dyd)
    with pytest.raises(ValueError, match="do not divide into H = 2 heads"):
        attend(g, alpha, x=up(np.zeros((200, 3), np.float32), dev))
    with pytest.raises(ValueError, match="scores must be a contiguous float32 device tensor"):
        attention_weights(g, sd[:-1])
    with pytest.raises(ValueError, match="alpha must be a contiguous float32 device tensor"):
        attend(g, alpha[:-1], x=xd)
    with pytest.raises(ValueError, match="dy must be a contiguous float32 device tensor"):
        attend_grad(g, alpha, dyd[:, :2].contiguous(), x=xd)
    with pytest.raises(ValueError, match="want must name some of"):
        attend_grad(g, alpha, dyd, x=xd, want=("alpha",))
    with pytest.raises(AthenaMPError, match="attn_softmax_fwd: the handle has no edge columns"):
        attention_weights(kipf, torch.zeros((0, 2), device=dev))
    got = device("attn_gather_fwd", g, (F, H), (alpha, xd), (300, F), dev)              # and the next call works
    assert same(got, ar.fwd(yardstick("knn3")[3], alpha.cpu().numpy(), x, H))
    kipf.close(); loops.close()


def test_empty_sets_succeed(dev):
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.geometry import attend, attend_grad, attention_weights

    some, none = _rng(9600).random((5, 2)).astype(np.float32), np.zeros((0, 2), np.float32)
    for q, s in ((some, none), (none, some), (none, none)):
        g, _, _ = DeviceGraph.from_point_sets(q, s, 1.0)
        nq, ns = q.shape[0], s.shape[0]
        assert g.n_edge_cols == 0
        alpha = attention_weights(g, torch.ones((0, 3), device=dev))
        assert tuple(alpha.shape) == (0, 3)
        for kw, rows in (({"x": torch.ones((ns, 6), device=dev)}, ns), ({"edges": torch.ones((0, 6), device=dev)}, 0)):
            y = attend(g, alpha, out=torch.full((nq, 6), np.nan, device=dev), **kw)
            assert tuple(y.shape) == (nq, 6) and not bits(y.cpu().numpy()).any()
            back = attend_grad(g, alpha, torch.ones((nq, 6), device=dev), out={"values": torch.full((rows, 6), np.nan, device=dev)}, **kw)
            assert tuple(back["values"].shape) == (rows, 6) and not bits(back["values"].cpu().numpy()).any()
            assert tuple(back["scores"].shape) == (0, 3)
        g.close()


# ---- host forms, Fortran -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,F,H", [("knn3", 7, 7), ("hub", 64, 4)])
def test_host_forms_give_the_device_entries_bytes(dev, name, F, H):
    from athena_amd import _capi
    from athena_amd.geometry import attend, attend_grad, attention_weights

    g, _ = handle(name)
    E = g.n_edge_cols
    x, h, dy = tp.features(name, "normal", F)
    s = scores(name, H, "normal")
    alpha_d = attention_weights(g, up(s, dev))
    alpha = alpha_d.cpu().numpy()
    for values, kw in ((x, "x"), (h, "edges")):
        first, second = (vp(values), None) if kw == "x" else (None, vp(values))
        ha, hy = np.full((E, H), np.nan, np.float32), np.full((300, F), np.nan, np.float32)
        _capi.call("athena_mp_attention_host", g.handle, F, H, vp(s), first, second, vp(ha), vp(hy))
        want_y = attend(g, alpha_d, **{kw: up(values, dev)}).cpu().numpy()
        assert ha.tobytes() == alpha.tobytes() and hy.tobytes() == want_y.tobytes()
        hy2 = np.full((300, F), np.nan, np.float32)
        _capi.call("athena_mp_attention_host", g.handle, F, H, vp(s), first, second, None, vp(hy2))
        assert hy2.tobytes() == want_y.tobytes()
        want = attend_grad(g, alpha_d, up(dy, dev), **{kw: up(values, dev)})
        rows = 200 if kw == "x" else E
        hv, hs = np.full((rows, F), np.nan, np.float32), np.full((E, H), np.nan, np.float32)
        outs = (vp(hv), None) if kw == "x" else (None, vp(hv))
        _capi.call("athena_mp_attention_bwd_host", g.handle, F, H, vp(alpha), first, second, vp(dy), *outs, vp(hs))
        assert hv.tobytes() == want["values"].cpu().numpy().tobytes() and hs.tobytes() == want["scores"].cpu().numpy().tobytes()
        hv2 = np.full((rows, F), np.nan, np.float32)
        _capi.call("athena_mp_attention_bwd_host", g.handle, F, H, vp(alpha), first, second, vp(dy), *((vp(hv2), None) if kw == "x" else (None, vp(hv2))), None)
        assert hv2.tobytes() == hv.tobytes()


def test_fortran_program_writes_the_device_entries_bytes(dev, tmp_path):
    if not os.path.exists(RUNNER):
        pytest.fail("attention_run is not built: __graft_entry__.build() compiles the Fortran host side")
    from athena_amd import DeviceGraph
    from athena_amd.geometry import attend, attend_grad, attention_weights

    rng = _rng(9700)
    nq, ns, k, F, H = 40, 90, 3, 6, 2
    q, s = rng.random((nq, 3)).astype(np.float32), rng.random((ns, 3)).astype(np.float32)
    sc = (3.0 * rng.standard_normal((nq * k, H))).astype(np.float32)
    x, h, dy = (rng.standard_normal(shape).astype(np.float32) for shape in ((ns, F), (nq * k, F), (nq, F)))
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        np.array([nq, ns, 3, k, F, H], np.int32).tofile(f)
        np.array([np.inf], np.float32).tofile(f)
        q.tofile(f); s.tofile(f); sc.tofile(f); x.tofile(f); h.tofile(f); dy.tofile(f)
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"attention_run failed ({out.returncode}): {out.stdout[-1000:]} {out.stderr[-2000:]}"
    g, _, _ = DeviceGraph.from_point_sets_knn(q, s, k)
    E = g.n_edge_cols
    assert E == nq * k
    alpha = attention_weights(g, up(sc, dev))
    yx, yh = attend(g, alpha, x=up(x, dev)), attend(g, alpha, edges=up(h, dev))
    gx, gh = attend_grad(g, alpha, up(dy, dev), x=up(x, dev)), attend_grad(g, alpha, up(dy, dev), edges=up(h, dev))
    raw = open(res, "rb").read()
    assert np.frombuffer(raw, np.int64, 1)[0] == E
    at = 8
    for what, t in (("alpha", alpha), ("y_x", yx), ("y_h", yh), ("dx", gx["values"]), ("dscores_x", gx["scores"]), ("dh", gh["values"]),
                    ("dscores_h", gh["scores"])):
        a = t.cpu().numpy()
        assert raw[at:at + a.nbytes] == a.tobytes(), what
        at += a.nbytes
    assert at == len(raw)
    g.close()
