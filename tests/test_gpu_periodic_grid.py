"""GPU: the grid route of the periodic builder (athena_amd/csrc/periodic_graph.hip) -- a cell grid in fractional coordinates that
prunes the atom pairs of large cells before the unchanged predicate decides them.  Every array must be what the walk route writes
and what the yardstick of tests/periodic_reference.py says, compared with np.array_equal; athena_mp_periodic_stats tells which
route a structure took.  ATHENA_MP_PERIODIC_ROUTE pins the route for a call."""
import contextlib
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import periodic_grid_reference as gr
import periodic_reference as pr
from test_gpu_periodic_graph import KEYS, RUNNER, _batch, _equal, _expected, _pairs_call, _same, _sizes, _structures

pytestmark = pytest.mark.gpu

F32 = np.float32


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


@contextlib.contextmanager
def _route(mode):
    old = os.environ.get("ATHENA_MP_PERIODIC_ROUTE")
    try:
        if mode is None:
            os.environ.pop("ATHENA_MP_PERIODIC_ROUTE", None)
        else:
            os.environ["ATHENA_MP_PERIODIC_ROUTE"] = mode
        yield
    finally:
        if old is None:
            os.environ.pop("ATHENA_MP_PERIODIC_ROUTE", None)
        else:
            os.environ["ATHENA_MP_PERIODIC_ROUTE"] = old


def _stats():
    from athena_amd.graph import periodic_stats

    s = periodic_stats()
    return [s[k] for k in ("structures_walked", "structures_grid", "walk_pairs", "grid_pairs", "grid_fallbacks")]


def _build(dev, mode, frac, lat, off, cmin=0.5, cmax=3.0, pbc=(1, 1, 1), **kw):
    with _route(mode):
        got = _pairs_call(dev, frac, lat, off, cmin, cmax, pbc, **kw)
        return got, _stats()


def _same_arrays(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), f"{what}: {k} differs"
    for x, y in zip(a["raw"], b["raw"]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), what


def _single(frac, lat):
    frac = np.ascontiguousarray(frac, F32)
    return frac, np.ascontiguousarray(lat, F32).reshape(1, 3, 3), np.array([0, frac.shape[0]], np.int32)


@functools.lru_cache(maxsize=None)
def _large():
    """the two large structures of the automatic-mode batch and their yardstick results (computed once, never changed)"""
    rng = _rng(21)
    a = (rng.random((1000, 3)).astype(F32), gr.cubic(24.0))
    b = (rng.random((700, 3)).astype(F32), gr.sheared_cell())
    return a, b, pr.structure_edges(*a, 0.5, 3.0, extra=1), pr.structure_edges(*b, 0.5, 3.0, extra=1)


@pytest.mark.parametrize("kind", ["cubic", "skewed", "small"])
def test_forced_grid_on_the_fixture_and_on_random_batches(dev, kind):
    from athena_amd import io

    if kind == "cubic":                                                       # the golden head fixture rides along once
        frac, lat, off = io.structures_from_frames(io.read_extxyz(os.path.join(os.path.dirname(__file__), "golden", "msgpass_chemical_head.xyz")))
        got, st = _build(dev, "grid", frac, lat, off)
        _equal(got, pr.reference_edges(frac, lat, off, 0.5, 3.0), "fixture")
        assert st[:2] == [0, 40] and st[4] == 0
    B = 65
    rng = _rng(B * 7 + len(kind))
    distinct = _structures(rng, kind, _sizes(rng, B))
    order = list(range(B))
    order[B // 2] = order[-1] = None                                          # empties in the middle and at the end
    frac, lat, off = _batch(distinct, order)
    cmin = 0.5 if kind != "small" else 0.0
    want = _expected(distinct, order, off, cmin, 3.0)
    got, st = _build(dev, "grid", frac, lat, off, cmin)
    walk, sw = _build(dev, "walk", frac, lat, off, cmin)
    assert want["pairs"].shape[1] > 0
    _equal(got, want, f"grid, {kind}")
    _same_arrays(got, walk, f"grid against walk, {kind}")
    sizes = np.diff(off)
    assert st == [0, B - 2, 0, int(np.sum(sizes * (sizes + 1) // 2)), 0]      # tiny cells: one cell, every pair is a candidate
    assert sw == [B - 2, 0, int(np.sum(sizes * (sizes + 1) // 2)), 0, 0]


def test_automatic_mode_sends_the_large_structures_through_the_grid(dev):
    a, b, ea, eb = _large()
    rng = _rng(23)
    small = _structures(rng, "cubic", [12, 9])
    mid = (rng.random((128, 3)).astype(F32), gr.cubic(11.0))                  # the last size that stays with the walk
    distinct = [small[0], a, b, mid, small[1]]
    order = [0, 1, None, 2, 3, 4]
    frac, lat, off = _batch(distinct, order)
    per = [pr.structure_edges(*small[0], 0.5, 3.0), ea, pr.structure_edges(np.zeros((0, 3), F32), a[1], 0.5, 3.0), eb,
           pr.structure_edges(*mid, 0.5, 3.0), pr.structure_edges(*small[1], 0.5, 3.0)]
    want = pr.assemble(per, off, 3.0)
    got, st = _build(dev, None, frac, lat, off)
    _equal(got, want, "automatic mode")
    all_pairs = 1000 * 1001 // 2 + 700 * 701 // 2
    kept_pairs = len(set(zip(ea[0].tolist(), ea[1].tolist()))) + len(set(zip(eb[0].tolist(), eb[1].tolist())))
    print(f"stats {st}: candidate share {st[3] / all_pairs:.3f}, {kept_pairs} distinct kept pairs")
    assert st[1] == 2 and st[0] == 3 and st[4] == 0
    assert st[2] == 12 * 13 // 2 + 128 * 129 // 2 + 9 * 10 // 2
    assert kept_pairs <= st[3] <= all_pairs // 2
    want_cand = sum(int(gr.candidate_matrix(f, gr.axis_cells(L, 3.0, (1, 1, 1), f.shape[0])[0]).sum()) for f, L in (a, b))
    assert st[3] == want_cand                                                 # the rule as the header states it, pair for pair


@pytest.mark.parametrize("which", ["boundary", "frac in [-2, 3)", "cutoff edge"])
def test_boundary_wrapped_and_cutoff_edge_sets_under_forced_grid(dev, which):
    if which == "boundary":
        frac, L = gr.boundary_set()
    elif which == "cutoff edge":
        frac, L = gr.cutoff_edge_set()
    else:
        frac, L = (_rng(29).random((600, 3)) * 5.0 - 2.0).astype(F32), gr.cubic(18.0)
    frac, lat, off = _single(frac, L)
    edges = pr.structure_edges(frac, L, 0.5, 3.0, extra=1 if frac.shape[0] >= 600 else 3)
    want = pr.assemble([edges], off, 3.0)
    got, st = _build(dev, "grid", frac, lat, off)
    _equal(got, want, which)
    assert st[:2] == [0, 1] and st[4] == 0 and st[3] < frac.shape[0] * (frac.shape[0] + 1) // 2
    if which == "cutoff edge":
        kept = set(zip(edges[0].tolist(), edges[1].tolist()))
        named = [(2 * k, 2 * k + 1) in kept for k in range(64)]
        assert any(named) and not all(named)                                  # the yardstick keeps some and drops some


def test_a_structure_far_from_the_origin_takes_the_walk(dev):
    """frac + 2^20 is outside the range the pruning rule is proved for (|frac| <= 64): the walk, in forced mode too"""
    rng = _rng(33)
    frac = (rng.random((40, 3)) + 2.0 ** 20).astype(F32)
    frac, lat, off = _single(frac, gr.cubic(6.0))
    want = pr.reference_edges(frac, lat, off, 0.0, 3.0)
    got, st = _build(dev, "grid", frac, lat, off, 0.0)
    _equal(got, want, "frac + 2^20")
    assert want["pairs"].shape[1] > 0 and st == [1, 0, 40 * 41 // 2, 0, 1]
    big = (rng.random((300, 3)) + 2.0 ** 20).astype(F32)                       # ... and in automatic mode when it would qualify
    bf, bl, bo = _single(big, gr.cubic(16.0))
    got, st = _build(dev, None, bf, bl, bo)
    _equal(got, pr.reference_edges(bf, bl, bo, 0.5, 3.0, extra=1), "frac + 2^20, automatic")
    assert st == [1, 0, 300 * 301 // 2, 0, 1]
    got, st = _build(dev, "grid", *_single(rng.random((40, 3)).astype(F32), gr.cubic(6.0)), 0.0, 3.0, (0, 0, 0))
    assert st == [1, 0, 40 * 41 // 2, 0, 1]                                    # no periodic axis: no h, the walk


def test_open_axes(dev):
    rng = _rng(37)
    slab = rng.random((400, 3)).astype(F32)
    L = np.diag([22.0, 19.0, 6.0]).astype(F32)
    frac, lat, off = _single(slab, L)
    want = pr.assemble([pr.structure_edges(slab, L, 0.5, 3.0, (1, 1, 0))], off, 3.0)
    got, st = _build(dev, None, frac, lat, off, pbc=(1, 1, 0))
    _equal(got, want, "slab, automatic mode")
    assert st[:2] == [0, 1] and 0 < st[3] < 400 * 401 // 4 and np.all(got["shift"][:, 2] == 0) and want["pairs"].shape[1] > 0
    distinct = _structures(rng, "cubic", _sizes(rng, 12))
    order = list(range(12))
    frac, lat, off = _batch(distinct, order)
    want = _expected(distinct, order, off, 0.0, 3.0, (0, 1, 1))
    got, st = _build(dev, "grid", frac, lat, off, 0.0, pbc=(0, 1, 1))
    _equal(got, want, "pbc (0, 1, 1), forced grid")
    assert st[:2] == [0, 12] and np.all(got["shift"][:, 0] == 0) and np.any(got["shift"] != 0)


def test_4096_atoms_grid_equals_walk(dev):
    frac, lat, off = _single(_rng(41).random((4096, 3)).astype(F32), gr.cubic(38.4))
    grid, sg = _build(dev, "grid", frac, lat, off)
    walk, sw = _build(dev, "walk", frac, lat, off)
    _same_arrays(grid, walk, "4096 atoms")
    print(f"4096 atoms: {grid['pairs'].shape[1]} edges, walk {sw[2]} pairs, grid {sg[3]} pairs")
    assert grid["pairs"].shape[1] > 0 and grid["first_count"].sum() == grid["pairs"].shape[1]
    assert sg[:2] == [0, 1] and sw[:2] == [1, 0] and sw[2] == 4096 * 4097 // 2 and sg[3] <= sw[2] // 4


GUARD = 16                      # words; torch allocations are 256-byte aligned, so word GUARD is 8-byte aligned, word GUARD + 1 is not
FENCE = 0x5A5A5A5A


class _Guarded:
    """`words` 4-byte words of device memory between two fences of GUARD words, the first one 8-byte aligned or (odd) only
    4-byte aligned"""

    def __init__(self, dev, words, dtype, odd, fill):
        import torch

        self.lo = GUARD + (1 if odd else 0)
        self.words = words
        self.raw = torch.full((self.lo + words + GUARD,), FENCE, dtype=torch.int32, device=dev)
        self.view = self.raw[self.lo:self.lo + words].view(dtype)
        self.view.copy_(fill if hasattr(fill, "shape") else torch.full((words,), fill, dtype=dtype, device=dev))
        assert (self.view.data_ptr() % 8 == 4) == bool(odd) and self.view.data_ptr() % 4 == 0

    def fences_intact(self):
        import torch

        return bool(torch.all(self.raw[:self.lo] == FENCE)) and bool(torch.all(self.raw[self.lo + self.words:] == FENCE))


def test_guard_words_alignment_size_query_and_byte_identical_builds(dev):
    import torch
    from athena_amd import _capi

    rng = _rng(43)
    small = _structures(rng, "cubic", [12, 9])
    distinct = [small[0], (rng.random((300, 3)).astype(F32), gr.cubic(16.0)), small[1]]
    frac, lat, off = _batch(distinct, [0, 1, 2])
    base, st = _build(dev, None, frac, lat, off)
    assert st[:2] == [2, 1]
    B, n, E = lat.shape[0], frac.shape[0], base["pairs"].shape[1]
    cap = E + 64
    pbc3 = np.ones(3, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    names = ("frac", "lat", "pairs", "feature", "vec", "shift", "first_count")
    previous = None
    for odd in (None,) + names:
        f32, i32 = torch.float32, torch.int32
        bufs = {"frac": _Guarded(dev, 3 * n, f32, odd == "frac", torch.from_numpy(frac.ravel()).to(dev)),
                "lat": _Guarded(dev, 9 * B, f32, odd == "lat", torch.from_numpy(lat.ravel()).to(dev)),
                "pairs": _Guarded(dev, 2 * cap, i32, odd == "pairs", -7), "feature": _Guarded(dev, cap, f32, odd == "feature", np.nan),
                "vec": _Guarded(dev, 3 * cap, f32, odd == "vec", np.nan), "shift": _Guarded(dev, 3 * cap, i32, odd == "shift", -99),
                "first_count": _Guarded(dev, n, i32, odd == "first_count", -5)}
        p = {k: C.c_void_p(v.view.data_ptr()) for k, v in bufs.items()}
        head = (B, n, vp(off), p["frac"], p["lat"], vp(pbc3), 0.5, 3.0)
        q, E2 = C.c_int64(-1), C.c_int64(-1)
        eoff = np.full(B + 1, -1, np.int64)
        _capi.call("athena_mp_periodic_pairs", *head, None, None, None, None, None, 0, C.byref(q), None)
        _capi.call("athena_mp_periodic_pairs", *head, p["pairs"], p["feature"], p["vec"], p["shift"], p["first_count"], cap, C.byref(E2),
                   vp(eoff))
        torch.cuda.synchronize()
        assert q.value == E2.value == E, odd                                   # the size query agrees with the fill
        assert _stats()[:2] == [2, 1]
        for k, v in bufs.items():
            assert v.fences_intact(), f"{k} (odd: {odd}): a guard word was written"
        out = {k: bufs[k].view.cpu().numpy() for k in names[2:]}
        assert np.array_equal(out["pairs"][:2 * E].reshape(E, 2).T, base["pairs"]) and np.all(out["pairs"][2 * E:] == -7)
        assert np.array_equal(out["feature"][:E], base["feature"]) and np.isnan(out["feature"][E:]).all()
        assert np.array_equal(out["vec"][:3 * E].reshape(E, 3), base["vec"]) and np.isnan(out["vec"][3 * E:]).all()
        assert np.array_equal(out["shift"][:3 * E].reshape(E, 3), base["shift"]) and np.all(out["shift"][3 * E:] == -99)
        assert np.array_equal(out["first_count"], base["first_count"]) and np.array_equal(eoff, base["edge_offsets"])
        if previous is not None:                                               # two builds are byte-identical
            assert all(out[k].tobytes() == previous[k].tobytes() for k in out)
        previous = out


@pytest.mark.parametrize("loops", [False, True])
def test_handle_from_the_1000_atom_cell(dev, loops):
    from athena_amd import DeviceGraph

    a, _, ea, _ = _large()
    frac, lat, off = _single(*a)
    want = pr.assemble([ea], off, 3.0)
    ref = DeviceGraph.from_edges(1000, want["pairs"], add_self_loops=loops)
    one, feature, vec, voff, eoff = DeviceGraph.from_structures(frac, lat, off, 0.5, 3.0, add_self_loops=loops)
    assert _stats()[:2] == [0, 1]
    assert np.array_equal(feature.cpu().numpy(), want["feature"]) and np.array_equal(vec.cpu().numpy(), want["vec"])
    assert np.array_equal(eoff, want["edge_offsets"])
    _same(one, ref)
    one.close()
    ref.close()


def test_builds_through_the_grid_do_not_leak_device_memory(dev):
    import torch
    from athena_amd import DeviceGraph

    a = _large()[0]
    frac, lat, off = _single(*a)
    fd, ld = torch.from_numpy(frac).to(dev), torch.from_numpy(lat).to(dev)

    def cycle():
        g, feature, vec, _, _ = DeviceGraph.from_structures(fd, ld, off, 0.5, 3.0, add_self_loops=True)
        assert feature.shape[0] > 1000
        g.close()
        del feature, vec

    cycle()
    assert _stats()[:2] == [0, 1]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(40):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 8 << 20, f"{(free0 - free1) >> 20} MiB of device memory lost over 40 builds through the grid"


def test_host_and_fortran_callers_under_forced_grid(dev, tmp_path):
    from athena_amd.graph import graph_type

    if not os.path.exists(RUNNER):
        pytest.fail("periodic_graph_run is not built: __graft_entry__.build() compiles the Fortran host side")
    rng = _rng(47)
    distinct = _structures(rng, ("cubic", "small", "skewed"), _sizes(rng, 20), max_range=8)
    distinct.append((rng.random((300, 3)).astype(F32), gr.cubic(16.0)))
    order = list(range(21)); order[7] = None
    frac, lat, off = _batch(distinct, order)
    B, n, loops, pbc = lat.shape[0], frac.shape[0], 1, (1, 1, 1)
    res = {}
    for mode in ("walk", "grid"):
        with _route(mode):
            g = graph_type(); g.set_num_vertices(n, 1)
            res[mode] = (g, *g.generate_periodic_adjacency_device(frac, lat, off, 0.5, 3.0, pbc=pbc, add_self_loops=True))
            st = _stats()
            assert (st[:2] == [0, 20]) if mode == "grid" else (st[:2] == [20, 0])
    (gw, *aw), (g, *ag) = res["walk"], res["grid"]
    assert np.array_equal(gw.adj_ia, g.adj_ia) and np.array_equal(gw.adj_ja, g.adj_ja) and all(np.array_equal(x, y) for x, y in zip(aw, ag))
    feature, vec, first, eoff = ag
    want = _expected(distinct, order, off, 0.5, 3.0)
    assert np.array_equal(feature, want["feature"]) and np.array_equal(vec, want["vec"]) and np.array_equal(first, want["first_count"])
    assert np.array_equal(eoff, want["edge_offsets"]) and g.num_edges == want["pairs"].shape[1]
    # the Fortran program as a child process with the switch in its environment
    case, out_path = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(case, "wb") as f:
        f.write(np.asarray([B, n, loops, *pbc], np.int32).tobytes() + np.asarray([0.5, 3.0], F32).tobytes() + off.tobytes()
                + frac.tobytes() + lat.tobytes())
    out = subprocess.run([RUNNER, case, out_path], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ATHENA_MP_PERIODIC_ROUTE="grid"))
    assert out.returncode == 0, f"periodic_graph_run failed ({out.returncode}): {out.stderr[-2000:]}"
    b = open(out_path, "rb").read()
    hB, hn, nnz, E = np.frombuffer(b, np.int32, 4)
    assert (hB, hn, nnz, E) == (B, n, g.nnz, g.num_edges)
    o = 16
    ia = np.frombuffer(b, np.int32, n + 1, o); o += 4 * (n + 1)
    ja = np.frombuffer(b, np.int32, 2 * nnz, o).reshape((2, nnz), order="F"); o += 8 * nnz
    ff = np.frombuffer(b, F32, E, o); o += 4 * E
    vf = np.frombuffer(b, F32, 3 * E, o).reshape(E, 3); o += 12 * E
    fc = np.frombuffer(b, np.int32, n, o); o += 4 * n
    eo = np.frombuffer(b, np.int64, B + 1, o); o += 8 * (B + 1)
    assert o == len(b)
    assert np.array_equal(ia, g.adj_ia) and np.array_equal(ja, g.adj_ja)
    assert np.array_equal(ff, feature) and np.array_equal(vf, vec) and np.array_equal(fc, first) and np.array_equal(eo, eoff)


def test_refusals_under_forced_grid_are_those_of_the_walk(dev):
    import torch
    from athena_amd import _capi

    rng = _rng(71)
    distinct = _structures(rng, "cubic", _sizes(rng, 10))
    order = list(range(10))
    frac, lat, off = _batch(distinct, order)
    want = _expected(distinct, order, off, 0.5, 3.0)
    E = want["pairs"].shape[1]
    f_nan = frac.copy(); f_nan[off[6] + 1, 2] = np.nan; f_nan[off[8], 0] = np.nan
    L_small = lat.copy(); L_small[2] = np.eye(3, dtype=F32) * F32(0.09)
    crowd = (rng.random((2000, 3)).astype(F32), np.tile((np.eye(3) * 0.1).astype(F32), (200, 1, 1)), np.arange(201) * 10)
    cases = [
        (dict(frac=f_nan), r"structure 7: frac\(3,%d\) = -?nan is not finite" % (off[6] + 2)),
        (dict(lat=L_small), r"structure 3: half-range 33 on axis 1 is above 31: the cell is too small"),
        (dict(capacity=E - 1, fill=True), r"buffers hold %d edges, the batch has %d" % (E - 1, E)),
        (dict(frac=crowd[0], lat=crowd[1], off=crowd[2]), r"1\d{9} edges among 2000 atoms: more than 2\^31 CSR entries"),
    ]
    for kw, pattern in cases:
        said = {}
        for mode in ("walk", "grid"):
            with _route(mode):
                with pytest.raises(_capi.AthenaMPError, match=pattern) as err:
                    _pairs_call(dev, kw.get("frac", frac), kw.get("lat", lat), kw.get("off", off), 0.5, 3.0, (1, 1, 1), kw.get("capacity"),
                                kw.get("fill", False))
                said[mode] = str(err.value)
                got = _pairs_call(dev, frac, lat, off, 0.5, 3.0)               # the library is usable after each
                _equal(got, want, f"after a refusal under {mode}")
                assert _stats()[:2] == ([0, 10] if mode == "grid" else [10, 0])
        assert said["walk"] == said["grid"]
    with _route("cells"):
        with pytest.raises(_capi.AthenaMPError, match=r"ATHENA_MP_PERIODIC_ROUTE = 'cells' is none of auto, walk, grid"):
            _pairs_call(dev, frac, lat, off, 0.5, 3.0, fill=False)
    torch.cuda.synchronize()
    _equal(_pairs_call(dev, frac, lat, off, 0.5, 3.0), want, "after the refusals")


def test_a_candidate_list_that_cannot_be_held_is_refused_by_its_count_pass(dev):
    """65 536 atoms in a cell with fewer than three cells per axis, forced grid: every pair i <= j is a candidate, 2^31 + 2^15 of
    them; the count pass finds it (a binary search per atom), names the structure, and nothing of that size is allocated"""
    import torch
    from athena_amd import _capi

    rng = _rng(83)
    small = (rng.random((10, 3)).astype(F32), gr.cubic(6.0))
    frac, lat, off = _batch([small, (rng.random((65536, 3)).astype(F32), gr.cubic(8.9))], [0, 1])
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with _route("grid"):
        with pytest.raises(_capi.AthenaMPError, match=r"structure 2: the cell grid's candidate list reaches 2147516471 atom pairs"):
            _pairs_call(dev, frac, lat, off, 0.5, 3.0, fill=False)
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 8 << 20
    f, L, o = _single(*small)
    _equal(_pairs_call(dev, f, L, o, 0.5, 3.0), pr.reference_edges(f, L, o, 0.5, 3.0), "after the refusal")
