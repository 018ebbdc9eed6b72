"""GPU: the bond-angle triplets of a neighbour graph with their gradients (athena_amd/csrc/triplets.hip) against the transcription of
the definition (tests/triplets_reference.py, its vectorised form; tests/test_triplets.py holds it to its plain loops).  The graphs
come from the library's own builders, whose handles are exported and handed to the yardstick: the golden head fixture and random
periodic batches (one-atom structures: self-image entries only; cells below the cutoff: multi-edges; empty structures; self loops),
radius clouds at dim 1, 2 and 3 with planted coincident points (den == 0), a hub row of 150 participants beside rows of 0, 1 and 2,
and a star whose count passes 2^31.  Every comparison is np.array_equal on the bits; every output is pre-filled with NaN or a
poison integer, so an element that was not written shows."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import geometry_reference as gr
import interp_reference as ir
import periodic_reference as pr
import pool_reference as pl
import triplets_reference as tr
from helpers import assert_close_elementwise

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "msgpass_chemical_head.xyz")
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "triplets_run")
CMIN, CMAX = 0.5, 3.0
POISON = 0x5A5A5A5A
INF = float("inf")
# case -> the finite three-body cutoff that goes with +inf
CASES = {"fixture": 2.2, "periodic": 2.0, "periodic_loops": 2.0, "cloud1": 0.05, "cloud2": 0.16, "cloud3": 0.3, "cloud3_loops": 0.3,
         "hub": 1.1}
HANDLE_ARRAYS = ("rowptr", "col", "eid", "coef", "t_rowptr", "t_src", "t_eid", "t_coef", "e_rowptr", "e_row", "e_entry", "deg_row",
                 "deg_col")

vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def _rng(seed):
    return np.random.default_rng(seed)


def up(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same(t, want):
    got = t.cpu().numpy()
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def periodic_batch(seed):
    """frac, lat, offsets: small cells of 1, 2 and 3 atoms (edges below the cutoff: self images, several edges per pair), cubic cells
    of 1, 2, 9 and 14 atoms, an empty structure in the middle and one at the end"""
    rng = _rng(seed)
    rows, lats = [], []
    for kind, m in (("small", 1), ("cubic", 9), ("small", 3), ("cubic", 0), ("cubic", 1), ("small", 2), ("cubic", 14), ("cubic", 2),
                    ("cubic", 0)):
        rows.append(rng.random((m, 3)).astype(np.float32))
        lats.append(pr.random_cell(rng, kind))
    off = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int32)
    return np.concatenate(rows).astype(np.float32), np.array(lats, np.float32).reshape(-1, 3, 3), off


def cloud_points(dim):
    """points in the unit cube with every seventh one on top of its predecessor: coords = 0 along that edge, den == 0"""
    rng = _rng(8500 + dim)
    p = rng.random(({1: 70, 2: 90, 3: 120}[dim], dim)).astype(np.float32)
    p[6::7] = p[5::7][:p[6::7].shape[0]]
    return p


HUB_LEAVES = 150


def hub_edges():
    """(n, index_list [2, E] 1-based, vec [E, 3]): vertex 0 joined to 150 leaves, three vertices without an edge, a chain of three
    (its middle holds two entries); vec drawn with lengths 0.6 .. 1.4, so that the finite cutoff drops about a third of the hub's row"""
    rng = _rng(8600)
    pairs = [(1, 2 + k) for k in range(HUB_LEAVES)] + [(HUB_LEAVES + 5, HUB_LEAVES + 6), (HUB_LEAVES + 6, HUB_LEAVES + 7)]
    u = rng.standard_normal((len(pairs), 3))
    vec = (u / np.sqrt((u * u).sum(axis=1, keepdims=True)) * rng.uniform(0.6, 1.4, (len(pairs), 1))).astype(np.float32)
    return HUB_LEAVES + 7, np.asfortranarray(np.array(pairs, np.int32).T), vec


class Case:
    def __init__(self, g, vec, dim, extra=None):
        self.g, self.vec, self.dim, self.extra = g, vec, dim, extra
        self.E, self.nnz = g.n_edge_cols, g.nnz
        self.A = {k: g.export(k) for k in ("rowptr", "col", "eid", "e_rowptr", "e_row", "e_entry")}
        self.vec_h = vec.cpu().numpy() if vec is not None else None


@functools.lru_cache(None)
def case(name):
    import torch
    from athena_amd import DeviceGraph, io

    dev = torch.device("cuda:0")
    loops = name.endswith("_loops")
    if name == "fixture":
        frac, lat, off = io.structures_from_frames(io.read_extxyz(FIXTURE))
        g, _, vec, voff, eoff = DeviceGraph.from_structures(frac, lat, off, CMIN, CMAX)
        assert g.n_edge_cols == 1849
        return Case(g, vec, 3, (lat, voff, eoff))
    if name.startswith("periodic"):
        frac, lat, off = periodic_batch(8400)
        g, _, vec, voff, eoff = DeviceGraph.from_structures(frac, lat, off, 0.0, 2.5, add_self_loops=loops)
        return Case(g, vec, 3, (lat, voff, eoff))
    if name.startswith("cloud"):
        dim = int(name[5])
        g, coords = DeviceGraph.from_points(cloud_points(dim), {1: 0.06, 2: 0.2, 3: 0.35}[dim], add_self_loops=loops)
        return Case(g, coords, dim)
    assert name == "hub"
    n, idx, vec = hub_edges()
    return Case(DeviceGraph.from_edges(n, idx), up(vec, dev), 3)


@functools.lru_cache(None)
def reference(name, cutoff3):
    c = case(name)
    rng = _rng(8700 + len(name))
    return tr.everything(c.A, c.E, c.vec_h, c.dim, cutoff3, lambda T: rng.standard_normal(T).astype(np.float32))


def inputs_are_what_the_test_needs(name, cutoff3):
    c, want = case(name), reference(name, cutoff3)
    rows, col, eid = tr.rows_of(c.A["rowptr"]), c.A["col"], c.A["eid"]
    m = np.bincount(rows[want["take"]], minlength=c.g.n_rows)
    T = want["pairs"].shape[0]
    assert T == int((m * (m - 1)).sum()) > 0
    if np.isfinite(cutoff3):
        assert 0 < want["take"].sum() < (eid >= 0).sum(), "the finite cutoff drops some entries and keeps some"
    if name.startswith("periodic"):
        assert ((rows == col) & (eid >= 0)).any(), "self-image entries"
        first = int(np.nonzero(np.diff(c.A["rowptr"]) > 0)[0][0])
        r0 = slice(c.A["rowptr"][first], c.A["rowptr"][first + 1])
        assert (col[r0][eid[r0] >= 0] == first).all(), "the one-atom structure holds self-image entries only"
        multi = (rows[1:] == rows[:-1]) & (col[1:] == col[:-1]) & (eid[1:] != eid[:-1]) & (eid[1:] >= 0) & (eid[:-1] >= 0)
        assert multi.any(), "multi-edges"
        assert (np.diff(c.A["rowptr"]) == (1 if name.endswith("_loops") else 0)).any(), "atoms without a neighbour"
        assert (eid < 0).any() == name.endswith("_loops")
    if name.startswith("cloud"):
        flat = ~(want["dir"][want["pairs"][:, 0]].any(axis=1) & want["dir"][want["pairs"][:, 1]].any(axis=1))
        assert flat.sum() >= 4 and not bits(want["cos"])[flat].any(), "coincident points: den == 0 gives +0"
    if name == "hub":
        assert m[0] > 64 and m[0] * (m[0] - 1) > 4096, "more than a wave holds in registers, more than one work item"
        if np.isinf(cutoff3):
            assert m[0] * (m[0] - 1) == 22350 and set(m[1:].tolist()) == {0, 1, 2}


def build(g, dim, vec, cutoff3, dev, want_pairs=True, want_rowptr=True):
    """athena_mp_triplet_pairs: size query, then the fill into poisoned buffers -> (T, pairs [T, 2], rowptr [nnz + 1])"""
    import torch
    from athena_amd import _capi

    _capi.use_torch_stream()
    T = C.c_int64(-1)
    _capi.call("athena_mp_triplet_pairs", g.handle, dim, ptr(vec), cutoff3, None, 0, None, C.byref(T))
    pairs = torch.full((T.value, 2), POISON, dtype=torch.int32, device=dev)
    rowptr = torch.full((g.nnz + 1,), POISON, dtype=torch.int32, device=dev)
    T2 = C.c_int64(-1)
    _capi.call("athena_mp_triplet_pairs", g.handle, dim, ptr(vec), cutoff3, ptr(pairs) if want_pairs else None, T.value,
               ptr(rowptr) if want_rowptr else None, C.byref(T2))
    torch.cuda.synchronize()
    assert T2.value == T.value, "the size query and the fill disagree"
    return T.value, pairs, rowptr


def triplet_handle(nnz, pairs):
    """athena_mp_graph_create_bipartite_dev on the device list"""
    from athena_amd import DeviceGraph, _capi

    T = int(pairs.shape[0])
    tg = DeviceGraph.__new__(DeviceGraph)
    ia, h = np.empty(nnz + 1, np.int32), C.c_void_p()
    _capi.call("athena_mp_graph_create_bipartite_dev", nnz, nnz, T, ptr(pairs), vp(ia), None, 0, C.byref(h))
    tg.handle, tg.n_rows, tg.n_cols, tg.nnz, tg.n_edge_cols = h, nnz, nnz, T, T
    return tg, ia


def device_chain(c, tg, dcos, dev):
    """the four geometry entries into NaN-filled outputs -> dir, cos, ddir, dvec"""
    import torch
    from athena_amd import _capi

    nan = lambda *shape: torch.full(shape, np.nan, dtype=torch.float32, device=dev)
    dirs, cosv, ddir, dvec = nan(c.nnz, c.dim), nan(tg.n_edge_cols), nan(c.nnz, c.dim), nan(c.E, c.dim)
    _capi.use_torch_stream()
    _capi.call("athena_mp_entry_vectors_fwd", c.g.handle, c.dim, ptr(c.vec), ptr(dirs))
    _capi.call("athena_mp_triplet_cos_fwd", tg.handle, c.dim, ptr(dirs), ptr(cosv))
    _capi.call("athena_mp_triplet_cos_bwd", tg.handle, c.dim, ptr(dirs), ptr(cosv), ptr(dcos), ptr(ddir))
    _capi.call("athena_mp_entry_vectors_bwd", c.g.handle, c.dim, ptr(ddir), ptr(dvec))
    torch.cuda.synchronize()
    return dirs, cosv, ddir, dvec


# ---- every entry against the yardstick -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("finite", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_every_array_equals_the_yardstick(dev, name, finite):
    from athena_amd import DeviceGraph

    cutoff3 = CASES[name] if finite else INF
    c, want = case(name), reference(name, cutoff3)
    inputs_are_what_the_test_needs(name, cutoff3)
    vec_before = c.vec.clone()
    T, pairs, rowptr = build(c.g, c.dim, c.vec, cutoff3, dev)
    print(f"{name}, cutoff3 = {cutoff3}: {c.nnz} entries, {T} triplets")
    assert T == want["pairs"].shape[0]
    assert np.array_equal(pairs.cpu().numpy(), (want["pairs"] + 1).astype(np.int32)), "pairs"
    assert np.array_equal(rowptr.cpu().numpy(), want["rowptr"].astype(np.int32)), "rowptr"
    # the triplet handle, array for array what athena_mp_graph_create builds from the yardstick's CSR
    tg, ia = triplet_handle(c.nnz, pairs)
    ref_ia, ref_ja = tr.triplet_csr(want["pairs"], want["rowptr"])
    assert np.array_equal(ia, ref_ia)
    TA = want["T"]
    rg = DeviceGraph(ref_ia, ref_ja, n_cols=c.nnz, n_edge_cols=T, row_deg=np.diff(TA["rowptr"]), col_deg=np.diff(TA["t_rowptr"]))
    for key in HANDLE_ARRAYS:
        assert np.array_equal(bits(tg.export(key)), bits(rg.export(key))), f"the triplet handle's {key}"
    for key in ("rowptr", "col", "eid", "t_rowptr", "t_src", "t_eid"):
        assert np.array_equal(tg.export(key), TA[key]), key
    dirs, cosv, ddir, dvec = device_chain(c, tg, up(want["dcos"], dev), dev)
    for key, got in (("dir", dirs), ("cos", cosv), ("ddir", ddir), ("dvec", dvec)):
        assert same(got, want[key]), f"{key} differs from the yardstick"
    assert same(c.vec, vec_before.cpu().numpy()), "vec changed"
    from athena_amd.geometry import triplet_stats

    build(c.g, c.dim, c.vec, cutoff3, dev)
    m = np.bincount(tr.rows_of(c.A["rowptr"])[want["take"]], minlength=c.g.n_rows)
    assert triplet_stats() == (T, int(want["take"].sum()), int(m.max() * (m.max() - 1)))


@pytest.mark.parametrize("name", ["fixture", "hub", "cloud2"])
def test_the_python_mirror_returns_the_same_and_two_builds_the_same_bytes(dev, name):
    from athena_amd import DeviceGraph
    from athena_amd.geometry import entry_vectors, entry_vectors_grad, triplet_cos, triplet_cos_grad

    c = case(name)
    for cutoff in (None, CASES[name]):
        want = reference(name, INF if cutoff is None else cutoff)
        tg, dirs = DeviceGraph.from_triplets(c.g, c.vec, cutoff)
        assert (tg.n_rows, tg.n_cols, tg.nnz, tg.n_edge_cols) == (c.nnz, c.nnz, want["pairs"].shape[0], want["pairs"].shape[0])
        assert same(dirs, want["dir"]) and same(entry_vectors(c.g, c.vec), want["dir"])
        for key in ("rowptr", "col", "eid", "t_rowptr", "t_src", "t_eid"):
            assert np.array_equal(tg.export(key), want["T"][key]), key
        cosv = triplet_cos(tg, dirs)
        ddir = triplet_cos_grad(tg, dirs, cosv, up(want["dcos"], dev))
        assert same(cosv, want["cos"]) and same(ddir, want["ddir"]) and same(entry_vectors_grad(c.g, ddir), want["dvec"])
        first, second = build(c.g, c.dim, c.vec, INF if cutoff is None else cutoff, dev), build(c.g, c.dim, c.vec, INF if cutoff is None else cutoff, dev)
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(first[1:], second[1:]))
    if name == "hub":                                                # without vec: the integer results alone
        tg, none = DeviceGraph.from_triplets(c.g)
        assert none is None and np.array_equal(tg.export("col"), reference(name, INF)["T"]["col"])
        with pytest.raises(ValueError):
            DeviceGraph.from_triplets(c.g, None, 1.0)


def test_a_size_query_and_an_absent_output_leave_the_buffers_untouched(dev):
    c, want = case("cloud3"), reference("cloud3", INF)
    T, pairs, rowptr = build(c.g, c.dim, c.vec, INF, dev, want_rowptr=False)
    assert np.array_equal(pairs.cpu().numpy(), (want["pairs"] + 1).astype(np.int32)) and (rowptr.cpu().numpy() == POISON).all()
    T, pairs, rowptr = build(c.g, c.dim, c.vec, INF, dev, want_pairs=False)
    assert np.array_equal(rowptr.cpu().numpy(), want["rowptr"].astype(np.int32)) and (pairs.cpu().numpy() == POISON).all()
    # vec may be absent without a cutoff: the same list
    T2, pairs2, _ = build(c.g, c.dim, None, INF, dev)
    assert T2 == T and np.array_equal(pairs2.cpu().numpy(), (want["pairs"] + 1).astype(np.int32))


# ---- the count past 2^31 ---------------------------------------------------------------------------------------------------------
def _star(leaves):
    from athena_amd import DeviceGraph

    idx = np.asfortranarray(np.stack([np.ones(leaves, np.int32), np.arange(2, leaves + 2, dtype=np.int32)]))
    return DeviceGraph.from_edges(leaves + 1, idx)


def test_a_star_at_the_limit_is_counted_and_one_past_it_refused(dev):
    from athena_amd import _capi
    from athena_amd.geometry import triplet_stats

    _capi.use_torch_stream()
    T = C.c_int64(-1)
    g = _star(46341)
    _capi.call("athena_mp_triplet_pairs", g.handle, 3, None, INF, None, 0, None, C.byref(T))
    assert T.value == 2147441940 == tr.star_count(46341)
    assert triplet_stats() == (2147441940, 2 * 46341, 2147441940)
    g2 = _star(46342)
    with pytest.raises(_capi.AthenaMPError, match="2147534622"):
        _capi.call("athena_mp_triplet_pairs", g2.handle, 3, None, INF, None, 0, None, C.byref(T))
    assert T.value == 0
    _capi.call("athena_mp_triplet_pairs", g.handle, 3, None, INF, None, 0, None, C.byref(T))      # the library stays usable
    assert T.value == 2147441940
    c = case("cloud3")
    assert build(c.g, c.dim, c.vec, INF, dev)[0] == reference("cloud3", INF)["pairs"].shape[0]


# ---- refusals and empty inputs ---------------------------------------------------------------------------------------------------
def test_every_refusal_has_a_message_and_the_library_stays_usable(dev):
    import torch
    from athena_amd import DeviceGraph, _capi

    c, want = case("cloud3"), reference("cloud3", INF)
    T = C.c_int64(-1)
    q = lambda g, dim, vec, cutoff3, pairs=None, cap=0: _capi.call("athena_mp_triplet_pairs", g.handle, dim, ptr(vec), cutoff3, ptr(pairs),
                                                                   cap, None, C.byref(T))
    n, idx, _ = hub_edges()
    kipf = DeviceGraph.from_edges(n, idx, with_edge_ids=False)
    rng = _rng(8800)
    two_sets, coords, _ = DeviceGraph.from_point_sets(rng.random((30, 3)).astype(np.float32), rng.random((20, 3)).astype(np.float32), 0.5)
    _capi.use_torch_stream()
    for args, text in (((kipf, 3, None, INF), "no edge columns"), ((two_sets, 3, coords, INF), "not square"),
                       ((c.g, 0, c.vec, INF), "dim = 0"), ((c.g, 4, c.vec, INF), "dim = 4"), ((c.g, 3, c.vec, float("nan")), "cutoff3"),
                       ((c.g, 3, c.vec, 0.0), "cutoff3"), ((c.g, 3, c.vec, -1.0), "cutoff3"), ((c.g, 3, None, 0.3), "needs vec")):
        with pytest.raises(_capi.AthenaMPError, match=text):
            q(*args)
    Tw = want["pairs"].shape[0]
    small = torch.full((Tw - 1, 2), POISON, dtype=torch.int32, device=dev)
    with pytest.raises(_capi.AthenaMPError, match=f"holds {Tw - 1} triplets, the graph has {Tw}"):
        q(c.g, 3, c.vec, INF, small, Tw - 1)
    torch.cuda.synchronize()
    assert (small.cpu().numpy() == POISON).all(), "a refused fill wrote into the buffer"
    # the cos entries: a square handle with two entries per edge column, and a two-set handle
    f = torch.zeros((max(c.nnz, 64), 3), dtype=torch.float32, device=dev)
    for g in (c.g, two_sets):
        with pytest.raises(_capi.AthenaMPError):
            _capi.call("athena_mp_triplet_cos_fwd", g.handle, 3, ptr(f), ptr(f))
        with pytest.raises(_capi.AthenaMPError):
            _capi.call("athena_mp_triplet_cos_bwd", g.handle, 3, ptr(f), ptr(f), ptr(f), ptr(f))
    for entry in ("athena_mp_entry_vectors_fwd", "athena_mp_entry_vectors_bwd"):
        with pytest.raises(_capi.AthenaMPError, match="not square"):
            _capi.call(entry, two_sets.handle, 3, ptr(f), ptr(f))
        with pytest.raises(_capi.AthenaMPError, match="dim = 4"):
            _capi.call(entry, c.g.handle, 4, ptr(f), ptr(f))
    assert build(c.g, c.dim, c.vec, INF, dev)[0] == Tw


def test_no_entries_and_no_triplets_succeed(dev):
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.geometry import entry_vectors_grad, triplet_cos, triplet_cos_grad

    empty = DeviceGraph.from_edges(5, np.zeros((2, 0), np.int32))
    assert empty.nnz == 0
    T, pairs, rowptr = build(empty, 3, None, INF, dev)
    assert T == 0 and rowptr.cpu().numpy().tolist() == [0]
    tg, dirs = DeviceGraph.from_triplets(empty, torch.zeros((0, 3), dtype=torch.float32, device=dev), 1.0)
    assert (tg.n_rows, tg.nnz) == (0, 0) and tuple(dirs.shape) == (0, 3)
    # a perfect matching with self loops: every row holds one participant
    idx = np.asfortranarray(np.array([[1, 3, 5], [2, 4, 6]], np.int32))
    g = DeviceGraph.from_edges(7, idx, add_self_loops=True)
    vec = up(_rng(8900).standard_normal((3, 3)).astype(np.float32), dev)
    T, pairs, rowptr = build(g, 3, vec, INF, dev)
    assert T == 0 and not rowptr.cpu().numpy().any()
    tg, dirs = DeviceGraph.from_triplets(g, vec)
    A = {k: g.export(k) for k in ("rowptr", "col", "eid", "e_rowptr", "e_row", "e_entry")}
    assert tg.n_rows == g.nnz == 13 and tg.nnz == 0 and same(dirs, tr.entry_vectors(A, vec.cpu().numpy(), 3))
    cosv = triplet_cos(tg, dirs)
    ddir = triplet_cos_grad(tg, dirs, cosv, cosv, out=torch.full((13, 3), np.nan, dtype=torch.float32, device=dev))
    assert tuple(cosv.shape) == (0,) and not bits(ddir.cpu().numpy()).any(), "an entry in no triplet gives +0"
    assert not bits(entry_vectors_grad(g, ddir).cpu().numpy()).any()


# ---- the row kernels on the triplet handle ----------------------------------------------------------------------------------------
def test_the_row_kernels_run_on_the_triplet_handle_and_the_chain_reaches_the_atoms(dev):
    from athena_amd import DeviceGraph
    from athena_amd.geometry import (entry_vectors_grad, interpolate, pool_max, structures_grad, triplet_cos, triplet_cos_grad)

    c, want = case("periodic"), reference("periodic", 2.0)
    lat, voff, eoff = c.extra
    tg, dirs = DeviceGraph.from_triplets(c.g, c.vec, 2.0)
    cosv = triplet_cos(tg, dirs)
    assert same(cosv, want["cos"])
    TA = want["T"]
    msg = _rng(9000).standard_normal((c.nnz, 5)).astype(np.float32)          # a message per entry (bond)
    y = interpolate(tg, cosv, up(msg, dev))                                    # sum over k' of cos(k, k') m[k']
    assert same(y, ir.fwd(TA, want["cos"], msg))
    top, arg = pool_max(tg, edges=cosv[:, None].contiguous())
    ref_top, ref_arg = pl.edges_fwd(TA, want["cos"][:, None])
    assert same(top, ref_top) and np.array_equal(arg.cpu().numpy(), ref_arg)
    ddir = triplet_cos_grad(tg, dirs, cosv, up(want["dcos"], dev))
    dvec = entry_vectors_grad(c.g, ddir)
    assert same(dvec, want["dvec"]) and np.abs(want["dvec"]).max() > 0
    got = structures_grad(c.g, lat, voff, eoff, c.vec, 2.5, dvec=dvec)
    ref = gr.structures_grad(c.A["rowptr"], c.A["col"], c.A["eid"], lat, voff, eoff, c.vec_h, 2.5, None, want["dvec"], np.float32)
    for key in ("cart", "frac"):
        assert same(got[key], ref[key]) and np.abs(ref[key]).max() > 0, key
    assert_close_elementwise(got["virial"].cpu().numpy(), ref["virial"], ref["virial_mag"], 1e-5, "virial")   # its order is free


# ---- Fortran ----------------------------------------------------------------------------------------------------------------------
def test_fortran_program_writes_the_python_mirrors_arrays(dev, tmp_path):
    if not os.path.exists(RUNNER):
        pytest.fail("triplets_run is not built: __graft_entry__.build() compiles the Fortran host side")
    from athena_amd import DeviceGraph
    from athena_amd.geometry import entry_vectors_grad, triplet_cos, triplet_cos_grad

    p, radius, cutoff3 = cloud_points(3), 0.35, 0.3
    g, coords = DeviceGraph.from_points(p, radius, add_self_loops=True)
    tg, dirs = DeviceGraph.from_triplets(g, coords, cutoff3)
    T, E, nnz = tg.n_edge_cols, g.n_edge_cols, g.nnz
    dcos = _rng(9100).standard_normal(T + 9).astype(np.float32)
    case_file, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case_file, "wb") as f:
        np.array([p.shape[0], 3, 1], np.int32).tofile(f)
        np.array([radius, cutoff3], np.float32).tofile(f)
        np.array([dcos.size], np.int64).tofile(f)
        p.tofile(f); dcos.tofile(f)
    out = subprocess.run([RUNNER, case_file, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"triplets_run failed ({out.returncode}): {out.stdout[-1000:]} {out.stderr[-2000:]}"
    cosv = triplet_cos(tg, dirs)
    dvec = entry_vectors_grad(g, triplet_cos_grad(tg, dirs, cosv, up(dcos[:T], dev)))
    with open(res, "rb") as f:
        assert np.fromfile(f, np.int64, 3).tolist() == [E, nnz, T] and T > 100
        assert np.array_equal(np.fromfile(f, np.int32, nnz + 1), tg.export("rowptr") + 1)
        ja = np.fromfile(f, np.int32, 2 * T).reshape(T, 2)
        assert np.array_equal(ja[:, 0], tg.export("col") + 1) and np.array_equal(ja[:, 1], tg.export("eid") + 1)
        for name, t in (("dir", dirs), ("cos", cosv), ("dvec", dvec)):
            want = t.cpu().numpy()
            assert np.array_equal(np.fromfile(f, np.int32, want.size), bits(want).ravel()), f"triplets_run: {name} differs from the Python mirror"
        assert f.read() == b""
