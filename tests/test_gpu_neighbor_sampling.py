"""GPU: neighbour-sampled mini-batches of one graph (athena_mp_sampler_create / athena_mp_sample_neighbors, NeighborSampler) against
tests/sampling_reference.py.  Every integer output is np.array_equal with the yardstick; the handle is, array for array, what
athena_mp_graph_create builds from the yardstick's CSR and degrees; two runs are byte-identical; hops chain; slot is put back after
a sample and after every refusal; the Fortran host program writes the same arrays; Kipf and graph_nop steps run on the blocks."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import sampling_reference as sr
from helpers import assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "neighbor_sample_run")
ARRAYS = ("rowptr", "col", "eid", "coef", "t_rowptr", "t_src", "t_eid", "t_coef", "e_rowptr", "e_row", "e_entry", "deg_row", "deg_col")
SETS = list(sr.seed_sets(160))


@functools.lru_cache(None)
def _graph(with_edges):
    ia, ja, ne = sr.shape_graph(with_edges)
    rowptr, col, eid = sr.parent_csr(ia, ja)
    return ia, ja, ne, rowptr, col, (eid if with_edges else None)


@functools.lru_cache(None)
def _parent(with_edges):
    """the parent handle and its sampler, shared by the tests of this file (a sample leaves no trace in either)"""
    from athena_amd import DeviceGraph, NeighborSampler

    ia, ja, ne = _graph(with_edges)[:3]
    g = DeviceGraph(ia, ja, n_edge_cols=ne)
    return g, NeighborSampler(g)


@functools.lru_cache(None)
def _want(with_edges, name, k, seed, degrees):
    ia, ja, ne, rowptr, col, eid = _graph(with_edges)
    return sr.sample_hop(rowptr, col, eid, sr.seed_sets(rowptr.size - 1)[name], k, seed, degrees)


def _exports(g):
    return {a: g.export(a).view(np.int32) for a in ARRAYS}


def _built_from(want):
    """the thirteen arrays of the handle athena_mp_graph_create builds from the yardstick's CSR and degrees"""
    from athena_amd import DeviceGraph

    g = DeviceGraph(want["adj_ia"], want["adj_ja"], n_cols=want["n_cols"], n_edge_cols=want["n_edge_cols"], row_deg=want["row_deg"],
                    col_deg=want["col_deg"])
    out = _exports(g)
    g.close()
    return out


def _check(block, want, what=""):
    assert (block.handle.n_rows, block.handle.n_cols, block.handle.nnz) == (want["m"], want["n_cols"], want["nnz"]), what
    assert block.n_seeds == want["m"]
    assert np.array_equal(block.vertex_map.cpu().numpy(), want["vertex_map"]), what
    assert np.array_equal(block.entry_map.cpu().numpy(), want["entry_map"]), what
    if want["edge_map"] is None:
        assert block.edge_map is None
    else:
        assert np.array_equal(block.edge_map.cpu().numpy(), want["edge_map"]), what
    got, ref = _exports(block.handle), _built_from(want)
    for a in ARRAYS:
        assert np.array_equal(got[a], ref[a]), f"{what}: {a}"
    return got


@pytest.mark.parametrize("with_edges", [False, True], ids=["no edge ids", "edge ids"])
@pytest.mark.parametrize("degrees", ["block", "parent"])
@pytest.mark.parametrize("k", sr.FANOUTS)
def test_every_array_is_the_yardsticks(dev, k, degrees, with_edges):
    g, sampler = _parent(with_edges)
    n = g.n_rows
    for name, seeds in sr.seed_sets(n).items():
        (b,) = sampler.sample(seeds, [k], seed=9, degrees=degrees)
        _check(b, _want(with_edges, name, k, sr.hop_seed(9, 0), degrees), f"{name}, k = {k}")
        b.close()


def test_the_draw_skips_most_steps_of_the_hub(dev):
    g, sampler = _parent(False)
    hub = sr.ROW_LENGTHS.index(sr.HUB)
    (b,) = sampler.sample([hub], [5])
    drawn, whole, steps, skipped = sampler.stats()[:4]
    b.close()
    assert (drawn, whole, steps) == (1, 0, (sr.HUB + 63) // 64)
    # the k-th smallest of the keys seen so far falls like k / seen: the expected number of steps with a key below it is about
    # k ln(steps), 22 of 79 here; half the steps is a loose bound on a fixed input
    print(f"hub row: {skipped} of {steps} steps skipped")
    assert skipped >= steps // 2
    (b,) = sampler.sample(np.arange(g.n_rows), [0])
    assert tuple(sampler.stats()[:4]) == (0, g.n_rows, 0, 0)
    b.close()


@pytest.mark.parametrize("with_edges", [False, True], ids=["no edge ids", "edge ids"])
def test_two_runs_are_byte_identical(dev, with_edges):
    g, sampler = _parent(with_edges)
    seeds = sr.seed_sets(g.n_rows)["shuffled"]
    runs = []
    for _ in range(2):
        (b,) = sampler.sample(seeds, [5], seed=3)
        runs.append((b.vertex_map.cpu().numpy().tobytes(), b.entry_map.cpu().numpy().tobytes(),
                     b.edge_map.cpu().numpy().tobytes() if with_edges else b"", {a: v.tobytes() for a, v in _exports(b.handle).items()}))
        b.close()
    assert runs[0] == runs[1]


@pytest.mark.parametrize("degrees", ["block", "parent"])
def test_three_hops_chain(dev, degrees):
    g, sampler = _parent(True)
    ia, ja, ne, rowptr, col, eid = _graph(True)
    seeds = np.array([3, 40, 17, 99], np.int32)
    fanouts = (2, 5, 1)
    blocks = sampler.sample(seeds, fanouts, seed=2 ** 64 - 5, degrees=degrees)
    want = sr.sample(rowptr, col, eid, seeds, fanouts, 2 ** 64 - 5, degrees)
    assert len(blocks) == 3
    for h, (b, w) in enumerate(zip(blocks, want)):
        _check(b, w, f"block {h}")
    for outer, inner in zip(blocks, blocks[1:]):
        assert np.array_equal(outer.vertex_map[:outer.n_seeds].cpu().numpy(), inner.vertex_map.cpu().numpy())
    assert np.array_equal(blocks[-1].vertex_map[:4].cpu().numpy(), seeds)
    for b in blocks:
        b.close()


def test_a_sample_after_each_refusal_is_correct(dev):
    """slot is put back: after a sample, and after a repeated seed, a seed outside the graph and a capacity too small"""
    import torch
    from athena_amd import NeighborSampler, _capi

    g = _parent(True)[0]
    sampler = NeighborSampler(g)                                      # its own plan: the refusals must not touch the shared one
    n = g.n_rows
    name = "descending"
    seeds = sr.seed_sets(n)[name]

    def good(what):
        (b,) = sampler.sample(seeds, [5], seed=9)
        _check(b, _want(True, name, 5, sr.hop_seed(9, 0), "block"), what)
        b.close()

    good("first")
    good("after a sample")
    with pytest.raises(_capi.AthenaMPError, match=r"seeds\(4\) = 8 repeats seeds\(2\)"):
        sampler.sample([5, 7, 9, 7, 5], [5])
    good("after a repeated seed")
    with pytest.raises(_capi.AthenaMPError, match=r"seeds\(3\) = %d outside \[1,%d\]" % (n + 1, n)):
        sampler.sample([5, 7, n, -1], [5])
    good("after a seed outside the graph")
    s1 = torch.from_numpy(seeds + np.int32(1)).to(dev)
    want = _want(True, name, 5, sr.hop_seed(9, 0), "block")
    n_cols, nnz = C.c_int32(), C.c_int64()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    vm, em = torch.empty(want["n_cols"], dtype=torch.int32, device=dev), torch.empty(want["nnz"], dtype=torch.int32, device=dev)
    _capi.use_torch_stream()
    for caps, which in (((want["n_cols"] - 1, want["nnz"], want["nnz"]), "vertex_map"), ((want["n_cols"], want["nnz"] - 1, want["nnz"]), "entry_map"),
                        ((want["n_cols"], want["nnz"], want["nnz"] - 1), "edge_map")):
        with pytest.raises(_capi.AthenaMPError, match=which):
            _capi.call("athena_mp_sample_neighbors", sampler._plan, seeds.size, ptr(s1), 5, C.c_uint64(sr.hop_seed(9, 0)), 0, ptr(vm), caps[0],
                       ptr(em), caps[1], ptr(em), caps[2], C.byref(n_cols), C.byref(nnz), None)
        good(f"after a small {which}")
    for k, mode in ((65, 0), (-1, 0), (5, 2)):
        with pytest.raises(_capi.AthenaMPError):
            _capi.call("athena_mp_sample_neighbors", sampler._plan, seeds.size, ptr(s1), k, C.c_uint64(0), mode, None, 0, None, 0, None, 0,
                       C.byref(n_cols), C.byref(nnz), None)
    good("after a fan-out of 65")
    # the maps alone, and the count pass alone
    _capi.call("athena_mp_sample_neighbors", sampler._plan, seeds.size, ptr(s1), 5, C.c_uint64(sr.hop_seed(9, 0)), 0, ptr(vm), vm.numel(), None, 0,
               None, 0, C.byref(n_cols), C.byref(nnz), None)
    assert (n_cols.value, nnz.value) == (want["n_cols"], want["nnz"]) and np.array_equal(vm.cpu().numpy() - 1, want["vertex_map"])
    rp = torch.empty(seeds.size + 1, dtype=torch.int32, device=dev)
    _capi.call("athena_mp_sample_count", sampler._plan, seeds.size, ptr(s1), 5, ptr(rp), C.byref(nnz))
    assert nnz.value == want["nnz"] and np.array_equal(rp.cpu().numpy(), want["rowptr"])
    sampler.close()


def test_a_rectangular_parent_is_refused(dev):
    from athena_amd import DeviceGraph, NeighborSampler

    w = _want(False, "m = 5", 2, 1, "block")
    g = DeviceGraph(w["adj_ia"], w["adj_ja"], n_cols=w["n_cols"], n_edge_cols=0, row_deg=w["row_deg"], col_deg=w["col_deg"])
    with pytest.raises(ValueError, match="rectangular"):
        NeighborSampler(g)
    g.close()


@pytest.mark.parametrize("with_edges", [False, True], ids=["no edge ids", "edge ids"])
def test_fortran_program_writes_the_arrays_of_the_yardstick(dev, tmp_path, with_edges):
    if not os.path.exists(RUNNER):
        pytest.fail("neighbor_sample_run is not built: __graft_entry__.build() compiles the Fortran host side")
    ia, ja, ne, rowptr, col, eid = _graph(with_edges)
    n = rowptr.size - 1
    seeds = sr.seed_sets(n)["m = 5"]
    fanouts, seed, mode = (5, 2), 77, "parent"
    want = sr.sample(rowptr, col, eid, seeds, fanouts, seed, mode)[::-1]          # in hop order
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        np.array([n, ja.shape[1], ne, seeds.size, *fanouts, 1], np.int32).tofile(f)
        np.array([sr.hop_seed(seed, 0), sr.hop_seed(seed, 1)], np.uint64).tofile(f)
        ia.tofile(f); np.ascontiguousarray(ja.T).tofile(f); (seeds + np.int32(1)).tofile(f)
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"neighbor_sample_run failed ({out.returncode}): {out.stdout[-1000:]} {out.stderr[-2000:]}"
    raw = open(res, "rb").read()
    at = 0

    def take(count, dt=np.int32):
        nonlocal at
        a = np.frombuffer(raw, dt, count, at)
        at += a.nbytes
        return a

    for h, w in enumerate(want):
        assert int(take(1)[0]) == w["n_cols"] and int(take(1, np.int64)[0]) == w["nnz"]
        assert np.array_equal(take(w["n_cols"]) - 1, w["vertex_map"]), f"hop {h}"
        assert np.array_equal(take(w["nnz"]) - 1, w["entry_map"]), f"hop {h}"
        if with_edges:
            assert np.array_equal(take(w["nnz"]) - 1, w["edge_map"]), f"hop {h}"
        assert np.array_equal(take(w["m"] + 1), w["adj_ia"]), f"hop {h}"
        assert np.array_equal(take(2 * w["nnz"]).reshape(-1, 2).T, w["adj_ja"]), f"hop {h}"
        ref = _built_from(w)
        for a in ARRAYS:
            count = int(take(1)[0])
            assert np.array_equal(take(count), ref[a]), f"hop {h}: {a}"
    stats = take(8, np.int64)
    assert at == len(raw) and stats[0] + stats[1] == want[-1]["m"]


# ---- the layers on the blocks ---------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _kipf_parent():
    from athena_amd import DeviceGraph, NeighborSampler, synth

    n = 400
    ia, ja = synth.random_graph_csr(n, 5 * n, seed=5)
    g = DeviceGraph(ia, ja, n_edge_cols=0)
    return n, g, NeighborSampler(g)


def test_kipf_on_a_whole_row_block_is_the_parents_step_bit_for_bit(dev):
    import torch
    from athena_amd import ops

    n, g, sampler = _kipf_parent()
    seeds = np.random.default_rng(1).permutation(n)[:37].astype(np.int32)
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((n, 24)).astype(np.float32)).to(dev)
    (b,) = sampler.sample(seeds, [0], degrees="parent")
    got = ops.kipf_propagate(b.handle, b.take_vertices(x))
    want = ops.kipf_propagate(g, x)[torch.from_numpy(seeds.astype(np.int64)).to(dev)]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    b.close()


def test_two_kipf_layers_over_two_hops_are_the_parents_on_the_seed_rows(dev):
    import torch
    from athena_amd import ops

    n, g, sampler = _kipf_parent()
    rng = np.random.default_rng(3)
    seeds = rng.permutation(n)[:21].astype(np.int32)
    Fi, Fh, Fo = 24, 16, 8
    x = torch.from_numpy(rng.standard_normal((n, Fi)).astype(np.float32)).to(dev)
    w1 = torch.from_numpy((rng.standard_normal(Fh * Fi) * 0.3).astype(np.float32)).to(dev)
    w2 = torch.from_numpy((rng.standard_normal(Fo * Fh) * 0.3).astype(np.float32)).to(dev)
    outer, inner = sampler.sample(seeds, [0, 0], degrees="parent")
    assert outer.handle.n_rows == inner.handle.n_cols
    _, h = ops.kipf_layer_fwd(outer.handle, outer.take_vertices(x), w1, Fh, act="tanh")
    _, z = ops.kipf_layer_fwd(inner.handle, h, w2, Fo)
    _, hp = ops.kipf_layer_fwd(g, x, w1, Fh, act="tanh")
    _, zp = ops.kipf_layer_fwd(g, hp, w2, Fo)
    assert_close(z.cpu().numpy(), zp.cpu().numpy()[seeds], 1e-5, "two layers")
    # the reverse step of the last layer: an upstream that is zero off the seed rows
    up = torch.from_numpy(rng.standard_normal((seeds.size, Fo)).astype(np.float32)).to(dev)
    full = torch.zeros((n, Fo), dtype=torch.float32, device=dev)
    idx = torch.from_numpy(seeds.astype(np.int64)).to(dev)
    full[idx] = up
    want = ops.kipf_layer_bwd_x(g, full, w2, Fh).cpu().numpy()
    dxb = ops.kipf_layer_bwd_x(inner.handle, up, w2, Fh).cpu().numpy()
    got = np.zeros((n, Fh), np.float32)
    got[inner.vertex_map.cpu().numpy()] = dxb
    assert_close(got, want, 1e-5, "dX")
    outer.close(); inner.close()


def test_graph_nop_without_its_local_term_on_a_block(dev, oracle):
    import torch
    from athena_amd.layers import graph_nop_layer_type

    g, sampler = _parent(True)
    ia, ja, ne, rowptr, col, eid = _graph(True)
    n = g.n_rows
    rng = np.random.default_rng(8)
    seeds = sr.seed_sets(n)["shuffled"]
    d, Fi, Fo, Hh = 2, 5, 7, 16
    coords = torch.from_numpy(rng.uniform(-1, 1, (ne, d)).astype(np.float32)).to(dev)
    x = torch.from_numpy(rng.uniform(-1, 1, (n, Fi)).astype(np.float32)).to(dev)
    (b,) = sampler.sample(seeds, [5], seed=4)
    want = _want(True, "shuffled", 5, sr.hop_seed(4, 0), "block")
    cb, xb = b.take_edges(coords), b.take_vertices(x)
    assert np.array_equal(cb.cpu().numpy(), coords.cpu().numpy()[np.maximum(want["edge_map"], 0)])
    assert np.array_equal(xb.cpu().numpy(), x.cpu().numpy()[want["vertex_map"]])
    assert np.array_equal(b.take_entries(torch.arange(ja.shape[1], dtype=torch.float32, device=dev)).cpu().numpy(),
                          want["entry_map"].astype(np.float32))
    layer = graph_nop_layer_type(num_outputs=Fo, coord_dim=d, kernel_hidden=Hh, num_inputs=Fi, activation="tanh", device=str(dev),
                                 local_term=False)
    layer.set_params(layer.get_params() + rng.standard_normal(layer.get_num_params()).astype(np.float32) * 0.05)
    theta, bias = layer.params[0].cpu().numpy(), layer.params[1].cpu().numpy()
    layer.set_graph_handle(b.handle)
    out = layer.forward(xb, cb)
    torch.cuda.synchronize()
    # the square embedding of the block: its rows first, empty rows for the columns that are not seeds
    m, nc, E = want["m"], want["n_cols"], want["nnz"]
    sq_ia = np.concatenate([want["adj_ia"], np.full(nc - m, E + 1, np.int32)])
    kap = oracle.gno_kernel_eval(cb.cpu().numpy(), theta, Hh, Fo * Fi)
    z = oracle.gno_aggregate(xb.cpu().numpy(), kap, sq_ia, want["adj_ja"], Fo)[:m] + bias
    print(f"max|z| = {np.abs(z).max():.3f}")
    assert_close(out.cpu().numpy(), np.tanh(z), 1e-5, "forward")
    b.close()
