"""GPU: mini-batches out of a device-resident dataset graph (athena_amd/csrc/batch_select.hip; athena_mp_batch_plan_create,
athena_mp_batch_select and the Python / Fortran mirrors).  A child handle is compared, array for array, with the handle
DeviceGraph.from_edges builds from the selection's own renumbered pair list, and with the yardstick of tests/batch_reference.py run
on the parent's exported arrays; ops and layers on a child with the same ops and layers on the from-scratch handle.  Every
comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import batch_reference as br
import periodic_reference as pr
from helpers import csr_from_index_list, placed_out, unwritten

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "msgpass_chemical_head.xyz")
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "batch_select_run")
CMIN, CMAX = 0.5, 3.0
SHAPES = ("first", "last", "all", "reversed", "half", "repeat")
PARENTS = ("golden", "golden_loops", "molecules", "no_edge_ids")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _up(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _export(handle):
    return {k: handle.export(k) for k in br.NAMES}


def _builds():
    from athena_amd import _capi

    b = C.c_int64()
    _capi.call("athena_mp_graph_cache_stats", None, None, C.byref(b))
    return b.value


def _fixture():
    from athena_amd import io

    return io.structures_from_frames(io.read_extxyz(FIXTURE))


def _selection(shape, B):
    if shape == "first":
        return [0]
    if shape == "last":
        return [B - 1]
    if shape == "all":
        return list(range(B))
    if shape == "reversed":
        return list(range(B))[::-1]
    if shape == "half":
        return [int(s) for s in _rng(B).permutation(B)[:B // 2]]
    assert shape == "repeat"
    return [B // 3, B - 1, B // 3, 0, B // 3]


_parents = {}


def _parent(kind, dev):
    """a dataset handle, built once per kind: dict(handle, off, eoff (None: no edge columns), pairs, pair_eoff, loops, with_ids, arrays)"""
    from athena_amd import DeviceGraph, synth
    from athena_amd.layers import _batched_graph

    if kind in _parents:
        return _parents[kind]
    p = {"loops": False, "with_ids": True}
    if kind in ("golden", "golden_loops"):
        frac, lat, off = _fixture()
        p["loops"] = kind == "golden_loops"
        p["handle"], _, _, p["off"], p["eoff"] = DeviceGraph.from_structures(frac, lat, off, CMIN, CMAX, add_self_loops=p["loops"])
        assert p["handle"].n_edge_cols == 1849
    elif kind == "molecules":
        # synth.molecule_batch(64) as a layer's set_graph assembles it from 64 graphs: the pair list of every molecule, then graph_type
        ia, ja, voff, E = synth.molecule_batch(64)
        rows = np.repeat(np.arange(ia.size - 1), np.diff(ia))
        half = np.nonzero((ja[1] > 0) & (rows < ja[0] - 1))[0]
        half = half[np.argsort(ja[1, half], kind="stable")]
        assert half.size == E
        sid = np.searchsorted(voff, rows[half], side="right") - 1
        graphs = []
        for s in range(64):
            mine = half[sid == s]
            local = np.stack([rows[mine] + 1 - voff[s], ja[0, mine] - voff[s]])
            graphs.append(csr_from_index_list(int(voff[s + 1] - voff[s]), local, self_loops=True))
        bg = _batched_graph(graphs, 0, True)
        p["loops"] = True
        p["handle"], p["off"], p["eoff"] = bg.device, bg.vertex_offsets.astype(np.int32), bg.edge_offsets.astype(np.int64)
        p["keep"] = bg
    else:
        assert kind == "no_edge_ids"
        rng = _rng(7)
        sizes = [int(v) for v in rng.integers(2, 40, 30)]
        sizes[5], sizes[11], sizes[29] = 0, 1, 3
        p["pairs"], p["off"], p["pair_eoff"] = br.random_block_pairs(rng, sizes, 2.5)
        p["loops"], p["with_ids"], p["eoff"] = True, False, None
        p["handle"] = DeviceGraph.from_edges(int(p["off"][-1]), p["pairs"], add_self_loops=True, with_edge_ids=False)
        assert p["handle"].n_edge_cols == 0
    p["arrays"] = _export(p["handle"])
    if "pairs" not in p:
        p["pairs"], p["pair_eoff"] = br.pairs_of_arrays(p["arrays"], p["handle"].n_edge_cols), p["eoff"]
    _parents[kind] = p
    return p


def _check_child(p, ds, sel, dev, keep=False):
    """one selection: size query, select, all thirteen arrays against from_edges of the child's own pair list and against the yardstick,
    both maps and both offset arrays against the yardstick"""
    import torch
    from athena_amd import DeviceGraph

    want, voff, ceoff, vmap, emap = br.select_reference(p["arrays"], p["off"], p["eoff"], sel)
    builds = _builds()
    qv, qe = ds.sizes(sel)
    assert _builds() == builds, "the size query built a handle"
    assert qv.dtype == np.int32 and qe.dtype == np.int64 and np.array_equal(qv, voff) and np.array_equal(qe, ceoff)
    b = ds.select(sel)
    assert np.array_equal(b.vertex_offsets, voff) and np.array_equal(b.edge_offsets, ceoff) and np.array_equal(b.ids, sel)
    assert b.vertex_map.dtype == torch.int32 and np.array_equal(b.vertex_map.cpu().numpy(), vmap)
    assert b.edge_map.dtype == torch.int32 and np.array_equal(b.edge_map.cpu().numpy(), emap)
    cp, n_child = br.child_pairs(p["pairs"], p["off"], p["pair_eoff"], sel)
    scratch = DeviceGraph.from_edges(n_child, cp, add_self_loops=p["loops"], with_edge_ids=p["with_ids"])
    assert (b.handle.n_rows, b.handle.n_cols, b.handle.nnz, b.handle.n_edge_cols) == (n_child, n_child, scratch.nnz, scratch.n_edge_cols)
    got = _export(b.handle)
    for k in br.NAMES:
        ref = scratch.export(k)
        assert got[k].shape == ref.shape and np.array_equal(got[k].view(np.int32), ref.view(np.int32)), f"{k} differs from the rebuild"
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), f"{k} differs from the yardstick"
    if keep:
        return b, scratch
    b.close()
    scratch.close()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", PARENTS)
def test_child_arrays_equal_the_rebuild_from_the_child_pair_list(dev, kind, shape):
    from athena_amd import DeviceDataset

    p = _parent(kind, dev)
    ds = DeviceDataset(p["handle"], p["off"], p["eoff"])
    B = len(ds)
    assert B == p["off"].size - 1 and (kind != "no_edge_ids" or (np.any(np.diff(p["off"]) == 0) and np.any(np.diff(p["off"]) == 1)))
    _check_child(p, ds, _selection(shape, B), dev)
    ds.close()


def test_hub_row_above_the_long_row_threshold(dev):
    """three structures, the middle one a single atom in a unit cubic cell: at cutoff 5.2 its row holds the 618 integer vectors with
    0.25 < |v|^2 < 27.04 -- above kLongRow = 512, so the child's long-row plans are rebuilt and used"""
    import torch
    from athena_amd import DeviceDataset, DeviceGraph, ops

    rng = _rng(11)
    frac = np.concatenate([rng.random((4, 3)), np.full((1, 3), 0.5), rng.random((3, 3))]).astype(np.float32)
    lat = np.stack([np.eye(3) * 6.0, np.eye(3), np.eye(3) * 7.0]).astype(np.float32)
    off = np.array([0, 4, 5, 8], np.int32)
    assert pr.structure_edges(frac[4:5], lat[1], 0.5, 5.2)[0].size == 618
    v = np.stack(np.meshgrid(*[np.arange(-6, 7)] * 3, indexing="ij"), -1).reshape(-1, 3)
    assert int(((v * v).sum(1) * 4 > 1).sum() - ((v * v).sum(1) * 100 >= 2704).sum()) == 618
    handle, feature, vec, voff, eoff = DeviceGraph.from_structures(frac, lat, off, 0.5, 5.2)
    p = {"handle": handle, "off": voff, "eoff": eoff, "loops": False, "with_ids": True, "arrays": _export(handle)}
    p["pairs"], p["pair_eoff"] = br.pairs_of_arrays(p["arrays"], handle.n_edge_cols), eoff
    assert np.diff(p["arrays"]["rowptr"])[4] == 618 and eoff[2] - eoff[1] == 618
    ds = DeviceDataset(handle, voff, eoff)
    for sel in ([1], [2, 1, 0], [1, 1]):
        b, scratch = _check_child(p, ds, sel, dev, keep=True)
        assert np.diff(b.handle.export("rowptr")).max() == 618
        n, E = b.handle.n_rows, b.handle.n_edge_cols
        x = _up(rng.uniform(-1, 1, (n, 16)).astype(np.float32), dev)
        e = _up(rng.uniform(-1, 1, (E, 3)).astype(np.float32), dev)
        for what, op in (("kipf_propagate", lambda g: ops.kipf_propagate(g, x)), ("kipf_propagate_bwd", lambda g: ops.kipf_propagate_bwd(g, x)),
                         ("duvenaud_propagate", lambda g: ops.duvenaud_propagate(g, x, e))):
            a, c = op(b.handle), op(scratch)
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and a.abs().max() > 0, (sel, what)
        b.close()
        scratch.close()
    ds.close()
    handle.close()


def test_duvenaud_layer_and_geometry_on_the_batches_of_an_epoch(dev):
    """the golden frames in batches of 8: the layer and structures_grad on each child, fed through take_vertices / take_edges /
    take_structures, against the same on from_structures of those frames' own coordinates"""
    import torch
    from athena_amd import DeviceDataset, DeviceGraph, structures_grad
    from athena_amd.layers import duvenaud_msgpass_layer_type

    frac, lat, off = _fixture()
    B, n = lat.shape[0], frac.shape[0]
    handle, feature, vec, voff, eoff = DeviceGraph.from_structures(frac, lat, off, CMIN, CMAX)
    ds = DeviceDataset(handle, voff, eoff)
    Fv, Fe, T, O = 6, 1, 2, 10
    layer = duvenaud_msgpass_layer_type(num_vertex_features=[Fv], num_edge_features=[Fe], num_time_steps=T, max_vertex_degree=10,
                                        num_outputs=O, min_vertex_degree=1, seed=3)
    rng = _rng(13)
    x_all = _up(rng.uniform(-1, 1, (n, Fv)).astype(np.float32), dev)
    lat_d = _up(lat, dev)
    bits = lambda t: t.contiguous().view(torch.int32)

    def run(h, vo, x, e, up):
        layer.set_graph_handle(h, vo)
        out = layer.forward(x, e).clone()
        dx, de = layer.backward(up, need_input_grad=True, need_edge_grad=True)
        return out, dx.clone(), de.clone(), torch.from_numpy(layer.get_gradients())

    seen = []
    for b in ds.batches(8, seed=1):
        sel = b.ids
        seen.extend(int(s) for s in sel)
        m = sel.size
        rows = np.concatenate([np.arange(off[s], off[s + 1]) for s in sel])
        off_s = np.concatenate([[0], np.cumsum(np.diff(off)[sel])]).astype(np.int32)
        h2, feature2, vec2, voff2, eoff2 = DeviceGraph.from_structures(frac[rows], lat[sel], off_s, CMIN, CMAX)
        assert np.array_equal(voff2, b.vertex_offsets) and np.array_equal(eoff2, b.edge_offsets)
        f_b, v_b, l_b, x_b = b.take_edges(feature), b.take_edges(vec), b.take_structures(lat_d), b.take_vertices(x_all)
        assert f_b.shape == feature2.shape and torch.equal(bits(f_b), bits(feature2)), "take_edges(feature)"
        assert v_b.shape == vec2.shape and torch.equal(bits(v_b), bits(vec2)), "take_edges(vec)"
        assert l_b.shape == (m, 3, 3) and np.array_equal(l_b.cpu().numpy(), lat[sel]), "take_structures(lat)"
        assert x_b.shape == (rows.size, Fv) and np.array_equal(x_b.cpu().numpy(), x_all.cpu().numpy()[rows]), "take_vertices(x)"
        up = _up(rng.uniform(-1, 1, (m, O)).astype(np.float32), dev)
        got = run(b.handle, b.vertex_offsets, x_b, f_b[:, None].contiguous(), up)
        want = run(h2, voff2, x_b.clone(), feature2[:, None].contiguous(), up)
        for a, c, what in zip(got, want, ("output", "dx", "de", "dparams")):
            assert a.shape == c.shape and torch.equal(bits(a), bits(c)), what
        assert got[0].shape == (m, O) and got[0].abs().max() > 0 and got[2].abs().max() > 0
        g1 = structures_grad(b.handle, l_b, b.vertex_offsets, b.edge_offsets, v_b, CMAX, dfeature=got[2])
        g2 = structures_grad(h2, _up(lat[sel], dev), voff2, eoff2, vec2, CMAX, dfeature=want[2])
        for k in ("cart", "frac", "virial", "lat"):
            assert torch.equal(bits(g1[k]), bits(g2[k])), k
        assert g1["cart"].abs().max() > 0
        b.close()
        h2.close()
    assert sorted(seen) == list(range(B)) and seen != list(range(B))       # one epoch: every structure once, shuffled
    assert [bb.ids.size for bb in ds.batches(16, shuffle=False, drop_last=True)] == [16, 16]
    ds.close()
    handle.close()


def test_graph_nop_layer_on_a_batch_of_small_radius_graphs(dev):
    """the GNO chain: small radius graphs assembled on the host (a layer's set_graph), a selection of them on the device"""
    import torch
    from athena_amd import DeviceDataset
    from athena_amd.graph import graph_type
    from athena_amd.layers import _batched_graph, graph_nop_layer_type
    from radius_reference import degree_radius

    rng = _rng(17)
    d, Fi, Fo, H = 3, 64, 64, 64
    graphs, coords = [], []
    for m in (150, 90, 220, 1, 130, 180):
        g = graph_type()
        coords.append(g.generate_radius_adjacency_device(rng.random((m, d)).astype(np.float32), degree_radius(max(m, 2), 10.0, d)))
        graphs.append(g)
    bg = _batched_graph(graphs, 0, True)
    ds = DeviceDataset(bg.device, bg.vertex_offsets, bg.edge_offsets.astype(np.int64))
    sel = [4, 1, 3, 1, 5]
    b = ds.select(sel)
    scratch = _batched_graph([graphs[s] for s in sel], 0, True)
    assert scratch.num_vertices == b.handle.n_rows and scratch.num_edges == b.handle.n_edge_cols
    for k in br.NAMES:
        assert np.array_equal(b.handle.export(k).view(np.int32), scratch.device.export(k).view(np.int32)), k
    x_all = rng.uniform(-1, 1, (bg.num_vertices, Fi)).astype(np.float32)
    c_all = np.concatenate(coords)
    x_b, c_b = b.take_vertices(_up(x_all, dev)), b.take_edges(_up(c_all, dev))
    rows = np.concatenate([np.arange(bg.vertex_offsets[s], bg.vertex_offsets[s + 1]) for s in sel])
    assert np.array_equal(x_b.cpu().numpy(), x_all[rows]) and np.array_equal(c_b.cpu().numpy(), np.concatenate([coords[s] for s in sel]))
    layer = graph_nop_layer_type(num_outputs=Fo, coord_dim=d, kernel_hidden=H, num_inputs=Fi, use_bias=True, activation="relu", seed=5)
    layer.set_params(layer.get_params() + _rng(1).standard_normal(layer.get_num_params()).astype(np.float32) * 0.05)
    up = _up(rng.uniform(-1, 1, (rows.size, Fo)).astype(np.float32), dev)
    res = []
    for h in (b.handle, scratch.device):
        layer.set_graph_handle(h)
        out = layer.forward(x_b.clone(), c_b.clone()).clone()
        dx, dc = layer.backward(up, need_coord_grad=True)
        res.append((out, dx.clone(), dc.clone(), torch.from_numpy(layer.get_gradients())))
    for a, c, what in zip(res[0], res[1], ("output", "dx", "dcoords", "dparams")):
        assert a.shape == c.shape and torch.equal(a.contiguous().view(torch.int32), c.contiguous().view(torch.int32)), what
    assert res[0][0].abs().max() > 0 and res[0][2].abs().max() > 0
    b.close()
    ds.close()


@pytest.mark.parametrize("k", [1, 2, 4])
def test_maps_at_chosen_addresses_between_guards(dev, k):
    import torch
    from athena_amd import DeviceDataset, _capi

    p = _parent("golden_loops", dev)
    ds = DeviceDataset(p["handle"], p["off"], p["eoff"])
    sel = np.asarray(_selection("repeat", len(ds)), np.int32)
    ref = ds.select(sel)
    nv, ne = int(ref.vertex_offsets[-1]), int(ref.edge_offsets[-1])
    vmap, check_v = placed_out((nv,), torch.int32, dev, k)
    emap, check_e = placed_out((ne,), torch.int32, dev, k)
    b = ds.select(sel, vertex_map=vmap, edge_map=emap)
    check_v(f"vertex_map {k} elements past a 512-byte boundary")
    check_e(f"edge_map {k} elements past a 512-byte boundary")
    assert b.vertex_map is vmap and unwritten(vmap) == 0 and torch.equal(vmap, ref.vertex_map)
    assert b.edge_map is emap and unwritten(emap) == 0 and torch.equal(emap, ref.edge_map)
    for name in br.NAMES:
        assert np.array_equal(b.handle.export(name).view(np.int32), ref.handle.export(name).view(np.int32)), name
    b.close()
    # each map may be NULL on its own: the other one is written, the buffer that was not passed stays as it was
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for which in ("vertex_map", "edge_map"):
        vmap, check_v = placed_out((nv,), torch.int32, dev, k)
        emap, check_e = placed_out((ne,), torch.int32, dev, k)
        child = C.c_void_p()
        _capi.use_torch_stream()
        _capi.call("athena_mp_batch_select", ds._plan, sel.size, sel.ctypes.data_as(C.c_void_p), C.byref(child), None, None,
                   ptr(vmap) if which == "vertex_map" else None, ptr(emap) if which == "edge_map" else None)
        check_v(which)
        check_e(which)
        given, other, want = (vmap, emap, ref.vertex_map) if which == "vertex_map" else (emap, vmap, ref.edge_map)
        assert unwritten(given) == 0 and torch.equal(given, want) and unwritten(other) == other.numel(), which
        _capi.call("athena_mp_graph_destroy", child)
    ref.close()
    ds.close()


def test_child_outlives_plan_and_parent_and_two_selects_are_byte_identical(dev):
    import torch
    from athena_amd import DeviceDataset, DeviceGraph, ops

    frac, lat, off = _fixture()
    handle, feature, vec, voff, eoff = DeviceGraph.from_structures(frac, lat, off, CMIN, CMAX, add_self_loops=True)
    ds = DeviceDataset(handle, voff, eoff)
    sel = [5, 30, 5, 12, 39, 0]
    b1, b2 = ds.select(sel), ds.select(sel)
    for k in br.NAMES:
        assert np.array_equal(b1.handle.export(k).view(np.int32), b2.handle.export(k).view(np.int32)), k
    assert torch.equal(b1.vertex_map, b2.vertex_map) and torch.equal(b1.edge_map, b2.edge_map)
    before = _export(b1.handle)
    x = _up(_rng(19).uniform(-1, 1, (b1.handle.n_rows, 32)).astype(np.float32), dev)
    e = _up(_rng(20).uniform(-1, 1, (b1.handle.n_edge_cols, 2)).astype(np.float32), dev)
    y0, c0 = ops.kipf_propagate(b1.handle, x).clone(), ops.duvenaud_propagate(b1.handle, x, e).clone()
    ds.close()
    handle.close()
    b2.close()
    fill = [torch.full((1 << 20,), 0x7F7F7F7F, dtype=torch.int32, device=dev) for _ in range(4)]      # whatever was freed is written over
    torch.cuda.synchronize()
    y1, c1 = ops.kipf_propagate(b1.handle, x), ops.duvenaud_propagate(b1.handle, x, e)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)) and torch.equal(c0.view(torch.int32), c1.view(torch.int32))
    after = _export(b1.handle)
    for k in br.NAMES:
        assert np.array_equal(before[k].view(np.int32), after[k].view(np.int32)), k
    del fill
    b1.close()


def test_refusals_name_the_structure_or_the_id_and_leave_the_device_usable(dev):
    import torch
    from athena_amd import DeviceDataset, DeviceGraph, _capi, ops, synth

    p = _parent("golden", dev)
    handle, off, eoff = p["handle"], p["off"], p["eoff"]
    B, n, E = off.size - 1, int(off[-1]), int(eoff[-1])
    x = _up(_rng(23).uniform(-1, 1, (n, 8)).astype(np.float32), dev)
    y0 = ops.kipf_propagate(handle, x).clone()

    def refused(match, fn):
        with pytest.raises(_capi.AthenaMPError, match=match):
            fn()
        assert torch.equal(ops.kipf_propagate(handle, x), y0), f"the device after the refusal {match!r}"

    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    plan = C.c_void_p()
    refused(r"batch_plan_create: null argument", lambda: _capi.call("athena_mp_batch_plan_create", None, B, vp(off), vp(eoff), C.byref(plan)))
    refused(r"batch_plan_create: null argument", lambda: _capi.call("athena_mp_batch_plan_create", handle.handle, B, None, vp(eoff), C.byref(plan)))
    refused(r"batch_plan_create: null out pointer", lambda: _capi.call("athena_mp_batch_plan_create", handle.handle, B, vp(off), vp(eoff), None))
    sel1 = np.zeros(1, np.int32)
    refused(r"batch_select: null argument", lambda: _capi.call("athena_mp_batch_select", None, 1, vp(sel1), None, None, None, None, None))
    # a rectangular handle, and a square one with explicit degrees
    ia, ja = synth.random_graph_csr(200, 800, seed=1)
    deg = np.diff(ia).astype(np.int32)
    rect = DeviceGraph(ia, ja, n_cols=205, n_edge_cols=0, row_deg=deg, col_deg=np.ones(205, np.int32))
    refused(r"a rectangular handle \(200 x 205\)", lambda: DeviceDataset(rect, [0, 100, 200]))
    rect.close()
    explicit = DeviceGraph(ia, ja, n_edge_cols=0, row_deg=deg + 1, col_deg=deg + 1)
    refused(r"row 1 has %d entries and degree %d: a handle with explicit degrees" % (deg[0], deg[0] + 1),
            lambda: DeviceDataset(explicit, [0, 100, 200]))
    explicit.close()
    # offsets and edge_offsets that do not run ascending from 0 to the handle's rows / edge columns
    bad = off.copy(); bad[0] = 1
    refused(r"offsets\(1\) = 1, not 0", lambda: DeviceDataset(handle, bad, eoff))
    bad = off.copy(); bad[4] = bad[3] - 1
    refused(r"structure 4: offsets descend from %d to %d" % (bad[3], bad[4]), lambda: DeviceDataset(handle, bad, eoff))
    bad = off.copy(); bad[-1] -= 1
    refused(r"offsets end at %d, the handle has %d rows" % (n - 1, n), lambda: DeviceDataset(handle, bad, eoff))
    bad = eoff.copy(); bad[0] = 2
    refused(r"edge_offsets\(1\) = 2, not 0", lambda: DeviceDataset(handle, off, bad))
    bad = eoff.copy(); bad[6] = bad[5] - 3
    refused(r"structure 6: edge_offsets descend from %d to %d" % (bad[5], bad[6]), lambda: DeviceDataset(handle, off, bad))
    bad = eoff.copy(); bad[-1] += 1
    refused(r"edge_offsets end at %d, the handle has %d edge columns" % (E + 1, E), lambda: DeviceDataset(handle, off, bad))
    refused(r"the handle has %d edge columns and edge_offsets is null" % E, lambda: DeviceDataset(handle, off, None))
    kipf = _parent("no_edge_ids", dev)
    refused(r"edge_offsets given, the handle has no edge columns", lambda: DeviceDataset(kipf["handle"], kipf["off"], kipf["pair_eoff"]))
    # an entry that leaves its structure: correct offsets with structure 4 (0-based 3) cut in two
    s = 3
    assert off[s + 1] - off[s] >= 2 and eoff[s + 1] - eoff[s] >= 2
    cut_v = np.insert(off, s + 1, (off[s] + off[s + 1]) // 2).astype(np.int32)
    cut_e = np.insert(eoff, s + 1, (eoff[s] + eoff[s + 1]) // 2).astype(np.int64)
    refused(r"structure 4\b.*an entry leaves its structure", lambda: DeviceDataset(handle, cut_v, cut_e))
    # the selection
    ds = DeviceDataset(handle, off, eoff)
    refused(r"n_sel = 0", lambda: ds.select([]))
    refused(r"id %d at position 1 is outside \[0, %d\)" % (B, B), lambda: ds.select([0, B]))
    refused(r"id -1 at position 2 is outside \[0, %d\)" % B, lambda: ds.sizes([0, 1, -1]))
    nw = np.diff(p["arrays"]["rowptr"][off])
    big = int(np.argmax(nw))
    pos = -(-((1 << 31) - 1) // int(nw[big])) - 1                          # the first position whose entries bring the batch to 2^31 - 1
    many = np.full(pos + 3, big, np.int32)
    refused(r"2\^31 entries or more at position %d \(id %d\)" % (pos, big), lambda: ds.sizes(many))
    b = ds.select([big, 0])                                                # ... and the plan is usable afterwards
    assert b.handle.nnz == int(nw[big] + nw[0])
    b.close()
    ds.close()


def test_fortran_program_writes_the_arrays_of_the_python_mirror(dev, tmp_path):
    from athena_amd import DeviceDataset, DeviceGraph

    if not os.path.exists(RUNNER):
        pytest.fail("batch_select_run is not built: __graft_entry__.build() compiles the Fortran host side")
    frac, lat, off = _fixture()
    handle, _, _, voff, eoff, ia, ja = DeviceGraph.from_structures(frac, lat, off, CMIN, CMAX, add_self_loops=True, want_adjacency=True)
    handle.close()
    n, nnz, E, B = ia.size - 1, ja.shape[1], int(eoff[-1]), voff.size - 1
    host = DeviceGraph(ia, ja, n_edge_cols=E)                              # the handle of that CSR, as the program acquires it
    ds = DeviceDataset(host, voff, eoff)
    for tag, sel in (("a", [7]), ("b", [39, 2, 2, 18, 0, 25])):
        sel = np.asarray(sel, np.int32)
        b = ds.select(sel)
        case_file, res_file = str(tmp_path / f"case_{tag}.bin"), str(tmp_path / f"result_{tag}.bin")
        with open(case_file, "wb") as f:
            f.write(np.asarray([n, nnz, E, B, sel.size], np.int32).tobytes() + ia.astype(np.int32).tobytes()
                    + np.asfortranarray(ja, np.int32).tobytes(order="F") + voff.astype(np.int32).tobytes() + eoff.astype(np.int64).tobytes()
                    + sel.tobytes())
        out = subprocess.run([RUNNER, case_file, res_file], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, f"batch_select_run failed ({out.returncode}): {out.stderr[-2000:]}"
        raw = open(res_file, "rb").read()
        nv, ne = int(b.vertex_offsets[-1]), int(b.edge_offsets[-1])
        assert tuple(np.frombuffer(raw, np.int32, 2)) == (nv, ne)
        o = 8
        for k in br.NAMES:
            want = b.handle.export(k).view(np.int32)
            assert int(np.frombuffer(raw, np.int32, 1, o)[0]) == want.size, k
            got = np.frombuffer(raw, np.int32, want.size, o + 4)
            o += 4 + 4 * want.size
            assert np.array_equal(got, want), f"batch_select_run: {k} differs from the Python mirror"
        m = sel.size
        assert np.array_equal(np.frombuffer(raw, np.int32, m + 1, o), b.vertex_offsets); o += 4 * (m + 1)
        assert np.array_equal(np.frombuffer(raw[o:o + 8 * (m + 1)], np.int64), b.edge_offsets); o += 8 * (m + 1)
        assert np.array_equal(np.frombuffer(raw, np.int32, nv, o), b.vertex_map.cpu().numpy()); o += 4 * nv
        assert np.array_equal(np.frombuffer(raw, np.int32, ne, o), b.edge_map.cpu().numpy()); o += 4 * ne
        assert o == len(raw)
        b.close()
    ds.close()
    host.close()
