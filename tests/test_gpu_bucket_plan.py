"""GPU: the Duvenaud degree-bucket plan built on the device (athena_amd/csrc/bucket_plan.hip; athena_mp_duvenaud_plan, _plan_export,
_plan_stats and the Python mirrors).  Twin handles of the same arrays are planned under ATHENA_MP_BUCKET_PLAN = host and = device;
all seven arrays of both are compared with each other and with the numpy yardstick of tests/bucket_plan_reference.py.  Every equality
is one of bytes; there are no tolerances."""
import contextlib
import os

import numpy as np
import pytest

import bucket_plan_reference as bp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "msgpass_chemical_head.xyz")
CMIN, CMAX = 0.5, 3.0


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


@contextlib.contextmanager
def _route(mode):
    """ATHENA_MP_BUCKET_PLAN pinned for the block (None: unset, the library chooses)"""
    old = os.environ.get("ATHENA_MP_BUCKET_PLAN")
    try:
        if mode is None:
            os.environ.pop("ATHENA_MP_BUCKET_PLAN", None)
        else:
            os.environ["ATHENA_MP_BUCKET_PLAN"] = mode
        yield
    finally:
        if old is None:
            os.environ.pop("ATHENA_MP_BUCKET_PLAN", None)
        else:
            os.environ["ATHENA_MP_BUCKET_PLAN"] = old


def _stats():
    from athena_amd import duvenaud_plan_stats

    return duvenaud_plan_stats()


def _delta(before):
    now = _stats()
    return {k: now[k] - before[k] for k in now}


def _ring(deg):
    """a ring of len(deg) vertices (neighbours v - 1 and v + 1, no edge columns) that carries the prescribed degrees"""
    from athena_amd import DeviceGraph

    deg = np.ascontiguousarray(deg, dtype=np.int32)
    n = deg.size
    ia = (1 + 2 * np.arange(n + 1)).astype(np.int32)
    ja = np.zeros((2, 2 * n), np.int32, order="F")
    ja[0, 0::2] = (np.arange(n) - 1) % max(n, 1) + 1
    ja[0, 1::2] = (np.arange(n) + 1) % max(n, 1) + 1
    return DeviceGraph(ia, ja, n_edge_cols=0, row_deg=deg, col_deg=deg)


def _assert_same(got, want, what):
    k = bp.same(got, want)
    assert k is None, f"{what}: {k} differs"


def _case(name):
    """(deg, min_deg, max_deg) of a named case"""
    if name.startswith("tail"):                       # one bucket, the tile tail
        n = int(name[4:])
        return _rng(n).integers(0, 9, n), 3, 3
    if name == "clamp_gap":                           # clamps at both ends, no vertex of degree 4: the tile offsets repeat
        deg = _rng(50).choice(np.array([0, 1, 2, 3, 5, 6, 7, 8, 9]), 50)
        deg[:9] = [0, 1, 2, 3, 5, 6, 7, 8, 9]
        return deg, 2, 6
    if name == "one_bucket":
        return _rng(40).integers(0, 8, 40), 3, 3
    if name == "all_first":
        return _rng(41).integers(0, 3, 100), 2, 9
    if name == "all_last":
        return _rng(42).integers(9, 15, 100), 2, 9
    if name.startswith("edge"):                       # the radix tile edges, stability across tiles
        n = int(name[4:])
        return _rng(n).integers(0, 13, n), 1, 10
    if name == "nb32":
        return _rng(32).integers(0, 41, 5000), 4, 35
    assert name == "nb256"                            # many one-vertex tiles
    return _rng(256).integers(0, 301, 5000), 0, 255


CASES = ("tail1", "tail15", "tail16", "tail17", "clamp_gap", "one_bucket", "all_first", "all_last", "edge4095", "edge4096", "edge4097",
         "edge8193", "nb32", "nb256")


@pytest.mark.parametrize("name", CASES)
def test_twin_handles_host_and_device(dev, name):
    deg, lo, hi = _case(name)
    if name == "clamp_gap":
        assert deg.min() < lo and deg.max() > hi and 4 not in deg
    if name in ("nb32", "nb256"):
        assert hi - lo + 1 == int(name[2:])
    want = bp.plan_reference(deg, lo, hi)
    if name == "clamp_gap":
        assert want["btile_off"][2] == want["btile_off"][3]
    if name == "nb256":
        count = want["btile_info"] & 255                                    # about 16.6 vertices a bucket: short second tiles
        assert np.count_nonzero(count == 1) >= 1 and np.count_nonzero(count < 16) > 128 and count.size > 256
    plans = {}
    for mode in ("host", "device"):
        g = _ring(deg)
        before = _stats()
        with _route(mode):
            assert g.plan_duvenaud(lo, hi) is g
        built = _delta(before)
        assert built == {"host_builds": int(mode == "host"), "device_builds": int(mode == "device"), "reused": 0}, (mode, built)
        plans[mode] = g.export_duvenaud_plan()
        assert np.array_equal(g.export("deg_row"), deg)
        g.close()
    _assert_same(plans["device"], want, "device plan against the yardstick")
    _assert_same(plans["host"], want, "host plan against the yardstick")
    _assert_same(plans["device"], plans["host"], "device plan against the host plan")


def test_replan_on_one_handle(dev):
    deg = _rng(5).integers(0, 13, 3000)
    g = _ring(deg)
    before = _stats()
    with _route("device"):
        for lo, hi in ((1, 10), (2, 5), (1, 10)):
            g.plan_duvenaud(lo, hi)
            _assert_same(g.export_duvenaud_plan(), bp.plan_reference(deg, lo, hi), f"plan ({lo}, {hi})")
        assert _delta(before) == {"host_builds": 0, "device_builds": 3, "reused": 0}
        g.plan_duvenaud(1, 10)
        assert _delta(before) == {"host_builds": 0, "device_builds": 3, "reused": 1}
        _assert_same(g.export_duvenaud_plan(), bp.plan_reference(deg, 1, 10), "the plan after a repeat")
    g.close()


def test_export_refuses_a_handle_without_a_plan(dev):
    from athena_amd import _capi

    g = _ring([2, 2, 2])
    with pytest.raises(_capi.AthenaMPError, match="no plan"):
        g.export_duvenaud_plan()
    g.close()


def _fixture():
    from athena_amd import io

    return io.structures_from_frames(io.read_extxyz(FIXTURE))


def test_real_handles_parent_and_child(dev):
    from athena_amd import DeviceDataset, DeviceGraph

    frac, lat, off = _fixture()
    B = lat.shape[0]
    sel = _rng(3).integers(0, B, 300).astype(np.int32)
    assert np.unique(sel).size < sel.size                                  # repeats
    plans = {}
    for mode in ("host", "device"):
        handle, _, _, voff, eoff = DeviceGraph.from_structures(frac, lat, off, CMIN, CMAX)
        ds = DeviceDataset(handle, voff, eoff)
        b = ds.select(sel)
        with _route(mode):
            handle.plan_duvenaud(1, 10)
            b.handle.plan_duvenaud(1, 10)
        plans[mode] = (handle.export_duvenaud_plan(), b.handle.export_duvenaud_plan())
        if mode == "device":
            _assert_same(plans[mode][0], bp.plan_reference(handle.export("deg_row"), 1, 10), "parent against the yardstick")
            _assert_same(plans[mode][1], bp.plan_reference(b.handle.export("deg_row"), 1, 10), "child against the yardstick")
            assert b.handle.n_rows == plans[mode][1]["bucket_perm"].size > 1000
        b.close()
        ds.close()
        handle.close()
    _assert_same(plans["device"][0], plans["host"][0], "parent: device against host")
    _assert_same(plans["device"][1], plans["host"][1], "child: device against host")


def _molecules(n_graphs):
    """synth.molecule_batch as (adj_ia, adj_ja, vertex_offsets, num_edges)"""
    from athena_amd import synth

    return synth.molecule_batch(n_graphs, seed=11)


def test_select_with_plan_degrees_hands_the_layer_a_planned_child(dev):
    import torch
    from athena_amd import DeviceDataset, DeviceGraph, ops

    frac, lat, off = _fixture()
    parent, _, _, voff, eoff = DeviceGraph.from_structures(frac, lat, off, CMIN, CMAX)
    ds = DeviceDataset(parent, voff, eoff)
    sel = _rng(9).integers(0, lat.shape[0], 300).astype(np.int32)
    before = _stats()
    with _route("device"):
        b = ds.select(sel, plan_degrees=(1, 6))
    assert _delta(before) == {"host_builds": 0, "device_builds": 1, "reused": 0}
    n = b.handle.n_rows
    assert n >= 1024                                                        # the update takes the bucketed route, which asks for the plan
    _assert_same(b.handle.export_duvenaud_plan(), bp.plan_reference(b.handle.export("deg_row"), 1, 6), "the child's plan")
    Fi, Fo = 72, 64
    a = torch.from_numpy(_rng(1).uniform(-1, 1, (n, Fi)).astype(np.float32)).to(dev)
    w = torch.from_numpy(_rng(2).uniform(-1, 1, Fo * Fi * 6).astype(np.float32)).to(dev)
    ops.duvenaud_update(b.handle, a, w, 1, 6, Fo)
    torch.cuda.synchronize()
    d = _delta(before)
    assert d["host_builds"] == 0 and d["device_builds"] == 1 and d["reused"] >= 1, d
    b.close()
    ds.close()
    parent.close()


def _run_layer(layer, handle, voff, x, e, up):
    import torch

    layer.set_graph_handle(handle, voff)
    out = layer.forward(x, e).clone()
    dx, de = layer.backward(up, need_input_grad=True, need_edge_grad=True)
    return out, dx.clone(), de.clone(), torch.from_numpy(layer.get_gradients())


@pytest.mark.parametrize("kind", ["mfma_64_8", "valu_6_7_10"])
def test_layer_is_bit_identical_over_host_and_device_plans(dev, kind):
    import torch
    from athena_amd import DeviceGraph
    from athena_amd.layers import duvenaud_msgpass_layer_type

    up_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = _rng(21)
    if kind == "mfma_64_8":
        ia, ja, voff, E = _molecules(70)
        make = lambda: (DeviceGraph(ia, ja, n_edge_cols=E), voff)
        n, m, Fv, Fe, T, O = ia.size - 1, voff.size - 1, 64, 8, 2, 8
        assert n >= 1100
        e = up_t(rng.uniform(-1, 1, (E, Fe)).astype(np.float32))
    else:
        frac, lat, off = _fixture()
        feats = {}

        def make():
            h, feature, _, vo, _ = DeviceGraph.from_structures(frac, lat, off, CMIN, CMAX)
            feats["e"] = feature[:, None].contiguous()
            return h, vo

        n, m, Fv, Fe, T, O = frac.shape[0], lat.shape[0], 6, 1, 2, 10
        e = None
    layer = duvenaud_msgpass_layer_type(num_vertex_features=[Fv], num_edge_features=[Fe], num_time_steps=T, max_vertex_degree=10,
                                        num_outputs=O, min_vertex_degree=1, seed=3)
    x = up_t(rng.uniform(-1, 1, (n, Fv)).astype(np.float32))
    up = up_t(rng.uniform(-1, 1, (m, O)).astype(np.float32))
    res, built = {}, {}
    for mode in ("host", "device"):
        h, vo = make()
        before = _stats()
        with _route(mode):
            res[mode] = _run_layer(layer, h, vo, x.clone(), (e if e is not None else feats["e"]).clone(), up)
        torch.cuda.synchronize()
        built[mode] = _delta(before)
        h.close()
    if kind == "mfma_64_8":                                                 # the bucketed route: each twin built its plan its own way
        assert (built["host"]["host_builds"], built["host"]["device_builds"]) == (1, 0), built
        assert (built["device"]["host_builds"], built["device"]["device_builds"]) == (0, 1), built
    bits = lambda t: t.contiguous().view(torch.int32)
    for a, c, what in zip(res["host"], res["device"], ("output", "dx", "de", "dparams")):
        assert a.shape == c.shape and torch.equal(bits(a), bits(c)), what
    assert res["device"][0].shape == (m, O) and res["device"][0].abs().max() > 0 and res["device"][2].abs().max() > 0


def test_auto_mode_routes(dev):
    from athena_amd import _capi

    deg = _rng(8).integers(0, 300, 2000)
    with _route(None):
        g = _ring(deg)
        before = _stats()
        g.plan_duvenaud(1, 10)                                              # no pin: the device route
        assert _delta(before) == {"host_builds": 0, "device_builds": 1, "reused": 0}
        _assert_same(g.export_duvenaud_plan(), bp.plan_reference(deg, 1, 10), "auto, 10 buckets")
        before = _stats()
        g.plan_duvenaud(0, 256)                                             # 257 buckets: beyond one digit, the host route
        assert _delta(before) == {"host_builds": 1, "device_builds": 0, "reused": 0}
        _assert_same(g.export_duvenaud_plan(), bp.plan_reference(deg, 0, 256), "auto, 257 buckets")
        before = _stats()
        g.plan_duvenaud(0, 255)                                             # 256 buckets: the last the device route takes
        assert _delta(before) == {"host_builds": 0, "device_builds": 1, "reused": 0}
        _assert_same(g.export_duvenaud_plan(), bp.plan_reference(deg, 0, 255), "auto, 256 buckets")
        empty = _ring(np.zeros(0, np.int32))
        before = _stats()
        empty.plan_duvenaud(1, 10)                                          # nothing to sort: the host route
        assert _delta(before) == {"host_builds": 1, "device_builds": 0, "reused": 0}
        _assert_same(empty.export_duvenaud_plan(), bp.plan_reference(np.zeros(0, np.int64), 1, 10), "auto, empty handle")
        empty.close()
    with _route("device"):
        before = _stats()
        with pytest.raises(_capi.AthenaMPError, match="256"):
            g.plan_duvenaud(0, 256)
        assert _delta(before) == {"host_builds": 0, "device_builds": 0, "reused": 0}
        _assert_same(g.export_duvenaud_plan(), bp.plan_reference(deg, 0, 255), "the plan a refused request leaves alone")
    g.close()


def test_device_plan_does_not_wait_for_the_stream(dev):
    """One-sided: about 50 ms of spinning is enqueued on the library's stream, then a fresh handle is planned on the device route; the
    event recorded behind the plan has not completed when the call returns, so the call neither synchronised nor copied to the host."""
    import torch

    if not hasattr(torch.cuda, "_sleep"):
        pytest.skip("torch.cuda._sleep is absent")
    deg = _rng(12).integers(0, 13, 5000)
    with _route("device"):
        _ring(deg).plan_duvenaud(1, 10).close()                             # the library's sort scratch exists from here on
        g = _ring(deg)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles = 20_000_000
        t0.record()
        torch.cuda._sleep(cycles)
        t1.record()
        t1.synchronize()
        per_ms = cycles / max(t0.elapsed_time(t1), 1e-3)
        before = _stats()
        torch.cuda._sleep(int(50 * per_ms))
        g.plan_duvenaud(1, 10)
        done = torch.cuda.Event()
        done.record()
        finished = done.query()
        assert _delta(before) == {"host_builds": 0, "device_builds": 1, "reused": 0}
        assert not finished, "plan_duvenaud returned only after the stream had drained"
        torch.cuda.synchronize()
        _assert_same(g.export_duvenaud_plan(), bp.plan_reference(deg, 1, 10), "the plan built behind the spin")
    g.close()
