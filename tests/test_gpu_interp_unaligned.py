"""GPU: the four device entries of the interpolation -- athena_mp_interp_weights, athena_mp_interp_fwd, athena_mp_interp_bwd_x,
athena_mp_interp_bwd_coords -- with each pointer operand in turn placed 1 and 2 elements past a 512-byte boundary (4- and 8-byte
aligned addresses) between guard words and the others on torch's own 256-byte alignment, the way test_gpu_bipartite_unaligned.py
places the operands of its entries; at F = 4, where the aligned call moves 16 bytes per lane and the moved one may not, and at
F = 7.  The results are the same words, no guard word is written, every output element is, and no input changes."""
import ctypes as C
import functools

import numpy as np
import pytest

import interp_reference as ir
import knn_bipartite_reference as kb
from helpers import placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

EPS = 1e-16
ptr = lambda t: C.c_void_p(t.data_ptr())
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(None)
def _case(F):
    rng = np.random.default_rng(53001)
    nq, ns = 70, 45
    q, s = rng.random((nq, 3)).astype(np.float32), rng.random((ns, 3)).astype(np.float32)
    q[3] = s[8]
    nbr, _ = kb.brute_force(q, s, 5)
    i, j, coords, _, _ = kb.graph_of(nbr, q, s)
    A = ir.arrays_of(i, j, nq, ns)
    x, dy = rng.standard_normal((ns, F)).astype(np.float32), rng.standard_normal((nq, F)).astype(np.float32)
    w, W = ir.weights(A, coords, EPS)
    y = ir.fwd(A, w, x)
    return q, s, coords, A, x, dy, w, W, y, ir.bwd_x(A, w, dy), ir.bwd_coords(A, coords, EPS, w, x, y, dy)


@functools.lru_cache(None)
def _handle():
    from athena_amd import DeviceGraph

    q, s, coords, A = _case(4)[:4]
    g, c, _ = DeviceGraph.from_point_sets_knn(q, s, 5)
    assert np.array_equal(bits(c.cpu().numpy()), bits(coords))
    return g


def _in(array, dev, here, at):
    import torch

    return placed(array, dev, at) if here else torch.from_numpy(np.ascontiguousarray(array)).to(dev)


def _out(shape, dev, here, at):
    import torch

    return placed_out(shape, torch.float32, dev, at if here else 0)


def _unchanged(pairs):
    import torch

    return all(torch.equal(now.view(torch.int32), before.view(torch.int32)) for now, before in pairs)


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("which", ["coords", "weights", "wsum"])
def test_the_weights_between_guards(dev, which, at):
    import torch
    from athena_amd import _capi

    g = _handle()
    _, _, coords, A, _, _, want_w, want_W = _case(4)[:8]
    cd = _in(coords, dev, which == "coords", at)
    before = cd.clone()
    w, check_w = _out((g.n_edge_cols,), dev, which == "weights", at)
    W, check_W = _out((g.n_rows,), dev, which == "wsum", at)
    assert {"coords": cd, "weights": w, "wsum": W}[which].data_ptr() % 16 == 4 * at
    _capi.use_torch_stream()
    _capi.call("athena_mp_interp_weights", g.handle, 3, ptr(cd), EPS, ptr(w), ptr(W))
    torch.cuda.synchronize()
    check_w("weights"); check_W("wsum")
    assert unwritten(w) == 0 and unwritten(W) == 0
    assert np.array_equal(bits(w.cpu().numpy()), bits(want_w)) and np.array_equal(bits(W.cpu().numpy()), bits(want_W))
    assert _unchanged([(cd, before)])


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("F", [4, 7])
@pytest.mark.parametrize("entry,which", [(e, o) for e in ("fwd", "bwd_x") for o in ("weights", "in", "out")])
def test_the_gather_between_guards(dev, entry, which, F, at):
    import torch
    from athena_amd import _capi

    g = _handle()
    _, _, _, _, x, dy, want_w, _, want_y, want_dx, _ = _case(F)
    src, want, rows = (x, want_y, g.n_rows) if entry == "fwd" else (dy, want_dx, g.n_cols)
    w, xd = _in(want_w, dev, which == "weights", at), _in(src, dev, which == "in", at)
    before = (w.clone(), xd.clone())
    out, check = _out((rows, F), dev, which == "out", at)
    assert {"weights": w, "in": xd, "out": out}[which].data_ptr() % 16 == 4 * at
    _capi.use_torch_stream()
    _capi.call("athena_mp_interp_" + entry, g.handle, F, ptr(w), ptr(xd), ptr(out))
    torch.cuda.synchronize()
    check("out")
    assert unwritten(out) == 0 and np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert _unchanged([(w, before[0]), (xd, before[1])])


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("F", [4, 7])
@pytest.mark.parametrize("which", ["coords", "weights", "x", "y", "dy", "dcoords"])
def test_the_coordinate_gradient_between_guards(dev, which, F, at):
    """dcoords is not bit-defined across implementations, but one implementation gives the same words wherever its operands lie:
    the summation order over f does not depend on an address"""
    import torch
    from athena_amd import _capi

    g = _handle()
    _, _, coords, A, x, dy, want_w, _, want_y, _, yard = _case(F)
    names = ("coords", "weights", "x", "y", "dy")
    arrays = dict(zip(names, (coords, want_w, x, want_y, dy)))

    def run(moved):
        ops = {n: _in(arrays[n], dev, n == moved, at) for n in names}
        before = {n: t.clone() for n, t in ops.items()}
        out, check = _out((g.n_edge_cols, 3), dev, moved == "dcoords", at)
        if moved is not None:
            assert (out if moved == "dcoords" else ops[moved]).data_ptr() % 16 == 4 * at
        _capi.use_torch_stream()
        _capi.call("athena_mp_interp_bwd_coords", g.handle, 3, F, ptr(ops["coords"]), EPS, ptr(ops["weights"]), ptr(ops["x"]),
                   ptr(ops["y"]), ptr(ops["dy"]), ptr(out))
        torch.cuda.synchronize()
        check("dcoords")
        assert unwritten(out) == 0 and _unchanged([(ops[n], before[n]) for n in names])
        return out.cpu().numpy()

    base, got = run(None), run(which)
    assert np.array_equal(bits(got), bits(base))
    zero = ir.zero_by_definition(coords, EPS)
    assert zero.any() and not bits(got[zero]).any()
    bound = ir.dcoords_bound(coords, EPS, want_w, x, want_y, dy, A)
    twin = ir.bwd_coords(A, coords, EPS, want_w, x, want_y, dy, np.float64)
    assert (np.abs(got.astype(np.float64) - twin)[~zero] <= bound[~zero]).all()
