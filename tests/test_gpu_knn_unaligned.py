"""GPU: the two device entries of the k-nearest-neighbour builder (athena_mp_knn_pairs_batched, athena_mp_knn_pairs) with every
pointer operand -- points, nbr, pairs, coords -- placed 1, 2 and 4 elements past a 512-byte boundary (4-, 8- and 16-byte aligned
addresses) between guard words, the way test_gpu_unaligned.py places the operands of the other entries.  The results equal the
yardstick's, no guard word is written, and in buffers of the always-sufficient capacity n * k the entries beyond the pairs stay
unwritten."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_reference as kr
from helpers import placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

INF = float("inf")


@functools.lru_cache(None)
def _case(batched):
    off = kr.offsets_of([700, 0, 333, 1, 501] if batched else [1535])
    p = kr._rng(80 + batched).random((int(off[-1]), 3)).astype(np.float32)
    k, r = 7, 0.11
    nbr = kr.large_form_neighbours(p, off, k, r)
    assert np.any((nbr > 0).sum(1) < k) and np.any((nbr > 0).sum(1) == k)
    return p, off, k, r, nbr


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("at", [1, 2, 4])
@pytest.mark.parametrize("batched", [True, False])
def test_operands_between_guards(dev, batched, at, mode):
    import torch
    from athena_amd import _capi

    p, off, k, r, want_nbr = _case(batched)
    n, dim = p.shape
    ri, rj, rc, reoff = kr.graph_of(want_nbr, p, off, mode)
    E, T = ri.size, n * k
    pts = placed(p, dev, at)
    before = pts.clone()
    nbr, check_n = placed_out((n, k), torch.int32, dev, at)
    pairs, check_p = placed_out((T, 2), torch.int32, dev, at)
    coords, check_c = placed_out((T, dim), torch.float32, dev, at)
    for t in (pts, nbr, pairs, coords):
        assert t.data_ptr() % 16 == (4 * at) % 16
    ptr = lambda t: C.c_void_p(t.data_ptr())
    got = C.c_int64(-1)
    _capi.use_torch_stream()
    if batched:
        eoff = np.full(off.size, -9, np.int64)
        _capi.call("athena_mp_knn_pairs_batched", off.size - 1, n, off.ctypes.data_as(C.c_void_p), dim, ptr(pts), k, r, mode, ptr(nbr),
                   ptr(pairs), ptr(coords), T, eoff.ctypes.data_as(C.c_void_p), C.byref(got))
        assert np.array_equal(eoff, reoff)
    else:
        _capi.call("athena_mp_knn_pairs", n, dim, ptr(pts), k, r, mode, ptr(nbr), ptr(pairs), ptr(coords), T, C.byref(got))
    torch.cuda.synchronize()
    check_n("nbr")
    check_p("pairs")
    check_c("coords")
    assert got.value == E and 0 < E < T
    assert unwritten(nbr) == 0 and np.array_equal(nbr.cpu().numpy(), want_nbr)
    assert np.array_equal(pairs[:E].cpu().numpy().astype(np.int64), np.stack([ri + 1, rj + 1], axis=1))
    assert np.array_equal(coords[:E].cpu().numpy(), rc)
    assert unwritten(pairs[:E]) == 0 and unwritten(coords[:E]) == 0
    assert unwritten(pairs[E:]) == 2 * (T - E) and unwritten(coords[E:]) == dim * (T - E), "entries beyond the pairs were written"
    assert torch.equal(pts.view(torch.int32), before.view(torch.int32))
