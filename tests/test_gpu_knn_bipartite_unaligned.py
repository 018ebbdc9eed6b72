"""GPU: athena_mp_knn_pairs_bipartite with each pointer operand in turn -- queries, sources, nbr, sqdist, pairs, coords, rowptr --
placed 1 or 2 elements past a 512-byte boundary (a 4- or an 8-byte aligned address) between guard words, the rest on 512-byte
boundaries, the way test_gpu_knn_unaligned.py places the operands of the one-set entries.  The results equal the yardstick's, no
guard word is written, and in buffers of the always-sufficient capacity n_queries * k the entries beyond the pairs stay unwritten."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_bipartite_reference as kb
from helpers import placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

OPERANDS = ("queries", "sources", "nbr", "sqdist", "pairs", "coords", "rowptr")


@functools.lru_cache(None)
def _case():
    qoff, soff = kb.offsets_of([401, 0, 333, 1, 200]), kb.offsets_of([350, 7, 0, 499, 3])
    rng = kb._rng(190)
    q = (rng.random((int(qoff[-1]), 3)) * 1.3 - 0.15).astype(np.float32)
    s = rng.random((int(soff[-1]), 3)).astype(np.float32)
    k, r = 7, 0.16
    nbr, sqd = kb.brute_force(q, s, k, r, qoff, soff)
    held = (nbr > 0).sum(1)
    assert np.any(held == 0) and np.any((held > 0) & (held < k)) and np.any(held == k)
    return q, s, qoff, soff, k, r, nbr, sqd, kb.graph_of(nbr, q, s, qoff)


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("operand", OPERANDS)
def test_one_operand_between_guards(dev, operand, at):
    import torch
    from athena_amd import _capi

    q, s, qoff, soff, k, r, want_nbr, want_s, (wi, wj, wc, wrow, weoff) = _case()
    nq, dim = q.shape
    E, T = wi.size, nq * k
    off = lambda name: at if name == operand else 0
    qd, sd = placed(q, dev, off("queries")), placed(s, dev, off("sources"))
    before = qd.clone(), sd.clone()
    nbr, check_n = placed_out((nq, k), torch.int32, dev, off("nbr"))
    sqd, check_s = placed_out((nq, k), torch.float32, dev, off("sqdist"))
    pairs, check_p = placed_out((T, 2), torch.int32, dev, off("pairs"))
    coords, check_c = placed_out((T, dim), torch.float32, dev, off("coords"))
    rowptr, check_r = placed_out((nq + 1,), torch.int32, dev, off("rowptr"))
    tensors = dict(zip(OPERANDS, (qd, sd, nbr, sqd, pairs, coords, rowptr)))
    for name, t in tensors.items():
        assert t.data_ptr() % 512 == 4 * off(name)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    got, eoff = C.c_int64(-1), np.full(qoff.size, -9, np.int64)
    _capi.use_torch_stream()
    _capi.call("athena_mp_knn_pairs_bipartite", qoff.size - 1, nq, vp(qoff), s.shape[0], vp(soff), dim, ptr(qd), ptr(sd), k, r, ptr(nbr),
               ptr(sqd), ptr(pairs), ptr(coords), T, ptr(rowptr), vp(eoff), C.byref(got))
    torch.cuda.synchronize()
    for check, name in ((check_n, "nbr"), (check_s, "sqdist"), (check_p, "pairs"), (check_c, "coords"), (check_r, "rowptr")):
        check(name)
    assert got.value == E and 0 < E < T and np.array_equal(eoff, weoff)
    assert unwritten(nbr) == 0 and np.array_equal(nbr.cpu().numpy(), want_nbr)
    assert unwritten(sqd) == 0 and np.array_equal(sqd.cpu().numpy().view(np.int32), want_s.view(np.int32))
    assert unwritten(rowptr) == 0 and np.array_equal(rowptr.cpu().numpy(), wrow)
    assert np.array_equal(pairs[:E].cpu().numpy().astype(np.int64), np.stack([wi + 1, wj + 1], axis=1))
    assert np.array_equal(coords[:E].cpu().numpy().view(np.int32), wc.view(np.int32))
    assert unwritten(pairs[:E]) == 0 and unwritten(coords[:E]) == 0
    assert unwritten(pairs[E:]) == 2 * (T - E) and unwritten(coords[E:]) == dim * (T - E), "entries beyond the pairs were written"
    assert torch.equal(qd.view(torch.int32), before[0].view(torch.int32)) and torch.equal(sd.view(torch.int32), before[1].view(torch.int32))
