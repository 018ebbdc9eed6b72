"""GPU: athena_mp_farthest_points with each pointer operand in turn -- points, sample, sample_points, sample_sqdist, cover_sqdist --
placed 1 or 2 elements past a 512-byte boundary (a 4- or an 8-byte aligned address) between guard words, the rest on 512-byte
boundaries, the way test_gpu_knn_bipartite_unaligned.py places the operands of the two-set builder.  The batch takes both routes
in one call.  The results equal the yardstick's, every output element is written, no guard word is, and the input is unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest

import fps_reference as fr
from helpers import placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

OPERANDS = ("points", "sample", "sample_points", "sample_sqdist", "cover_sqdist")


@functools.lru_cache(None)
def _case():
    off, soff = fr.offsets_of([300, 0, fr.CAPACITY + 104, 5]), fr.offsets_of([30, 0, 12, 5])
    p = fr.clustered(int(off[-1]), 3, 71, spread=0.03)
    start = np.array([17, 0, 0, int(off[-1])], np.int32)
    return p, off, soff, start, fr.brute_force(p, soff, off, start)


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("operand", OPERANDS)
def test_one_operand_between_guards(dev, operand, at):
    import torch
    from athena_amd import _capi

    p, offsets, soff, start, want = _case()
    n, dim = p.shape
    B, m = offsets.size - 1, int(soff[-1])
    off = lambda name: at if name == operand else 0
    pd = placed(p, dev, off("points"))
    before = pd.clone()
    sample, check_s = placed_out((m,), torch.int32, dev, off("sample"))
    sp, check_p = placed_out((m, dim), torch.float32, dev, off("sample_points"))
    sq, check_q = placed_out((m,), torch.float32, dev, off("sample_sqdist"))
    cover, check_c = placed_out((B,), torch.float32, dev, off("cover_sqdist"))
    tensors = dict(zip(OPERANDS, (pd, sample, sp, sq, cover)))
    for name, t in tensors.items():
        assert t.data_ptr() % 512 == 4 * off(name)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _capi.use_torch_stream()
    _capi.call("athena_mp_farthest_points", B, n, vp(offsets), dim, ptr(pd), m, vp(soff), vp(start), ptr(sample), ptr(sp), ptr(sq),
               ptr(cover))
    torch.cuda.synchronize()
    stats = np.zeros(4, np.int64)
    _capi.call("athena_mp_fps_stats", vp(stats))
    assert stats[3] == 1, "the batch must take both routes"
    for check, name in ((check_s, "sample"), (check_p, "sample_points"), (check_q, "sample_sqdist"), (check_c, "cover_sqdist")):
        check(name)
    for t, w in zip((sample, sp, sq, cover), want):
        assert unwritten(t) == 0 and np.array_equal(t.cpu().numpy().view(np.int32), w.view(np.int32))
    assert torch.equal(pd.view(torch.int32), before.view(torch.int32))
