"""GPU: athena_mp_grid_clusters and its reverse step with each pointer operand in turn placed 1 or 2 elements past a 512-byte boundary
(a 4- or an 8-byte aligned address) between guard words, the rest on 512-byte boundaries, the way test_gpu_fps_unaligned.py places
the operands of the sampler.  The batch holds a cloud of two work items, an empty cloud and a hub.  The results equal the
yardstick's, every output element is written, no guard word is, and the inputs are unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest

import grid_clusters_reference as gr
from helpers import placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

OPERANDS = ("points", "cluster", "pairs", "rowptr", "weights", "centroid", "nearest", "cell")
GRAD_OPERANDS = ("cluster", "rowptr", "dcentroid", "dpoints")


@functools.lru_cache(None)
def _case():
    hub = gr.cloud_of_sizes([700, 1, 2, 65], 3, 0.25, 73, row=2)
    big = gr._rng(74).random((4096 + 131, 3)).astype(np.float32)
    p = np.ascontiguousarray(np.concatenate([hub, big, big[:5] - np.float32(2)]))
    off = gr.offsets_of([hub.shape[0], 0, big.shape[0], 5])
    return p, off, 0.125, gr.clusters(p, off, 0.125)


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("operand", OPERANDS)
def test_one_operand_between_guards(dev, operand, at):
    import torch
    from athena_amd import _capi

    p, offsets, size, want = _case()
    n, dim = p.shape
    B, m = offsets.size - 1, want["m"]
    off = lambda name: at if name == operand else 0
    pd = placed(p, dev, off("points"))
    before = pd.clone()
    shapes = dict(cluster=((n,), torch.int32), pairs=((n, 2), torch.int32), rowptr=((m + 1,), torch.int32), weights=((n,), torch.float32),
                  centroid=((m, dim), torch.float32), nearest=((m,), torch.int32), cell=((m, dim), torch.int32))
    outs = {k: placed_out(shape, dt, dev, off(k)) for k, (shape, dt) in shapes.items()}
    for name, t in [("points", pd)] + [(k, v[0]) for k, v in outs.items()]:
        assert t.data_ptr() % 512 == 4 * off(name)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    coff, count = np.zeros(B + 1, np.int32), C.c_int64()
    _capi.use_torch_stream()
    _capi.call("athena_mp_grid_clusters", B, n, vp(offsets), dim, ptr(pd), size, None, m, *(ptr(outs[k][0]) for k in OPERANDS[1:]), vp(coff),
               None, C.byref(count))
    torch.cuda.synchronize()
    assert count.value == m and np.array_equal(coff, want["cluster_offsets"])
    for k in OPERANDS[1:]:
        t, check = outs[k]
        check(k)
        assert unwritten(t) == 0, k
        assert np.array_equal(t.cpu().numpy().view(np.int32), want[k].view(np.int32)), k
    assert torch.equal(pd.view(torch.int32), before.view(torch.int32))


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("operand", GRAD_OPERANDS)
def test_one_operand_of_the_reverse_step_between_guards(dev, operand, at):
    import torch
    from athena_amd import _capi

    p, offsets, size, want = _case()
    n, dim = p.shape
    m = want["m"]
    G = gr._rng(75).standard_normal((m, dim)).astype(np.float32)
    off = lambda name: at if name == operand else 0
    ins = dict(cluster=placed(want["cluster"], dev, off("cluster")), rowptr=placed(want["rowptr"], dev, off("rowptr")),
               dcentroid=placed(G, dev, off("dcentroid")))
    before = {k: t.clone() for k, t in ins.items()}
    out, check = placed_out((n, dim), torch.float32, dev, off("dpoints"))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    _capi.use_torch_stream()
    _capi.call("athena_mp_grid_clusters_grad", n, dim, m, ptr(ins["cluster"]), ptr(ins["rowptr"]), ptr(ins["dcentroid"]), ptr(out))
    torch.cuda.synchronize()
    check("dpoints")
    assert unwritten(out) == 0
    assert np.array_equal(out.cpu().numpy().view(np.int32), gr.grad(want["cluster"], want["rowptr"], G).view(np.int32))
    for k, t in ins.items():
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k
