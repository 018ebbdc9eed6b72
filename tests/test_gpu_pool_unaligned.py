"""GPU: the four device entries of max pooling -- athena_mp_pool_max_fwd, athena_mp_pool_max_edges_fwd, athena_mp_pool_max_bwd_x,
athena_mp_pool_max_bwd_edges -- with each pointer operand in turn placed 1 and 2 elements past a 512-byte boundary (4- and 8-byte
aligned addresses) between guard words and the others on torch's own 256-byte alignment, the way test_gpu_interp_unaligned.py
places the operands of its entries; on the knn3 and the hub handle of test_gpu_pool.py at F = 4 and 64, where the aligned call moves
16 bytes per lane and the moved one may not, and at F = 66.  The results are the yardstick's words, no guard word is written, every
output element is, and no input changes."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_pool as tp
from helpers import placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

ptr = lambda t: C.c_void_p(t.data_ptr())
bits = tp.bits
# entry -> (its three pointer operands in call order, the outputs among them)
ENTRIES = {"fwd": (("x", "y", "arg"), ("y", "arg")), "edges_fwd": (("h", "y", "arg"), ("y", "arg")),
           "bwd_x": (("arg", "dy", "dx"), ("dx",)), "bwd_edges": (("arg", "dy", "dh"), ("dh",))}


def _operands(entry, name, F):
    """name -> the yardstick's array: the inputs as they go in, the outputs as they must come back"""
    x, h, dy = tp.features(name, "ties", F)
    want = tp.reference(name, "ties", F)
    edge = entry in ("edges_fwd", "bwd_edges")
    return {"x": x, "h": h, "dy": dy, "y": want["yh" if edge else "yx"], "arg": want["ah" if edge else "ax"], "dx": want["dx"],
            "dh": want["dh"]}


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("F", [4, 64, 66])
@pytest.mark.parametrize("name", ["knn3", "hub"])
@pytest.mark.parametrize("entry,which", [(e, o) for e, (ops, _) in ENTRIES.items() for o in ops])
def test_each_operand_between_guards(dev, entry, which, name, F, at):
    import torch
    from athena_amd import _capi

    g, _ = tp.handle(name)
    names, outputs = ENTRIES[entry]
    arrays = _operands(entry, name, F)
    tensors, checks, before = {}, {}, {}
    for n in names:
        a = arrays[n]
        if n in outputs:
            tensors[n], checks[n] = placed_out(a.shape, torch.int32 if a.dtype == np.int32 else torch.float32, dev, at if n == which else 0)
        else:
            tensors[n] = placed(a, dev, at) if n == which else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            before[n] = tensors[n].clone()
    assert tensors[which].data_ptr() % 16 == 4 * at
    _capi.use_torch_stream()
    _capi.call("athena_mp_pool_max_" + entry, g.handle, F, *(ptr(tensors[n]) for n in names))
    torch.cuda.synchronize()
    for n in outputs:
        checks[n](n)
        assert unwritten(tensors[n]) == 0, f"{n}: an element was not written"
        assert np.array_equal(bits(tensors[n].cpu().numpy()), bits(arrays[n])), n
    for n, t in before.items():
        assert torch.equal(t.view(torch.int32), tensors[n].view(torch.int32)), f"{n} changed"
