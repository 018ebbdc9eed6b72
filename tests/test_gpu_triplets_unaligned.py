"""GPU: the five device entries of the bond-angle triplets -- athena_mp_triplet_pairs, athena_mp_entry_vectors_fwd,
athena_mp_entry_vectors_bwd, athena_mp_triplet_cos_fwd, athena_mp_triplet_cos_bwd -- with each pointer operand in turn placed 1, 2 and
4 elements past a 512-byte boundary (4-, 8- and 16-byte aligned addresses) between guard words and the others on torch's own
256-byte alignment, the way test_gpu_pool_unaligned.py places the operands of its entries; on the hub and the cloud3 handle of
test_gpu_triplets.py (the pair list is stored 8 bytes per lane where it starts on an 8-byte boundary and 4 bytes at a time where it
does not).  The results are the yardstick's words, no guard word is written, every output element is, and no input changes."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_triplets as tt
from helpers import placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
bits = tt.bits
# entry -> (its pointer operands in call order, the outputs among them)
ENTRIES = {"triplet_pairs": (("vec", "pairs", "rowptr"), ("pairs", "rowptr")), "entry_vectors_fwd": (("vec", "dir"), ("dir",)),
           "entry_vectors_bwd": (("ddir", "dvec"), ("dvec",)), "triplet_cos_fwd": (("dir", "cos"), ("cos",)),
           "triplet_cos_bwd": (("dir", "cos", "dcos", "ddir"), ("ddir",))}


def _operands(name, cutoff3):
    """name -> the yardstick's array: the inputs as they go in, the outputs as they must come back"""
    c, want = tt.case(name), tt.reference(name, cutoff3)
    return {"vec": c.vec_h, "pairs": (want["pairs"] + 1).astype(np.int32), "rowptr": want["rowptr"].astype(np.int32), "dir": want["dir"],
            "cos": want["cos"], "dcos": want["dcos"], "ddir": want["ddir"], "dvec": want["dvec"]}


@pytest.mark.parametrize("at", [1, 2, 4])
@pytest.mark.parametrize("name", ["cloud3", "hub"])
@pytest.mark.parametrize("entry,which", [(e, o) for e, (ops, _) in ENTRIES.items() for o in ops])
def test_each_operand_between_guards(dev, entry, which, name, at):
    import torch
    from athena_amd import _capi

    cutoff3 = tt.CASES[name]
    c = tt.case(name)
    names, outputs = ENTRIES[entry]
    arrays = _operands(name, cutoff3)
    tensors, checks, before = {}, {}, {}
    for n in names:
        a = arrays[n]
        if n in outputs:
            tensors[n], checks[n] = placed_out(a.shape, torch.int32 if a.dtype == np.int32 else torch.float32, dev, at if n == which else 0)
        else:
            tensors[n] = placed(a, dev, at) if n == which else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            before[n] = tensors[n].clone()
    assert tensors[which].data_ptr() % 16 == (4 * at) % 16
    _capi.use_torch_stream()
    if entry == "triplet_pairs":
        T = C.c_int64(-1)
        _capi.call("athena_mp_triplet_pairs", c.g.handle, c.dim, ptr(tensors["vec"]), cutoff3, ptr(tensors["pairs"]), arrays["pairs"].shape[0],
                   ptr(tensors["rowptr"]), C.byref(T))
        assert T.value == arrays["pairs"].shape[0]
    else:
        handle = c.g if entry.startswith("entry") else _triplet_handle(name, cutoff3)
        _capi.call("athena_mp_" + entry, handle.handle, c.dim, *(ptr(tensors[n]) for n in names))
    torch.cuda.synchronize()
    for n in outputs:
        checks[n](n)
        assert unwritten(tensors[n]) == 0, f"{n}: an element was not written"
        assert np.array_equal(bits(tensors[n].cpu().numpy()), bits(arrays[n])), n
    for n, t in before.items():
        assert torch.equal(t.view(torch.int32), tensors[n].view(torch.int32)), f"{n} changed"


_handles = {}


def _triplet_handle(name, cutoff3):
    """the triplet handle of the case, from the yardstick's pair list (built once)"""
    import torch

    if (name, cutoff3) not in _handles:
        c, want = tt.case(name), tt.reference(name, cutoff3)
        pairs = torch.from_numpy((want["pairs"] + 1).astype(np.int32)).to(torch.device("cuda:0"))
        _handles[name, cutoff3] = tt.triplet_handle(c.nnz, pairs)[0]
    return _handles[name, cutoff3]
