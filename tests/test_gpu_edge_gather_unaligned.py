"""GPU: both device entries of the edge gather -- athena_mp_edge_gather_fwd, athena_mp_edge_gather_bwd -- with each pointer operand in
turn placed 1 and 2 elements past a 512-byte boundary (4- and 8-byte aligned addresses) between guard words and the others on
torch's own 256-byte alignment, the way test_gpu_pool_unaligned.py places the operands of its entries; on the knn3 and the hub
handle of test_gpu_edge_gather.py at (Fs, Fq, dim, relative) = (4, 4, 0, 1) and (64, 64, 3, 0), at the padded pitch, where the
aligned call moves 16 bytes per lane and the moved one may not, and at (66, 7, 2, 0).  The results are the yardstick's words, no
guard word is written, every defined element is (and no pad element of h), and no input changes."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_edge_gather as tg
from helpers import SENTINEL, placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
bits = tg.bits
# entry -> (its pointer operands in call order, the outputs among them)
ENTRIES = {"fwd": (("xs", "xq", "coords", "h"), ("h",)), "bwd": (("dh", "dxs", "dxq", "dcoords"), ("dxs", "dxq", "dcoords"))}
WIDTHS = ((4, 4, 0, 1), (64, 64, 3, 0), (66, 7, 2, 0))
BLOCK = {"xs": 0, "dxs": 0, "xq": 1, "dxq": 1, "coords": 2, "dcoords": 2}       # operand -> the width it has; h and dh always exist
# every operand that is present, in turn: (4, 4, 0, 1) has no coords and no dcoords
PLACED = [(e, o, w) for e, (ops, _) in ENTRIES.items() for o in ops for w in WIDTHS if o not in BLOCK or w[BLOCK[o]] > 0]


def _pitch(widths):
    """the next multiple of 4 from W: 8, 132, 76"""
    return -(-sum(widths[:3]) // 4) * 4


@functools.lru_cache(None)
def _operands(name, widths):
    """name -> the yardstick's array at the pitch of this test (None for a block of width 0): the inputs as they go in, the outputs
    as they must come back -- h's pad columns hold the sentinel of an output that was not written"""
    Fs, Fq, dim, rel = widths
    A = tg.yardstick(name)[3]
    xs, xq, coords = tg.features(name, widths)
    E, W, ld = A["col"].size, Fs + Fq + dim, _pitch(widths)
    h = tg.er.fwd(A, xs, xq, coords, rel, np.full((E, ld), SENTINEL["float32"], np.int32).view(np.float32))
    dh = np.random.default_rng(9950 + W).standard_normal((E, ld)).astype(np.float32)
    dh[:, W:] = np.nan
    dxs, dxq, dc = tg.er.bwd(A, dh, (Fs, Fq, dim), rel)
    return {"xs": xs, "xq": xq, "coords": coords, "h": h, "dh": dh, "dxs": dxs if Fs else None, "dxq": dxq if Fq else None,
            "dcoords": dc if dim else None}


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("name", ["knn3", "hub"])
@pytest.mark.parametrize("entry,which,widths", PLACED)
def test_each_operand_between_guards(dev, entry, which, widths, name, at):
    import torch
    from athena_amd import _capi

    g, _ = tg.handle(name)
    Fs, Fq, dim, rel = widths
    W, ld = Fs + Fq + dim, _pitch(widths)
    names, outputs = ENTRIES[entry]
    arrays = _operands(name, widths)
    tensors, checks, before = {}, {}, {}
    for n in names:
        a = arrays[n]
        if a is None:
            tensors[n] = None
        elif n in outputs:
            tensors[n], checks[n] = placed_out(a.shape, torch.float32, dev, at if n == which else 0)
        else:
            tensors[n] = placed(a, dev, at) if n == which else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            before[n] = tensors[n].clone()
    assert tensors[which].data_ptr() % 16 == 4 * at
    _capi.use_torch_stream()
    if entry == "fwd":
        _capi.call("athena_mp_edge_gather_fwd", g.handle, Fs, ptr(tensors["xs"]), Fq, ptr(tensors["xq"]), dim, ptr(tensors["coords"]),
                   rel, ld, ptr(tensors["h"]))
    else:
        _capi.call("athena_mp_edge_gather_bwd", g.handle, Fs, Fq, dim, rel, ld, *(ptr(tensors[n]) for n in names))
    torch.cuda.synchronize()
    for n in outputs:
        if tensors[n] is None:
            continue
        checks[n](n)
        pads = g.n_edge_cols * (ld - W) if n == "h" else 0
        assert unwritten(tensors[n]) == pads, f"{n}: an element was not written, or a pad element was"
        assert np.array_equal(bits(tensors[n].cpu().numpy()), bits(arrays[n])), n
    for n, t in before.items():
        assert torch.equal(t.view(torch.int32), tensors[n].view(torch.int32)), f"{n} changed"
