"""GPU: every device entry of attention pooling -- athena_mp_attn_softmax_fwd, _gather_fwd, _gather_edges_fwd, _gather_bwd_x,
_gather_bwd_edges, _gather_bwd_alpha in both forms, _softmax_bwd -- with each pointer operand in turn placed 1 and 2 elements past a
512-byte boundary (4- and 8-byte aligned addresses) between guard words and the others on torch's own 256-byte alignment, the way
test_gpu_pool_unaligned.py places the operands of its entries; on the knn3 and the hub handle at (F, H) = (4, 4), (64, 4) and
(64, 64), where the aligned call moves 16 bytes per lane, takes a weight fast path, and the moved one may not.  The bit-defined
results are the transcription's words from the given inputs (tests/test_gpu_attention.py, reference); alpha, and dalpha where it is
a sum, are inside their bounds and the bytes of the aligned call, since both load routes add in one order.  No guard word is
written, every output element is, and no input changes."""
import ctypes as C

import numpy as np
import pytest

import activation_reference as act
import attention_reference as ar
import test_gpu_attention as ta
from helpers import placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
bits = ta.bits
# entry -> (the C entry, takes F, its pointer operands in call order (None: a NULL), the output among them)
ENTRIES = {"softmax_fwd": ("attn_softmax_fwd", False, ("scores", "alpha"), "alpha"),
           "gather_fwd": ("attn_gather_fwd", True, ("alpha", "x", "y"), "y"),
           "gather_edges_fwd": ("attn_gather_edges_fwd", True, ("alpha", "h", "yh"), "yh"),
           "bwd_x": ("attn_gather_bwd_x", True, ("alpha", "dy", "dx"), "dx"),
           "bwd_edges": ("attn_gather_bwd_edges", True, ("alpha", "dy", "dh"), "dh"),
           "bwd_alpha_x": ("attn_gather_bwd_alpha", True, ("x", None, "dy", "dalpha"), "dalpha"),
           "bwd_alpha_h": ("attn_gather_bwd_alpha", True, (None, "h", "dy", "dalpha_h"), "dalpha_h"),
           "softmax_bwd": ("attn_softmax_bwd", False, ("alpha", "dalpha", "dscores"), "dscores")}


def _operands(name, F, H):
    """name -> the array: the inputs as they go in, the bit-defined outputs as they must come back"""
    x, h, dy = ta.tp.features(name, "normal", F)
    want = dict(ta.reference(name, F, H))
    want.update(x=x, h=h, dy=dy, scores=ta.scores(name, H, "normal"))
    return want


def _call(entry, g, F, H, tensors):
    from athena_amd import _capi

    symbol, takes_f, names, _ = ENTRIES[entry]
    _capi.use_torch_stream()
    _capi.call("athena_mp_" + symbol, g.handle, *((F, H) if takes_f else (H,)), *(ptr(tensors.get(n)) for n in names))


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("F,H", [(4, 4), (64, 4), (64, 64)])
@pytest.mark.parametrize("name", ["knn3", "hub"])
@pytest.mark.parametrize("entry,which", [(e, o) for e, (_, _, ops, _) in ENTRIES.items() for o in ops if o is not None])
def test_each_operand_between_guards(dev, entry, which, name, F, H, at):
    import torch

    g, _ = ta.handle(name)
    A = ta.yardstick(name)[3]
    E = g.n_edge_cols
    _, _, names, output = ENTRIES[entry]
    arrays = _operands(name, F, H)
    shapes = {"alpha": (E, H), "dalpha": (E, H), "dalpha_h": (E, H)}
    shape_of = lambda n: shapes[n] if n in shapes else arrays[n].shape
    tensors, before = {}, {}
    for n in names:
        if n is None:
            continue
        if n == output:
            tensors[n], check = placed_out(shape_of(n), torch.float32, dev, at if n == which else 0)
        else:
            tensors[n] = placed(arrays[n], dev, at) if n == which else torch.from_numpy(np.ascontiguousarray(arrays[n])).to(dev)
            before[n] = tensors[n].clone()
    assert tensors[which].data_ptr() % 16 == 4 * at
    _call(entry, g, F, H, tensors)
    torch.cuda.synchronize()
    check(output)
    assert unwritten(tensors[output]) == 0, f"{output}: an element was not written"
    got = tensors[output].cpu().numpy()
    bit_defined = output not in ("alpha", "dalpha", "dalpha_h") or (output != "alpha" and F == H)
    if output == "dalpha_h":
        want = ar.bwd_alpha(A, E, None, arrays["h"], arrays["dy"], H)
    else:
        want = arrays[output]
    if bit_defined:
        assert np.array_equal(bits(got), bits(want)), output
    else:
        aligned = {n: torch.from_numpy(np.ascontiguousarray(arrays[n])).to(dev) for n in names if n is not None and n != output}
        aligned[output] = torch.full(shape_of(output), np.nan, dtype=torch.float32, device=dev)
        _call(entry, g, F, H, aligned)
        assert aligned[output].cpu().numpy().tobytes() == got.tobytes(), f"{output}: the two load routes differ"
        if output == "alpha":
            o32, f64, scale, a = ta.alpha_reference(name, H, "normal")
            act.assert_each(got, o32, f64, scale, a, 0.0, f"alpha {name} H={H} at +{at}")
        else:
            f64, bnd = ar.alpha_bound(A, E, arrays["x"] if output == "dalpha" else None, arrays["h"] if output == "dalpha_h" else None,
                                      arrays["dy"], H)
            assert (np.abs(got - f64) <= bnd).all(), output
    for n, t in before.items():
        assert torch.equal(t.view(torch.int32), tensors[n].view(torch.int32)), f"{n} changed"
