"""GPU: athena_mp_topk_vertices, athena_mp_select_rows_fwd and athena_mp_select_rows_bwd (with and without a gate) with each
pointer operand in turn placed 1 or 2 elements past a 512-byte boundary (a 4- or an 8-byte aligned address) between guard words,
the rest on 512-byte boundaries, the way test_gpu_contract_unaligned.py places the operands of the contraction.  The selection is
the three-tile graph among small graphs, its outputs sized exactly m; the rows are 8 wide, so that the operand off its boundary is
what takes the call from the 16-byte route to the 4-byte one.  The results equal the yardstick's, every output element is written,
no guard word is, and the inputs are unchanged; the gate's gradient is the same bytes at every placement."""
import ctypes as C
import functools

import numpy as np
import pytest

import topk_reference as tr
from helpers import placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

NAME = "three tiles and small graphs"
F = 8
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
vp = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("operand", ["score", "cluster", "selected", "order"])
def test_one_operand_of_the_selection_between_guards(dev, operand, at):
    import torch
    from athena_amd import _capi

    c, want = tr.case(NAME), tr.expected(NAME)
    s, offsets = c["score"], c["offsets"]
    n, B, m = s.size, offsets.size - 1, want["m"]
    kk = tr.counts_of(c)
    assert m == int(np.minimum(kk, np.diff(offsets)).sum())           # no min_score: exactly the room the entry asks for
    off = lambda name: at if name == operand else 0
    score = placed(np.array(s), dev, off("score"))
    before = score.clone()
    outs = {k: placed_out((n if k == "cluster" else m,), torch.int32, dev, off(k)) for k in ("cluster", "selected", "order")}
    for name, t in [("score", score)] + [(k, v[0]) for k, v in outs.items()]:
        assert t.data_ptr() % 512 == 4 * off(name)
    soff, count = np.full(B + 1, -1, np.int32), C.c_int64(-1)
    _capi.use_torch_stream()
    _capi.call("athena_mp_topk_vertices", B, n, vp(offsets), ptr(score), 0, vp(kk), 0, 0.0, ptr(outs["cluster"][0]), ptr(outs["selected"][0]),
               ptr(outs["order"][0]), vp(soff), C.byref(count))
    torch.cuda.synchronize()
    assert count.value == m and np.array_equal(soff, want["sel_offsets"])
    for k, (t, check) in outs.items():
        check(k)
        assert unwritten(t) == 0, k
        assert np.array_equal(t.cpu().numpy(), want[k]), k
    assert torch.equal(score.view(torch.int32), before.view(torch.int32))


@functools.lru_cache(None)
def _rows(gated):
    cluster, selected, x, gate, dy = tr.rows_case(90 + int(gated), 1500, 400, F, gated=gated)
    return dict(cluster=cluster, selected=selected, x=x, gate=gate, dy=dy)


@functools.lru_cache(None)
def _aligned_dgate(gated):
    """the gate's gradient with every operand on a 512-byte boundary: the bytes every placement must give"""
    import torch
    from athena_amd.geometry import select_rows_grad

    kw = _rows(gated)
    t = lambda a: torch.from_numpy(a).cuda() if a is not None else None
    return select_rows_grad(t(kw["cluster"]), t(kw["dy"]), x=t(kw["x"]), gate=t(kw["gate"]), want=("gate",))["gate"].cpu().numpy()


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("operand", ["selected", "x", "gate", "y"])
def test_one_operand_of_the_forward_rows_between_guards(dev, operand, at):
    import torch
    from athena_amd import _capi

    kw = _rows(True)
    n, m = kw["cluster"].size, kw["selected"].size
    off = lambda name: at if name == operand else 0
    ins = {k: placed(kw[k], dev, off(k)) for k in ("selected", "x", "gate")}
    before = {k: t.clone() for k, t in ins.items()}
    y, check = placed_out((m, F), torch.float32, dev, off("y"))
    _capi.use_torch_stream()
    _capi.call("athena_mp_select_rows_fwd", n, m, F, ptr(ins["selected"]), ptr(ins["x"]), ptr(ins["gate"]), ptr(y))
    torch.cuda.synchronize()
    check("y")
    assert unwritten(y) == 0
    assert np.array_equal(y.cpu().numpy().view(np.int32), tr.rows_fwd(kw["selected"], kw["x"], kw["gate"]).view(np.int32))
    if operand != "gate":                                             # and the copy, which takes no gate
        y2, check2 = placed_out((m, F), torch.float32, dev, off("y"))
        _capi.call("athena_mp_select_rows_fwd", n, m, F, ptr(ins["selected"]), ptr(ins["x"]), None, ptr(y2))
        check2("y without a gate")
        assert unwritten(y2) == 0 and np.array_equal(y2.cpu().numpy().view(np.int32), tr.rows_fwd(kw["selected"], kw["x"]).view(np.int32))
    for k, t in ins.items():
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("gated,operand", [(True, o) for o in ("cluster", "dy", "x", "gate", "dx", "dgate")] +
                         [(False, o) for o in ("cluster", "dy", "x", "dx", "dgate")])
def test_one_operand_of_the_reverse_rows_between_guards(dev, gated, operand, at):
    import torch
    from athena_amd import _capi

    kw = _rows(gated)
    n, m = kw["cluster"].size, kw["selected"].size
    off = lambda name: at if name == operand else 0
    ins = {k: placed(kw[k], dev, off(k)) for k in ("cluster", "dy", "x") + (("gate",) if gated else ())}
    before = {k: t.clone() for k, t in ins.items()}
    dx, check_dx = placed_out((n, F), torch.float32, dev, off("dx"))
    dgate, check_dgate = placed_out((n,), torch.float32, dev, off("dgate"))
    _capi.use_torch_stream()
    _capi.call("athena_mp_select_rows_bwd", n, m, F, ptr(ins["cluster"]), ptr(ins["dy"]), ptr(ins["x"]), ptr(ins.get("gate")), ptr(dx), ptr(dgate))
    torch.cuda.synchronize()
    check_dx("dx")
    check_dgate("dgate")
    assert unwritten(dx) == 0 and unwritten(dgate) == 0
    assert np.array_equal(dx.cpu().numpy().view(np.int32), tr.rows_bwd_x(kw["cluster"], kw["dy"], kw["gate"]).view(np.int32))
    got = dgate.cpu().numpy()
    ref, scale = tr.rows_bwd_gate(kw["cluster"], kw["dy"], kw["x"])
    assert (np.abs(got.astype(np.float64) - ref) <= 1e-5 * scale).all() and (got.view(np.int32)[kw["cluster"] == 0] == 0).all()
    assert np.array_equal(got.view(np.int32), _aligned_dgate(gated).view(np.int32))
    for k, t in ins.items():
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k
