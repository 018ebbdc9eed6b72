"""GPU: athena_mp_contract_pairs, athena_mp_graph_pairs and athena_mp_cell_pairs with each pointer operand in turn placed 1 or 2
elements past a 512-byte boundary (a 4- or an 8-byte aligned address) between guard words, the rest on 512-byte boundaries, the way
test_gpu_grid_clusters_unaligned.py places the operands of the clustering.  The contraction is the two-set case of three radix tiles
(both maps and both point sets are arrays of their own).  The results equal the yardstick's, every output element is written, no
guard word is, and the inputs are unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest

import contract_reference as cr
from helpers import placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

INPUTS = ("pairs", "row_cluster", "col_cluster", "row_points", "col_points")
OPERANDS = INPUTS + cr.KEYS
ptr = lambda t: C.c_void_p(t.data_ptr())


@functools.lru_cache(None)
def _case():
    kw = cr.case("three tiles, 300 x 200 clusters, mode 1")
    return kw, cr.contract(*cr.args_of(kw))


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("operand", OPERANDS)
def test_one_operand_of_the_contraction_between_guards(dev, operand, at):
    import torch
    from athena_amd import _capi

    kw, want = _case()
    E, P, M, dim = kw["pairs"].shape[0], want["P"], want["M"], kw["row_points"].shape[1]
    off = lambda name: at if name == operand else 0
    ins = {k: placed(kw[k], dev, off(k)) for k in INPUTS}
    before = {k: t.clone() for k, t in ins.items()}
    shapes = dict(coarse_pairs=((P, 2), torch.int32), rowptr=((P + 1,), torch.int32), members=((M, 2), torch.int32), weights=((M,), torch.float32),
                  edge_pair=((E,), torch.int32), coords=((P, dim), torch.float32))
    outs = {k: placed_out(shape, dt, dev, off(k)) for k, (shape, dt) in shapes.items()}
    for name, t in list(ins.items()) + [(k, v[0]) for k, v in outs.items()]:
        assert t.data_ptr() % 512 == 4 * off(name)
    n1, n2 = C.c_int64(), C.c_int64()
    _capi.use_torch_stream()
    _capi.call("athena_mp_contract_pairs", E, ptr(ins["pairs"]), kw["n_rows"], kw["n_cols"], ptr(ins["row_cluster"]), ptr(ins["col_cluster"]),
               kw["m_rows"], kw["m_cols"], 1, dim, ptr(ins["row_points"]), ptr(ins["col_points"]), P, M, *(ptr(outs[k][0]) for k in cr.KEYS),
               C.byref(n1), C.byref(n2))
    torch.cuda.synchronize()
    assert (n1.value, n2.value) == (P, M)
    for k in cr.KEYS:
        t, check = outs[k]
        check(k)
        assert unwritten(t) == 0, k
        assert np.array_equal(t.cpu().numpy().view(np.int32), want[k].view(np.int32)), k
    for k, t in ins.items():
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k


@pytest.mark.parametrize("at", [1, 2])
def test_the_pair_list_of_a_handle_between_guards(dev, at):
    import torch
    from athena_amd import DeviceGraph, _capi

    r = cr._rng(70)
    n, E = 300, 4096 + 9
    idx = np.stack([r.integers(1, n + 1, E), r.integers(1, n + 1, E)]).astype(np.int32)
    g = DeviceGraph.from_edges(n, idx)
    out, check = placed_out((E, 2), torch.int32, dev, at)
    _capi.use_torch_stream()
    _capi.call("athena_mp_graph_pairs", g.handle, ptr(out), E)
    torch.cuda.synchronize()
    check("pairs")
    assert unwritten(out) == 0
    assert np.array_equal(out.cpu().numpy(), np.stack([idx.min(axis=0), idx.max(axis=0)], axis=1))


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("operand", ["cells", "pairs"])
@pytest.mark.parametrize("cell_type", [1, 2, 3, 4])
def test_one_operand_of_cell_pairs_between_guards(dev, cell_type, operand, at):
    import torch
    from athena_amd import _capi

    cells, nvert, _, _, _ = cr.grid_mesh(cell_type, 9, 7, 3)
    total = cells.shape[0] * len(cr.LOCAL[cell_type])
    off = lambda name: at if name == operand else 0
    cd = placed(cells, dev, off("cells"))
    before = cd.clone()
    out, check = placed_out((total, 2), torch.int32, dev, off("pairs"))
    count = C.c_int64()
    _capi.use_torch_stream()
    _capi.call("athena_mp_cell_pairs", nvert, cells.shape[0], cell_type, ptr(cd), ptr(out), total, C.byref(count))
    torch.cuda.synchronize()
    check("pairs")
    assert count.value == total and unwritten(out) == 0
    assert np.array_equal(out.cpu().numpy(), cr.cell_pairs(cells, cell_type))
    assert torch.equal(cd, before)
