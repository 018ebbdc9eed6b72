"""GPU: athena_mp_sample_neighbors with each pointer operand in turn placed 1 or 2 elements past a 512-byte boundary (a 4- or an
8-byte aligned address) between guard words, the rest on 512-byte boundaries, the way test_gpu_grid_clusters_unaligned.py places the
operands of the clusters.  The seeds hold the hub, whole rows and drawn rows.  The results equal the yardstick's, every output
element is written, no guard word is, and the seeds are unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest

import sampling_reference as sr
from helpers import placed, placed_out, unwritten

pytestmark = pytest.mark.gpu

OPERANDS = ("seeds", "vertex_map", "entry_map", "edge_map")
K, SEED = 5, 123


@functools.lru_cache(None)
def _case():
    ia, ja, ne = sr.shape_graph(True)
    rowptr, col, eid = sr.parent_csr(ia, ja)
    seeds = sr.seed_sets(rowptr.size - 1)["the length rows"][::-1].copy()
    return ia, ja, ne, seeds, sr.sample_hop(rowptr, col, eid, seeds, K, SEED, "block")


@pytest.mark.parametrize("at", [1, 2])
@pytest.mark.parametrize("operand", OPERANDS)
def test_one_operand_between_guards(dev, operand, at):
    import torch
    from athena_amd import DeviceGraph, NeighborSampler, _capi

    ia, ja, ne, seeds, want = _case()
    g = DeviceGraph(ia, ja, n_edge_cols=ne)
    sampler = NeighborSampler(g)
    off = lambda name: at if name == operand else 0
    sd = placed(seeds + np.int32(1), dev, off("seeds"))
    before = sd.clone()
    shapes = dict(vertex_map=want["n_cols"], entry_map=want["nnz"], edge_map=want["nnz"])
    outs = {k: placed_out((count,), torch.int32, dev, off(k)) for k, count in shapes.items()}
    for name, t in [("seeds", sd)] + [(k, v[0]) for k, v in outs.items()]:
        assert t.data_ptr() % 512 == 4 * off(name)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    n_cols, nnz, block = C.c_int32(), C.c_int64(), C.c_void_p()
    _capi.use_torch_stream()
    _capi.call("athena_mp_sample_neighbors", sampler._plan, seeds.size, ptr(sd), K, C.c_uint64(SEED), 0, ptr(outs["vertex_map"][0]),
               want["n_cols"], ptr(outs["entry_map"][0]), want["nnz"], ptr(outs["edge_map"][0]), want["nnz"], C.byref(n_cols), C.byref(nnz),
               C.byref(block))
    torch.cuda.synchronize()
    child = DeviceGraph.borrow(block)
    child._borrowed = False
    assert (n_cols.value, nnz.value) == (want["n_cols"], want["nnz"])
    for k in OPERANDS[1:]:
        t, check = outs[k]
        check(k)
        assert unwritten(t) == 0, k
        assert np.array_equal(t.cpu().numpy() - 1, want[k]), k                 # 1-based through the C ABI
    assert np.array_equal(child.export("col"), want["local"]) and np.array_equal(child.export("rowptr"), want["rowptr"])
    assert torch.equal(sd, before)
    child.close()
    sampler.close()
    g.close()
