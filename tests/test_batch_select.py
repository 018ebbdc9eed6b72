"""CPU: the yardstick of the mini-batch selection (tests/batch_reference.py) -- a slice of a block-diagonal handle equals the handle
rebuilt from the selection's own renumbered pair list -- and the three new entries in the header, the ctypes binding, the Fortran
interface module, the library and the package."""
import os
import re

import numpy as np
import pytest

import batch_reference as br
import periodic_reference as pr
from helpers import csr_from_index_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "msgpass_chemical_head.xyz")
ENTRIES = ("athena_mp_batch_plan_create", "athena_mp_batch_plan_destroy", "athena_mp_batch_select")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _arrays(n, pairs, loops):
    g = csr_from_index_list(n, pairs, self_loops=loops)
    return br.handle_arrays(g.adj_ia, g.adj_ja, pairs.shape[1])


def _slice_equals_rebuild(n, pairs, off, eoff, loops, sel, what):
    parent = _arrays(n, pairs, loops)
    child, voff, ceoff, vmap, emap = br.select_reference(parent, off, eoff, sel)
    cp, n_child = br.child_pairs(pairs, off, eoff, sel)
    assert n_child == voff[-1] == vmap.size and cp.shape[1] == ceoff[-1] == emap.size, what
    g = csr_from_index_list(n_child, cp, self_loops=loops)
    # the arrays that matter: the forward CSR against the reference-convention builder itself ...
    assert np.array_equal(child["rowptr"] + 1, g.adj_ia), what
    assert np.array_equal(child["col"] + 1, g.adj_ja[0]) and np.array_equal(child["eid"] + 1, g.adj_ja[1]), what
    # ... and every array against the handle of that CSR
    want = br.handle_arrays(g.adj_ia, g.adj_ja, cp.shape[1])
    for k in br.NAMES:
        assert child[k].dtype == want[k].dtype and np.array_equal(child[k].view(np.int32), want[k].view(np.int32)), (what, k)
    # the maps say where every vertex and edge column of the batch sits in the dataset
    sel = np.asarray(sel)
    for t, s in enumerate(sel):
        assert np.array_equal(vmap[voff[t]:voff[t + 1]], np.arange(off[s], off[s + 1])), what
        assert np.array_equal(emap[ceoff[t]:ceoff[t + 1]], np.arange(eoff[s], eoff[s + 1])), what
    return child


@pytest.fixture(scope="module")
def golden_batch():
    from athena_amd import io

    frac, lat, off = io.structures_from_frames(io.read_extxyz(FIXTURE))
    batch = pr.reference_edges(frac, lat, off, 0.5, 3.0)
    assert lat.shape[0] == 40 and batch["pairs"].shape[1] == 1849
    return int(off[-1]), batch["pairs"], np.asarray(off, np.int32), batch["edge_offsets"]


@pytest.mark.parametrize("loops", [False, True])
def test_slice_equals_rebuild_on_the_golden_frames(golden_batch, loops):
    n, pairs, off, eoff = golden_batch
    B = off.size - 1
    rng = _rng(5)
    for what, sel in (("first", [0]), ("last", [B - 1]), ("reversed", list(range(B))[::-1]), ("repeat", [3, 17, 3, 3, 9]),
                      ("shuffled half", rng.permutation(B)[:B // 2])):
        _slice_equals_rebuild(n, pairs, off, eoff, loops, sel, f"golden, {what}, loops {loops}")


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_slice_equals_rebuild_on_random_block_diagonal_multigraphs(seed, loops):
    rng = _rng(seed)
    sizes = [int(v) for v in rng.integers(2, 12, 14)]
    sizes[4] = 0                                                           # an empty structure
    sizes[9] = 1                                                           # one atom with self pairs
    sizes[13] = 0                                                          # ... and an empty one at the end
    pairs, off, eoff = br.random_block_pairs(rng, sizes)
    assert eoff[10] - eoff[9] >= 2 and np.all(pairs[:, eoff[9]:eoff[10]] == off[9] + 1)
    n, B = int(off[-1]), len(sizes)
    for what, sel in (("empty alone", [4]), ("one atom alone", [9]), ("with empty, one atom, repeat", [9, 4, 2, 9, 13, 0, 2]),
                      ("reversed", list(range(B))[::-1]), ("shuffled", rng.permutation(B)[:7])):
        child = _slice_equals_rebuild(n, pairs, off, eoff, loops, sel, f"seed {seed}, {what}, loops {loops}")
        assert child["rowptr"][-1] == child["col"].size


@pytest.mark.parametrize("loops", [False, True])
def test_identity_selection_returns_the_parent(golden_batch, loops):
    n, pairs, off, eoff = golden_batch
    parent = _arrays(n, pairs, loops)
    child, voff, ceoff, vmap, emap = br.select_reference(parent, off, eoff, np.arange(off.size - 1))
    for k in br.NAMES:
        assert np.array_equal(child[k].view(np.int32), parent[k].view(np.int32)), k
    assert np.array_equal(voff, off) and np.array_equal(ceoff, eoff)
    assert np.array_equal(vmap, np.arange(n)) and np.array_equal(emap, np.arange(pairs.shape[1]))


def test_pairs_of_arrays_recovers_the_pair_list(golden_batch):
    n, pairs, off, eoff = golden_batch
    for loops in (False, True):
        assert np.array_equal(br.pairs_of_arrays(_arrays(n, pairs, loops), pairs.shape[1]), pairs)


def test_header_binding_and_fortran_module_declare_the_entries():
    from athena_amd import _capi

    declared = _capi.declared_symbols()
    f90 = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    for name in ENTRIES:
        assert name in declared, name
        assert name in _capi._PROTOS, name
        assert re.search(r'bind\(C, name="%s"\)' % name, f90), name
        assert re.search(r"public ::.*\b%s\b" % name, f90), name
    assert len(_capi._PROTOS["athena_mp_batch_plan_create"]) == 5 and len(_capi._PROTOS["athena_mp_batch_select"]) == 8
    header = open(_capi.HEADER_PATH).read()
    assert "typedef struct athena_mp_batch_plan athena_mp_batch_plan;" in header


def test_library_and_package_export_the_entries():
    import athena_amd
    from athena_amd import _capi

    lib = _capi.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert athena_amd.DeviceDataset is athena_amd.batching.DeviceDataset and athena_amd.Batch is athena_amd.batching.Batch
    for name in ("select", "batches", "sizes", "close"):
        assert callable(getattr(athena_amd.DeviceDataset, name)), name
    for name in ("take_vertices", "take_edges", "take_structures"):
        assert callable(getattr(athena_amd.Batch, name)), name
