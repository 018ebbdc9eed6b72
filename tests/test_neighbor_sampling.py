"""CPU: the yardstick of neighbour sampling against itself (tests/sampling_reference.py).  The loop form is pinned to the whole-array
form on the graph and the seed sets the GPU tests run; the properties the definition promises are checked on it; the selection is
shown to be uniform.  These are conditions on the definition, not on the kernel.  Also: the C ABI, ctypes and Fortran declarations
of the new entries agree."""
import itertools
import os
import re

import numpy as np
import pytest

import sampling_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"athena_mp_sampler_create": 2, "athena_mp_sampler_destroy": 1, "athena_mp_sample_count": 6, "athena_mp_sample_neighbors": 15,
           "athena_mp_sample_neighbors_host": 16, "athena_mp_sample_stats": 1}


@pytest.fixture(autouse=True)
def the_library_declares_what_the_yardstick_defines():
    """the yardstick stands for entries of the library: without them there is nothing it measures"""
    from athena_amd import _capi

    missing = [name for name in ENTRIES if name not in _capi._PROTOS]
    assert not missing, f"athena_amd._capi lacks {missing}"


def _graph(with_edges):
    ia, ja, ne = sr.shape_graph(with_edges)
    rowptr, col, eid = sr.parent_csr(ia, ja)
    return rowptr, col, (eid if with_edges else None)


def _same(a, b):
    return [k for k in a if not (np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k])]


@pytest.mark.parametrize("with_edges", [False, True])
@pytest.mark.parametrize("k", sr.FANOUTS)
def test_the_two_forms_of_the_yardstick_agree(k, with_edges):
    rowptr, col, eid = _graph(with_edges)
    for name, seeds in sr.seed_sets(rowptr.size - 1).items():
        for degrees in ("block", "parent"):
            a = sr.sample_hop(rowptr, col, eid, seeds, k, 77, degrees)
            b = sr.sample_hop_vectorised(rowptr, col, eid, seeds, k, 77, degrees)
            assert _same(a, b) == [], name


def test_the_vectorised_keys_are_the_keys():
    r, p = np.array([0, 1, 159, 2 ** 31 - 1, 12345]), np.array([0, 7, 4999, 2 ** 31 - 2, 3])
    for seed in (0, 1, 2 ** 63, 2 ** 64 - 1):
        assert [int(v) for v in sr.keys_vectorised(seed, r, p)] == [sr.key(seed, a, b) for a, b in zip(r, p)]


@pytest.mark.parametrize("k", sr.FANOUTS)
def test_invariants(k):
    rowptr, col, eid = _graph(True)
    n = rowptr.size - 1
    L = np.diff(rowptr)
    for name, seeds in sr.seed_sets(n).items():
        b = sr.sample_hop(rowptr, col, eid, seeds, k, 5)
        want = L[seeds] if k == 0 else np.minimum(L[seeds], k)
        assert np.array_equal(np.diff(b["rowptr"]), want), "row lengths are min(L, k)"
        for s, r in enumerate(seeds):
            w = b["entry_map"][b["rowptr"][s]:b["rowptr"][s + 1]].astype(np.int64)
            assert (np.diff(w) > 0).all() and (w >= rowptr[r]).all() and (w < rowptr[r + 1]).all(), "ascending and inside the row"
        vm = b["vertex_map"]
        assert np.array_equal(vm[:seeds.size], seeds) and (np.diff(vm[seeds.size:]) > 0).all() and np.unique(vm).size == vm.size
        assert np.array_equal(vm[b["local"]], col[b["entry_map"]]) and np.array_equal(b["edge_map"], eid[b["entry_map"]])
        if b["nnz"]:
            assert set(b["local"][b["local"] >= seeds.size].tolist()) == set(range(seeds.size, b["n_cols"])), "no column without an entry"


def test_a_rows_choice_depends_on_the_seed_and_the_row_alone():
    rowptr, col, eid = _graph(False)
    n = rowptr.size - 1
    hub = sr.ROW_LENGTHS.index(sr.HUB)
    sets = sr.seed_sets(n)
    a, b = sets["m = 5"], sets["all vertices"]
    ba, bb = (sr.sample_hop(rowptr, col, eid, s, 5, 31) for s in (a, b))
    for s, r in enumerate(a):
        sa = ba["entry_map"][ba["rowptr"][s]:ba["rowptr"][s + 1]]
        assert np.array_equal(sa, bb["entry_map"][bb["rowptr"][r]:bb["rowptr"][r + 1]])
    # ... and differs between hops: the hub row is drawn with another seed in each
    blocks = sr.sample(rowptr, col, eid, np.array([hub]), (5, 5, 5), 31)
    picks = []
    for blk in blocks:
        s = int(np.nonzero(blk["vertex_map"][:blk["m"]] == hub)[0][0])
        picks.append(tuple(blk["entry_map"][blk["rowptr"][s]:blk["rowptr"][s + 1]]))
    assert len(set(picks)) == 3
    for outer, inner in zip(blocks, blocks[1:]):
        assert np.array_equal(outer["vertex_map"][:outer["m"]], inner["vertex_map"])


def _frequencies(picks, L):
    """picks [trials, 2] positions -> (single frequencies [L], pair frequencies over the L (L - 1) / 2 pairs)"""
    single = np.bincount(picks.reshape(-1), minlength=L) / picks.shape[0]
    code = picks[:, 0] * L + picks[:, 1]
    pair = np.array([np.count_nonzero(code == i * L + j) for i, j in itertools.combinations(range(L), 2)]) / picks.shape[0]
    return single, pair


def test_the_selection_is_uniform():
    """A row of 5 entries at k = 2: every entry is chosen with probability 0.4, every pair with 0.1.  Over 20 000 trials the standard
    deviations are 0.0035 and 0.0021; the bounds are 0.02 and 0.012 (more than 5 sigma).  Over 20 000 values of seed at a fixed row,
    and over 20 000 rows at a fixed seed."""
    T, L = 20000, 5
    for seeds, rows in ((np.arange(T), np.full(T, 3)), (np.full(T, 12345), np.arange(T))):
        keys = np.stack([sr.keys_vectorised(seeds, rows, np.full(T, p)) for p in range(L)], axis=1)
        picks = np.sort(np.argsort(keys, axis=1)[:, :2], axis=1)
        for t in (0, 1, T - 1):
            assert list(picks[t]) == sr.choose(int(seeds[t]), int(rows[t]), L, 2)
        single, pair = _frequencies(picks, L)
        assert np.abs(single - 0.4).max() <= 0.02, single
        assert np.abs(pair - 0.1).max() <= 0.012, pair


def test_declarations_agree():
    from athena_amd import _capi

    header = open(os.path.join(ROOT, "include", "athena_mp.h")).read()
    fortran = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    build = open(os.path.join(ROOT, "athena_amd", "csrc", "build.sh")).read()
    assert " neighbor_sample.hip " in build
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "neighbor_sample_run.f90" in entry
    for name, n_args in ENTRIES.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in athena_mp.h"
        assert len(m.group(1).split(",")) == n_args
        assert len(_capi._PROTOS[name]) == n_args
        m = re.search(r"function %s\(([^)]*)\)" % name, fortran)
        assert m and 'name="%s"' % name in fortran, f"{name} has no interface in athena_mp_c.f90"
        assert len(m.group(1).replace("&", "").split(",")) == n_args
    assert "DEPENDS ON (seed, r) ALONE" in header
