"""CPU: the yardstick of the batched radius-graph builder against the definition evaluated on ALL pairs under a same-cloud
mask, the edge_offsets it implies, and the two new entries in the header, the ctypes binding and the Fortran interface module."""
import os
import re

import numpy as np
import pytest

from radius_batch_reference import all_pairs_batched, cloud_sizes, edge_offsets_of, reference_pairs_batched
from radius_reference import degree_radius, reference_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("athena_mp_radius_pairs_batched", "athena_mp_radius_graph_batched_host")


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_reference_pairs_batched_equals_the_definition_on_all_pairs_of_one_cloud(dim):
    """clouds that overlap in space, empty clouds first, in the middle and last, a one-point cloud, coincident points"""
    rng = np.random.Generator(np.random.PCG64(dim))
    off = np.array([0, 0, 400, 401, 401, 403, 1100, 1500, 1500], np.int64)
    p = rng.random((1500, dim)).astype(np.float32)
    p[402] = p[401]                                   # a two-point cloud of coincident points
    p[900] = p[450]                                   # coincident points of one cloud are joined
    p[1200] = p[10]                                   # ... of two clouds are not
    r = degree_radius(500, 10.0, dim)
    i, j, c, eoff = reference_pairs_batched(p, off, r)
    ai, aj, ac = all_pairs_batched(p, off, r)
    assert i.size > 1500
    for x, y in ((i, ai), (j, aj), (c, ac)):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert np.all(i < j) and np.all(np.diff(i * 1500 + j) > 0)             # lexicographic in the global (i, j), no duplicates
    assert np.any((i == 401) & (j == 402)) and np.any((i == 450) & (j == 900)) and not np.any((i == 10) & (j == 1200))
    # the cloud-blind list of all points has pairs the batch must not have
    bi, bj, _ = reference_pairs(p, r)
    assert bi.size > i.size
    # edge_offsets: where each cloud's pairs start == the number of pairs whose i is below offsets[b]
    assert eoff.dtype == np.int64 and eoff[0] == 0 and eoff[-1] == i.size
    assert np.array_equal(eoff, edge_offsets_of(i, off))
    assert np.array_equal(eoff, [int((i < o).sum()) for o in off])
    assert eoff[1] == 0 and eoff[3] == eoff[4] and eoff[5] == eoff[4] + 1 and eoff[7] == eoff[8]


def test_reference_pairs_batched_of_nothing():
    z = np.zeros((0, 3), np.float32)
    for off in ([0], [0, 0, 0]):
        i, j, c, eoff = reference_pairs_batched(z, off, 0.5)
        assert i.size == j.size == 0 and c.shape == (0, 3) and np.array_equal(eoff, np.zeros(len(off), np.int64))


def test_cloud_sizes_are_the_clipped_rounded_normal():
    s = cloud_sizes(np.random.Generator(np.random.PCG64(5)), 3000)
    assert s.min() >= 4 and s.max() <= 29 and 17.5 < s.mean() < 18.5 and np.unique(s).size > 10


def test_header_binding_and_fortran_module_declare_the_entries():
    from athena_amd import _capi

    declared = _capi.declared_symbols()
    f90 = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    for name in ENTRIES:
        assert name in declared, name
        assert name in _capi._PROTOS, name
        assert re.search(r'bind\(C, name="%s"\)' % name, f90), name
        assert re.search(r"public ::.*\b%s\b" % name, f90), name
    assert len(_capi._PROTOS["athena_mp_radius_pairs_batched"]) == 11
    assert len(_capi._PROTOS["athena_mp_radius_graph_batched_host"]) == 15
    header = open(_capi.HEADER_PATH).read()
    assert "with offsets[b] added to both indices" in header


def test_library_exports_the_entries():
    from athena_amd import _capi

    lib = _capi.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_python_mirror_has_the_two_builders():
    from athena_amd.graph import DeviceGraph, graph_type

    assert callable(DeviceGraph.from_point_clouds) and callable(graph_type.generate_radius_batch_adjacency_device)
