"""CPU: the yardstick of the radius-graph builder against the definition evaluated on ALL pairs, and the three new
entries in the header, the ctypes binding and the Fortran interface module."""
import os
import re

import numpy as np
import pytest

from radius_reference import all_pairs, degree_radius, reference_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("athena_mp_radius_pairs", "athena_mp_graph_create_from_edges_dev", "athena_mp_radius_graph_host")


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_reference_pairs_equals_the_definition_on_all_pairs(dim):
    rng = np.random.Generator(np.random.PCG64(dim))
    p = rng.random((3000, dim)).astype(np.float32)
    p[1234] = p[77]                                   # two points at the same place are joined
    r = degree_radius(3000, 12.0, dim)
    a, b = reference_pairs(p, r), all_pairs(p, r)
    assert a[0].size > 3000
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert np.all(a[0] < a[1])
    k = a[0] * 3000 + a[1]
    assert np.all(np.diff(k) > 0)                      # lexicographic, no duplicates
    assert np.any((a[0] == 77) & (a[1] == 1234))


def test_reference_pairs_translated_cloud_has_borderline_pairs_decided_in_fp32():
    """around 1000 the fp32 spacing is 6e-5: distances come in few values and many candidates sit on the radius"""
    rng = np.random.Generator(np.random.PCG64(9))
    p = (rng.random((2000, 3)) * 0.5 + 1000.0).astype(np.float32)
    r = 0.04
    a, b = reference_pairs(p, r), all_pairs(p, r)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_header_binding_and_fortran_module_declare_the_entries():
    from athena_amd import _capi

    declared = _capi.declared_symbols()
    f90 = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    for name in ENTRIES:
        assert name in declared, name
        assert name in _capi._PROTOS, name
        assert re.search(r'bind\(C, name="%s"\)' % name, f90), name
    assert len(_capi._PROTOS["athena_mp_radius_pairs"]) == 8
    assert len(_capi._PROTOS["athena_mp_graph_create_from_edges_dev"]) == len(_capi._PROTOS["athena_mp_graph_create_from_edges"])
    assert len(_capi._PROTOS["athena_mp_radius_graph_host"]) == 12


def test_library_exports_the_entries():
    from athena_amd import _capi

    lib = _capi.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_python_mirror_has_the_two_builders():
    from athena_amd.graph import DeviceGraph, graph_type

    assert callable(DeviceGraph.from_points) and callable(graph_type.generate_radius_adjacency_device)
