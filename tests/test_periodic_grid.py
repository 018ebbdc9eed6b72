"""CPU: the pruning rule of the periodic builder's grid route (tests/periodic_grid_reference.py, a transcription of the header of
athena_amd/csrc/periodic_graph.hip) against the yardstick of tests/periodic_reference.py -- every pair with a kept image must be
a candidate -- and the new stats entry in the header, the ctypes binding, the Fortran interface module, the library and the
Python mirror."""
import os
import re

import numpy as np
import pytest

import periodic_grid_reference as gr
import periodic_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = gr.cpu_sets()


@pytest.mark.parametrize("name", list(SETS))
def test_no_pair_with_a_kept_image_is_pruned(name):
    frac, lat, pbc = SETS[name]
    m = frac.shape[0]
    nc, ok = gr.axis_cells(lat, 3.0, pbc, m)
    assert ok and gr.frac_in_range(frac), "the set must meet the rule's preconditions"
    i, j, sh, r, x = pr.structure_edges(frac, lat, 0.5, 3.0, pbc, extra=1 if m >= 600 else 3)
    cand = gr.candidate_matrix(frac, nc)
    kept = np.zeros((m, m), bool)
    kept[i, j] = True
    share = cand.sum() / (m * (m + 1) / 2)
    print(f"{name}: cells {nc}, {i.size} edges on {int(kept.sum())} pairs, surviving share {share:.3f}")
    assert i.size > 0 and np.all(i <= j)
    lost = kept & ~cand
    assert not lost.any(), f"{int(lost.sum())} pairs with a kept image are pruned, first {np.argwhere(lost)[0]}"
    assert np.all(cand[np.arange(m), np.arange(m)])                       # an atom is always its own candidate (self images)
    if max(nc) >= 5:
        assert share < 0.5


def test_cells_per_axis():
    assert gr.axis_cells(gr.cubic(24.0), 3.0)[0] == [7, 7, 7]             # 1 / h = 8 exactly: the margin takes one cell
    assert gr.axis_cells(gr.cubic(12.0), 3.0)[0] == [3, 3, 3]
    assert gr.axis_cells(gr.cubic(11.0), 3.0)[0] == [3, 3, 3]
    assert gr.axis_cells(gr.cubic(8.9), 3.0)[0] == [1, 1, 1]              # two cells prune nothing: one
    assert gr.axis_cells(np.diag([15.0, 15.0, 4.0]), 3.0)[0] == [4, 4, 1]
    assert gr.axis_cells(np.diag([22.0, 19.0, 6.0]), 3.0, (1, 1, 0))[0] == [7, 6, 1]
    assert gr.axis_cells(gr.cubic(3000.0), 3.0)[0] == [128, 128, 128]     # the cap
    assert gr.axis_cells(gr.cubic(24.0), 3.0, m=8)[0] == [1, 4, 4]        # at most 2 m cells
    nc = gr.axis_cells(gr.sheared_cell(), 3.0)[0]
    assert min(nc) >= 4 and max(nc) <= 6
    assert gr.axis_cells(gr.cubic(24.0), 3.0, (0, 0, 0)) == ([1, 1, 1], False)
    assert gr.axis_cells(gr.cubic(24.0), 3.0)[1] and not gr.axis_cells(gr.cubic(3000.0), 3.0)[1]      # (P2): 3 * 2 * 3000 > 4096 * 3
    assert gr.frac_in_range(np.full((1, 3), 64.0)) and not gr.frac_in_range(np.full((1, 3), 2.0 ** 20))


def test_the_boundary_atoms_sit_where_the_rule_says():
    nc = [5, 5, 5]
    plane = np.float32(np.float64(2) / 5)
    f = np.array([[-1e-9, 1.0, 0.0], [plane, np.nextafter(plane, np.float32(0)), np.nextafter(plane, np.float32(1))],
                  [-2.0, 2.999999, -1.2]], np.float32)
    assert gr.cell_coords(f, nc).tolist() == [[4, 0, 0], [2, 1, 2], [0, 4, 3]]
    frac, lat = gr.boundary_set()
    cc = gr.cell_coords(frac, gr.axis_cells(lat, 3.0, (1, 1, 1), frac.shape[0])[0])
    assert cc.min() == 0 and cc.max() == 4 and cc[0, 0] == 4 and cc[1, 0] == 0


def test_the_cutoff_edge_set_has_pairs_on_both_sides_of_the_cutoff():
    frac, lat = gr.cutoff_edge_set()
    i, j, sh, r, x = pr.structure_edges(frac, lat, 0.5, 3.0)
    kept = set(zip(i.tolist(), j.tolist()))
    named = [(2 * k, 2 * k + 1) in kept for k in range(64)]
    assert 16 <= sum(named) <= 48
    nc = gr.axis_cells(lat, 3.0, (1, 1, 1), 128)[0]
    cc = gr.cell_coords(frac, nc)
    apart = [int(np.abs(cc[2 * k] - cc[2 * k + 1]).max()) for k in range(64)]
    assert 0 in apart and 1 in apart and max(apart) == max(nc) - 1        # inside a cell, across a plane, across the wrap
    cand = gr.candidate_matrix(frac, nc)
    assert all(cand[a, b] for a, b in kept)


def test_header_binding_fortran_module_and_library_have_the_stats_entry():
    from athena_amd import _capi

    name = "athena_mp_periodic_stats"
    assert name in _capi.declared_symbols() and name in _capi._PROTOS and len(_capi._PROTOS[name]) == 1
    f90 = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    assert re.search(r'bind\(C, name="%s"\)' % name, f90)
    assert re.search(r"public ::.*\b%s\b" % name, f90)
    assert hasattr(_capi.load(), name)
    header = open(_capi.HEADER_PATH).read()
    assert "ATHENA_MP_PERIODIC_ROUTE" in header


def test_python_mirror_has_periodic_stats():
    from athena_amd import graph

    assert callable(graph.periodic_stats)
    assert graph.PERIODIC_STATS == ("structures_walked", "structures_grid", "walk_pairs", "grid_pairs", "grid_fallbacks")
