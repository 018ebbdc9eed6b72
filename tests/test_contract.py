"""CPU: the yardstick of the graph contraction against itself (tests/contract_reference.py).  The sorted transcription of the
definition is pinned to the dictionary form on every shape class the GPU tests run; the properties the definition promises are
checked on it (strictly ascending lists, the identity, composition); the inputs of the GPU tests are shown to be what those tests
need (three radix tiles, one pass, a key beyond 32 bits, a member run across a tile).  Also: the transcriptions of the two small
entries, the C ABI, ctypes and Fortran declarations of the new entries, and the argument checks of the two Python methods that need
no device."""
import os
import re

import numpy as np
import pytest

import contract_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"athena_mp_contract_pairs": 22, "athena_mp_contract_pairs_host": 22, "athena_mp_contract_stats": 1, "athena_mp_graph_pairs": 3,
           "athena_mp_cell_pairs": 7}
CASES = cr.shape_cases()
NAMES = [c[0] for c in CASES]


@pytest.fixture(autouse=True)
def the_library_declares_what_the_yardstick_defines():
    """the yardstick stands for entries of the library: without them there is nothing it measures"""
    from athena_amd import _capi

    missing = [name for name in ENTRIES if name not in _capi._PROTOS]
    assert not missing, f"athena_amd._capi lacks {missing}"


def _ascending(a):
    k = a[:, 0].astype(np.int64) * (2 ** 32) + a[:, 1]
    return bool((np.diff(k) > 0).all())


@pytest.mark.parametrize("c", range(len(CASES)), ids=NAMES)
def test_the_two_forms_of_the_yardstick_agree(c):
    name, kw = CASES[c]
    a, b = cr.contract(*cr.args_of(kw)), cr.brute_force(*cr.args_of(kw))
    assert cr.same(a, b) == [] and (a["P"], a["M"], a["bits"], a["largest"]) == (b["P"], b["M"], b["bits"], b["largest"])


@pytest.mark.parametrize("c", range(len(CASES)), ids=NAMES)
def test_invariants(c):
    name, kw = CASES[c]
    r = cr.contract(*cr.args_of(kw))
    E, P, M = kw["pairs"].shape[0], r["P"], r["M"]
    assert r["coarse_pairs"].shape == (P, 2) and r["members"].shape == (M, 2) and r["rowptr"].shape == (P + 1,) and r["edge_pair"].shape == (E,)
    assert _ascending(r["coarse_pairs"]) and _ascending(r["members"])
    assert r["rowptr"][0] == 0 and r["rowptr"][-1] == M and (np.diff(r["rowptr"]) > 0).all()
    if kw["mode"] == 0:
        assert (r["coarse_pairs"][:, 0] < r["coarse_pairs"][:, 1]).all()
    assert (r["edge_pair"] > 0).sum() == M
    assert np.array_equal(r["edge_pair"][r["members"][:, 1] - 1], r["members"][:, 0])
    # mean pooling: the weights of a coarse pair add up to one, to rounding
    sums = np.bincount(r["members"][:, 0] - 1, r["weights"].astype(np.float64), minlength=P)
    assert np.allclose(sums, 1.0, rtol=0, atol=1e-6)


def test_the_inputs_are_what_the_gpu_tests_need():
    kw = cr.case("three tiles, 300 clusters, mode 0")
    r = cr.contract(*cr.args_of(kw))
    p = kw["pairs"]
    assert p.shape[0] == 2 * 4096 + 77 and r["bits"] == 19 and (kw["row_cluster"] == 0).any()
    assert (p == 0).all(axis=1).any() and ((p[:, 0] == 0) != (p[:, 1] == 0)).any() and ((p[:, 0] == p[:, 1]) & (p[:, 0] > 0)).any()
    assert r["largest"] > 1 and 0 < r["M"] < p.shape[0]
    for name in ("7 clusters, one pass", "7 x 5 clusters, one pass, mode 1"):
        assert cr.contract(*cr.args_of(cr.case(name)))["bits"] <= 8
    kw = cr.case("identity over 2^17 + 3 vertices")
    r = cr.contract(*cr.args_of(kw))
    assert r["bits"] == 37 and r["coarse_pairs"].max() == 2 ** 17 + 3 and r["largest"] >= 64
    r = cr.contract(*cr.args_of(cr.case("hub of thousands")))
    assert r["largest"] > 4096
    hub = int(np.argmax(np.diff(r["rowptr"])))
    assert 0 < hub < r["P"] - 1 and r["rowptr"][hub] // 4096 != (r["rowptr"][hub + 1] - 1) // 4096
    assert cr.contract(*cr.args_of(cr.case("E = 0")))["P"] == 0
    r = cr.contract(*cr.args_of(cr.case("every edge dropped")))
    assert (r["P"], r["M"]) == (0, 0) and r["rowptr"].tolist() == [0]
    r = cr.contract(*cr.args_of(cr.case("P = 1")))
    assert r["P"] == 1 and r["M"] > 1 and r["coarse_pairs"].tolist() == [[4, 8]]
    dims = {(cr.case(f"mode {m}, dim {d}")["mode"], cr.case(f"mode {m}, dim {d}")["row_points"].shape[1]) for m in (0, 1) for d in (1, 2, 3)}
    assert len(dims) == 6


def test_the_identity_on_a_simple_ascending_list_returns_it():
    r = cr._rng(40)
    n = 500
    k = np.unique(r.integers(0, n * n, 3000))
    u, v = k // n + 1, k % n + 1
    keep = u < v
    pairs = np.stack([u[keep], v[keep]], axis=1).astype(np.int32)
    E = pairs.shape[0]
    for form in (cr.contract, cr.brute_force):
        got = form(pairs, n, n, None, None, n, n, 0)
        assert np.array_equal(got["coarse_pairs"], pairs) and np.array_equal(got["edge_pair"], np.arange(1, E + 1))
        assert np.array_equal(got["rowptr"], np.arange(E + 1)) and (got["weights"] == 1).all() and got["P"] == got["M"] == E


@pytest.mark.parametrize("mode", [0, 1])
def test_composition(mode):
    """contracting by c1 and then the result by c2 gives the coarse pairs of contracting by c2 after c1"""
    kw = cr._random_case(41 + mode, 3000, 700, 700 if mode == 0 else 450, 90, 90 if mode == 0 else 60, mode, 0)
    r = cr._rng(43)
    m2r, m2c = 11, 11 if mode == 0 else 7
    c2r = r.integers(0, m2r + 1, kw["m_rows"]).astype(np.int32)
    c2c = c2r if mode == 0 else r.integers(0, m2c + 1, kw["m_cols"]).astype(np.int32)
    first = cr.contract(*cr.args_of(kw))
    second = cr.contract(first["coarse_pairs"], kw["m_rows"], kw["m_cols"], c2r, c2c, m2r, m2c, mode)
    through = lambda c1, c2: np.where(c1 > 0, np.concatenate([[0], c2])[c1], 0).astype(np.int32)
    direct = cr.contract(kw["pairs"], kw["n_rows"], kw["n_cols"], through(kw["row_cluster"], c2r), through(kw["col_cluster"], c2c), m2r, m2c, mode)
    assert second["P"] > 1 and np.array_equal(second["coarse_pairs"], direct["coarse_pairs"])
    # and the members: a fine edge's pair on the second level is the second-level pair of its first-level pair
    lifted = np.where(first["edge_pair"] > 0, np.concatenate([[0], second["edge_pair"]])[first["edge_pair"]], 0)
    assert np.array_equal(lifted, direct["edge_pair"])


def test_the_yardstick_refuses_what_the_library_refuses():
    kw = cr.case("mode 1, dim 2")
    bad = lambda **ch: cr.args_of(dict(kw, **ch))
    p = kw["pairs"].copy(); p[5, 1] = kw["n_cols"] + 1; p[9, 0] = -1
    rc = kw["row_cluster"].copy(); rc[3] = kw["m_rows"] + 1
    cc = kw["col_cluster"].copy(); cc[8] = -1
    for args, why in ((bad(mode=2), "mode"), (bad(n_rows=-1), "size"), (bad(mode=0), "one set"), (bad(row_cluster=None), "identity"),
                      (bad(col_points=None), "only one"), (bad(row_points=np.zeros((kw["m_rows"], 4), np.float32)), "dim"),
                      (bad(pairs=p), r"pairs\(:,6\)"),
                      (bad(row_cluster=rc), r"row_cluster\(4\)"), (bad(col_cluster=cc), r"col_cluster\(9\)")):
        for form in (cr.contract, cr.brute_force):
            with pytest.raises(cr.Refused, match=why):
                form(*args)
    # int32 cluster counts need at most 31 + 31 key bits: the bound of 62 cannot be reached through this interface
    assert cr.bits_for(2 ** 31 - 1) == 31


def test_graph_pairs_and_cell_pairs_transcriptions():
    # the edge index of the from_edges handle of pairs (3, 1), (2, 2), (1, 3) with a column nothing carries in between
    rowptr, col, eid = np.array([0, 2, 3, 5]), np.array([2, 2, 1, 0, 0]), np.array([0, 3, 1, 0, 3])
    e_rowptr, e_row, e_entry = np.array([0, 2, 3, 3, 5]), np.array([0, 2, 1, 0, 2]), np.array([0, 3, 2, 1, 4])
    assert all(eid[e_entry[k]] == e for e in range(4) for k in range(e_rowptr[e], e_rowptr[e + 1]))
    assert cr.graph_pairs(e_rowptr, e_row, e_entry, col).tolist() == [[1, 3], [2, 2], [0, 0], [1, 3]]
    cells = np.array([[5, 6, 7, 8]], np.int32)
    assert cr.cell_pairs(cells[:, :2], 1).tolist() == [[5, 6]]
    assert cr.cell_pairs(cells[:, :3], 2).tolist() == [[5, 6], [5, 7], [6, 7]]
    assert cr.cell_pairs(cells, 3).tolist() == [[5, 6], [6, 7], [7, 8], [8, 5]]
    assert cr.cell_pairs(cells, 4).tolist() == [[5, 6], [5, 7], [5, 8], [6, 7], [6, 8], [7, 8]]


@pytest.mark.parametrize("cell_type,shape", [(1, (5, 3)), (2, (5, 3)), (3, (5, 3)), (4, (3, 2, 2))])
def test_the_edge_graph_of_a_structured_mesh(cell_type, shape):
    cells, nvert, edges, boundary, pts = cr.grid_mesh(cell_type, *shape)
    assert cells.shape[1] == cr.NV[cell_type] and cells.min() == 1 and cells.max() == nvert and pts.shape[0] == nvert
    r = cr.contract(cr.cell_pairs(cells, cell_type), nvert, nvert, None, None, nvert, nvert, 0)
    assert r["P"] == edges and r["M"] == cells.shape[0] * len(cr.LOCAL[cell_type])
    count = np.diff(r["rowptr"])
    if boundary is not None:
        assert (count == 1).sum() == boundary and count.max() == (1 if cell_type == 1 else 2)
    # a cell with a repeated vertex loses that pair only
    if cell_type == 2:
        bad = cells.copy(); bad[0, 1] = bad[0, 0]
        d = cr.contract(cr.cell_pairs(bad, cell_type), nvert, nvert, None, None, nvert, nvert, 0)
        assert d["M"] == r["M"] - 1 and d["edge_pair"][0] == 0


def test_header_binding_and_fortran_module_declare_the_entries():
    from athena_amd import _capi

    header = open(os.path.join(ROOT, "include", "athena_mp.h")).read()
    fortran = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    build = open(os.path.join(ROOT, "athena_amd", "csrc", "build.sh")).read()
    assert " contract.hip " in build
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "contract_run.f90" in entry
    assert "athena_amd/fortran/contract_run\n" in open(os.path.join(ROOT, ".gitignore")).read()
    for name, n_args in ENTRIES.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in athena_mp.h"
        assert len(m.group(1).split(",")) == n_args
        assert len(_capi._PROTOS[name]) == n_args
        m = re.search(r"function %s\(([^)]*)\)" % name, fortran)
        assert m and 'name="%s"' % name in fortran, f"{name} has no interface in athena_mp_c.f90"
        assert len(m.group(1).replace("&", "").split(",")) == n_args


def test_argument_checks_of_the_python_methods_that_need_no_device():
    import torch
    from athena_amd import DeviceGraph

    pairs = torch.tensor([[1, 2], [2, 3]], dtype=torch.int32)
    cluster = np.array([1, 1, 2], np.int32)
    fc = DeviceGraph.from_contraction
    with pytest.raises(ValueError, match="needs n_vertices"):
        fc(pairs, cluster, 2)
    with pytest.raises(ValueError, match=r"int32 tensor \[E, 2\]"):
        fc(pairs.to(torch.int64), cluster, 2, n_vertices=3)
    with pytest.raises(ValueError, match=r"int32 tensor \[E, 2\]"):
        fc(pairs.t().contiguous()[:, :1].repeat(1, 3), cluster, 2, n_vertices=3)
    with pytest.raises(ValueError, match=r"int32 tensor \[E, 2\]"):
        fc(np.array([[1, 2]], np.int32), cluster, 2, n_vertices=3)
    with pytest.raises(ValueError, match="cluster must have 3 rows, not 2"):
        fc(pairs, cluster[:2], 2, n_vertices=3)
    with pytest.raises(ValueError, match="points must have 2 rows, not 3"):
        fc(pairs, cluster, 2, n_vertices=3, points=np.zeros((3, 2), np.float32))
    with pytest.raises(ValueError, match="needs col_cluster"):
        fc(pairs, cluster, 2, n_vertices=3, n_col_vertices=4)
    with pytest.raises(ValueError, match="col_cluster needs n_col_clusters"):
        fc(pairs, cluster, 2, col_cluster=cluster, n_vertices=3)
    with pytest.raises(ValueError, match="needs col_points"):
        fc(pairs, cluster, 2, col_cluster=cluster, n_col_clusters=2, n_vertices=3, points=np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError, match="two-set mode"):
        fc(pairs, cluster, 2, n_vertices=3, col_points=np.zeros((2, 2), np.float32))
    g = DeviceGraph.__new__(DeviceGraph)                                       # a handle's sizes without a device behind them
    g.handle, g.n_rows, g.n_cols, g.nnz, g.n_edge_cols = None, 3, 3, 4, 0
    try:
        with pytest.raises(ValueError, match="no edge columns"):
            fc(g, cluster, 2)
        g.n_edge_cols = 2
        with pytest.raises(ValueError, match="a DeviceGraph knows its own"):
            fc(g, cluster, 2, n_vertices=3)
    finally:
        g.handle = None
    fm = DeviceGraph.from_mesh
    tri = np.array([[1, 2, 3]], np.int32)
    with pytest.raises(ValueError, match="cell_type must be"):
        fm(tri, 3, 5)
    with pytest.raises(ValueError, match="cell_type must be"):
        fm(tri, 3, "hexagon")
    with pytest.raises(ValueError, match=r"cells must be \[n_cells, 4\] for cell_type 4"):
        fm(tri, 3, "tetrahedron")
    with pytest.raises(ValueError, match="points must have 3 rows, not 2"):
        fm(tri, 3, 2, points=np.zeros((2, 2), np.float32))
