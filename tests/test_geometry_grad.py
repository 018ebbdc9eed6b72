"""CPU: the yardstick of the geometry gradients (tests/geometry_reference.py) -- its float64 twin against central differences of a
frozen-edge-set energy, the fp32 definition against the twin, points mode against a dense O(n^2) evaluation -- and the four new
entries in the header, the ctypes binding and the Fortran interface module."""
import os
import re

import numpy as np

import geometry_reference as gr
import periodic_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("athena_mp_edge_grad_to_points", "athena_mp_periodic_grad", "athena_mp_edge_grad_to_points_host",
           "athena_mp_periodic_grad_host")
CMIN, CMAX = 0.5, 3.0
MARGIN = 1e-4


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _batch(seed=3):
    """structures of all three random_cell kinds plus two one-atom structures -> frac, lat, offsets"""
    rng = _rng(seed)
    sizes = [("cubic", 9), ("small", 4), ("skewed", 3), ("small", 1), ("skewed", 1), ("skewed", 2), ("small", 3)]
    rows = [rng.random((m, 3)).astype(np.float32) for _, m in sizes]
    lat = np.array([pr.random_cell(rng, kind, 8) for kind, _ in sizes], np.float32)
    off = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int32)
    return np.concatenate(rows), lat, off


def _frozen_edges(frac, lat, off):
    """the builder's edges with everything integer frozen: global i, j, the structure, shift - wrap (what is added to f_i - f_j), and
    the batch dict of the yardstick"""
    per = [pr.structure_edges(frac[off[s]:off[s + 1]], lat[s], CMIN, CMAX) for s in range(lat.shape[0])]
    batch = pr.assemble(per, off, CMAX)
    i, j = batch["pairs"][0].astype(np.int64) - 1, batch["pairs"][1].astype(np.int64) - 1
    f = frac[i] - frac[j]
    wrap = np.ceil(f - np.float32(0.5))
    sid = np.repeat(np.arange(lat.shape[0]), np.diff(batch["edge_offsets"]))
    return i, j, sid, batch["shift"].astype(np.float64) - wrap.astype(np.float64), batch


def _csr(n, pairs):
    from athena_amd.graph import graph_type

    g = graph_type()
    g.set_num_vertices(n, 1)
    g.generate_adjacency(pairs)
    return gr.csr_of_graph(g)


def _geometry64(frac64, lat64, i, j, sid, add):
    x = np.einsum("ea,eac->ec", (frac64[i] - frac64[j]) + add, lat64[sid])
    return x, np.sqrt((x * x).sum(1)) / float(np.float32(CMAX))


def test_the_float64_twin_equals_central_differences_of_a_frozen_edge_set_energy():
    frac, lat, off = _batch()
    B, n = lat.shape[0], frac.shape[0]
    # no r within MARGIN of a cutoff: the edge set is the same a margin inside and a margin outside
    for s in range(B):
        rows = frac[off[s]:off[s + 1]]
        inner = pr.structure_edges(rows, lat[s], CMIN + MARGIN, CMAX - MARGIN)[0].size
        outer = pr.structure_edges(rows, lat[s], CMIN - MARGIN, CMAX + MARGIN)[0].size
        assert inner == outer, f"structure {s}: an r within {MARGIN} of a cutoff"
    i, j, sid, add, batch = _frozen_edges(frac, lat, off)
    E = i.size
    assert E > 250 and (i == j).sum() > 50
    coef = _rng(8).uniform(-1, 1, (E, 3))

    def energy(f64, l64):
        x, feature = _geometry64(f64, l64, i, j, sid, add)
        return float(np.sin(3.0 * feature).sum() + (coef * x).sum())

    f0, l0 = frac.astype(np.float64), lat.astype(np.float64)
    x, feature = _geometry64(f0, l0, i, j, sid, add)
    rowptr, col, eid = _csr(n, batch["pairs"])
    got = gr.structures_grad(rowptr, col, eid, l0, off, batch["edge_offsets"], x, CMAX, dfeature=3.0 * np.cos(3.0 * feature), dvec=coef,
                             dtype=np.float64)
    h = 1e-6
    dfrac = np.zeros((n, 3))
    for a in range(n):
        for k in range(3):
            p, m = f0.copy(), f0.copy()
            p[a, k] += h
            m[a, k] -= h
            dfrac[a, k] = (energy(p, l0) - energy(m, l0)) / (2 * h)
    dlat = np.zeros((B, 3, 3))
    for s in range(B):
        for a in range(3):
            for c in range(3):
                p, m = l0.copy(), l0.copy()
                p[s, a, c] += h
                m[s, a, c] -= h
                dlat[s, a, c] = (energy(f0, p) - energy(f0, m)) / (2 * h)
    e_frac = np.abs(got["frac"] - dfrac).max() / np.abs(dfrac).max()
    e_lat = np.abs(got["lat"] - dlat).max() / np.abs(dlat).max()
    # the direct form of the cell gradient, sum v (x) gx, is the same number
    _, gx = gr.edge_terms(x, CMAX, 3.0 * np.cos(3.0 * feature), coef, np.float64)
    v = (f0[i] - f0[j]) + add
    direct = np.zeros((B, 3, 3))
    np.add.at(direct, sid, v[:, :, None] * gx[:, None, :])
    e_direct = np.abs(got["lat"] - direct).max() / np.abs(direct).max()
    print(f"dfrac {e_frac:.2e}, dlat {e_lat:.2e} of the maximum from central differences; L^-T virial against sum v (x) gx {e_direct:.2e}")
    assert e_frac <= 1e-5 and e_lat <= 1e-5 and e_direct <= 1e-9
    assert np.abs(got["cart"] @ np.ones(3)).max() > 0
    for s in range(B):
        rows = slice(off[s], off[s + 1])
        assert np.abs(got["cart"][rows].sum(0)).max() <= 1e-12 * max(got["cart_mag"][rows].sum(), 1.0), s      # no net force
        assert np.allclose(got["frac"][rows], got["cart"][rows] @ l0[s].T, rtol=0, atol=1e-12 * np.abs(got["frac"]).max())
        if off[s + 1] - off[s] == 1:                                       # one atom: its images only -- no force, but a cell gradient
            assert np.all(got["cart"][rows] == 0) and np.all(got["frac"][rows] == 0)
            assert batch["edge_offsets"][s + 1] > batch["edge_offsets"][s] and np.abs(got["lat"][s]).max() > 0
    assert np.any(np.diff(off) == 1)
    assert np.abs(got["virial"] - np.swapaxes(got["virial"], 1, 2)).max() > 1e-3       # dvec makes it asymmetric


def test_the_fp32_definition_is_within_rounding_of_the_twin():
    frac, lat, off = _batch(seed=4)
    i, j, sid, add, batch = _frozen_edges(frac, lat, off)
    n, E = frac.shape[0], i.size
    rng = _rng(9)
    rowptr, col, eid = _csr(n, batch["pairs"])
    for fe_cols, with_dvec in ((1, True), (8, False), (0, True)):
        de = rng.uniform(-1, 1, (E, fe_cols)).astype(np.float32) if fe_cols else None
        dv = rng.uniform(-1, 1, (E, 3)).astype(np.float32) if with_dvec else None
        args = (rowptr, col, eid, lat, off, batch["edge_offsets"], batch["vec"], CMAX)
        a = gr.structures_grad(*args, dfeature=de, dvec=dv, dtype=np.float32)
        b = gr.structures_grad(*args, dfeature=de, dvec=dv, dtype=np.float64)
        for k in ("cart", "frac", "virial"):
            assert a[k].dtype == np.float32
            bad = np.abs(a[k].astype(np.float64) - b[k]) > 1e-5 * b[k + "_mag"] + 1e-30
            assert not bad.any(), (fe_cols, with_dvec, k)
        scale = np.abs(np.linalg.inv(lat.astype(np.float64))).transpose(0, 2, 1) @ b["virial_mag"]
        assert np.all(np.abs(a["lat"].astype(np.float64) - b["lat"]) <= 1e-5 * scale)
        assert np.abs(a["cart"]).max() > 0


def test_points_mode_equals_a_dense_evaluation():
    n = 200
    for dim in (1, 2, 3):
        rng = _rng(20 + dim)
        p = rng.random((n, dim)).astype(np.float32)
        radius = (0.02, 0.12, 0.25)[dim - 1]
        i, j = np.triu_indices(n, 1)
        d2 = ((p[i].astype(np.float64) - p[j]) ** 2).sum(1)
        keep = d2 <= radius * radius
        pairs = np.asfortranarray(np.stack([i[keep] + 1, j[keep] + 1]).astype(np.int32))
        E = pairs.shape[1]
        assert E > n
        dc = rng.uniform(-1, 1, (E, dim)).astype(np.float32)
        rowptr, col, eid = _csr(n, pairs)
        got32, mag = gr.points_grad(rowptr, col, eid, dc, np.float32)
        got64, _ = gr.points_grad(rowptr, col, eid, dc, np.float64)
        dense = np.zeros((n, n, dim))                                      # T[i, j] = dE/d(p_i - p_j) on the pair i < j
        dense[i[keep], j[keep]] = dc
        want = dense.sum(1) - dense.sum(0)                                 # p_i enters coords[e] with + as the first, - as the second index
        assert np.abs(got64 - want).max() <= 1e-13 * mag.max()
        assert got32.dtype == np.float32 and np.all(np.abs(got32.astype(np.float64) - want) <= 1e-5 * mag + 1e-30)
        assert np.abs(want).max() > 0


def test_header_binding_and_fortran_module_declare_the_entries():
    from athena_amd import _capi

    declared = _capi.declared_symbols()
    f90 = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    for name in ENTRIES:
        assert name in declared, name
        assert name in _capi._PROTOS, name
        assert re.search(r'bind\(C, name="%s"\)' % name, f90), name
        assert re.search(r"public ::.*\b%s\b" % name, f90), name
    assert len(_capi._PROTOS["athena_mp_edge_grad_to_points"]) == len(_capi._PROTOS["athena_mp_edge_grad_to_points_host"]) == 4
    assert len(_capi._PROTOS["athena_mp_periodic_grad"]) == len(_capi._PROTOS["athena_mp_periodic_grad_host"]) == 15


def test_library_and_package_export_the_entries():
    import athena_amd
    from athena_amd import _capi

    lib = _capi.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name
    for name in ("points_grad", "structures_grad", "structures_grad_host"):
        assert callable(getattr(athena_amd, name)) and callable(getattr(athena_amd.geometry, name))
