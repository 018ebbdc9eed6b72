"""CPU: the yardstick of the voxel-grid clusters against itself (tests/grid_clusters_reference.py).  The sorted transcription of the
definition is pinned to the dictionary form on every shape class the GPU tests run; the properties the definition promises are
checked on it; its reverse step is held to central differences of the float64 twin; the inputs of the GPU tests are shown to be
what those tests need (the wide key needs more than 32 bits, the hub holds thousands, heads sit on both sides of the scan tile and
the work item).  Also: the C ABI, ctypes and Fortran declarations of the new entries agree."""
import os
import re

import numpy as np
import pytest

import grid_clusters_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"athena_mp_grid_clusters": 18, "athena_mp_grid_clusters_grad": 7, "athena_mp_grid_clusters_host": 18,
           "athena_mp_grid_clusters_grad_host": 7, "athena_mp_grid_clusters_stats": 1}
CASES = gr.shape_cases()
NAMES = [c[0] for c in CASES]


@pytest.fixture(autouse=True)
def the_library_declares_what_the_yardstick_defines():
    """the yardstick stands for entries of the library: without them there is nothing it measures"""
    from athena_amd import _capi

    missing = [name for name in ENTRIES if name not in _capi._PROTOS]
    assert not missing, f"athena_amd._capi lacks {missing}"


def _case(name):
    _, p, off, size, origin = CASES[NAMES.index(name)]
    return p, off, size, origin, gr.clusters(p, off, size, origin)


@pytest.mark.parametrize("c", range(len(CASES)), ids=NAMES)
def test_the_two_forms_of_the_yardstick_agree(c):
    name, p, off, size, origin = CASES[c]
    a, b = gr.clusters(p, off, size, origin), gr.brute_force(p, off, size, origin)
    assert gr.same(a, b) == [] and (a["m"], a["bits"], a["passes"], a["largest"]) == (b["m"], b["bits"], b["passes"], b["largest"])


@pytest.mark.parametrize("c", range(len(CASES)), ids=NAMES)
def test_invariants(c):
    name, p, off, size, origin = CASES[c]
    r = gr.clusters(p, off, size, origin)
    n, m, dim = p.shape[0], r["m"], p.shape[1]
    count = np.diff(r["rowptr"])
    # the clusters partition the points, and none is empty
    assert r["rowptr"][0] == 0 and r["rowptr"][-1] == n and (count > 0).all()
    assert sorted(r["pairs"][:, 1].tolist()) == list(range(1, n + 1))
    assert np.array_equal(r["cluster"][r["pairs"][:, 1] - 1], r["pairs"][:, 0])
    assert np.array_equal(np.bincount(r["cluster"] - 1, minlength=m), count)
    # pairs is strictly ascending in (cluster, point)
    k = r["pairs"][:, 0].astype(np.int64) * (n + 1) + r["pairs"][:, 1]
    assert (np.diff(k) > 0).all()
    # ids ascend with the key (cloud, c_{dim-1}, .., c_0), and no key repeats
    cloud = np.searchsorted(r["cluster_offsets"], np.arange(m), side="right") - 1
    keys = [(int(cloud[i]),) + tuple(int(v) for v in r["cell"][i][::-1]) for i in range(m)]
    assert all(a < b for a, b in zip(keys, keys[1:]))
    assert r["cluster_offsets"][0] == 0 and r["cluster_offsets"][-1] == m and (np.diff(r["cluster_offsets"]) >= 0).all()
    assert ((np.diff(r["cluster_offsets"]) > 0) == (np.diff(off) > 0)).all(), "a cloud has clusters iff it has points"
    # nearest is a member; weights * count is exactly 1 where count is a power of two
    assert np.array_equal(r["cluster"][r["nearest"] - 1], np.arange(1, m + 1))
    w = r["weights"][r["rowptr"][:-1]]
    pow2 = (count & (count - 1)) == 0
    assert (w[pow2] * count[pow2].astype(np.float32) == 1).all()
    # every member lies in its cluster's cell: the cell function again, point by point
    inv, lo, nc, _, _ = gr.grids(p, off, size, origin)
    c_pts, cl = gr.cells_of(p, off, inv, lo)
    assert np.array_equal(c_pts, r["cell"][r["cluster"] - 1])
    for b in range(off.size - 1):
        if off[b + 1] > off[b]:
            assert tuple(c_pts[off[b]:off[b + 1]].max(axis=0) + 1) == nc[b], "the largest coordinate that occurs is nc - 1: the clamp never acts"


def test_the_inputs_are_what_the_gpu_tests_need():
    for dim in (1, 2, 3):
        r = _case(f"sizes 1..65 and a hub, dim {dim}")[4]
        assert tuple(np.diff(r["rowptr"])) == gr.HUB_SIZES and r["largest"] == 5000
    for m in (63, 64, 65):
        assert _case(f"m = {m}")[4]["m"] == m
    for n in (4095, 4096, 4097, 8193):
        p, off, size, origin, r = _case(f"n = {n}")
        assert p.shape[0] == n and tuple(np.diff(r["rowptr"])) == tuple(gr.BOUNDARY_N[n])
        heads = set(r["rowptr"][:-1].tolist())
        for edge in (4096, 8192):                      # the scan64 tile and the 4 096-point work item
            if n > edge:
                assert edge - 1 in heads and edge in heads, "a head on both sides of the boundary"
        if n == 4095:
            assert 4092 in heads
        order = r["pairs"][:, 1]
        assert (np.diff(order) < 0).any(), "the members must not arrive in key order"
    p, off, size, origin, r = _case("wide key")
    assert r["bits"] == 35 and r["passes"] == 5 and r["bits"] > 32
    inv, lo, nc, _, _ = gr.grids(p, off, size)
    assert nc[0] == (2049, 2049, 2049) and 2049 ** 3 > 2 ** 33
    p, off, size, origin, r = _case("mixed batch")
    sizes = np.diff(off)
    assert sizes[0] == 0 and sizes[3] == 0 and sizes[-1] == 0 and sizes[2] == 1 and sizes[4] == 37
    per = np.diff(r["cluster_offsets"])
    assert per[2] == 1 and per[4] == 1, "the one-point cloud and the coincident cloud are one cluster each"
    assert np.array_equal(p[off[1]:off[2]], p[off[5]:off[6]]) and per[1] == per[5]
    a, b = slice(r["cluster_offsets"][1], r["cluster_offsets"][2]), slice(r["cluster_offsets"][5], r["cluster_offsets"][6])
    assert np.array_equal(r["cell"][a], r["cell"][b]) and np.array_equal(r["centroid"][a].view(np.int32), r["centroid"][b].view(np.int32))
    assert per[6] == 125, "every lattice point is a cell of its own"
    assert np.signbit(p[off[9]]).any() and not np.signbit(r["origin_out"][9]).any() and (r["origin_out"][9] == 0).all(), "-0 becomes +0"
    assert (r["origin_out"][7] >= 1e6).all() and (p[off[8]:off[9]] < 0).any()
    for name in ("mixed batch, one cluster per cloud", "mixed batch, size 3e38"):
        r = _case(name)[4]
        assert np.array_equal(np.diff(r["cluster_offsets"]), (np.diff(off) > 0).astype(np.int32))
    p, off, size, origin, r = _case("uniform and graded clouds, origin below")
    assert (p.min(axis=0) - origin > 1).all() and (r["origin_out"] == origin).all() and (r["cell"].min(axis=0) >= 16).all()


def test_the_centroid_is_relative_to_lo_for_a_reason():
    """5 000 points around 1e6 in one cell: the plain sequential fp32 sum of the coordinates is off by many ulps, the lo-relative one
    by a small fraction of the cell"""
    rng = gr._rng(3)
    p = (1e6 + rng.random((5000, 3))).astype(np.float32)
    r = gr.clusters(p, gr.offsets_of([5000]), 4.0)
    assert r["m"] == 1
    exact = p.astype(np.float64).mean(axis=0)
    plain = np.zeros(3, np.float32)
    for row in p:
        plain = plain + row
    plain = plain / np.float32(5000)
    ulp = np.spacing(np.float32(1e6))
    assert np.abs(r["centroid"][0] - exact).max() <= ulp and np.abs(plain - exact).max() > 16 * ulp


def test_grad_agrees_with_central_differences_of_the_float64_twin():
    """The centroid is linear in the points for a fixed membership, so central differences of the float64 twin are exact up to
    float64 rounding (relative 1e-10 at h = 1e-3 and values of order 1).  The fp32 reverse step is one correctly rounded division:
    within 2^-24 relative of dcentroid / count.  Bound: 2^-23 relative plus 1e-9 absolute for the differences."""
    p, off, size, origin, r = _case("uniform and graded clouds")
    m, n, dim = r["m"], p.shape[0], p.shape[1]
    rng = gr._rng(5)
    G = rng.standard_normal((m, dim)).astype(np.float32)
    got = gr.grad(r["cluster"], r["rowptr"], G)
    p64, h = p.astype(np.float64), 1e-3
    loss = lambda q: float((gr.centroid64(q, r["cluster"], m) * G.astype(np.float64)).sum())
    for j in rng.choice(n, 40, replace=False):
        for k in range(dim):
            up, down = p64.copy(), p64.copy()
            up[j, k] += h
            down[j, k] -= h
            fd = (loss(up) - loss(down)) / (2 * h)
            assert abs(float(got[j, k]) - fd) <= 2.0 ** -23 * abs(fd) + 1e-9
    count = np.diff(r["rowptr"])
    assert np.array_equal(got, (G / count[:, None].astype(np.float32))[r["cluster"] - 1])


def test_the_yardstick_refuses_what_the_library_refuses():
    p = gr._rng(9).random((50, 3)).astype(np.float32)
    off = gr.offsets_of([50])
    for kw, why in ((dict(size=0.0), "size"), (dict(size=np.inf), "size"), (dict(size=1e-45), "inverse"), (dict(size=2.0 ** -22), "axis"),
                    (dict(size=0.1, origin=[0.5, 0.0, 0.0]), "origin")):
        with pytest.raises(gr.Refused, match=why):
            gr.grids(p, off, **kw)
    q = np.array([[0, 0, 0], [1 - 2.0 ** -24] * 3], np.float32)
    with pytest.raises(gr.Refused, match="bits"):
        gr.grids(q, gr.offsets_of([2]), 2.0 ** -21)                  # 2^21 cells on each axis: 63 + 1 bits
    q = np.array([[-3e38, 0, 0], [3e38, 0, 0]], np.float32)
    with pytest.raises(gr.Refused, match="extent"):
        gr.grids(q, gr.offsets_of([2]), 1.0)


def test_declarations_agree():
    from athena_amd import _capi

    header = open(os.path.join(ROOT, "include", "athena_mp.h")).read()
    fortran = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    build = open(os.path.join(ROOT, "athena_amd", "csrc", "build.sh")).read()
    assert " grid_clusters.hip " in build
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "grid_clusters_run.f90" in entry
    for name, n_args in ENTRIES.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in athena_mp.h"
        assert len(m.group(1).split(",")) == n_args
        assert len(_capi._PROTOS[name]) == n_args
        m = re.search(r"function %s\(([^)]*)\)" % name, fortran)
        assert m and 'name="%s"' % name in fortran, f"{name} has no interface in athena_mp_c.f90"
        assert len(m.group(1).replace("&", "").split(",")) == n_args
