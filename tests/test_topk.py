"""CPU: the yardstick of the top-k vertex selection against itself (tests/topk_reference.py).  The sorted form is pinned to the
counting form on every named case the GPU tests run; the properties the definition promises are checked on it; the inputs are
shown to be what the GPU tests need (three radix tiles, 9 graph bits, both routes side by side, every special value).  Also: the
C ABI, ctypes and Fortran declarations of the new entries, and the argument checks of the Python wrappers that need no device."""
import os
import re

import numpy as np
import pytest

import topk_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"athena_mp_topk_vertices": 13, "athena_mp_topk_vertices_host": 13, "athena_mp_topk_stats": 1, "athena_mp_select_rows_fwd": 7,
           "athena_mp_select_rows_bwd": 9, "athena_mp_select_rows_host": 7, "athena_mp_select_rows_bwd_host": 9}


@pytest.fixture(autouse=True)
def the_library_declares_what_the_yardstick_defines():
    """the yardstick stands for entries of the library: without them there is nothing it measures"""
    from athena_amd import _capi

    missing = [name for name in ENTRIES if name not in _capi._PROTOS]
    assert not missing, f"athena_amd._capi lacks {missing}"


@pytest.mark.parametrize("name", tr.NAMES)
def test_the_two_forms_of_the_yardstick_agree(name):
    c = tr.case(name)
    a = tr.expected(name)
    b = tr.select_counting(c["score"], c["offsets"], tr.counts_of(c), c["min_score"])
    assert tr.same(a, b) == []


@pytest.mark.parametrize("name", tr.NAMES)
def test_invariants(name):
    c, r = tr.case(name), tr.expected(name)
    s, off = c["score"], c["offsets"]
    n, B, m = s.size, off.size - 1, r["m"]
    sizes = np.diff(off.astype(np.int64))
    kk = np.minimum(np.broadcast_to(np.asarray(tr.counts_of(c), np.int64), (B,)), sizes)
    assert r["cluster"].shape == (n,) and r["selected"].shape == (m,) and r["order"].shape == (m,) and r["sel_offsets"].shape == (B + 1,)
    assert r["sel_offsets"][0] == 0 and r["sel_offsets"][-1] == m and (np.diff(r["sel_offsets"]) <= kk).all()
    if c["min_score"] is None:
        assert np.array_equal(np.diff(r["sel_offsets"]), kk)
    # the new ids number the kept vertices in ascending vertex index; selected inverts cluster
    assert (np.diff(r["selected"]) > 0).all() and np.array_equal(r["cluster"][r["selected"] - 1], np.arange(1, m + 1))
    assert (r["cluster"] > 0).sum() == m
    for g in range(B):
        run = r["order"][r["sel_offsets"][g]:r["sel_offsets"][g + 1]] - 1
        assert ((run >= off[g]) & (run < off[g + 1])).all()
        assert np.array_equal(np.sort(run), r["selected"][r["sel_offsets"][g]:r["sel_offsets"][g + 1]] - 1)   # graphs stay contiguous
        nan = np.isnan(s[run])
        v = np.where(nan, -np.inf, s[run]).astype(np.float64)         # NaNs last; among themselves by index, like every tie
        assert (v[1:] <= v[:-1]).all() and (np.diff(nan.astype(int)) >= 0).all()
        tie = (v[1:] == v[:-1]) & (nan[1:] == nan[:-1])
        assert (np.diff(run)[tie] > 0).all()
        if c["min_score"] is not None:
            assert (s[run] >= np.float32(c["min_score"])).all()
        # nobody left out beats the last one kept
        if run.size and run.size < kk[g] and c["min_score"] is not None:
            left = np.setdiff1d(np.arange(off[g], off[g + 1]), run)
            with np.errstate(invalid="ignore"):
                assert not (s[left] >= np.float32(c["min_score"])).any()


def test_every_prefix_of_a_run_is_the_top_k_prime():
    c = tr.case("k per graph")
    full = tr.expected("k per graph")
    less = tr.select(c["score"], c["offsets"], np.minimum(c["k"], 2))
    for g in range(c["offsets"].size - 1):
        a = full["order"][full["sel_offsets"][g]:full["sel_offsets"][g + 1]]
        b = less["order"][less["sel_offsets"][g]:less["sel_offsets"][g + 1]]
        assert np.array_equal(a[:b.size], b)


def test_the_inputs_are_what_the_gpu_tests_need():
    for name in ("three tiles, three values", "three tiles, all equal"):
        c = tr.case(name)
        assert c["score"].size == 2 * tr.TILE + 9 and np.unique(c["score"]).size == (3 if "three values" in name else 1)
        assert tr.stats(c["offsets"]) == (0, 1, 33, 5)
        assert 0 < tr.expected(name)["m"] < c["score"].size
    all_equal = tr.expected("three tiles, all equal")
    assert np.array_equal(all_equal["order"], np.arange(1, all_equal["m"] + 1))       # stability alone decides
    c = tr.case("300 small graphs")
    assert c["offsets"].size == 301 and tr.stats(c["offsets"]) == (300, 0, 0, 0) and tr.stats(c["offsets"], "sort") == (0, 300, 41, 6)
    assert tr.bits_for(299) == 9 and (np.diff(c["offsets"]) == 0).any()
    for name in ("sizes 0 1 2 63 64 65 128 129", "the same sizes reversed"):
        sizes = np.diff(tr.case(name)["offsets"])
        assert sorted(sizes.tolist()) == sorted(tr.SIZES) and tr.stats(tr.case(name)["offsets"])[:2] == (5, 3)
    assert np.diff(tr.case("the same sizes reversed")["offsets"]).tolist() == list(tr.SIZES[::-1])
    sp = tr.special_values().view(np.uint32)
    for name, route in (("special values, wave", (1, 0)), ("special values, sort", (0, 1))):
        c = tr.case(name)
        w = c["score"].view(np.uint32)
        assert set(sp.tolist()) <= set(w.tolist()) and tr.stats(c["offsets"])[:2] == route
        r = tr.expected(name)
        assert r["m"] == c["score"].size                              # k = n_g and no min_score: the NaNs are kept, last
        nans = int(np.isnan(c["score"]).sum())
        assert nans >= 7 and np.isnan(c["score"][r["order"][-nans:] - 1]).all() and not np.isnan(c["score"][r["order"][:-nans] - 1]).any()
        assert (np.diff(r["order"][-nans:]) > 0).all()               # every NaN equals every other: by index
        zeros = np.nonzero(c["score"] == 0)[0]
        at = np.nonzero(np.isin(r["order"] - 1, zeros))[0]
        assert zeros.size >= 4 and (np.diff(at) == 1).all() and (np.diff(r["order"][at]) > 0).all()   # -0 and +0: one tie
    assert tr.expected("special values, sort, min_score NaN")["m"] == 0
    c = tr.case("special values, sort, min_score -inf")
    assert tr.expected("special values, sort, min_score -inf")["m"] == int((~np.isnan(c["score"])).sum())
    c = tr.case("special values, wave, min_score -0")
    with np.errstate(invalid="ignore"):
        assert tr.expected("special values, wave, min_score -0")["m"] == int((c["score"] >= 0).sum())
    r = tr.expected("min_score above a graph's scores")
    assert r["sel_offsets"][2] == r["sel_offsets"][3] and r["m"] > 0
    c = tr.case("min_score equal to a score")
    assert (c["score"][tr.expected("min_score equal to a score")["selected"] - 1] == np.float32(c["min_score"])).any()
    c = tr.case("ratio 0.5 on odd sizes")
    sizes = np.diff(c["offsets"])
    assert (sizes % 2 == 1).sum() >= 4 and tr.counts_of(c).tolist() == [(s + 1) // 2 for s in sizes.tolist()]
    assert tr.counts_of(tr.case("ratio 1")).tolist() == sizes.tolist()
    assert tr.ratio_counts([10, 3, 0, 7], 0.3).tolist() == [3, 1, 0, 3]               # ceil(0.3 * 10) = 3 in float64, not 4
    assert tr.stats(tr.case("every graph at most 64")["offsets"])[1] == 0
    c = tr.case("three tiles and small graphs")
    assert tr.stats(c["offsets"])[0] > 0 and tr.stats(c["offsets"])[1] > 1 and np.diff(c["offsets"]).max() == 2 * tr.TILE + 9
    assert tr.expected("n = 0, B = 3")["sel_offsets"].tolist() == [0, 0, 0, 0] and tr.expected("B = 0")["sel_offsets"].tolist() == [0]


def test_the_yardstick_refuses_what_the_library_refuses():
    c = tr.case("k per graph")
    s, off = c["score"], c["offsets"]
    down = off.copy(); down[3] = off[2] - 1
    short = off.copy(); short[-1] -= 1
    first = off.copy(); first[0] = 1
    kneg = c["k"].copy(); kneg[4] = -2
    for args, why in (((s, down, 3), r"offsets\(4\)"), ((s, short, 3), "end at"), ((s, first, 3), r"offsets\(1\)"), ((s, off, -1), "k ="),
                      ((s, off, kneg), r"k\(5\)"), ((s, np.zeros(1, np.int32), 3), "end at")):
        for form in (tr.select, tr.select_counting):
            with pytest.raises(tr.Refused, match=why):
                form(*args)


def test_the_gated_rows_of_the_yardstick():
    cluster, selected, x, gate, dy = tr.rows_case(50, 40, 13, 5)
    y = tr.rows_fwd(selected, x, gate)
    assert y.shape == (27, 5) and np.array_equal(y[3], x[selected[3] - 1] * gate[selected[3] - 1])
    dx = tr.rows_bwd_x(cluster, dy, gate)
    assert (dx[cluster == 0] == 0).all() and not np.signbit(dx[cluster == 0]).any()
    assert np.array_equal(dx[selected - 1], dy * gate[selected - 1][:, None])
    dgate, scale = tr.rows_bwd_gate(cluster, dy, x)
    assert (dgate[cluster == 0] == 0).all() and np.allclose(dgate[selected - 1], (dy.astype(np.float64) * x[selected - 1]).sum(axis=1), atol=1e-5)
    assert (scale >= np.abs(dgate)).all()
    # un-pooling after pooling: the kept rows, bit for bit, and +0 elsewhere
    cluster, selected, x, _, _ = tr.rows_case(51, 40, 13, 5, gated=False, special=True)
    back = tr.rows_bwd_x(cluster, tr.rows_fwd(selected, x))
    assert np.array_equal(back.view(np.int32)[selected - 1], x.view(np.int32)[selected - 1]) and (back.view(np.int32)[cluster == 0] == 0).all()


def test_header_binding_and_fortran_module_declare_the_entries():
    from athena_amd import _capi

    header = open(os.path.join(ROOT, "include", "athena_mp.h")).read()
    fortran = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    build = open(os.path.join(ROOT, "athena_amd", "csrc", "build.sh")).read()
    assert " topk_select.hip " in build
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "topk_run.f90" in entry
    assert "athena_amd/fortran/topk_run\n" in open(os.path.join(ROOT, ".gitignore")).read()
    for name, n_args in ENTRIES.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in athena_mp.h"
        assert len(m.group(1).split(",")) == n_args
        assert len(_capi._PROTOS[name]) == n_args
        m = re.search(r"function %s\(([^)]*)\)" % name, fortran)
        assert m and 'name="%s"' % name in fortran, f"{name} has no interface in athena_mp_c.f90"
        assert len(m.group(1).replace("&", "").split(",")) == n_args
    assert "ATHENA_MP_TOPK_ROUTE" in open(os.path.join(ROOT, "README.md")).read()


def test_argument_checks_of_the_python_wrappers_that_need_no_device():
    import torch
    from athena_amd import geometry as geo

    s = np.linspace(0, 1, 10).astype(np.float32)
    off = np.array([0, 4, 10], np.int32)
    tk = geo.topk_vertices
    with pytest.raises(ValueError, match="exactly one of k and ratio"):
        tk(s, off)
    with pytest.raises(ValueError, match="exactly one of k and ratio"):
        tk(s, off, k=2, ratio=0.5)
    for ratio in (0, 0.0, -0.5, 1.5, float("nan"), "half", True):
        with pytest.raises(ValueError, match=r"ratio must be a number in \(0, 1\]"):
            tk(s, off, ratio=ratio)
    for k in (-1, np.array([1, -1]), np.array([1, 2, 3]), 1.5, np.array([[1, 2]])):
        with pytest.raises(ValueError, match="k must be a non-negative int, or one per graph"):
            tk(s, off, k=k)
    with pytest.raises(ValueError, match=r"score must be float32 \[n\]"):
        tk(s.astype(np.float64), off, k=1)
    with pytest.raises(ValueError, match=r"score must be float32 \[n\]"):
        tk(s.reshape(2, 5), off, k=1)
    with pytest.raises(ValueError, match=r"score must be float32 \[n\]"):
        tk(torch.zeros(10, dtype=torch.float64), off, k=1)
    with pytest.raises(ValueError, match="offsets must ascend from 0 to n = 10"):
        tk(s, np.array([0, 4, 9], np.int32), k=1)
    with pytest.raises(ValueError, match="offsets must ascend from 0 to n = 10"):
        tk(s, np.array([0, 11, 10], np.int32), k=1)
    with pytest.raises(ValueError, match=r"offsets must be \[B \+ 1\]"):
        tk(s, np.zeros((2, 2), np.int32), k=1)
    with pytest.raises(ValueError, match="min_score must be a number or None"):
        tk(s, off, k=1, min_score="high")
    host_i, host_f = torch.zeros(3, dtype=torch.int32), torch.zeros((4, 2), dtype=torch.float32)
    with pytest.raises(ValueError, match="selected must be a contiguous int32 device tensor"):
        geo.select_rows(host_i, host_f)
    with pytest.raises(ValueError, match="selected must be a contiguous int32 device tensor"):
        geo.select_rows(np.zeros(3, np.int32), host_f)
    with pytest.raises(ValueError, match='want must name some of'):
        geo.select_rows_grad(host_i, host_f, want=("scores",))
    with pytest.raises(ValueError, match='want must name some of'):
        geo.select_rows_grad(host_i, host_f, want=())
    with pytest.raises(ValueError, match="cluster must be a contiguous int32 device tensor"):
        geo.select_rows_grad(host_i, host_f)
    with pytest.raises(ValueError, match="cluster must be a contiguous int32 device tensor"):
        geo.unpool(host_i.to(torch.int64), host_f)
