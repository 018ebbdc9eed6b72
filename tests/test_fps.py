"""CPU: the yardstick of farthest-point sampling against itself (tests/fps_reference.py).  A Python transcription of fps.hip's
stream route -- chunks of 64 points in cell order, each with its bounding box and cached best key, skipped when the clamped
distance of the new sample to the box is no smaller than the chunk's largest live dmin -- is pinned to the brute-force
transcription of the definition on every shape class the GPU tests use.  One case shows that a bound taken from the box's CENTRE
gives a wrong sample: the comparison can see a bad bound.  The properties the definition promises are checked on the brute force
itself.  Also: the C ABI, ctypes and Fortran declarations of the new entries agree."""
import functools
import os
import re

import numpy as np
import pytest

import fps_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"athena_mp_farthest_points": 12, "athena_mp_farthest_points_host": 12, "athena_mp_fps_stats": 1}
CASES = fr.shape_cases()


@functools.lru_cache(None)
def _brute(c):
    name, p, off, soff, start = CASES[c]
    return fr.brute_force(p, soff, off, start)


def _same(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
            and np.array_equal(got[2].view(np.int32), want[2].view(np.int32)) and np.array_equal(got[3].view(np.int32), want[3].view(np.int32)))


@pytest.mark.parametrize("c", range(len(CASES)), ids=[c[0] for c in CASES])
def test_the_pruned_search_equals_brute_force(c):
    name, p, off, soff, start = CASES[c]
    want = _brute(c)
    got = fr.pruned(p, soff, off, start)
    print(f"{name}: {got[4][0]} chunk tests, {got[4][1]} skipped")
    assert _same(got, want)
    assert not np.isnan(want[2]).any() and not np.isnan(want[3]).any()
    if "3e38" in name:
        assert np.isinf(want[2][1:]).any(), "the case must hold a squared distance that overflows"
    if "clustered" in name:
        assert got[4][1] > 0, "a clustered cloud must skip chunks"


@pytest.mark.parametrize("order", ["identity", "reversed", "shuffled"])
def test_any_point_order_is_correct(order):
    p = fr.clustered(700, 3, 21)
    pick = {"identity": lambda q: np.arange(q.shape[0]), "reversed": lambda q: np.arange(q.shape[0])[::-1].copy(),
            "shuffled": lambda q: fr._rng(5).permutation(q.shape[0])}[order]
    soff = fr.offsets_of([80])
    assert _same(fr.pruned(p, soff, order=pick), fr.brute_force(p, soff))


def test_a_bound_from_the_box_centre_gives_a_wrong_sample():
    """the probe: the distance to a box's centre is no lower bound of the distance to its points, and the comparison sees it"""
    p = fr._rng(41).random((640, 2)).astype(np.float32)
    soff = fr.offsets_of([64])
    want = fr.brute_force(p, soff)
    assert _same(fr.pruned(p, soff, order=lambda q: np.arange(q.shape[0])), want)
    wrong = fr.pruned(p, soff, order=lambda q: np.arange(q.shape[0]), bound="centre")
    assert wrong[4][1] > 0 and not np.array_equal(wrong[0], want[0])


def test_prefix_monotone_and_cover():
    p = fr._rng(51).random((500, 3)).astype(np.float32)
    s, sp, sq, cover = fr.brute_force(p, fr.offsets_of([100]))
    for m in (1, 2, 37, 99):
        s2, _, sq2, cover2 = fr.brute_force(p, fr.offsets_of([m]))
        assert np.array_equal(s2, s[:m]) and np.array_equal(sq2, sq[:m])
        assert cover2[0] == sq[m], "the cover of a prefix is the dmin of the next choice"
    assert np.isinf(sq[0]) and (np.diff(sq[1:]) <= 0).all() and cover[0] <= sq[-1]
    assert np.unique(s).size == s.size and np.array_equal(sp, p[s - 1])


def test_lattice_is_decided_by_ties():
    s, _, sq, cover = fr.brute_force(fr.lattice(), fr.offsets_of([125]))
    assert sorted(s.tolist()) == list(range(1, 126)) and cover[0] == 0
    assert sq[:6].tolist() == [np.inf, 48.0, 20.0, 20.0, 20.0, 8.0]


def test_repeated_points_come_last_in_index_order():
    s, _, sq, cover = fr.brute_force(fr.repeated(), fr.offsets_of([20]))
    assert sorted(s[:5].tolist()) == [1, 2, 3, 4, 5] and s[5:].tolist() == list(range(6, 21))
    assert (sq[1:5] > 0).all() and (sq[5:] == 0).all() and cover[0] == 0


def test_batch_equals_the_single_calls():
    p, off, soff = fr.mixed_batch()
    s, sp, sq, cover = fr.brute_force(p, soff, off)
    assert cover[1] == 0 and np.isinf(cover[3]) and cover[4] == 0
    for b in range(off.size - 1):
        m = int(soff[b + 1] - soff[b])
        if m == 0:
            continue
        one = fr.brute_force(p[off[b]:off[b + 1]], fr.offsets_of([m]))
        assert np.array_equal(one[0] + off[b], s[soff[b]:soff[b + 1]]) and one[3][0] == cover[b]


def test_declarations_agree():
    from athena_amd import _capi

    header = open(os.path.join(ROOT, "include", "athena_mp.h")).read()
    fortran = open(os.path.join(ROOT, "athena_amd", "fortran", "athena_mp_c.f90")).read()
    build = open(os.path.join(ROOT, "athena_amd", "csrc", "build.sh")).read()
    assert " fps.hip " in build
    for name, n_args in ENTRIES.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in athena_mp.h"
        assert len(m.group(1).split(",")) == n_args
        assert len(_capi._PROTOS[name]) == n_args
        m = re.search(r"function %s\(([^)]*)\)" % name, fortran)
        assert m and 'name="%s"' % name in fortran, f"{name} has no interface in athena_mp_c.f90"
        assert len(m.group(1).replace("&", "").split(",")) == n_args
