"""CPU: tests/bipartite_reference.py, the yardstick of the two-set radius builder, pinned to the one-set yardstick and to cases
worked out by hand."""
import numpy as np
import pytest

import bipartite_reference as br
import radius_reference as rr


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_one_set_against_itself_is_the_one_set_graph_plus_diagonal_and_mirror(dim):
    p = np.random.default_rng(dim).random((300, dim)).astype(np.float32)
    r = rr.degree_radius(300, 6, dim)
    i, j, c, rowptr, eoff = br.reference_pairs(p, p, r)
    wi, wj, wc = rr.reference_pairs(p, r)
    assert wi.size >= 300
    up = i < j
    assert np.array_equal(i[up], wi) and np.array_equal(j[up], wj) and np.array_equal(c[up], wc)
    diag = i == j
    assert np.array_equal(i[diag], np.arange(300)) and not c[diag].any()
    lo = i > j
    o = np.lexsort((i[lo], j[lo]))                              # the mirror pairs in the order of their (j, i)
    assert np.array_equal(j[lo][o], wi) and np.array_equal(i[lo][o], wj) and np.array_equal(c[lo][o], -wc)
    assert rowptr[0] == 0 and rowptr[-1] == i.size and np.array_equal(np.diff(rowptr), np.bincount(i, minlength=300))
    assert np.array_equal(eoff, [0, i.size])


def test_a_line_by_hand():
    q = np.array([[0.0], [2.5], [10.0]], np.float32)
    s = np.array([[1.0], [2.0], [3.5], [-1.0]], np.float32)
    i, j, c, rowptr, eoff = br.reference_pairs(q, s, 1.0)
    # |0 - 1| = 1 and |0 - -1| = 1 (s == r^2 exactly: kept), |2.5 - 2| = .5, |2.5 - 3.5| = 1; 10 reaches nothing
    assert np.array_equal(i, [0, 0, 1, 1]) and np.array_equal(j, [0, 3, 1, 2])
    assert np.array_equal(c, np.array([[-1.0], [1.0], [0.5], [-1.0]], np.float32))
    assert np.array_equal(rowptr, [0, 2, 4, 4]) and np.array_equal(eoff, [0, 4])


def test_a_3_4_5_lattice_by_hand_and_in_two_clouds():
    s = np.array([[3, 4, 0], [0, 0, 5], [3, 4, 1], [0, 3, 4], [5, 0, 0]], np.float32)
    q = np.array([[0, 0, 0], [3, 4, 0]], np.float32)
    i, j, c, rowptr, _ = br.reference_pairs(q, s, 5.0)
    # from the origin 9 + 16 = 25 == r^2 for sources 0, 1, 3, 4 and 26 for source 2; from (3,4,0): itself, (3,4,1) and (0,3,4)
    # at 9 + 1 + 16 = 26 > 25, (5,0,0) at 4 + 16 = 20
    assert np.array_equal(i, [0, 0, 0, 0, 1, 1, 1]) and np.array_equal(j, [0, 1, 3, 4, 0, 2, 4])
    assert np.array_equal(c[0], [-3, -4, 0]) and np.array_equal(c[4], [0, 0, 0]) and np.array_equal(c[6], [-2, 4, 0])
    assert np.array_equal(rowptr, [0, 4, 7])
    # cut in two clouds: query 0 sees sources 0..2, query 1 sources 3..4; an empty cloud in between changes nothing
    i, j, c, rowptr, eoff = br.reference_pairs(q, s, 5.0, br.offsets_of([1, 0, 1]), br.offsets_of([3, 0, 2]))
    assert np.array_equal(i, [0, 0, 1]) and np.array_equal(j, [0, 1, 4]) and np.array_equal(eoff, [0, 2, 2, 3])
    ia, ja = br.csr_of(i, j, 2)
    assert np.array_equal(ia, [1, 3, 4]) and np.array_equal(ja, [[1, 2, 5], [1, 2, 3]])


def test_the_gradient_by_hand():
    i, j = np.array([0, 0, 2, 2, 2]), np.array([0, 1, 0, 1, 1])      # a doubled pair is not a graph, but it is a sum
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    d = np.array([[big, 1], [one, 2], [one, 4], [-big, 8], [one, 16]], np.float32)
    dq, ds = br.reference_grad(i, j, d, 3, 3)
    # query 0: (2^24 + 1) rounds to 2^24; query 2: (1 - 2^24) + 1 = -2^24 + 2 in this order (-2^24 + 1 is representable);
    # source 0: (-2^24) - 1 rounds to -2^24; source 1: ((-1) + 2^24) - 1 = 2^24 - 2; source 2 and query 1 have no edge: +0
    assert np.array_equal(dq, np.array([[big, 3], [0, 0], [-big + 2, 28]], np.float32))
    assert np.array_equal(ds, np.array([[-big, -5], [big - 2, -26], [0, 0]], np.float32))
    assert not np.signbit(dq[1]).any() and not np.signbit(ds[2]).any()
