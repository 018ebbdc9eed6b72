"""CPU: the exact yardstick of tests/exact_reference.py is tied to the fp32 oracle, is independent of the order of summation, and
its conditions (every partial sum exact in fp32; expected tensors mostly non-zero) hold for every case that
tests/test_gpu_many_chunks.py runs -- evaluated here at the MI355X's 256 compute units, so a bad case is found without a GPU."""
import numpy as np
import pytest

import exact_reference as er

N_SMALL = 3000


@pytest.fixture(scope="module")
def small():
    """a 3 000-row instance of the family, 128 -> 128, with the 256-entry rows"""
    ia, ja = er.exact_graph(N_SMALL, seed=3)
    er.assert_one_launch_route(ia, ja)
    return er.KipfReference(ia, ja, *er.kipf_operands(N_SMALL, 128, 128, seed=5))


def test_coefficients_are_powers_of_two_and_the_check_of_the_words_notices(small):
    c = er.coefficients(small.ia, small.ja).astype(np.float32)
    er.assert_power_of_two_words(c, 8)
    assert c.min() == 2.0 ** -8
    bad = c.copy()
    bad[7] = np.float32(3.0) ** np.float32(-0.5)
    with pytest.raises(AssertionError, match="power of two"):
        er.assert_power_of_two_words(bad, 8)
    with pytest.raises(AssertionError):
        er.assert_power_of_two_words(c, 6)


def test_fp32_oracle_equals_the_exact_reference(oracle, small):
    """every op of the step in the oracle's fp32 and its own order: the same bits as the float64 reference"""
    r = small
    F = r.Fo
    P = oracle.kipf_propagate(r.x, r.ia, r.ja)
    assert np.array_equal(P, r.P)
    Z = oracle.matmul(r.W, P, F)
    assert np.array_equal(Z, r.Z("none", bias=False))
    Zb = oracle.add_bias_rows(Z, r.bias)
    assert np.array_equal(Zb, r.Z("none"))
    assert np.array_equal(oracle.activation("relu", Zb), r.Z("relu"))
    assert np.array_equal(oracle.activation("relu", Z), r.Z("relu", bias=False))
    dP = oracle.matmul_dx(r.W, r.dZ, r.Fi)
    for exact in (False, True):
        assert np.array_equal(oracle.kipf_propagate_bwd(dP, r.ia, r.ja, exact=exact), r.dX(exact))
    assert np.array_equal(oracle.matmul_dw(r.dZ, P), r.dW)
    assert r.dW.shape == (r.Fi * r.Fo,)


def test_fp32_oracle_equals_the_exact_dense_reference(oracle):
    M, K, N = 3001, 64, 32
    r = er.gemm_case(M, K, N)
    Z = oracle.matmul(r.W, r.Pm, N)
    assert np.array_equal(Z, r.Z("none", bias=False))
    assert np.array_equal(oracle.add_bias_rows(Z, r.bias), r.Z("none"))
    assert np.array_equal(oracle.activation("relu", oracle.add_bias_rows(Z, r.bias)), r.Z("relu"))
    assert np.array_equal(oracle.matmul_dx(r.W, r.dZ, K), r.dP)
    assert np.array_equal(oracle.matmul_dw(r.dZ, r.Pm), r.dW)


def test_every_order_and_association_gives_the_same_bits(oracle, small):
    """fp32 sums with each row's entries shuffled, the features of the contraction and the rows of the dW sum in a random order,
    and the other association of dX and dW (aggregate first, as the one-launch kernels do)"""
    r = small
    rng = np.random.default_rng(11)
    n, F = r.n, r.Fo
    row_of = np.repeat(np.arange(n), np.diff(r.ia))
    order = np.lexsort((rng.random(row_of.size), row_of))            # a random order inside every row
    ja = np.asfortranarray(r.ja[:, order])
    assert not np.array_equal(ja, r.ja) and np.array_equal(np.sort(ja[0]), np.sort(r.ja[0]))
    P = oracle.kipf_propagate(r.x, r.ia, ja)
    assert np.array_equal(P, r.P)
    for exact in (False, True):
        # (A^T dZ) W: the sum over the entries first (in the shuffled order), then the contraction
        Q = oracle.kipf_propagate_bwd(r.dZ, r.ia, ja, exact=exact)
        assert np.array_equal(oracle.matmul_dx(r.W, Q, r.Fi), r.dX(exact))
    k = rng.permutation(r.Fi)                                          # the contraction index in a random order
    Wk = np.ascontiguousarray(r.W.reshape(r.Fi, F)[k]).reshape(-1)
    assert np.array_equal(oracle.matmul(Wk, np.ascontiguousarray(r.P[:, k]), F), r.Z("none", bias=False))
    v = rng.permutation(n)                                             # the rows of the dW sum in a random order
    assert np.array_equal(oracle.matmul_dw(np.ascontiguousarray(r.dZ[v]), np.ascontiguousarray(r.P[v])), r.dW)
    # dW = sum over u of (A^^T dZ)[u] (x) x[u]: what the folded kernel adds up
    Qc = oracle.kipf_propagate_bwd(r.dZ, r.ia, ja, exact=True)
    assert np.array_equal(oracle.matmul_dw(np.ascontiguousarray(Qc[v]), np.ascontiguousarray(r.x[v])), r.dW)


def test_operands_scaled_by_1024_are_rejected(small):
    """the guard is live: the same case with x times 2^10 needs more than 24 bits for Z and dW"""
    r = small
    big = er.KipfReference(r.ia, r.ja, r.x * np.float32(1024), r.W, r.bias, r.dZ)
    assert big.P.shape == r.P.shape and big.bits["P"] == pytest.approx(r.bits["P"] + 10)      # 21.9 bits: still exact
    with pytest.raises(AssertionError, match="fp32 holds 24"):
        big.Z("none")
    with pytest.raises(AssertionError, match="fp32 holds 24"):
        big.dW
    P, W, b, dZ = er.gemm_operands(70000, 64, 64)
    with pytest.raises(AssertionError, match="fp32 holds 24"):
        er.GemmReference(P, W, b, dZ * np.float32(1024))
    with pytest.raises(AssertionError, match="must hold integers"):
        er.GemmReference(P * np.float32(0.5), W, b, dZ)


def test_a_zero_block_or_a_sparse_tensor_is_rejected():
    a = np.ones((300, 8), np.float32)
    er.assert_not_mostly_zero("ones", a)
    a[64:128] = 0
    with pytest.raises(AssertionError, match="all zero"):
        er.assert_not_mostly_zero("a dead block", np.concatenate([a, np.ones((2000, 8), np.float32)]))
    with pytest.raises(AssertionError, match="non-zero"):
        er.assert_not_mostly_zero("sparse", a)


# ---- the GPU file's cases at 256 compute units ----------------------------------------------------------------------------------------
C = er.MI355X_CUS


def _report(what, r):
    print(what, "bits", {k: round(v, 1) for k, v in r.bits.items()}, "non-zero", {k: round(v, 2) for k, v in r.nonzero.items()})
    assert all(b < 24 for b in r.bits.values())
    assert all(f > 0.8 for f in r.nonzero.values())


@pytest.mark.parametrize("F", er.FUSED_WIDTHS)
def test_conditions_of_the_fused_cases(F):
    n = er.fused_rows(C)
    assert n == 66003
    chunks = er.ceil_div(n, er.FUSED_CHUNK_ROWS[F])
    assert chunks == {64: 1032, 128: 2063, 256: 4126}[F] and chunks > 3 * C and n % er.FUSED_CHUNK_ROWS[F]
    r = er.fused_case(C, F)
    assert r.g == 8
    r.P, r.Z("none"), r.Z("relu"), r.dX(False), r.dX(True)
    _report(f"fused {F}", r)


@pytest.mark.parametrize("n,live_tail", er.dw_cases(C))
def test_conditions_of_the_folded_dw_cases(n, live_tail):
    grid, chunks, most, how_many = er.dw_trips(n, C)
    assert (n, most, how_many) in ((8192, 1, 256), (8193, 2, 1), (16499, 3, 4), (66003, 9, 15))
    r = er.dw_case(n, live_tail)
    assert r.g == 6
    last = int(np.diff(r.ia)[-1])
    assert last == (16 if live_tail else 0)
    r.dX(False), r.dX(True), r.dW
    _report(f"dW {n}", r)


@pytest.mark.parametrize("M,K,N", er.gemm_cases(C) + [(er.blocked_dw_rows(C), 256, 256)])
def test_conditions_of_the_dense_cases(M, K, N):
    assert M in (65765, 131301)
    r = er.gemm_case(M, K, N)
    if K <= 128:
        grid, slabs, most, how_many = er.gemm_trips(M, K, N, C)
        assert grid == C and how_many == 8 and most == (3 if M == 131301 or er.gemm_waves(K, N) == 4 else 2)
        r.Z("relu"), r.Z("none"), r.Z("none", bias=False), r.dP
    else:
        nx, rpw = er.blocked_dw_ranges(M, C)
        assert nx == 256 and rpw == 130
    r.dW
    _report(f"dense {M} x {K} x {N}", r)
