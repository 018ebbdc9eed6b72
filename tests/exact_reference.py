"""An order-independent yardstick for the Kipf step and the dense kernels: operands for which EVERY partial sum, in every order
and every association, is exact in fp32 -- so a kernel that re-associates its sums (the one-launch kernels, the slab sums of dW)
is held to np.array_equal over the whole tensor, with no tolerance and no float64 anchor.

The graph: row lengths from {0, 1, 4, 16, 64, 256} (powers of four), the column counts a permutation of the row lengths over the
non-empty vertices (a vertex with an empty row is never a column: no powf(0, -0.5)).  Every Kipf coefficient
(deg_v deg_u)^-1/2 is then a power of two, at least 2^-8 (2^-6 without the 256-entry rows).  x, dZ and the bias hold small
integers, W holds -1 / 0 / 1.  Every term of every sum is a multiple of 2^-g (g = 8 or 6; 0 where no coefficient enters), so
is every partial sum, and a partial sum is no larger than the sum of the magnitudes of all terms: where
    max over the elements of (sum of |terms|) * 2^g < 2^24
every partial sum is an integer below 2^24 times 2^-g, which fp32 holds exactly.  That is a CONDITION on the operands, evaluated
from the reference alone (the same formulas on the absolute values), never a measurement of a kernel; KipfReference
asserts it for every tensor it hands out, with the conditions that keep a kernel that writes zeros from passing.

The reference itself is float64 numpy / scipy.sparse from the layer's formulas (P = A^ x, Z = act(P Wt + b),
dX = (A^T dZ) W, dW = P^T dZ), cast to fp32 at the end: exact for the same reason, with 29 bits to spare.

tests/test_exact_reference.py ties it to the fp32 oracle; tests/test_gpu_many_chunks.py holds the persistent kernels to it at
sizes derived from the number of compute units."""
import math

import numpy as np

from helpers import graph_from_lengths

LENGTHS = (0, 1, 4, 16, 64, 256)
PROBS = (.02, .30, .40, .22, .05, .01)          # of the lengths above
PROBS_NO_256 = (.02, .30, .40, .22, .06)        # the dW cases: 2^-6 is the smallest coefficient
K_LONG_ROW = 512                                # common.h kLongRow: longer rows / columns leave the one-launch route
BAND_MAX, BAND_ENTRIES = 32, 8                  # agg.hip banded_ok: the LDS-gather route needs both
MI355X_CUS = 256                                # what the CPU tests evaluate the GPU file's cases at
N_FUSED = 66003                                 # 1 032 / 2 063 / 4 126 chunks of 64 / 32 / 16 rows: above 3 * 256, ragged at every size
MANTISSA = 0x007FFFFF


# ---- the graph ----------------------------------------------------------------------------------------------------------------------
def exact_graph(n, seed=0, long_rows=True, live_tail=False):
    """(adj_ia, adj_ja) of the family above on n vertices; long_rows=False leaves the 256-entry rows out.  The last five rows are
    empty; live_tail=True instead makes the last row a 16-entry one (a case whose last chunk is that one row)"""
    rng = np.random.default_rng(seed)
    probs = PROBS if long_rows else PROBS_NO_256
    row_len = rng.choice(np.array(LENGTHS[:len(probs)], np.int64), n, p=probs)
    if live_tail:
        row_len[-1] = 16
    else:
        row_len[-5:] = 0
    live = np.nonzero(row_len)[0]
    col_len = np.zeros(n, np.int64)
    col_len[live] = rng.permutation(row_len[live])
    ia, ja = graph_from_lengths(row_len, col_len, rng)
    return ia, ja


def route_facts(ia, ja):
    """what decides the route of the Kipf entry points, in numpy from the CSR arrays alone"""
    n = ia.size - 1
    row_len = np.diff(ia.astype(np.int64))
    col_len = np.bincount(ja[0] - 1, minlength=n)
    rows = np.repeat(np.arange(n), row_len)
    return {"max_row": int(row_len.max()), "max_col": int(col_len.max()), "band": int(np.abs(rows - (ja[0] - 1)).max()),
            "empty_rows": int((row_len == 0).sum()), "lengths": set(row_len.tolist()),
            "empty_row_is_a_column": bool(col_len[row_len == 0].any())}


def assert_one_launch_route(ia, ja, long_rows=True):
    """no hub row or column (the one-launch kernels are taken), not banded (no LDS-gather route), lengths of the family"""
    f = route_facts(ia, ja)
    assert f["max_row"] <= 256 < K_LONG_ROW and f["max_col"] <= 256 < K_LONG_ROW, f
    assert f["band"] > BAND_MAX and f["max_row"] > BAND_ENTRIES and f["max_col"] > BAND_ENTRIES, f
    assert not f["empty_row_is_a_column"], "an empty row's vertex is listed as a column: its coefficient is powf(0, -0.5)"
    assert f["lengths"] == set(LENGTHS if long_rows else LENGTHS[:-1]), f["lengths"]    # 64 (and 256): the second index blocks
    assert f["empty_rows"] >= 5


def coefficients(ia, ja):
    """(deg_v deg_u)^-1/2 of every entry as float64, by exponent arithmetic (no pow): (4^a 4^b)^-1/2 = 2^-(a+b)"""
    row_len = np.diff(ia.astype(np.int64))
    assert set(row_len.tolist()) <= set(LENGTHS)
    log4 = np.zeros(row_len.size, np.int64)
    live = row_len > 0
    log4[live] = np.round(np.log2(row_len[live])).astype(np.int64) // 2
    assert np.array_equal(4 ** log4[live], row_len[live])
    rows = np.repeat(np.arange(row_len.size), row_len)
    cols = ja[0].astype(np.int64) - 1
    assert live[cols].all()
    return np.ldexp(1.0, -(log4[rows] + log4[cols]))


def assert_power_of_two_words(a, g):
    """every fp32 word of a (coefficients exported from a device handle) has a zero mantissa and lies in [2^-g, 1]"""
    a = np.ascontiguousarray(a, np.float32)
    words = a.view(np.uint32)
    assert a.size and not (words & MANTISSA).any(), "a coefficient is not a power of two"
    assert a.min() >= 2.0 ** -g and a.max() <= 1.0, (float(a.min()), float(a.max()))


# ---- operands -----------------------------------------------------------------------------------------------------------------------
def _draw(rng, values, probs, shape):
    return rng.choice(np.array(values, np.float32), shape, p=probs)


def kipf_operands(n, Fi, Fo, seed=0):
    """x [n, Fi] integers in [-2, 2], W flat [Fo * Fi] in {-1, 0, 1}, bias [Fo] small integers, dZ [n, Fo] integers in [-2, 2], about
    half of them zero.  x and W lean to the positive side and the bias is positive, so that most of Z survives a relu (the
    non-zero condition holds for the relu tensor too) while a few per cent of it is cut"""
    rng = np.random.default_rng(1000 + seed)
    x = _draw(rng, (-2, -1, 0, 1, 2), (.10, .15, .10, .35, .30), (n, Fi))
    W = _draw(rng, (-1, 0, 1), (.30, .20, .50), Fo * Fi)
    bias = rng.integers(1, 4, Fo).astype(np.float32)
    dZ = _draw(rng, (-2, -1, 0, 1, 2), (.10, .15, .50, .15, .10), (n, Fo))
    return x, W, bias, dZ


def gemm_operands(M, K, N, seed=0):
    """the dense kernels' operands: P [M, K] integers in [-2, 2], W flat [N * K] in {-1, 0, 1}, bias [N] integers in [0, 6],
    dZ [M, N] integers in [-2, 2], half of them zero (no graph, no coefficient).  P and W lean to the positive side, as in
    kipf_operands: most of Z survives a relu, some of it is cut at every K"""
    rng = np.random.default_rng(2000 + seed + K + N)
    P = _draw(rng, (-2, -1, 0, 1, 2), (.05, .10, .10, .40, .35), (M, K))
    W = _draw(rng, (-1, 0, 1), (.25, .25, .50), N * K)
    bias = rng.integers(0, 7, N).astype(np.float32)
    dZ = _draw(rng, (-2, -1, 0, 1, 2), (.10, .15, .50, .15, .10), (M, N))
    return P, W, bias, dZ


# ---- the conditions -----------------------------------------------------------------------------------------------------------------
def bits_needed(magnitude, g):
    """log2 of (largest sum of |terms|) * 2^g: below 24, every partial sum in every order is exact in fp32"""
    m = float(np.max(magnitude))
    return (math.log2(m) if m > 0 else -math.inf) + g


def assert_exact_in_fp32(what, magnitude, g):
    b = bits_needed(magnitude, g)
    assert float(np.max(magnitude)) * 2.0 ** g < 2.0 ** 24, f"{what}: the sums need {b:.1f} bits with g = {g}; fp32 holds 24"
    return b


def assert_not_mostly_zero(what, a, rows=64):
    """more than 80 % of the expected tensor is non-zero and no block of 64 rows is all zero: a kernel that writes zeros, or skips a
    chunk of a zero-initialised output, cannot pass"""
    a = np.asarray(a)
    frac = float(np.count_nonzero(a)) / a.size
    assert frac > 0.8, f"{what}: only {frac:.2f} of the expected tensor is non-zero"
    a2 = a.reshape(-1, a.shape[-1])
    starts = np.arange(0, max(a2.shape[0] - rows + 1, 1), rows)      # a ragged tail of fewer than 64 rows belongs to the last block
    live = np.add.reduceat((a2 != 0).sum(axis=1), starts)
    assert live.all(), f"{what}: the 64-row block(s) {np.nonzero(live == 0)[0][:8].tolist()} of the expected tensor are all zero"
    return frac


# ---- the Kipf step ------------------------------------------------------------------------------------------------------------------
class KipfReference:
    """P, Z, dX (both forms) and dW of one Kipf step on a graph of the family, each computed on first use in float64, checked
    against the conditions above and kept as fp32.  bits / nonzero record what the conditions evaluated to.

    W is the flat params%val(:, 1) = W(Fo, Fi) column-major, i.e. Wt [Fi, Fo] row-major; dW has the same flat layout
    (ops.kipf_layer_bwd, ops.matmul_dw)."""

    def __init__(self, ia, ja, x, W, bias, dZ, g_max=8):
        import scipy.sparse as sp

        n = ia.size - 1
        self.n, self.Fi, self.Fo = n, x.shape[1], dZ.shape[1]
        assert x.shape[0] == n and dZ.shape[0] == n and W.size == self.Fi * self.Fo and bias.shape == (self.Fo,)
        self.ia, self.ja, self.x, self.W, self.bias, self.dZ = ia, ja, x, W, bias, dZ
        coef = coefficients(ia, ja)
        self.g = int(-np.log2(coef.min()))
        assert self.g <= g_max and coef.max() <= 1.0, f"smallest coefficient 2^-{self.g}, expected at least 2^-{g_max}"
        for name, t in (("x", x), ("W", W), ("bias", bias), ("dZ", dZ)):
            assert t.dtype == np.float32 and np.array_equal(t, np.round(t)), f"{name} must hold integers"
        indptr, indices = ia.astype(np.int64) - 1, ja[0].astype(np.int64) - 1
        self._A = {True: sp.csr_matrix((coef, indices, indptr), shape=(n, n)),
                   False: sp.csr_matrix((np.ones_like(coef), indices, indptr), shape=(n, n))}
        self._At = {}
        self._Wt = W.reshape(self.Fi, self.Fo).astype(np.float64)
        self._done, self.bits, self.nonzero = {}, {}, {}

    def _finish(self, name, value, magnitude, g, block_rows=64):
        self.bits[name] = assert_exact_in_fp32(name, magnitude, g)
        out = value.astype(np.float32)
        assert np.array_equal(out.astype(np.float64), value), f"{name}: the reference is not representable in fp32"
        self.nonzero[name] = assert_not_mostly_zero(name, out, block_rows)
        out.setflags(write=False)
        self._done[name] = out
        return out

    def _transposed(self, coef):
        if coef not in self._At:
            self._At[coef] = self._A[coef].T.tocsr()
        return self._At[coef]

    def _P64(self):
        if "P64" not in self._done:
            self._done["P64"] = self._A[True] @ self.x.astype(np.float64)
            self._done["absP64"] = self._A[True] @ np.abs(self.x).astype(np.float64)
        return self._done["P64"], self._done["absP64"]

    @property
    def P(self):
        """kipf_propagate(x)"""
        if "P" not in self._done:
            p, ap = self._P64()
            self._finish("P", p, ap, self.g)
        return self._done["P"]

    def Z(self, act="none", bias=True):
        """act(P Wt + bias), act in none / relu"""
        assert act in ("none", "relu")
        name = f"Z[{act}{',bias' if bias else ''}]"
        if name not in self._done:
            if "PW64" not in self._done:          # one product for every epilogue
                p, ap = self._P64()
                self._done["PW64"] = p @ self._Wt, ap @ np.abs(self._Wt)
            z, mag = self._done["PW64"]
            if bias:
                z = z + self.bias.astype(np.float64)
                mag = mag + np.abs(self.bias).astype(np.float64)
            if act == "relu":
                cut = float((z < 0).mean())
                assert cut > 0.005, f"{name}: the relu cuts only {cut:.4f} of the tensor"
                z = np.maximum(z, 0.0)
            self._finish(name, z, mag, self.g)
        return self._done[name]

    def dX(self, exact):
        """(A^T dZ) W, the sum over the column's entries without (exact = 0) or with (exact = 1) the coefficient"""
        exact = bool(exact)
        name = f"dX[exact={int(exact)}]"
        if name not in self._done:
            At = self._transposed(exact)
            q = At @ self.dZ.astype(np.float64)
            aq = At @ np.abs(self.dZ).astype(np.float64)
            self._finish(name, q @ self._Wt.T, aq @ np.abs(self._Wt).T, self.g if exact else 0)
        return self._done[name]

    @property
    def dW(self):
        """dZ . P^T in the flat layout of W"""
        if "dW" not in self._done:
            p, ap = self._P64()
            dw = p.T @ self.dZ.astype(np.float64)
            mag = ap.T @ np.abs(self.dZ).astype(np.float64)
            out = self._finish("dW", dw, mag, self.g)
            self._done["dW"] = out.reshape(-1)
        return self._done["dW"]


# ---- the dense kernels --------------------------------------------------------------------------------------------------------------
class GemmReference:
    """Z = act(P Wt + bias), dP = dZ W, dW = P^T dZ (flat) of integer operands in float64, cast to fp32.  No coefficient: g = 0, and
    the sum of the magnitudes is bounded from the operands' maxima (terms * max * max), which is all the condition needs"""

    def __init__(self, P, W, bias, dZ):
        self.M, self.K = P.shape
        self.N = dZ.shape[1]
        assert W.size == self.K * self.N and dZ.shape[0] == self.M
        for name, t in (("P", P), ("W", W), ("bias", bias), ("dZ", dZ)):
            assert t.dtype == np.float32 and np.array_equal(t, np.round(t)), f"{name} must hold integers"
        self.Pm, self.W, self.bias, self.dZ = P, W, bias, dZ
        self._Wt = W.reshape(self.K, self.N).astype(np.float64)
        mp, mw, mb, mz = (float(np.abs(t).max()) for t in (P, W, bias, dZ))
        self.bits = {"Z": assert_exact_in_fp32("Z", self.K * mp * mw + mb, 0),
                     "dP": assert_exact_in_fp32("dP", self.N * mz * mw, 0),
                     "dW": assert_exact_in_fp32("dW", self.M * mp * mz, 0)}
        self._done, self.nonzero = {}, {}

    def _finish(self, name, value):
        out = value.astype(np.float32)
        assert np.array_equal(out.astype(np.float64), value)
        self.nonzero[name] = assert_not_mostly_zero(name, out)
        out.setflags(write=False)
        self._done[name] = out
        return out

    def Z(self, act="none", bias=True):
        assert act in ("none", "relu")
        name = f"Z[{act}{',bias' if bias else ''}]"
        if name not in self._done:
            if "PW64" not in self._done:          # one product for every epilogue
                self._done["PW64"] = self.Pm.astype(np.float64) @ self._Wt
            z = self._done["PW64"]
            if bias:
                z = z + self.bias.astype(np.float64)
            if act == "relu":
                cut = float((z < 0).mean())
                assert cut > 0.005, f"{name}: the relu cuts only {cut:.4f} of the tensor"
                z = np.maximum(z, 0.0)
            self._finish(name, z)
        return self._done[name]

    @property
    def dP(self):
        if "dP" not in self._done:
            self._finish("dP", self.dZ.astype(np.float64) @ self._Wt.T)
        return self._done["dP"]

    @property
    def dW(self):
        if "dW" not in self._done:
            self._done["dW"] = self._finish("dW", self.Pm.astype(np.float64).T @ self.dZ).reshape(-1)
        return self._done["dW"]


# ---- the cases of tests/test_gpu_many_chunks.py, as functions of the number of compute units -----------------------------------------
FUSED_WIDTHS = (64, 128, 256)
FUSED_CHUNK_ROWS = {64: 64, 128: 32, 256: 16}    # fused.hip: rows per chunk of agg_gemm_kernel<64|128> and agg_gemm256_kernel
DW_CHUNK_ROWS = 32                               # fused_dw.hip kCH
SLAB_ROWS = 32                                   # gemm.hip: rows of one wave's slab


def ceil_div(a, b):
    return -(-a // b)


def fused_rows(C):
    """the smallest row count of the family's shape (a multiple of 64 plus 19) with more than 3 C chunks of 64 rows and a ragged
    tail at every chunk size; 66 003 on 256 compute units"""
    return max(N_FUSED, 64 * (3 * C + 8) + 19)


def dw_cases(C):
    """(n, live_tail) of the folded-dW cases: one chunk per workgroup; a second trip of one workgroup over a one-row chunk (an
    empty row, and once more with a live one); a third trip of four workgroups with a ragged tail; the fused cases' size"""
    k = DW_CHUNK_ROWS
    return [(k * C, False), (k * C + 1, False), (k * C + 1, True), (2 * k * C + 115, False), (fused_rows(C), False)]


def dw_trips(n, C):
    """(workgroups, chunks, most trips of a workgroup, workgroups that make that many) of agg_gemm_dw_kernel"""
    chunks = ceil_div(n, DW_CHUNK_ROWS)
    grid = min(chunks, C)
    most = ceil_div(chunks, grid)
    return grid, chunks, most, chunks - (most - 1) * grid


GEMM_SHAPES = [(K, N) for K in (32, 64, 128) for N in (32, 64, 128)]


def gemm_waves(K, N):
    """waves per workgroup of the weight-resident kernel that gemm_dispatch picks (launch_bres2)"""
    return 8 if K >= 64 and N >= 64 else 4


def gemm_cases(C):
    """(M, K, N): every shape at the third trip of the 4-wave form's first waves, the 8-wave shapes also at their own third trip"""
    m4, m8 = 2 * SLAB_ROWS * 4 * C + 229, 2 * SLAB_ROWS * 8 * C + 229
    return [(m4, K, N) for K, N in GEMM_SHAPES] + [(m8, K, N) for K, N in GEMM_SHAPES if gemm_waves(K, N) == 8]


def gemm_trips(M, K, N, C):
    """(workgroups, slabs, most trips of a wave, waves that make that many) of gemm_bres_kernel / gemm_bres8_kernel"""
    waves = gemm_waves(K, N)
    slabs = ceil_div(M, SLAB_ROWS)
    grid = min(ceil_div(slabs, waves), C)
    most = ceil_div(slabs, grid * waves)
    return grid, slabs, most, slabs - (most - 1) * grid * waves


def blocked_dw_rows(C):
    """M of the 256 x 256 weight gradient (the blocked register-resident route of gemm_dw_dispatch)"""
    return 2 * SLAB_ROWS * 8 * C + 229


def blocked_dw_ranges(M, C):
    """(row ranges nx, rows per wave rpw) as gemm_dw_dispatch lays the blocked route out"""
    nx = min(ceil_div(M, 128), C)
    rpw = ceil_div(M, nx * 4)
    rpw = (rpw + 1) & ~1
    nx = ceil_div(M, rpw * 4)
    return (nx + 7) & ~7, rpw


# ---- the cases built: what tests/test_gpu_many_chunks.py runs and tests/test_exact_reference.py evaluates on the CPU ----------------
_GRAPHS = {}


def cached_graph(n, seed, long_rows, live_tail=False):
    key = (n, seed, long_rows, live_tail)
    if key not in _GRAPHS:
        ia, ja = exact_graph(n, seed, long_rows, live_tail)
        assert_one_launch_route(ia, ja, long_rows)
        ia.setflags(write=False); ja.setflags(write=False)
        _GRAPHS[key] = (ia, ja)
    return _GRAPHS[key]


def fused_case(C, F):
    """the fused forward / reverse case at width F: one graph for the three widths, 256-entry rows included (g = 8)"""
    ia, ja = cached_graph(fused_rows(C), 0, True)
    return KipfReference(ia, ja, *kipf_operands(ia.size - 1, F, F, seed=F), g_max=8)


def dw_case(n, live_tail):
    """a folded-dW case, 128 -> 128, without the 256-entry rows (g = 6)"""
    ia, ja = cached_graph(n, 1, False, live_tail)
    return KipfReference(ia, ja, *kipf_operands(n, 128, 128, seed=n + int(live_tail)), g_max=6)


def gemm_case(M, K, N):
    return GemmReference(*gemm_operands(M, K, N))
