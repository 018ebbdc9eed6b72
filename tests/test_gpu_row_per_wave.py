"""GPU: the one-launch Kipf kernel at 128 features (fused.hip, agg_gemm_kernel<128>), whose gather takes a whole wave per row, at
every edge of its row loop.

A wave gathers its two rows one after the other; a row's start, length, entry ids and coefficients live in scalar registers.
Lane j holds entry j of the row's current 64-entry block (BLOCK), the first PREFETCH row loads fly under the matrix work of the
chunk before, the rest stream GROUP at a time, and a row leaves each chain at its own length.  The graphs here are built by hand
so that row lengths sit on both sides of each of those numbers, in both positions of a wave's pair, beside the longest row the
route takes (512), at odd row starts, and so that the last rows are short: a read of a full block from their start would pass the
end of the handle's exactly sized entry arrays.  n takes 1, 31, 32, 33 (one chunk is 32 rows) and a size derived from the number of
compute units at which every workgroup redraws a chunk after its first three and the last chunk is ragged.

Routes: ops.kipf_layer_fwd (no activation / relu, with / without bias), ops.kipf_layer_bwd_x (exact 0 / 1) and ops.pull_gemm.
P is held to np.array_equal against ops.kipf_propagate (the two-kernel route) and the oracle, both CSR-order sums; Z and dX to 1e-5
of the oracle on random floats, and to np.array_equal on operands whose sums are exact in any order: integers where no coefficient
enters (any row length), and the family of tests/exact_reference.py (power-of-two coefficients) where one does."""
import numpy as np
import pytest

import exact_reference as er
from helpers import assert_close, graph_from_lengths, spread_lengths

pytestmark = pytest.mark.gpu

F = 128
CHUNK = er.FUSED_CHUNK_ROWS[F]      # 32 rows, two per wave
PREFETCH = 16                       # fused.hip kFirst
GROUP = 4                           # fused.hip kUn
BLOCK = 64                          # entries of a row whose ids one load holds, one per lane
LONGEST = er.K_LONG_ROW             # 512: the longest row of the one-launch route
EDGES = (0, 1, 2, PREFETCH - 1, PREFETCH, PREFETCH + 1, PREFETCH + GROUP - 1, PREFETCH + GROUP, PREFETCH + GROUP + 1,
         BLOCK - 1, BLOCK, BLOCK + 1, BLOCK + GROUP + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, LONGEST)
TAIL = (2, 0, 1, 1)                 # the last rows: their entries end the entry arrays


def T(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def edge_lengths(n, rng):
    """row lengths [n]: below 256 rows a cycle through the edges that fit; otherwise chunk 0 = (512, 1) in wave 0 beside 30 rows of
    one entry, chunk 1 = (1, 512), then every edge as (L, 1), (1, L) and (L, L), then 0 .. 24 at random; TAIL at the end"""
    if n < 256:
        lens = np.resize(np.array((PREFETCH + 1, 1, 2, PREFETCH - 1, PREFETCH, BLOCK - 1, BLOCK, BLOCK + 1, 0, PREFETCH + GROUP + 1),
                                  np.int64), n)
    else:
        lens = rng.integers(0, 25, n).astype(np.int64)
        lens[:2 * CHUNK] = 1
        lens[0] = lens[CHUNK + 1] = LONGEST
        p = 2 * CHUNK
        for L in EDGES:
            lens[p:p + 6] = (L, 1, 1, L, L, L)
            p += 6
        assert set(EDGES) <= set(lens.tolist())
    if n >= 8:
        lens[-len(TAIL):] = TAIL
    return lens


class Case:
    """one hand-built graph in both roles -- rows of the chosen lengths (forward, pull) and columns of the chosen lengths (the
    reverse walks the transposed structure) -- with random float operands and the oracle's results"""

    def __init__(self, n, dev, oracle):
        from athena_amd import DeviceGraph

        rng = np.random.default_rng(7000 + n)
        self.n, self.dev = n, dev
        lens = self.lens = edge_lengths(n, rng)
        other = spread_lengths(int(lens.sum()), lens > 0)      # an empty row's vertex is never listed: no powf(0, -0.5)
        self.ia, self.ja = graph_from_lengths(lens, other, rng)
        self.ia_t, self.ja_t = graph_from_lengths(other, lens, rng)
        for ia, ja in ((self.ia, self.ja), (self.ia_t, self.ja_t)):
            f = er.route_facts(ia, ja)                               # the one-launch route: no hub, not the banded LDS gather
            assert f["max_row"] <= LONGEST and f["max_col"] <= LONGEST and not f["empty_row_is_a_column"], f
            assert f["max_row"] > er.BAND_ENTRIES and f["max_col"] > er.BAND_ENTRIES, f
        starts = np.cumsum(lens)[:-1][lens[1:] > 0]
        if n > 1:
            assert (starts % 2 == 1).any() and (starts % 4 != 0).any()     # rows that start 4-byte aligned and no better
            assert lens[-4:].sum() < PREFETCH                              # a full block read from the last rows' starts ends outside
        assert lens[-1] < BLOCK
        self.g, self.g_t = DeviceGraph(self.ia, self.ja, n_edge_cols=0), DeviceGraph(self.ia_t, self.ja_t, n_edge_cols=0)
        nnz = int(lens.sum())
        assert self.g.export("coef").size == nnz and self.g_t.export("t_coef").size == nnz     # exactly sized
        self.x = rng.standard_normal((n, F)).astype(np.float32)
        self.dZ = rng.standard_normal((n, F)).astype(np.float32)
        self.W = (rng.standard_normal(F * F) / np.sqrt(F)).astype(np.float32)
        self.bias = rng.standard_normal(F).astype(np.float32)
        self.P = oracle.kipf_propagate(self.x, self.ia, self.ja)
        self.PW = oracle.matmul(self.W, self.P, F)
        self.d = {k: T(getattr(self, k), dev) for k in ("x", "dZ", "W", "bias")}
        assert all(t.data_ptr() % 16 == 0 for t in self.d.values())

    def rows_matrix(self, coef):
        """the forward rows as a float64 sparse matrix, with the handle's own coefficients or ones"""
        import scipy.sparse as sp

        v = self.g.export("coef").astype(np.float64) if coef else np.ones(self.ja.shape[1])
        return sp.csr_matrix((v, self.ja[0].astype(np.int64) - 1, self.ia.astype(np.int64) - 1), shape=(self.n, self.n))

    def cols_matrix(self):
        import scipy.sparse as sp

        return sp.csr_matrix((np.ones(self.ja_t.shape[1]), self.ja_t[0].astype(np.int64) - 1, self.ia_t.astype(np.int64) - 1),
                             shape=(self.n, self.n)).T.tocsr()


def many_chunks_rows(C):
    """more than three chunks per workgroup (a redraw returns a live chunk) and a last chunk of 7 rows"""
    return CHUNK * (3 * C + 5) + 7


@pytest.fixture(scope="module")
def C(dev):
    import torch

    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


@pytest.fixture(scope="module", params=[1, CHUNK - 1, CHUNK, CHUNK + 1, "many"], ids=lambda p: f"n_{p}")
def case(request, dev, oracle, C):
    n = many_chunks_rows(C) if request.param == "many" else request.param
    if request.param == "many":
        chunks = er.ceil_div(n, CHUNK)
        assert chunks > 3 * C and n % CHUNK not in (0, 1)
    return Case(n, dev, oracle)


def twice(fn):
    """fn() two times: the same bits from both launches"""
    import torch

    a, b = fn(), fn()
    torch.cuda.synchronize()
    for s, t in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(s, t), "two launches of the same call differ"
    return a


def scale_close(got, ref, what):
    assert_close(got.cpu().numpy(), ref, rtol=1e-5, what=what)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("act", ["none", "relu"])
def test_forward(case, oracle, act, with_bias):
    from athena_amd import ops

    c, d = case, case.d
    P, Z = twice(lambda: ops.kipf_layer_fwd(c.g, d["x"], d["W"], F, bias=d["bias"] if with_bias else None, act=act))
    assert np.array_equal(P.cpu().numpy(), c.P), "P differs from the oracle's CSR-order sums"
    assert np.array_equal(P.cpu().numpy(), ops.kipf_propagate(c.g, d["x"]).cpu().numpy()), "P differs from the two-kernel route"
    z = c.PW + c.bias if with_bias else c.PW
    scale_close(Z, np.maximum(z, 0.0) if act == "relu" else z, f"Z, {act}, bias {with_bias}")
    none, Z2 = ops.kipf_layer_fwd(c.g, d["x"], d["W"], F, bias=d["bias"] if with_bias else None, act=act, keep_P=False)
    assert none is None and np.array_equal(Z2.cpu().numpy(), Z.cpu().numpy()), "Z without a stored P"


@pytest.mark.parametrize("exact", [False, True])
def test_reverse(case, oracle, exact):
    from athena_amd import ops

    c, d = case, case.d
    dX = twice(lambda: ops.kipf_layer_bwd_x(c.g_t, d["dZ"], d["W"], F, exact=exact))
    q = oracle.kipf_propagate_bwd(c.dZ, c.ia_t, c.ja_t, exact=exact)
    assert np.array_equal(ops.kipf_propagate_bwd(c.g_t, d["dZ"], exact=exact).cpu().numpy(), q)     # the gather alone, CSR order
    scale_close(dX, oracle.matmul_dx(c.W, q, F), f"dX, exact {exact}")


@pytest.mark.parametrize("exact", [False, True])
def test_pull(case, oracle, exact):
    from athena_amd import ops

    c, d = case, case.d
    dX = twice(lambda: ops.pull_gemm(c.g, d["dZ"], d["W"], F, exact=exact))
    q = oracle.kipf_propagate(c.dZ, c.ia, c.ja) if exact else (c.rows_matrix(False) @ c.dZ.astype(np.float64)).astype(np.float32)
    scale_close(dX, oracle.matmul_dx(c.W, q, F), f"pull dX, exact {exact}")


def test_sums_without_coefficients_are_exact_at_every_length(case):
    """integers in, no coefficient: every partial sum of (A^T dZ) W and of (A dZ) W is an integer below 2^24 whatever the row
    lengths, so the reverse and the pull are held to np.array_equal over the whole tensor"""
    from athena_amd import ops

    c = case
    _, W, _, dZ = er.kipf_operands(c.n, F, F, seed=c.n)
    Wt = W.reshape(F, F).astype(np.float64)
    Wd, dZd = T(W, c.dev), T(dZ, c.dev)
    for what, A, got in (("reverse", c.cols_matrix(), lambda: ops.kipf_layer_bwd_x(c.g_t, dZd, Wd, F, exact=False)),
                         ("pull", c.rows_matrix(False), lambda: ops.pull_gemm(c.g, dZd, Wd, F, exact=False))):
        want = (A @ dZ.astype(np.float64)) @ Wt.T
        er.assert_exact_in_fp32(what, (A @ np.abs(dZ).astype(np.float64)) @ np.abs(Wt).T, 0)
        assert np.count_nonzero(want) > 0.5 * want.size or c.n == 1
        assert np.array_equal(got().cpu().numpy(), want.astype(np.float32)), f"{what}: dX differs from the exact sums"


# ---- with coefficients: the family of tests/exact_reference.py (rows of 0, 1, 4, 16, 64, 256 entries: PREFETCH and BLOCK themselves) ----
@pytest.fixture(scope="module")
def family(dev):
    from athena_amd import DeviceGraph

    n = CHUNK * 75 + 9
    ia, ja = er.exact_graph(n, seed=11)
    er.assert_one_launch_route(ia, ja)
    r = er.KipfReference(ia, ja, *er.kipf_operands(n, F, F, seed=11))
    g = DeviceGraph(ia, ja, n_edge_cols=0)
    for name in ("coef", "t_coef"):
        er.assert_power_of_two_words(g.export(name), 8)
    return {"r": r, "g": g, **{k: T(getattr(r, k), dev) for k in ("x", "W", "bias", "dZ")}}


@pytest.mark.parametrize("act", ["none", "relu"])
def test_family_forward_is_exact(family, act):
    from athena_amd import ops

    f, r = family, family["r"]
    P, Z = twice(lambda: ops.kipf_layer_fwd(f["g"], f["x"], f["W"], F, bias=f["bias"], act=act))
    assert np.array_equal(P.cpu().numpy(), r.P)
    assert np.array_equal(Z.cpu().numpy(), r.Z(act))


@pytest.mark.parametrize("exact", [False, True])
def test_family_reverse_and_pull_are_exact(family, exact):
    import scipy.sparse as sp

    from athena_amd import ops

    f, r = family, family["r"]
    dX = twice(lambda: ops.kipf_layer_bwd_x(f["g"], f["dZ"], f["W"], F, exact=exact))
    assert np.array_equal(dX.cpu().numpy(), r.dX(exact))
    v = er.coefficients(r.ia, r.ja) if exact else np.ones(r.ja.shape[1])
    A = sp.csr_matrix((v, r.ja[0].astype(np.int64) - 1, r.ia.astype(np.int64) - 1), shape=(r.n, r.n))
    Wt = r.W.reshape(F, F).astype(np.float64)
    want = (A @ r.dZ.astype(np.float64)) @ Wt.T
    er.assert_exact_in_fp32("pull", (A @ np.abs(r.dZ).astype(np.float64)) @ np.abs(Wt).T, r.g if exact else 0)
    got = twice(lambda: ops.pull_gemm(f["g"], f["dZ"], f["W"], F, exact=exact))
    assert np.array_equal(got.cpu().numpy(), want.astype(np.float32))


# ---- a gathered tensor of 4 GiB and more: no buffer descriptor, the row's 64-bit address is formed in scalar registers ----
def test_pull_from_a_tensor_beyond_4_gib(dev):
    """ops.pull_gemm over a rectangular handle whose sources are the rows of a 4.3 GB tensor, among them row 0, the last row, the
    first rows past 2^31 and 2^32 bytes; the reference sums the listed rows in float64"""
    import scipy.sparse as sp
    import torch

    from athena_amd import DeviceGraph, ops

    n_cols = 2 ** 32 // (4 * F) + 4096
    n = 4 * CHUNK + 5
    rng = np.random.default_rng(4096)
    lens = edge_lengths(n, rng)
    nnz = int(lens.sum())
    ids = rng.integers(0, n_cols, nnz)
    ids[:6] = (0, n_cols - 1, 2 ** 31 // (4 * F), 2 ** 31 // (4 * F) - 1, 2 ** 32 // (4 * F), 2 ** 32 // (4 * F) - 1)
    ia = np.concatenate([[1], 1 + np.cumsum(lens)]).astype(np.int32)
    ja = np.zeros((2, nnz), np.int32, order="F")
    ja[0] = ids + 1
    g = DeviceGraph(ia, ja, n_cols=n_cols, n_edge_cols=0, row_deg=np.maximum(lens, 1), col_deg=np.full(n_cols, 4))
    assert n_cols * F * 4 >= 2 ** 32 and g.export("coef").size == nnz
    gen = torch.Generator(device=dev).manual_seed(5)
    dZ = torch.empty((n_cols, F), dtype=torch.float32, device=dev).normal_(generator=gen)
    W = (rng.standard_normal(F * F) / np.sqrt(F)).astype(np.float32)
    Wd = T(W, dev)
    listed = dZ[torch.from_numpy(ids).to(dev)].cpu().numpy().astype(np.float64)
    for exact in (False, True):
        v = g.export("coef").astype(np.float64) if exact else np.ones(nnz)
        q = sp.csr_matrix((v, np.arange(nnz), ia.astype(np.int64) - 1), shape=(n, nnz)) @ listed
        got = twice(lambda: ops.pull_gemm(g, dZ, Wd, F, exact=exact))
        assert_close(got.cpu().numpy(), q @ W.reshape(F, F).astype(np.float64).T, rtol=1e-5, what=f"pull from 4.3 GB, exact {exact}")
