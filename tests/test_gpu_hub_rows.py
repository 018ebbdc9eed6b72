"""Hub rows bit for bit.  A row (or, on the transposed side, a column) of more than 512 entries leaves the main gather launch: its
512-entry segments are summed as tasks of their own and added in segment order by a combine kernel (agg.hip, capi.hip:
build_long_plan).  That result is a fixed fp32 expression; tests/segment_reference.py is its executable definition, and every
comparison here is np.array_equal against it over the WHOLE output -- hub rows, short rows and empty rows together, into outputs
pre-filled with NaN, so a row nobody wrote shows as well.

The graphs hold every length at which the route changes (helpers.HUB_LENGTHS) at the positions where an index can slip: a hub as
row 0, as the last row, hubs side by side, a hub beside an empty row; as row lengths, as column counts, and both."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import segment_reference as sr
from helpers import (HUB_LENGTHS, assert_close, graph_from_lengths, hub_length_layout, placed, placed_out, spread_lengths)

pytestmark = pytest.mark.gpu

N = 1500
E_COLS = 48                      # edge columns of the graphs that carry edge ids
WIDTHS = [1, 2, 3, 4, 6, 7, 64, 130, 256, 260, 516]   # vec = 1 / 2 / 4, G = 1 .. 64, Fp = F and Fp > F, more than one pass over the row


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def H(t):
    return t.cpu().numpy()


def nan_out(shape, dev):
    return torch.full(tuple(shape), float("nan"), device=dev, dtype=torch.float32)


class Case:
    """a graph on the host (athena's CSR, degrees) and its device handle"""

    def __init__(self, ia, ja, n_cols=None, row_deg=None, col_deg=None, n_edge_cols=0):
        from athena_amd import DeviceGraph

        self.ia, self.ja = ia, ja
        self.n_rows = ia.size - 1
        self.n_cols = self.n_rows if n_cols is None else n_cols
        self.rd, self.cd, self.n_edge_cols = row_deg, col_deg, n_edge_cols
        self.deg = np.diff(ia)
        self.cdeg = np.bincount(ja[0] - 1, minlength=self.n_cols)
        if row_deg is None:                                  # implicit degrees: a listed column needs entries of its own
            assert (self.deg[ja[0] - 1] > 0).all()
        self.g = DeviceGraph(ia, ja, n_cols=self.n_cols, n_edge_cols=n_edge_cols, row_deg=row_deg, col_deg=col_deg)

    def operands(self, F, seed=0):
        rng = np.random.default_rng(1000 * seed + 7 * F + self.n_rows)
        return rng.uniform(-1, 1, (self.n_cols, F)).astype(np.float32), rng.uniform(-1, 1, (self.n_rows, F)).astype(np.float32)

    # the yardstick, by op
    def fwd(self, x):
        return sr.kipf_propagate(x, self.ia, self.ja, self.rd, self.cd)

    def bwd(self, gr, exact):
        return sr.kipf_propagate_bwd(gr, self.ia, self.ja, exact=exact, n_out=self.n_cols, row_deg=self.rd, col_deg=self.cd)


def _lengths_graph(hub_rows, hub_cols, seed, edge_cols=0):
    rng = np.random.default_rng(seed)
    lay = hub_length_layout(N, rng)
    nz = lay > 0
    if hub_rows:
        row_len = lay
        col_len = np.zeros(N, np.int64)
        col_len[nz] = np.roll(lay[nz], 5) if hub_cols else spread_lengths(int(lay.sum()), nz)[nz]
    else:
        col_len = lay
        row_len = spread_lengths(int(col_len.sum()), col_len > 0)
    return graph_from_lengths(row_len, col_len, rng, edge_cols)


def _edge_hubs(ja, rng):
    """edge column 1 carried by 513 entries, edge column 2 by 1025, nobody else on them"""
    e = np.where(ja[1] > 0, 3 + ja[1] % (E_COLS - 2), 0)
    pos = rng.permutation(ja.shape[1])
    e[pos[:513]], e[pos[513:513 + 1025]] = 1, 2
    ja[1] = e
    assert np.bincount(ja[1], minlength=E_COLS + 1)[1:3].tolist() == [513, 1025] and ja[1].max() <= E_COLS


_CASES = {}


def case(name):
    """the graphs of this module, built once"""
    if name in _CASES:
        return _CASES[name]
    rng = np.random.default_rng(len(name))
    if name == "rows":          # hub rows, no hub column: lp_fwd alone; edge ids, two edge columns carried by 513 and 1025 entries
        ia, ja = _lengths_graph(True, False, 21, edge_cols=E_COLS)
        _edge_hubs(ja, rng)
        c = Case(ia, ja, n_edge_cols=E_COLS)
        assert c.deg.max() == 2600 and c.cdeg.max() <= 512
    elif name == "cols":        # hub columns, no hub row: lp_bwd alone
        ia, ja = _lengths_graph(False, True, 22, edge_cols=E_COLS)
        c = Case(ia, ja, n_edge_cols=E_COLS)
        assert c.deg.max() <= 512 and set(HUB_LENGTHS) <= set(c.cdeg.tolist())
    elif name == "both":        # every length as a row length AND as a column count
        ia, ja = _lengths_graph(True, True, 23, edge_cols=E_COLS)
        c = Case(ia, ja, n_edge_cols=E_COLS)
        assert set(HUB_LENGTHS) <= set(c.deg.tolist()) and set(HUB_LENGTHS) <= set(c.cdeg.tolist())
    elif name == "rect":        # a shard: more columns than rows, explicit degrees
        lay = hub_length_layout(N, rng)
        col_len = np.concatenate([np.zeros(19, np.int64), np.roll(lay, 11), np.zeros(18, np.int64)])
        ia, ja = graph_from_lengths(lay, col_len, rng)
        c = Case(ia, ja, n_cols=col_len.size, row_deg=(lay + rng.integers(1, 4, N)).astype(np.int32),
                 col_deg=rng.integers(1, 60, col_len.size).astype(np.int32))
    elif name == "only_row":    # n_rows = 1: the graph IS a hub (and, square, a hub column of the same entries)
        ia = np.array([1, 1026], np.int32)
        ja = np.zeros((2, 1025), np.int32, order="F")
        ja[0] = 1
        c = Case(ia, ja)
    elif name == "only_row_rect":   # one row of 2600 entries over 40 columns
        ia = np.array([1, 2601], np.int32)
        ja = np.zeros((2, 2600), np.int32, order="F")
        ja[0] = rng.integers(1, 41, 2600)
        c = Case(ia, ja, n_cols=40, row_deg=np.array([2600], np.int32), col_deg=rng.integers(1, 90, 40).astype(np.int32))
    elif name in ("one513", "one513_col"):   # exactly one row (column) of 513, every other of at most 3: n_long = 1, n_tasks = 2
        lens = rng.integers(1, 4, N)
        lens[N // 3] = 513
        flat = spread_lengths(int(lens.sum()), np.ones(N, bool))
        ia, ja = graph_from_lengths(lens, flat, rng) if name == "one513" else graph_from_lengths(flat, lens, rng)
        c = Case(ia, ja)
        assert sorted([c.deg.max(), c.cdeg.max()]) == [int(flat.max()), 513] and flat.max() <= 3
    elif name == "many_tasks":  # four rows of 2600 and four of 1537: 40 tasks
        lens = rng.integers(1, 4, 600)
        lens[[0, 100, 101, 300]] = 2600
        lens[[7, 299, 400, 599]] = 1537
        ia, ja = graph_from_lengths(lens, spread_lengths(int(lens.sum()), np.ones(600, bool)), rng)
        c = Case(ia, ja)
        assert sr.split_rows(ia.astype(np.int64) - 1)[2].size - (600 - 8) == 40
    elif name == "banded":      # every neighbour within 8 rows, at most 8 entries a row -- but for one row of 513 duplicates
        n = 600
        lens = rng.integers(1, 9, n)
        lens[300] = 513
        ia = np.concatenate([[1], 1 + np.cumsum(lens)]).astype(np.int32)
        rows = np.repeat(np.arange(n), lens)
        ja = np.zeros((2, rows.size), np.int32, order="F")
        ja[0] = np.clip(rows + rng.integers(-8, 9, rows.size), 0, n - 1) + 1
        c = Case(ia, ja)
        assert np.abs(ja[0] - 1 - rows).max() <= 8 and c.cdeg.max() <= 512
    else:
        raise KeyError(name)
    _CASES[name] = c
    return c


def same(got, want, what):
    got = H(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError(f"{what}: {bad.size} row(s) differ from the yardstick, the first {bad[:8].tolist()}; "
                             f"worst |diff| {np.nanmax(np.abs(got - want)):.3e}, NaN left: {int(np.isnan(got).sum())}")


def kipf_entries(c, F, dev, oracle=None):
    """every Kipf entry of one graph at one width against the yardstick"""
    from athena_amd import ops

    x, gr = c.operands(F)
    xd, gd = T(x, dev), T(gr, dev)
    y = c.fwd(x)
    d = {ex: c.bwd(gr, ex) for ex in (False, True)}
    same(ops.kipf_propagate(c.g, xd, out=nan_out((c.n_rows, F), dev)), y, "kipf_propagate")
    same(ops.kipf_propagate_act(c.g, xd, "none", out=nan_out((c.n_rows, F), dev)), y, "kipf_propagate_act none")
    for ex in (False, True):
        same(ops.kipf_propagate_bwd(c.g, gd, exact=ex, out=nan_out((c.n_cols, F), dev)), d[ex], f"kipf_propagate_bwd exact={ex}")
    same(ops.reverse_kipf_propagate(c.g, gd, out=nan_out((c.n_cols, F), dev)), d[False], "reverse_kipf_propagate")
    same(ops.reverse_kipf_propagate_partial(c.g, xd, out=nan_out((c.n_rows, F), dev)), y, "reverse_kipf_propagate_partial")
    same(ops.reverse_kipf_propagate_partial(c.g, gd, val_form=True, out=nan_out((c.n_cols, F), dev)), d[False],
         "reverse_kipf_propagate_partial_val")
    # with hubs the dual entries are two single passes: the single entries' bits
    plain, coef = ops.pull_dual(c.g, xd, plain=nan_out((c.n_rows, F), dev), coef=nan_out((c.n_rows, F), dev))
    same(plain, sr.neighbour_sum(x, c.ia, c.ja), "fwd_dual plain")
    same(coef, y, "fwd_dual coef")
    plain, coef = ops.kipf_propagate_bwd_dual(c.g, gd)
    same(plain, d[False], "bwd_dual plain")
    same(coef, d[True], "bwd_dual coef")
    return x, gr, y, d


@pytest.mark.parametrize("F", WIDTHS)
def test_kipf_entries_at_every_length_position_and_width(dev, oracle, F):
    """row lengths AND column counts 0, 1, 511, 512, 513, 1023, 1024, 1025, 1536, 1537, 2600 in one graph, at every width that changes
    vec, G or Fp: forward, activation none, both reverse forms, the three reverse_kipf_propagate aliases, both dual entries"""
    c = case("both")
    x, gr, y, d = kipf_entries(c, F, dev)
    # 512 entries is still a short row: the oracle's sequential sum
    r512, c512 = np.nonzero(c.deg == 512)[0], np.nonzero(c.cdeg == 512)[0]
    assert np.array_equal(y[r512], oracle.kipf_propagate(x, c.ia, c.ja)[r512])
    assert np.array_equal(d[True][c512], oracle.kipf_propagate_bwd(gr, c.ia, c.ja, exact=True)[c512])
    assert np.array_equal(d[False][c512], oracle.kipf_propagate_bwd(gr, c.ia, c.ja)[c512])
    assert (y[c.deg == 0] == 0).all() and (d[False][c.cdeg == 0] == 0).all()


@pytest.mark.parametrize("F", [3, 64, 260])
@pytest.mark.parametrize("name", ["rows", "cols", "rect", "only_row", "only_row_rect", "one513", "one513_col"])
def test_kipf_entries_with_one_plan_empty_shards_and_tiny_plans(dev, name, F):
    """hub rows without a hub column and the reverse (each plan beside an empty one), a rectangular shard with explicit degrees,
    a graph whose only row is a hub, and the smallest plan there is: one row of 513 entries, n_long = 1, n_tasks = 2"""
    kipf_entries(case(name), F, dev)


@pytest.mark.parametrize("F", [3, 64, 130])
@pytest.mark.parametrize("kind", ["relu", "sigmoid", "tanh"])
def test_kipf_activation_is_applied_once_after_the_combine(dev, kind, F):
    """relu in numpy on the yardstick; sigmoid / tanh: ops.activation on the bit-exact pre-activation rows -- the device's expf /
    tanhf on identical inputs, hence the same bits, unless the activation touched the segment partials"""
    from athena_amd import ops

    for name in ("both", "rect"):
        c = case(name)
        x, _ = c.operands(F, seed=2)
        y = c.fwd(x)
        got = ops.kipf_propagate_act(c.g, T(x, dev), kind, out=nan_out((c.n_rows, F), dev))
        want = np.where(y > 0, y, np.float32(0)) if kind == "relu" else H(ops.activation(kind, T(y, dev)))
        same(got, want, f"{name}: kipf_propagate_act {kind}")
        assert (y[c.deg > 512] < 0).any() and not np.array_equal(want, y)


@pytest.mark.parametrize("Fv,Fe", [(64, 0), (0, 8), (0, 3), (7, 3), (5, 4), (3, 1), (64, 8), (130, 2)])
def test_duvenaud_propagate_on_hub_rows(dev, oracle, Fv, Fe):
    """the vertex part alone, the edge part alone (the Fv == 0 form) and packed rows; Fv odd: the edge part starts at c + Fv and
    drops to one float per lane while the vertex part keeps its own vector width"""
    from athena_amd import ops

    for name in ("rows", "both"):
        c = case(name)
        rng = np.random.default_rng(Fv * 31 + Fe)
        x = rng.uniform(-1, 1, (N, Fv)).astype(np.float32) if Fv else None
        e = rng.uniform(-1, 1, (E_COLS, Fe)).astype(np.float32) if Fe else None
        want = sr.duvenaud_propagate(x, e, c.ia, c.ja)
        if Fe == 0:
            got = ops.neighbour_sum(c.g, T(x, dev), out=nan_out((N, Fv), dev))
        elif Fv == 0:
            got = ops.duvenaud_propagate_edges(c.g, T(e, dev), out=nan_out((N, Fe), dev))
        else:
            got = ops.duvenaud_propagate(c.g, T(x, dev), T(e, dev), out=nan_out((N, Fv + Fe), dev))
        same(got, want, f"{name}: duvenaud_propagate {Fv}+{Fe}")
        short = c.deg <= 512
        if Fv and Fe:
            assert np.array_equal(want[short], oracle.duvenaud_propagate(x, e, c.ia, c.ja)[short])


@pytest.mark.parametrize("Fv,Fe", [(7, 3), (64, 8), (3, 0), (130, 2)])
def test_duvenaud_propagate_bwd_x_on_hub_columns(dev, Fv, Fe):
    """the vertex part of packed rows [n, Fv + Fe] gathered over hub columns"""
    from athena_amd import ops

    for name in ("cols", "both"):
        c = case(name)
        up = np.random.default_rng(Fv + Fe).uniform(-1, 1, (N, Fv + Fe)).astype(np.float32)
        same(ops.duvenaud_propagate_bwd_x(c.g, T(up, dev), Fv), sr.duvenaud_propagate_bwd_x(up, Fv, c.ia, c.ja), f"{name}: bwd_x {Fv}+{Fe}")


@pytest.mark.parametrize("Fv,Fe", [(7, 3), (64, 8), (0, 5)])
def test_duvenaud_propagate_bwd_e_sums_a_long_edge_column_entry_by_entry(dev, oracle, Fv, Fe):
    """athena_mp_duvenaud_propagate_bwd_e passes NO long-row plan: an edge column carried by 513 or by 1025 entries is summed
    sequentially, in entry order, and equals the ORACLE bit for bit -- not the segmented yardstick.  Cutting such a column into
    segments would be a change of the definition; this assertion is where that decision becomes visible."""
    from athena_amd import ops

    c = case("rows")
    assert np.bincount(c.ja[1])[1:3].tolist() == [513, 1025]
    up = np.random.default_rng(Fe).uniform(-1, 1, (N, Fv + Fe)).astype(np.float32)
    want = oracle.duvenaud_propagate_bwd_e(up, Fv, E_COLS, c.ia, c.ja)
    same(ops.duvenaud_propagate_bwd_e(c.g, T(up, dev), Fv), want, "bwd_e")
    # ... and the 1025-entry column is one whose segmented sum would have other bits
    rows = np.repeat(np.arange(N), c.deg)[c.ja[1] == 2]
    seg = sr.gather_sum(np.array([0, rows.size]), rows, np.ascontiguousarray(up[:, Fv:]))
    assert not np.array_equal(seg[0], want[1])


def test_banded_graph_with_one_hub_row_takes_the_general_gather(dev):
    """band <= 8 and at most 8 entries a row, but for one row of 513 duplicate entries: max_row_len keeps the graph off the
    LDS-staged and the short-row gathers, and the hub gets the yardstick's bits at F = 64"""
    kipf_entries(case("banded"), 64, dev)


@pytest.mark.parametrize("F", [64, 128])
@pytest.mark.parametrize("name", ["one513", "one513_col", "both"])
def test_layer_steps_leave_the_fused_route_on_hub_graphs(dev, oracle, name, F):
    """the four `n_long == 0` predicates of fused.hip: forward step and pull_gemm (lp_fwd), bwd_x and the dW step (lp_bwd), on a
    graph with one 513-entry row, one with one 513-entry column, and the graph of every length.  Where a plan is not empty the call
    is the unfused composition of the public ops, bit for bit, and its aggregated intermediate is the yardstick's; against the
    oracle's order the outputs keep the existing 1e-5, anchored on float64."""
    from athena_amd import ops
    from oracle import oracle64 as o64

    c = case(name)
    rng = np.random.default_rng(F)
    x, dz = c.operands(F, seed=3)
    w = (rng.standard_normal(F * F) * np.sqrt(2.0 / F)).astype(np.float32)
    b = rng.standard_normal(F).astype(np.float32)
    xd, dzd, wd, bd = (T(a, dev) for a in (x, dz, w, b))
    hub_rows, hub_cols = c.deg.max() > 512, c.cdeg.max() > 512
    # forward step
    P, Z = ops.kipf_layer_fwd(c.g, xd, wd, F, bias=bd, act="tanh")
    same(P, c.fwd(x), "layer_fwd: P")
    if hub_rows:
        assert torch.equal(Z, ops.matmul(wd, P, F, bias=bd, act="tanh")), "layer_fwd: Z is not matmul(P)"
    assert_close(H(Z), oracle.activation("tanh", oracle.add_bias_rows(oracle.matmul(w, oracle.kipf_propagate(x, c.ia, c.ja), F), b)), 1e-5,
                 "layer_fwd: Z", f64=lambda: o64.activation("tanh", o64.add_bias_rows(o64.matmul(w, o64.kipf_propagate(x, c.ia, c.ja), F), b)))
    # pull_gemm over the forward rows
    for ex in (False, True):
        q = ops.kipf_propagate(c.g, dzd) if ex else ops.neighbour_sum(c.g, dzd)
        same(q, c.fwd(dz) if ex else sr.neighbour_sum(dz, c.ia, c.ja), f"pull_gemm exact={ex}: gathered rows")
        dX = ops.pull_gemm(c.g, dzd, wd, F, exact=ex)
        if hub_rows:
            assert torch.equal(dX, ops.matmul_dx(wd, q, F)), f"pull_gemm exact={ex} is not matmul_dx(gather)"
        assert_close(H(dX), oracle.matmul_dx(w, H(q), F), 1e-5, f"pull_gemm exact={ex}", f64=lambda: o64.matmul_dx(w, H(q), F))
    # bwd_x and the dW step over the transposed side
    for ex in (False, True):
        dp = ops.matmul_dx(wd, dzd, F)
        dX = ops.kipf_layer_bwd_x(c.g, dzd, wd, F, exact=ex)
        if hub_cols:
            same(ops.kipf_propagate_bwd(c.g, dp, exact=ex), c.bwd(H(dp), ex), f"bwd_x exact={ex}: scatter of dZ.W")
            assert torch.equal(dX, ops.kipf_propagate_bwd(c.g, dp, exact=ex)), f"bwd_x exact={ex} is not bwd(matmul_dx)"
        ref = lambda o: o.kipf_propagate_bwd(o.matmul_dx(w, dz, F), c.ia, c.ja, exact=ex)
        assert_close(H(dX), ref(oracle), 1e-5, f"bwd_x exact={ex}", f64=lambda: ref(o64))
        dX2, dW = ops.kipf_layer_bwd(c.g, dzd, wd, xd, exact=ex)
        qc = ops.kipf_propagate_bwd(c.g, dzd, exact=True)
        qp = qc if ex else ops.kipf_propagate_bwd(c.g, dzd)
        same(qc, c.bwd(dz, True), "dW step: coefficient-weighted gather")
        same(qp, c.bwd(dz, ex), "dW step: gather for dX")
        if hub_cols:
            assert torch.equal(dW, ops.matmul_dw(xd, qc)), f"layer_bwd exact={ex}: dW is not matmul_dw(x, gather)"
            assert torch.equal(dX2, ops.matmul_dx(wd, qp, F)), f"layer_bwd exact={ex}: dX is not matmul_dx(gather)"
        assert_close(H(dW), oracle.matmul_dw(dz, oracle.kipf_propagate(x, c.ia, c.ja)), 1e-5, f"layer_bwd exact={ex}: dW",
                     f64=lambda: o64.matmul_dw(dz, o64.kipf_propagate(x, c.ia, c.ja)))
        assert_close(H(dX2), ref(oracle), 1e-5, f"layer_bwd exact={ex}: dX", f64=lambda: ref(o64))


def test_partial_buffer_is_reused_across_plans_and_widths(dev):
    """one stream, no synchronisation in between: a graph of 40 tasks at F = 256, one of 2 tasks at F = 3 (Fp = 4), the first
    again -- the partials live in one workspace slot that only grows, so a stale or mis-strided partial shows here"""
    from athena_amd import ops

    a, b = case("many_tasks"), case("one513")
    xa, ga = a.operands(256, seed=4)
    xb, gb = b.operands(3, seed=4)
    got = []
    for c, x, F in ((a, xa, 256), (b, xb, 3), (a, xa, 256), (b, xb, 3)):
        got.append((c, x, ops.kipf_propagate(c.g, T(x, dev), out=nan_out((c.n_rows, F), dev)),
                    ops.neighbour_sum(c.g, T(x, dev), out=nan_out((c.n_rows, F), dev))))
    for k, (c, x, y, s) in enumerate(got):
        same(y, c.fwd(x), f"call {k}: kipf_propagate")
        same(s, sr.neighbour_sum(x, c.ia, c.ja), f"call {k}: neighbour_sum")


def _edge_list_with_degrees(deg, rng):
    """pairs [2, E] (1-based, no self pair) of an undirected multigraph in which vertex v has deg[v] ends: shuffled stubs, paired"""
    stubs = rng.permutation(np.repeat(np.arange(deg.size), deg))
    assert stubs.size % 2 == 0
    a, b = stubs[0::2].copy(), stubs[1::2].copy()
    for i in np.nonzero(a == b)[0]:              # a self pair trades its second end with a pair that shares no vertex with it
        j = int(np.nonzero((a != a[i]) & (b != a[i]))[0][0])
        b[i], b[j] = b[j], b[i]
    assert (a != b).all() and np.array_equal(np.bincount(np.concatenate([a, b]), minlength=deg.size), deg)
    return np.asfortranarray(np.stack([a, b]).astype(np.int32) + 1)


def test_every_builder_gives_the_same_hub_rows(dev):
    """the host builder, the device builder, DeviceGraph.from_edges and a mini-batch child that contains the hubs: the plan arrays
    are not exported, so the outputs stand in for them -- the same bits from all four, the yardstick's"""
    from athena_amd import DeviceGraph, batching, graph_type, ops

    rng = np.random.default_rng(77)
    deg = hub_length_layout(N, rng)
    if deg.sum() % 2:
        deg[20 + int(np.argmax(deg[20:100] > 0))] += 1
    pairs = _edge_list_with_degrees(deg, rng)
    tail = np.asfortranarray(np.array([[N + 1, N + 2, N + 3], [N + 2, N + 3, N + 4]], np.int32))   # a second, tiny structure
    both = np.asfortranarray(np.concatenate([pairs, tail], axis=1))
    gt = graph_type()
    gt.set_num_vertices(N, 0)
    gt.generate_adjacency(pairs)
    ia, ja = gt.adj_ia, gt.adj_ja
    assert np.array_equal(np.diff(ia), deg) and set(HUB_LENGTHS) <= set(deg.tolist())
    F = 6
    x = rng.uniform(-1, 1, (N, F)).astype(np.float32)
    e = rng.uniform(-1, 1, (pairs.shape[1], 2)).astype(np.float32)
    want = {"fwd": sr.kipf_propagate(x, ia, ja), "bwd": sr.kipf_propagate_bwd(x, ia, ja), "bwd_exact": sr.kipf_propagate_bwd(x, ia, ja, exact=True),
            "duv": sr.duvenaud_propagate(x, e, ia, ja)}

    def outputs(g, xd, ed):
        return {"fwd": H(ops.kipf_propagate(g, xd)), "bwd": H(ops.kipf_propagate_bwd(g, xd)),
                "bwd_exact": H(ops.kipf_propagate_bwd(g, xd, exact=True)), "duv": H(ops.duvenaud_propagate(g, xd, ed))}

    graphs = {}
    old = os.environ.get("ATHENA_MP_GRAPH_BUILD")
    try:
        for mode in ("host", "device"):
            os.environ["ATHENA_MP_GRAPH_BUILD"] = mode
            graphs[mode] = DeviceGraph(ia, ja, n_edge_cols=pairs.shape[1])
    finally:
        if old is None:
            os.environ.pop("ATHENA_MP_GRAPH_BUILD", None)
        else:
            os.environ["ATHENA_MP_GRAPH_BUILD"] = old
    graphs["from_edges"], ia2, ja2 = DeviceGraph.from_edges(N, pairs, want_adjacency=True)
    assert np.array_equal(ia2, ia) and np.array_equal(ja2, ja)
    for name, g in graphs.items():
        got = outputs(g, T(x, dev), T(e, dev))
        for k in want:
            same(got[k], want[k], f"{name}: {k}")
    # a dataset of two structures (the hub graph, a path of four vertices); the batch [1, 0] holds the hub graph as its rows 4 ..
    ds_g = DeviceGraph.from_edges(N + 4, both)
    ds = batching.DeviceDataset(ds_g, np.array([0, N, N + 4], np.int32), np.array([0, pairs.shape[1], both.shape[1]], np.int64))
    batch = ds.select([1, 0])
    try:
        assert batch.vertex_offsets.tolist() == [0, 4, N + 4] and batch.handle.n_rows == N + 4
        xb = np.concatenate([np.ones((4, F), np.float32), x])
        eb = np.concatenate([np.ones((3, 2), np.float32), e])
        got = outputs(batch.handle, T(xb, dev), T(eb, dev))
        for k in want:
            same(np.ascontiguousarray(got[k][4:, :want[k].shape[1]]), want[k], f"batch child: {k}")
    finally:
        batch.close()
        ds.close()


ENTRIES = [   # (C entry, (inputs ...), outputs ...) by name; "x": [n_cols, F], "g": [n_rows, F], "xe": packed rows [n_rows, F + 2]
    ("athena_mp_kipf_propagate_fwd", ("x",), ("y",)),
    ("athena_mp_kipf_propagate_act_fwd", ("x",), ("y_relu",)),
    ("athena_mp_kipf_propagate_bwd", ("g",), ("d",)),
    ("athena_mp_kipf_propagate_bwd:exact", ("g",), ("d_exact",)),
    ("athena_mp_reverse_kipf_propagate_fwd", ("g",), ("d",)),
    ("athena_mp_reverse_kipf_propagate_partial", ("x",), ("y",)),
    ("athena_mp_reverse_kipf_propagate_partial_val", ("g",), ("d",)),
    ("athena_mp_kipf_propagate_fwd_dual", ("x",), ("s", "y")),
    ("athena_mp_kipf_propagate_bwd_dual", ("g",), ("d", "d_exact")),
    ("athena_mp_duvenaud_propagate_fwd", ("x", "e"), ("c",)),
    ("athena_mp_duvenaud_propagate_fwd:edges", ("e",), ("c_e",)),
    ("athena_mp_duvenaud_propagate_bwd_x", ("xe",), ("dx",)),
    ("athena_mp_duvenaud_propagate_bwd_e", ("xe",), ("de",)),
]


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("F", [6, 64])
def test_hub_rows_at_4_and_16_byte_aligned_operands_between_guards(dev, oracle, F, k):
    """every entry with its operands k elements past a 512-byte boundary, flush between sentinel guards (helpers.placed): the partial
    buffer is the library's own, the hub rows of the caller's output are written value by value by the combine kernel -- the
    yardstick's bits, and not a word outside the output"""
    from athena_amd import _capi

    c = case("both")
    x, gr = c.operands(F, seed=5)
    rng = np.random.default_rng(F + k)
    e = rng.uniform(-1, 1, (E_COLS, 2)).astype(np.float32)
    xe = np.ascontiguousarray(np.concatenate([gr, gr[:, :2]], axis=1))
    y = c.fwd(x)
    want = {"y": y, "y_relu": np.where(y > 0, y, np.float32(0)), "d": c.bwd(gr, False), "d_exact": c.bwd(gr, True),
            "s": sr.neighbour_sum(x, c.ia, c.ja), "c": sr.duvenaud_propagate(x, e, c.ia, c.ja), "c_e": sr.duvenaud_propagate(None, e, c.ia, c.ja),
            "dx": sr.duvenaud_propagate_bwd_x(xe, F, c.ia, c.ja), "de": oracle.duvenaud_propagate_bwd_e(xe, F, E_COLS, c.ia, c.ja)}
    ins = {"x": x, "g": gr, "e": e, "xe": xe}
    _capi.use_torch_stream()
    for entry, inputs, outputs in ENTRIES:
        cname = entry.split(":")[0]
        ti = [placed(ins[n], dev, k) for n in inputs]
        to = [placed_out(want[n].shape, torch.float32, dev, k) for n in outputs]
        pi, po = [C.c_void_p(t.data_ptr()) for t in ti], [C.c_void_p(t.data_ptr()) for t, _ in to]
        if cname.startswith("athena_mp_duvenaud_propagate_fwd"):
            args = (F, 2, pi[0], pi[1], po[0]) if entry == cname else (0, 2, None, pi[0], po[0])
        elif cname.startswith("athena_mp_duvenaud_propagate_bwd"):
            args = (F, 2, pi[0], po[0])
        elif cname == "athena_mp_kipf_propagate_act_fwd":
            args = (F, pi[0], 1, po[0])
        elif cname == "athena_mp_kipf_propagate_bwd":
            args = (F, pi[0], po[0], int(entry.endswith("exact")))
        else:
            args = (F, *pi, *po)
        _capi.call(cname, c.g.handle, *args)
        for n, (t, check) in zip(outputs, to):
            check(f"{entry}: {n}")
            same(t, want[n], f"{entry} at k={k}: {n}")
