"""Every site that evaluates an activation or a softmax, held element by element at the values where such functions go wrong:
saturation, the range where expf overflows or goes subnormal, the thresholds with the float on either side, both zeros, softmax
rows that are all equal, that are led by 10 .. 1e4, shifted by +-1e4, tied, with the maximum in every place.

The yardstick is tests/activation_reference.py: float64 forms and the bound of assert_each,
    |dev - f64| <= |oracle - f64| + 1e-5 scale max(1, |a|/32) + FLT_MIN max(1, |t|),
which the CPU oracle alone meets with room (tests/test_activation_reference.py).  Kinds with no transcendental are held to the
oracle's BITS, the sign of a zero included.

The epilogues inside the contraction and gather kernels are reached with PLANTED pre-activations: an identity weight, and a graph
whose every row has one entry of coefficient 1, make the pre-activation equal the planted operand bit for bit (a multiply by 1 and
adds of 0 are exact, on the matrix cores too).  Each such case first asserts that premise with act = "none"."""
import numpy as np
import pytest
import torch

import activation_reference as ar
from helpers import assert_close_elementwise, placed_out

pytestmark = pytest.mark.gpu

ONE_TRIP = 8192 * 256            # elements of one trip of the element-wise grid-stride loops (grid_for caps a launch at 8192 blocks)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def H(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and bool((a.view(np.int32) == b.view(np.int32)).all())


def upstream(n, seed=3):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


# ---- 2.1 the stand-alone entries on the grid -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "linear", "relu", "sigmoid", "tanh"])
def test_plain_kinds_on_the_grid(dev, oracle, kind):
    """act_f / act_b (elementwise.hip).  ops.activation is the yardstick of tests/test_gpu_hub_rows.py, so it is held here to more
    than those tests ask of the kernels they check with it"""
    from athena_amd import ops

    t = ar.edge_grid()
    g = upstream(t.size)
    y = H(ops.activation(kind, T(t, dev)))
    yo = oracle.activation(kind, t)
    if kind in ar.TRANSCENDENTAL:
        ar.assert_each(y, yo, *ar.forward(kind, t), t, f"activation {kind}")
        assert (y >= (0.0 if kind == "sigmoid" else -1.0)).all() and (y <= 1.0).all()
    else:
        assert same_bits(y, yo), f"activation {kind}: not the oracle's bits"
    d = H(ops.activation_bwd(kind, T(y, dev), T(g, dev)))
    assert same_bits(d, oracle.activation_bwd(kind, y, g)), f"activation_bwd {kind}: not the oracle's bits from the same y"


@pytest.mark.parametrize("name,attrs", ar.attributed_cases())
def test_attributed_kinds_on_the_grid(dev, oracle, name, attrs):
    """actp_f / actp_b (elementwise.hip) with the default and the non-default attributes, and with `scale`.  An actv_type without a
    non-default attribute collapses to the plain kind, whose reverse factor takes the output"""
    from athena_amd import ops

    t = ar.edge_grid()
    g = upstream(t.size)
    a = ops.actv_type(name, **attrs)
    kind = ops.resolve_activation(a)
    scale, p0, p1 = ar.resolve(name, attrs)
    assert ((a.scale if a.apply_scaling else 1.0), a.p[0], a.p[1]) == (scale, p0, p1)
    what = f"{name} {attrs}"
    exact = name not in ar.TRANSCENDENTAL
    y = H(ops.activation(kind, T(t, dev)))
    yo = oracle.activation_param(name, t, scale, p0, p1)
    if exact:
        assert same_bits(y, yo), f"{what}: not the oracle's bits"
    else:
        ar.assert_each(y, yo, *ar.forward(name, t, scale, p0, p1), t, what)
    d = H(ops.activation_bwd(kind, T(y, dev), T(g, dev), z=T(t, dev)))
    if isinstance(kind, str):
        assert kind in ops.ACT
        assert same_bits(d, oracle.activation_bwd(kind, y, g)), f"{what}: reverse from the output, not the oracle's bits"
        return
    do = oracle.activation_param_bwd(name, t, g, scale, p0, p1)
    if exact:
        assert same_bits(d, do), f"{what}: reverse, not the oracle's bits"
    else:
        ar.assert_each(d, do, *ar.reverse(name, t, g, scale, p0, p1), t, what + " reverse")


@pytest.mark.parametrize("beta", ar.SWISH_BETAS)
def test_swish_on_the_grid(dev, oracle, beta):
    """swish_fwd_kernel / swish_bwd_kernel.  The reverse factor is the reference's formula, NaN where (e + 1)^2 overflows: the NaN
    mask is the oracle's, and up to beta x = 44 the factor is finite and inside the bound"""
    from athena_amd import ops

    t = ar.edge_grid()
    g = ar.swish_upstream(t.size)
    y = H(ops.activation("swish", T(t, dev), beta=beta))
    ar.assert_each(y, oracle.swish(t, beta), *ar.forward("swish", t, beta=beta), t, f"swish beta {beta}")
    y2 = H(ops.activation(ops.actv_type("swish", beta=beta), T(t, dev)))
    assert same_bits(y, y2), "swish through actv_type"
    d = H(ops.activation_bwd("swish", T(y, dev), T(g, dev), z=T(t, dev), beta=beta))
    do = oracle.swish_bwd(t, g, beta)
    assert np.array_equal(np.isnan(d), np.isnan(do)), "swish reverse: NaN where the oracle has none, or none where it has one"
    fin = np.float32(beta) * t <= ar.SWISH_FINITE
    assert np.isfinite(d[fin]).all() and np.isnan(d[np.float32(beta) * t >= 45.0]).all()
    ar.assert_each(d[fin], do[fin], *(r[fin] for r in ar.reverse("swish", t, g, beta=beta)), t[fin], f"swish beta {beta} reverse")


# ---- 2.3 softmax rows ----------------------------------------------------------------------------------------------------------------
def hold_softmax(y, yo, z, what):
    """forward: inside the bound, no NaN, every value in [0, 1], each row summing to 1 within F 2^-23"""
    w = ar.assert_each(y, yo, *ar.softmax(z), z, what)
    assert not np.isnan(y).any() and (y >= 0.0).all() and (y <= 1.0).all(), what
    F = z.shape[1]
    assert (np.abs(y.astype(np.float64).sum(1) - 1.0) <= F * 2.0 ** -23).all(), f"{what}: a row does not sum to 1"
    return w


@pytest.mark.parametrize("F", ar.SOFTMAX_F)
def test_softmax_rows(dev, oracle, F):
    """softmax_fwd_kernel / softmax_bwd_kernel<4 | 16 | 64> (F <= 8, <= 48, above) on the rows of activation_reference.softmax_rows;
    N = 70, and 1 / 63 / 65 so that the last block is partial at every G.  Reverse: against float64 from the device's own y"""
    from athena_amd import ops

    rows = ar.softmax_rows(F)
    for N in (rows.shape[0], 1, 63, 65):
        z = np.ascontiguousarray(rows[:N])
        g = upstream(z.size, seed=F).reshape(z.shape)
        yd = ops.activation("softmax", T(z, dev))
        y = H(yd)
        hold_softmax(y, oracle.softmax_cols(z), z, f"softmax F = {F}, N = {N}")
        d = H(ops.activation_bwd("softmax", yd, T(g, dev)))
        ar.assert_each(d, oracle.softmax_cols_bwd(y, g), *ar.softmax_reverse(y, g), z, f"softmax reverse F = {F}, N = {N}")


# ---- 2.2 epilogue sites with planted pre-activations ---------------------------------------------------------------------------------
def hold_epilogue(route, run, t, oracle, ulp_premise=False):
    """run(act) -> the route's output where the planted pre-activations t [n, F] are.  Premise: with act = "none" it EQUALS t (or,
    ulp_premise, is within 1 ulp of it: relu and tanh are then held from the device's own "none" output, the sigmoid from t).
    Then relu holds the oracle's bits, sigmoid / tanh the per-element bound"""
    z0 = H(run("none"))
    arg = t
    if ulp_premise:
        assert (np.abs(z0.astype(np.float64) - t) <= np.spacing(np.abs(t)).astype(np.float64)).all(), f"{route}: premise, more than 1 ulp from the planted values"
        print(f"{route}: {int((z0 != t).sum())} of {t.size} pre-activations 1 ulp off the quotient")
        arg = z0
    else:
        assert np.array_equal(z0, t), f"{route}: premise, act = none does not return the planted values"
    assert np.array_equal(H(run("relu")), oracle.activation("relu", arg)), f"{route}: relu"
    worst = {}
    for act in ("sigmoid", "tanh"):
        x = arg if act == "tanh" else t
        worst[act] = ar.assert_each(H(run(act)), oracle.activation(act, x), *ar.forward(act, x), x, f"{route} {act}")
    return worst


def identity(F, Fi=None):
    """W(Fo, Fi) column-major with W[o, i] = (o == i)"""
    return np.eye(F, Fi or F, dtype=np.float32).flatten(order="F")


def rows_for(F, at_least=1):
    """rows of F values that hold the whole grid"""
    return max(at_least, -(-ar.edge_grid().size // F))


@pytest.mark.parametrize("K,M,route", [(32, 261, "weight-resident"), (64, 131, "weight-resident"), (128, 67, "weight-resident"),
                                       (24, 345, "tiled"), (5, 1653, "small"), (24, 100, "small")])
@pytest.mark.parametrize("with_bias", [False, True])
def test_matmul_epilogues(dev, oracle, K, M, route, with_bias):
    """ops.matmul(W = I) on the three routes of gemm_dispatch: K = N in {32, 64, 128} is weight-resident (launch_bres, gemm.hip:
    the run-time switch and the constexpr form), 24 x 24 with M >= 128 is gemm_tiled.hip, 5 x 5 and M = 100 < 128 take
    gemm_small_kernel.  With a bias the planted value is fl32(p + b)"""
    from athena_amd import ops

    t = ar.planted((M, K))
    bias = None
    P = t
    if with_bias:
        bias = np.resize(np.asarray([0.0, 0.5, -0.25, 2.0 ** -20], np.float32), K)
        P = (t - bias[None, :]).astype(np.float32)
        t = (P + bias[None, :]).astype(np.float32)
        assert np.array_equal(t[:, bias == 0], ar.planted((M, K))[:, bias == 0]) and (np.abs(t - ar.planted((M, K))) <= np.spacing(np.maximum(np.abs(t), np.float32(0.5)))).all()
    W, Pd, bd = T(identity(K), dev), T(P, dev), (T(bias, dev) if with_bias else None)
    hold_epilogue(f"matmul {route} {K}x{K}, M = {M}{', bias' if with_bias else ''}", lambda act: ops.matmul(W, Pd, K, bias=bd, act=act), t, oracle)


def one_entry_graph(n, kind, seed=0):
    """(ia, ja, source): every row has ONE entry, so every degree is 1 and every coefficient 1.  "self": row v lists v (band 0);
    "perm": row v lists a random permutation's perm[v], with perm[0] = n - 1 so that the band is wider than any banded kernel takes"""
    if kind == "self":
        src = np.arange(n)
    else:
        src = np.random.default_rng(seed + n).permutation(n)
        k = int(np.nonzero(src == n - 1)[0][0])
        src[k], src[0] = src[0], n - 1
        assert n > 130 and sorted(src.tolist()) == list(range(n))
    ia = np.arange(1, n + 2, dtype=np.int32)
    ja = np.zeros((2, n), np.int32, order="F")
    ja[0] = src + 1
    return ia, ja, src


@pytest.mark.parametrize("F", [5, 64, 128])
@pytest.mark.parametrize("graph", ["self", "perm"])
def test_kipf_propagate_act_epilogue(dev, oracle, graph, F):
    """ops.kipf_propagate_act: the activation in the store of the lane-group gather (agg.hip, gather_agg -> launch_v; vec = 1 at
    F = 5, 4 at 64 / 128)"""
    from athena_amd import DeviceGraph, ops

    n = rows_for(F, 131)
    ia, ja, src = one_entry_graph(n, graph)
    x = ar.planted((n, F))
    g = DeviceGraph(ia, ja, n_edge_cols=0)
    xd = T(x, dev)
    hold_epilogue(f"kipf_propagate_act {graph} F = {F}", lambda act: ops.kipf_propagate_act(g, xd, act=act), x[src], oracle)


@pytest.mark.parametrize("F", [64, 128, 256])
@pytest.mark.parametrize("graph", ["self", "perm"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_kipf_layer_fwd_epilogue(dev, oracle, graph, F, with_bias):
    """ops.kipf_layer_fwd(W = I).  athena_mp_kipf_layer_fwd selects, for these operands (no hub rows, 16-byte aligned):
      perm graph (band > 64, so not banded): the one-launch kernels of fused.hip -- launch_fused<64>, launch_fused<128>, and
          fused256_dispatch at 256
      self-loop graph (band 0, one entry per row, so banded at 64 and 128): 64 -> 64 is banded_agg_gemm64 (banded_fused.hip);
          128 is csr_gather_banded64 (agg.hip) followed by the weight-resident launch_bres<128, 128> (gemm.hip); 256 is not a banded
          width and takes fused256_dispatch
    P is the gathered x, bit for bit, on every one of them"""
    from athena_amd import DeviceGraph, ops

    n = 300
    ia, ja, src = one_entry_graph(n, graph)
    t = ar.planted((n, F))
    bias = None
    P = t
    if with_bias:
        bias = np.resize(np.asarray([0.0, 0.5, -0.25, 2.0 ** -20], np.float32), F)
        P = (t - bias[None, :]).astype(np.float32)
        t = (P + bias[None, :]).astype(np.float32)
    x = np.empty_like(P)
    x[src] = P                                        # row v gathers x[src[v]] = P[v]
    g = DeviceGraph(ia, ja, n_edge_cols=0)
    W, xd, bd = T(identity(F), dev), T(x, dev), (T(bias, dev) if with_bias else None)

    def run(act):
        Pd, Z = ops.kipf_layer_fwd(g, xd, W, F, bias=bd, act=act)
        assert np.array_equal(H(Pd), P), "P is not the gathered x"
        _, Z2 = ops.kipf_layer_fwd(g, xd, W, F, bias=bd, act=act, keep_P=False)
        assert torch.equal(Z, Z2), "keep_P = False changes Z"
        return Z

    hold_epilogue(f"kipf_layer_fwd {graph} F = {F}{', bias' if with_bias else ''}", run, t, oracle)


def degree_graph(n, seed=0):
    """(ia, ja, d): row v has d[v] = 1 + v % 4 entries (random columns): buckets 1 .. 4 of the Duvenaud update"""
    d = 1 + np.arange(n) % 4
    ia = np.concatenate([[1], 1 + np.cumsum(d)]).astype(np.int32)
    ja = np.zeros((2, int(d.sum())), np.int32, order="F")
    ja[0] = np.random.default_rng(seed + n).integers(1, n + 1, ja.shape[1])
    return ia, ja, d.astype(np.float32)


DUV_SHAPES = [(7, 7, 300, "VALU kernels + athena_mp_activation_fwd"), (64, 64, 1100, "duv_mfma.hip"), (32, 32, 1100, "duv_mfma.hip")]


@pytest.mark.parametrize("Fi,Fo,n,route", DUV_SHAPES)
def test_duvenaud_update_act_epilogue(dev, oracle, Fi, Fo, n, route):
    """ops.duvenaud_update_act with W_d = I for every bucket and planted a = d t (exact: the grid's low three mantissa bits are
    clear).  (7, 7, 300) is below duv_use_mfma (Fi, Fo >= 16, n >= 1024): duv_update_fwd_kernel, then athena_mp_activation_fwd.
    (64, 64, 1100) and (32, 32, 1100) take duv_mfma.hip, whose sigmoid is the hardware exp2 / rcp with the bucket divisor folded
    into the constant, and whose div_by may be 1 ulp off the quotient: the "none" premise is <= 1 ulp there and nothing else"""
    from athena_amd import DeviceGraph, ops

    ia, ja, d = degree_graph(n)
    t = ar.planted((n, Fi), exact_div=True)
    a = (d[:, None] * t).astype(np.float32)
    assert np.array_equal(a.astype(np.float64), d[:, None].astype(np.float64) * t) and np.array_equal(a / d[:, None], t)
    g = DeviceGraph(ia, ja, n_edge_cols=0)
    W, ad = T(np.tile(identity(Fo, Fi), 4), dev), T(a, dev)
    mfma = Fi >= 16 and Fo >= 16 and n >= 1024
    hold_epilogue(f"duvenaud_update_act ({Fi}, {Fo}, {n}) {route}", lambda act: ops.duvenaud_update_act(g, ad, W, 1, 4, Fo, act=act), t, oracle,
                  ulp_premise=mfma)
    if not mfma:
        assert np.array_equal(H(ops.duvenaud_update(g, ad, W, 1, 4, Fo)), t)


READOUT_O = (1, 3, 4, 5, 10, 16)


def logit_rows(n, O, exact_div=False):
    """the softmax rows of activation_reference.softmax_rows(O), repeated over n vertices"""
    z = np.resize(ar.softmax_rows(O), (n, O)).astype(np.float32)
    return ar.clear_low_bits(z) if exact_div else z


def ragged_segments(n, seed=0):
    """0-based vertex offsets of graphs of 0 .. 40 vertices that add up to n, the first and some others empty"""
    rng = np.random.default_rng(seed + n)
    sizes = [0]
    while sum(sizes) < n:
        sizes.append(int(min(rng.integers(0, 41), n - sum(sizes))))
    sizes.append(0)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def hold_readout(p, out, logits, seg, oracle, what):
    """p per vertex inside the bound of the softmax of `logits` (fp32, as the device formed them); the per-graph sums of the
    device's own p element-wise within 1e-5 of the sum of their terms"""
    p = H(p)
    w = hold_softmax(p, oracle.softmax_cols(logits), logits, what)
    if out is not None:
        sums = np.stack([p[seg[s]:seg[s + 1]].astype(np.float64).sum(0) for s in range(seg.size - 1)])
        assert_close_elementwise(H(out), sums, sums, 1e-5, what + ": per-graph sums")
    return w


@pytest.mark.parametrize("O", READOUT_O)
@pytest.mark.parametrize("Fv,n", [(64, 1100), (16, 333), (24, 333)])
def test_duvenaud_readout_softmax(dev, oracle, Fv, n, O):
    """ops.duvenaud_readout with R[o, f] = (o == f): the logits are the first O features of z.  Fv = 64 and 16 take
    readout_fwd_kernel<J> (readout.hip, libm expf); Fv = 24 takes the composed chain (gemm + softmax_rows_kernel)"""
    from athena_amd import ops

    logits = logit_rows(n, O)
    z = np.zeros((n, Fv), np.float32)
    z[:, :O] = logits
    z[:, O:] = upstream(n * (Fv - O), seed=O).reshape(n, Fv - O)
    seg = ragged_segments(n)
    p, out = ops.duvenaud_readout(T(identity(O, Fv), dev), T(z, dev), T(seg, dev), O)
    hold_readout(p, out, logits, seg, oracle, f"duvenaud_readout Fv = {Fv}, O = {O}")


@pytest.mark.parametrize("O", READOUT_O + (65,))
def test_softmax_segsum_rows(dev, oracle, O):
    """ops.softmax_segsum: softmax_rows_kernel (duvenaud.hip), one thread per vertex"""
    from athena_amd import ops

    n = 333
    logits = logit_rows(n, O)
    seg = ragged_segments(n)
    p, out = ops.softmax_segsum(T(logits, dev), T(seg, dev))
    hold_readout(p, out, logits, seg, oracle, f"softmax_segsum O = {O}")


@pytest.mark.parametrize("act", ["none", "sigmoid"])
@pytest.mark.parametrize("Fo,n,O", [(64, 1100, O) for O in READOUT_O] + [(7, 300, O) for O in READOUT_O if O <= 7])
def test_duvenaud_update_readout_softmax(dev, oracle, Fo, n, O, act):
    """ops.duvenaud_update_act_readout with W_d = I, R[o, f] = (o == f) and planted a = d z, whose first O features are the softmax
    rows.  (64, 64, 1100) is duv_mfma_fwd_readout (duv_mfma.hip: the fused softmax on the hardware exp2 / rcp); (7, 7, 300) is the
    VALU update, the activation launch and the readout's composed chain.  z is the one of duvenaud_update_act, bit for bit; p is
    held against the softmax of the device's OWN z, so the 1 ulp of div_by is not charged to the softmax"""
    from athena_amd import DeviceGraph, ops

    ia, ja, d = degree_graph(n)
    t = np.zeros((n, Fo), np.float32)
    t[:, :O] = logit_rows(n, O, exact_div=True)
    t[:, O:] = ar.clear_low_bits(upstream(n * (Fo - O), seed=O).reshape(n, Fo - O))
    a = (d[:, None] * t).astype(np.float32)
    assert np.array_equal(a / d[:, None], t)
    g = DeviceGraph(ia, ja, n_edge_cols=0)
    W, R, ad = T(np.tile(identity(Fo), 4), dev), T(identity(O, Fo), dev), T(a, dev)
    z, p = ops.duvenaud_update_act_readout(g, ad, W, 1, 4, Fo, R, O, act=act)
    assert torch.equal(z, ops.duvenaud_update_act(g, ad, W, 1, 4, Fo, act=act)), "z differs from duvenaud_update_act"
    logits = np.ascontiguousarray(H(z)[:, :O])
    if act == "none":
        assert (np.abs(logits.astype(np.float64) - t[:, :O]) <= np.spacing(np.abs(t[:, :O])).astype(np.float64)).all(), "premise: z is not the planted rows"
    hold_readout(p, None, logits, None, oracle, f"duvenaud_update_act_readout ({Fo}, {Fo}, {n}) {act}, O = {O}")


@pytest.mark.parametrize("O", READOUT_O)
@pytest.mark.parametrize("Fe", [16, 5])
def test_duvenaud_update_readout_split_softmax(dev, oracle, Fe, O):
    """ops.duvenaud_update_act_readout_split at Fv = Fo = 64, W_d = [I | 0]: Fe = 16 is the split form of duv_mfma_fwd_readout in one
    launch; Fe = 5 packs a and takes whichever route the packed call takes"""
    from athena_amd import DeviceGraph, ops

    n, Fv = 1100, 64
    ia, ja, d = degree_graph(n)
    t = np.zeros((n, Fv), np.float32)
    t[:, :O] = logit_rows(n, O, exact_div=True)
    t[:, O:] = ar.clear_low_bits(upstream(n * (Fv - O), seed=O).reshape(n, Fv - O))
    a_x = (d[:, None] * t).astype(np.float32)
    a_e = upstream(n * Fe, seed=Fe).reshape(n, Fe)
    g = DeviceGraph(ia, ja, n_edge_cols=0)
    W = T(np.tile(identity(Fv, Fv + Fe), 4), dev)
    z, p = ops.duvenaud_update_act_readout_split(g, T(a_x, dev), T(a_e, dev), W, 1, 4, Fv, T(identity(O, Fv), dev), O, act="none")
    logits = np.ascontiguousarray(H(z)[:, :O])
    assert (np.abs(H(z).astype(np.float64) - t) <= np.spacing(np.abs(t)).astype(np.float64)).all(), "premise: z is not the planted rows"
    hold_readout(p, None, logits, None, oracle, f"duvenaud_update_act_readout_split Fe = {Fe}, O = {O}")


# ---- 2.4 past the first trip of the grid-stride loops, every element compared -------------------------------------------------------
BIG = ONE_TRIP + 257


def test_relu_past_the_first_trip(dev, oracle):
    from athena_amd import ops

    t = np.resize(ar.edge_grid(), BIG)
    t[-300:] = upstream(300, seed=9)                  # the second trip's elements are their own
    g = upstream(BIG)
    y = H(ops.activation("relu", T(t, dev)))
    assert same_bits(y, oracle.activation("relu", t))
    assert same_bits(H(ops.activation_bwd("relu", T(y, dev), T(g, dev))), oracle.activation_bwd("relu", y, g))


def test_swish_past_the_first_trip(dev, oracle):
    from athena_amd import ops

    t = np.resize(ar.edge_grid(), BIG)
    t[-300:] = upstream(300, seed=9) * 4
    y = H(ops.activation("swish", T(t, dev), beta=1.0))
    ar.assert_each(y, oracle.swish(t, 1.0), *ar.forward("swish", t), t, "swish past the first trip")


@pytest.mark.parametrize("N,F", [(524291, 8), (131075, 48), (32771, 49)])
def test_softmax_past_the_first_trip(dev, oracle, N, F):
    """one case per G = 4 / 16 / 64: the rows past 8192 (256 / G) are the second trip of softmax_fwd_kernel / softmax_bwd_kernel"""
    from athena_amd import ops

    G = 4 if F <= 8 else (16 if F <= 48 else 64)
    assert N > 8192 * (256 // G) and N * F * 4 <= 26e6
    z = np.resize(ar.softmax_rows(F), (N, F)).astype(np.float32)
    z[::2] = (np.random.default_rng(F).standard_normal((z[::2].shape)) * 3).astype(np.float32)
    g = upstream(N * F, seed=F).reshape(N, F)
    yd = ops.activation("softmax", T(z, dev))
    y = H(yd)
    hold_softmax(y, oracle.softmax_cols(z), z, f"softmax ({N}, {F})")
    d = H(ops.activation_bwd("softmax", yd, T(g, dev)))
    ar.assert_each(d, oracle.softmax_cols_bwd(y, g), *ar.softmax_reverse(y, g), z, f"softmax reverse ({N}, {F})")


@pytest.mark.parametrize("n", [1, 1000, BIG])
@pytest.mark.parametrize("alpha", [1.0, -0.3, 1e-3])
def test_axpy_is_a_rounded_multiply_then_a_rounded_add(dev, n, alpha):
    from athena_amd import ops

    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    want = y + np.float32(alpha) * x
    assert want.dtype == np.float32
    out, check = placed_out((n,), torch.float32, dev, 0, init=y)
    r = ops.axpy(alpha, T(x, dev), out)
    assert r is out and same_bits(H(out), want)
    check("axpy")


@pytest.mark.parametrize("n,F", [(1000, 1), (333, 3), (BIG // 130 + 1, 130)])
def test_add_row_bias(dev, n, F):
    from athena_amd import ops

    rng = np.random.default_rng(F)
    y, b = rng.standard_normal((n, F)).astype(np.float32), rng.standard_normal(F).astype(np.float32)
    out, check = placed_out((n, F), torch.float32, dev, 0, init=y)
    r = ops.add_row_bias(T(b, dev), out)
    assert r is out and same_bits(H(out), y + b[None, :])
    check("add_row_bias")


@pytest.mark.parametrize("N,Fa,Fb", [(1000, 1, 1), (333, 3, 14), (BIG // 131 + 1, 130, 1)])
def test_concat_features_and_its_reverse(dev, oracle, N, Fa, Fb):
    """concat_fwd_kernel / concat_bwd_kernel; the reverse with either output absent, between guards"""
    from athena_amd import _capi, ops
    import ctypes as C

    rng = np.random.default_rng(Fa + Fb)
    a, b = rng.standard_normal((N, Fa)).astype(np.float32), rng.standard_normal((N, Fb)).astype(np.float32)
    out = H(ops.concat_features(T(a, dev), T(b, dev)))
    assert same_bits(out, np.concatenate([a, b], axis=1)) and same_bits(out, oracle.concat(a, b))
    gr = rng.standard_normal((N, Fa + Fb)).astype(np.float32)
    grd = T(gr, dev)
    da, db = ops.concat_features_bwd(grd, Fa)
    assert same_bits(H(da), gr[:, :Fa]) and same_bits(H(db), gr[:, Fa:])
    da, none = ops.concat_features_bwd(grd, Fa, need_b=False)
    assert none is None and same_bits(H(da), gr[:, :Fa])
    none, db = ops.concat_features_bwd(grd, Fa, need_a=False)
    assert none is None and same_bits(H(db), gr[:, Fa:])
    # the same through the C entry into outputs between guards: nothing outside them is written, with either output absent
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    for need_a, need_b in ((True, True), (True, False), (False, True)):
        oa, ca = placed_out((N, Fa), torch.float32, dev, 1) if need_a else (None, None)
        ob, cb = placed_out((N, Fb), torch.float32, dev, 1) if need_b else (None, None)
        _capi.use_torch_stream()
        _capi.call("athena_mp_concat_bwd", N, Fa, Fb, p(grd), p(oa), p(ob))
        if need_a:
            ca("concat_bwd da")
            assert same_bits(H(oa), gr[:, :Fa])
        if need_b:
            cb("concat_bwd db")
            assert same_bits(H(ob), gr[:, Fa:])
    oc, cc = placed_out((N, Fa + Fb), torch.float32, dev, 1)
    ad, bd = T(a, dev), T(b, dev)
    _capi.use_torch_stream()
    _capi.call("athena_mp_concat_fwd", N, Fa, Fb, p(ad), p(bd), p(oc))
    cc("concat_fwd")
    assert same_bits(H(oc), out)
