"""GPU: the persistent kernels past their first chunk, whole tensors, zero tolerance.

The one-launch Kipf kernels (fused.hip, fused_dw.hip) and the weight-resident GEMMs (gemm.hip) are persistent workgroups that walk
many chunks of rows through two alternating LDS buffers with the next chunk's loads in flight.  The small shapes of the other
files end in the first trip of that loop, and the full-size tests sample 2 % of the rows.  Here every size is derived from the
number of compute units C of the device the test runs on, so that the trips a case claims are made -- each test asserts its
chunk / slab arithmetic -- and every result is compared with np.array_equal over the WHOLE tensor against
tests/exact_reference.py: operands for which every partial sum in every order is exact in fp32 (its conditions are asserted
when the reference is built, and evaluated for these cases on the CPU by tests/test_exact_reference.py).

A HIP error in any call ends the file (pytest.exit): nothing more runs on a device in that state, nothing is retried."""
import numpy as np
import pytest

import exact_reference as er

pytestmark = pytest.mark.gpu


def T(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(what, fn):
    """fn() and a synchronisation; a HIP error (a fault, a failed launch) is not a wrong result: the file ends there"""
    import torch

    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except RuntimeError as ex:
        if "hip" in str(ex).lower():
            pytest.exit(f"{what}: {ex}", returncode=3)
        raise


def same(got, ref, what, chunk_rows=None):
    """np.array_equal over the whole tensor; on a difference, where it lies (rows, and the chunks / slabs they belong to)"""
    got = run(what, lambda: got.cpu().numpy())
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if np.array_equal(got, ref):
        return
    bad = got != ref
    msg = f"{what}: {int(bad.sum())} of {bad.size} elements differ from the exact reference"
    if ref.ndim == 2:
        rows = np.nonzero(bad.any(axis=1))[0]
        msg += f", in {rows.size} rows (first {rows[:6].tolist()}, last {rows[-3:].tolist()})"
        if chunk_rows:
            ch = np.unique(rows // chunk_rows)
            msg += f", {ch.size} chunk(s) of {chunk_rows} rows (first {ch[:6].tolist()}, last {ch[-3:].tolist()})"
    where = np.argwhere(bad)[0]
    msg += f"; first at {where.tolist()}: got {got[tuple(where)]!r}, expected {ref[tuple(where)]!r}"
    raise AssertionError(msg)


@pytest.fixture(scope="module")
def C(dev):
    import torch

    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def _handle(r, g_bits):
    """the device graph of a reference, with its coefficients re-checked word by word: powers of two, none below 2^-g"""
    from athena_amd import DeviceGraph

    g = DeviceGraph(r.ia, r.ja, n_edge_cols=0)
    for name in ("coef", "t_coef"):
        c = g.export(name)
        assert c.size == r.ja.shape[1]
        er.assert_power_of_two_words(c, g_bits)
    return g


def _device_operands(r, dev):
    ts = {k: T(getattr(r, k), dev) for k in ("x", "W", "bias", "dZ")}
    assert all(t.data_ptr() % 16 == 0 for t in ts.values())        # the one-launch routes want 16-byte aligned operands
    return ts


# =====================================================================================================================================
# agg_gemm_kernel<64|128>, agg_gemm256_kernel: three tickets per workgroup in the prologue; the redraw inside the loop returns a
# live chunk only with more than 3 C chunks
# =====================================================================================================================================
@pytest.fixture(scope="module", params=er.FUSED_WIDTHS, ids=lambda F: f"F{F}")
def fused(request, dev, C):
    F = request.param
    r = er.fused_case(C, F)
    rows = er.FUSED_CHUNK_ROWS[F]
    chunks = er.ceil_div(r.n, rows)
    assert chunks > 3 * C and r.n % rows != 0, (r.n, rows, chunks, C)        # steady-state redraws; a ragged tail chunk
    assert r.g == 8 and 256 in set(np.diff(r.ia).tolist())
    case = {"r": r, "F": F, "g": _handle(r, 8), "rows": rows, **_device_operands(r, dev)}
    print(f"fused {F}: n = {r.n}, {chunks} chunks of {rows} rows on {C} compute units: {chunks / min(chunks, C):.1f} per workgroup")
    yield case
    case.clear()


@pytest.mark.parametrize("act", ["none", "relu"])
def test_fused_forward_whole_tensors(fused, act):
    """ops.kipf_layer_fwd with bias: P and Z, Z again without a stored P, and the two-kernel route on the same operands"""
    from athena_amd import ops

    c, r, F, g = fused, fused["r"], fused["F"], fused["g"]
    tag = f"fused forward {F}, {act}"
    P, Z = run(tag, lambda: ops.kipf_layer_fwd(g, c["x"], c["W"], F, bias=c["bias"], act=act))
    same(P, r.P, tag + ": P", c["rows"])
    same(Z, r.Z(act), tag + ": Z", c["rows"])
    none, Z2 = run(tag, lambda: ops.kipf_layer_fwd(g, c["x"], c["W"], F, bias=c["bias"], act=act, keep_P=False))
    assert none is None
    same(Z2, r.Z(act), tag + ": Z without a stored P", c["rows"])
    P3 = run(tag, lambda: ops.kipf_propagate(g, c["x"]))
    Z3 = run(tag, lambda: ops.matmul(c["W"], P3, F, bias=c["bias"], act=act))
    same(P3, r.P, tag + ": P of kipf_propagate")
    same(Z3, r.Z(act), tag + ": Z of kipf_propagate + matmul", er.SLAB_ROWS)
    print(tag, "bits", {k: round(v, 1) for k, v in r.bits.items()})


@pytest.mark.parametrize("exact", [False, True])
def test_fused_reverse_whole_tensor(fused, exact):
    """ops.kipf_layer_bwd_x over the transposed structure of the same graph: n columns in the same chunks"""
    from athena_amd import ops

    c, r, F, g = fused, fused["r"], fused["F"], fused["g"]
    tag = f"fused reverse {F}, exact = {int(exact)}"
    dX = run(tag, lambda: ops.kipf_layer_bwd_x(g, c["dZ"], c["W"], F, exact=exact))
    same(dX, r.dX(exact), tag + ": dX", c["rows"])
    print(tag, "bits", {k: round(v, 1) for k, v in r.bits.items()})


# =====================================================================================================================================
# agg_gemm_dw_kernel, 128 -> 128: min(ceil(n / 32), C) workgroups, workgroup b takes the chunks b, b + grid, ...
# =====================================================================================================================================
DW_CASES = ["one_chunk_each", "second_trip_of_one_row", "second_trip_of_one_live_row", "third_trip_ragged", "many_trips"]


@pytest.fixture(scope="module", params=range(len(DW_CASES)), ids=DW_CASES)
def folded(request, dev, C):
    which = DW_CASES[request.param]
    n, live_tail = er.dw_cases(C)[request.param]
    grid, chunks, most, how_many = er.dw_trips(n, C)
    k = er.DW_CHUNK_ROWS
    if which == "one_chunk_each":
        assert (grid, chunks, most) == (C, C, 1) and n % k == 0
    elif which.startswith("second_trip_of_one"):
        assert (grid, chunks, most, how_many) == (C, C + 1, 2, 1) and n % k == 1           # a second trip over a one-row chunk
    elif which == "third_trip_ragged":
        assert (grid, most, how_many) == (C, 3, 4) and n % k not in (0, 1)                 # the buffers alternate back
    else:
        assert grid == C and most >= 7 and n % k not in (0, 1)
    r = er.dw_case(n, live_tail)
    assert r.g == 6 and int(np.diff(r.ia)[-1]) == (16 if live_tail else 0)
    case = {"r": r, "g": _handle(r, 6), "which": which, **_device_operands(r, dev)}
    print(f"folded dW, {which}: n = {n}, {chunks} chunks on {grid} workgroups: at most {most} trips, made by {how_many} workgroup(s)")
    yield case
    case.clear()


@pytest.mark.parametrize("exact", [False, True])
def test_reverse_with_the_folded_weight_gradient_whole_tensors(folded, exact):
    """ops.kipf_layer_bwd: dX and dW, and the same dW without the input gradient"""
    from athena_amd import ops

    c, r, g = folded, folded["r"], folded["g"]
    tag = f"folded dW, {c['which']}, n = {r.n}, exact = {int(exact)}"
    dX, dW = run(tag, lambda: ops.kipf_layer_bwd(g, c["dZ"], c["W"], c["x"], exact=exact))
    same(dX, r.dX(exact), tag + ": dX", er.DW_CHUNK_ROWS)
    same(dW, r.dW, tag + ": dW")
    none, dW2 = run(tag, lambda: ops.kipf_layer_bwd(g, c["dZ"], c["W"], c["x"], exact=exact, need_dx=False))
    assert none is None
    same(dW2, r.dW, tag + ": dW without dX")
    print(tag, "bits", {k: round(v, 1) for k, v in r.bits.items()})


# =====================================================================================================================================
# gemm_bres_kernel (four waves; a side of 32) and gemm_bres8_kernel (eight waves; both sides at least 64): wave w of workgroup b takes
# the 32-row slabs b W + w, + grid W, ...
# =====================================================================================================================================
GEMM_CASES = [(4, K, N) for K, N in er.GEMM_SHAPES] + [(8, K, N) for K, N in er.GEMM_SHAPES if er.gemm_waves(K, N) == 8]


@pytest.mark.parametrize("form,K,N", GEMM_CASES)
def test_weight_resident_gemms_whole_tensors(dev, C, form, K, N):
    """ops.matmul (bias + relu, bias, neither), ops.matmul_dx and ops.matmul_dw at M = 64 form C + 229: the third trip of the first
    eight waves of the `form`-wave kernel (the second trip where the shape takes the eight-wave kernel at the four-wave size)"""
    from athena_amd import ops

    M = 2 * er.SLAB_ROWS * form * C + 229
    assert (M, K, N) in er.gemm_cases(C)
    waves = er.gemm_waves(K, N)
    grid, slabs, most, how_many = er.gemm_trips(M, K, N, C)
    assert grid == C and slabs > 2 * form * C and M % er.SLAB_ROWS != 0               # more than two slabs per wave; a ragged last slab
    assert (most, how_many) == ((3, 8) if waves == form else (2, 8)), (most, how_many)
    r = er.gemm_case(M, K, N)
    P, W, b, dZ = (T(t, dev) for t in (r.Pm, r.W, r.bias, r.dZ))
    tag = f"gemm {M} x {K} -> {N}"
    print(f"{tag}: {slabs} slabs on {grid} workgroups of {waves} waves: at most {most} trips, made by {how_many} wave(s); bits",
          {k: round(v, 1) for k, v in r.bits.items()})
    same(run(tag, lambda: ops.matmul(W, P, N, bias=b, act="relu")), r.Z("relu"), tag + ": Z, bias + relu", er.SLAB_ROWS)
    same(run(tag, lambda: ops.matmul(W, P, N, bias=b)), r.Z("none"), tag + ": Z, bias", er.SLAB_ROWS)
    same(run(tag, lambda: ops.matmul(W, P, N)), r.Z("none", bias=False), tag + ": Z", er.SLAB_ROWS)
    same(run(tag, lambda: ops.matmul_dx(W, dZ, K)), r.dP, tag + ": dP", er.SLAB_ROWS)
    same(run(tag, lambda: ops.matmul_dw(P, dZ)), r.dW, tag + ": dW")


def test_blocked_weight_gradient_whole_tensor(dev, C):
    """ops.matmul_dw at 256 x 256: 128 x 128 blocks of dW on the register-resident kernel, every block over nx row ranges of four
    waves with rpw rows each"""
    from athena_amd import ops

    M = er.blocked_dw_rows(C)
    nx, rpw = er.blocked_dw_ranges(M, C)
    assert M >= 4096 and nx >= 8 and nx % 8 == 0 and rpw >= 64 and M % (4 * rpw) != 0, (M, nx, rpw)
    r = er.gemm_case(M, 256, 256)
    tag = f"blocked dW {M} x 256 x 256"
    print(f"{tag}: {nx} row ranges of 4 x {rpw} rows; bits", {k: round(v, 1) for k, v in r.bits.items()})
    same(run(tag, lambda: ops.matmul_dw(T(r.Pm, dev), T(r.dZ, dev))), r.dW, tag)
