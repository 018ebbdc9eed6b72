"""GPU: every device entry of the C ABI with its operands at 4-, 8- and 16-byte aligned addresses, between guards.

The contract (include/athena_mp.h): a `float *` / `int32_t *` device argument needs only the alignment of its element type; the
fast routes are taken when the operands are 16-byte aligned, every other call takes the entry's generic route.  A fresh torch
tensor is 256-byte aligned and its allocation rounded up to 512 bytes, so no other test hands the library a pointer that is not
16-byte aligned, and none sees a store past the end of an output.  Here every operand sits k elements past a 512-byte boundary
(helpers.placed / placed_out; k = 1: 4-byte aligned, k = 2: 8-byte, k = 4: 16-byte but off every larger boundary) with sentinel
words on both sides, and each entry runs with
  * every operand at k = 1, every operand at k = 2, every operand at k = 4,
  * each operand in turn at k = 1 and the others at k = 4 (what tells a predicate that looks at dZ and W apart from one that
    forgets X).
The placement list is generated from the entry's argument list.  Each case asserts
  * the result against the reference and tolerance of the entry's aligned test (test_gpu_ops.py, test_gpu_network.py,
    test_gpu_train.py, test_gpu_radius_graph.py, test_gpu_periodic_graph.py): np.array_equal with the fp32 oracle where that test
    is bit-exact, helpers.assert_close at 1e-5 anchored on the oracle's float64 twin elsewhere, 2e-6 / 1e-6 for the expf / tanhf
    element-wise kinds.  Nothing is compared with the library's own aligned result;
  * no guard word of any output was written, and no element of an output was left unwritten (outputs start out as sentinels);
  * every input holds the same bits after the call;
  * for the two documented refusals (athena_mp_device_copy, athena_mp_gno_aggregate_fwd_save): the call raises with "aligned" in
    the message, the outputs still hold the sentinel, and the same call with aligned operands then works.
The entries are called through _capi.call, the C ABI the ops wrappers call after their shape checks: half of the wrappers
allocate their outputs themselves, and an output is an operand here.  One oracle evaluation per shape, shared by its placements."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_close, csr_from_index_list, placed, placed_out, random_graph, rel_err, unwritten

pytestmark = pytest.mark.gpu

KS = (1, 2, 4)
G = object()          # the graph handle of the case


class Arg:
    def __init__(self, kind, name, key=None):
        self.kind, self.name, self.key = kind, name, key or name


def I(name, key=None):
    """a device input: operand `name` (what the placement is keyed by), data c[key]"""
    return Arg("in", name, key)


def O(name):
    """a device output: shape, dtype and expected values from the entry's references"""
    return Arg("out", name)


def IO(name, key=None):
    """an in-place operand: starts as c[key], expected values from the entry's references"""
    return Arg("inout", name, key)


class Ref:
    """expected values of one output: mode 'exact' (np.array_equal; rows under `loose` -- hub rows, summed in segments on every
    route -- at 1e-5 instead), 'close' (assert_close at rtol, anchored on f64 when given) or 'scratch' (guards only)"""

    def __init__(self, ref, mode="close", f64=None, rtol=1e-5, loose=None):
        self.ref, self.mode, self.f64, self.rtol, self.loose = ref, mode, f64, rtol, loose


def exact(ref, loose=None, f64=None):
    return Ref(ref, "exact", f64=f64, loose=loose)


class Entry:
    def __init__(self, id, cname, args, expect, refuses=None, route=None):
        """args: the C argument list -- G, Arg, a key of the case (str), a literal, or a callable of (case, state);
        expect(case) -> {output name: Ref}; refuses(placement) -> bool: a documented refusal; route(case, placement, state)"""
        self.id, self.cname, self.args, self.expect, self.refuses, self.route = id, cname, args, expect, refuses, route

    @property
    def operands(self):
        names = []
        for a in self.args:
            if isinstance(a, Arg) and a.name not in names:
                names.append(a.name)
        return names


def placements(entry):
    names = entry.operands
    out = [(f"all{k}", {n: k for n in names}) for k in KS]
    if len(names) > 1:
        out += [(f"only_{n}", {m: (1 if m == n else 4) for m in names}) for n in names]
    return out


def cases(entries):
    return [pytest.param(e, pl, id=f"{e.id}-{tag}") for e in entries for tag, pl in placements(e)]


_CACHE = {}


def cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def _expect(e, c):
    return cached(("expect", e.id, id(c)), lambda: e.expect(c))


def _dtype(a):
    import torch

    return {"float32": torch.float32, "int32": torch.int32}[str(np.asarray(a).dtype)]


def _compare(got, r, what):
    if r.mode == "scratch":
        return
    ref = np.asarray(r.ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if r.mode == "exact":
        if r.loose is None:
            assert np.array_equal(got, ref), f"{what}: differs from the oracle ({rel_err(got, ref):.3e})"
        else:
            assert np.array_equal(got[~r.loose], ref[~r.loose]), f"{what}: rows of at most 512 entries differ from the oracle"
            assert_close(got, ref, 1e-5, what + " (hub rows)", f64=r.f64)
    else:
        print(f"{what}: {rel_err(got, ref):.3e} from the reference (allowed {r.rtol})")
        assert_close(got, ref, r.rtol, what, f64=r.f64)


def run(dev, e, c, pl):
    """one placement of one entry on one case"""
    import torch
    from athena_amd import _capi

    exp = _expect(e, c)
    refused = bool(e.refuses and e.refuses(pl))
    for attempt in ((pl, True), ({n: 4 for n in pl}, False)) if refused else ((pl, False),):
        place, expect_refusal = attempt
        ins, outs, ptr, state, argv = {}, {}, {}, {}, []
        for a in e.args:
            if isinstance(a, Arg):
                if a.name not in ptr:
                    if a.kind == "in":
                        t = placed(c[a.key], dev, place[a.name])
                        ins[a.name] = (t, np.ascontiguousarray(c[a.key]))
                    else:
                        ref = np.asarray(exp[a.name].ref)
                        t, chk = placed_out(ref.shape, _dtype(ref), dev, place[a.name], init=c[a.key] if a.kind == "inout" else None)
                        outs[a.name] = (t, chk)
                    ptr[a.name] = C.c_void_p(t.data_ptr())
                argv.append(ptr[a.name])
            elif a is G:
                argv.append(c["g"].handle)
            elif callable(a):
                argv.append(a(c, state))
            elif isinstance(a, str):
                argv.append(c[a])
            else:
                argv.append(a)
        _capi.use_torch_stream()
        if expect_refusal:
            with pytest.raises(_capi.AthenaMPError, match="aligned"):
                _capi.call(e.cname, *argv)
            torch.cuda.synchronize()
            for name, (t, chk) in outs.items():
                chk(f"{e.id}: {name} (refused call)")
                assert unwritten(t) == t.numel(), f"{e.id}: the refused call wrote {name}"
            continue
        try:
            _capi.call(e.cname, *argv)
            torch.cuda.synchronize()
        except RuntimeError as ex:
            # a HIP error (a fault, a failed launch) is not a wrong result: nothing more of this file runs on a device in that state
            if "hip" in str(ex).lower():
                pytest.exit(f"{e.id} at {place}: {ex}", returncode=3)
            raise
        for name, (t, chk) in outs.items():
            chk(f"{e.id}: {name}")
            _compare(t.cpu().numpy(), exp[name], f"{e.id}: {name}")
        for name, (t, src) in ins.items():
            assert np.array_equal(t.cpu().numpy().reshape(-1).view(np.int32), src.reshape(-1).view(np.int32)), f"{e.id}: input {name} changed"
        if e.route:
            e.route(c, place, state)


def o32():
    from oracle import oracle

    oracle.lib()
    return oracle


def o64():
    from oracle import oracle64

    return oracle64


# =====================================================================================================================================
# Kipf gather: n = 301, 900 pairs, 3 isolated rows, one hub vertex of 700 more entries (> kLongRow = 512: the segmented path and its
# partial buffer, in the forward and in the transposed structure)
# =====================================================================================================================================
def _add_hub(ia, ja, n, hub_entries, seed):
    rng = np.random.default_rng(seed)
    extra = rng.integers(2, n - 2, hub_entries)
    rows = np.repeat(np.arange(1, n + 1), np.diff(ia))
    src = np.concatenate([rows, np.ones(hub_entries, np.int64), extra])
    dst = np.concatenate([ja[0], extra, np.ones(hub_entries, np.int64)])
    order = np.argsort(src, kind="stable")
    ia = np.concatenate([[1], 1 + np.cumsum(np.bincount(src - 1, minlength=n))]).astype(np.int32)
    ja = np.zeros((2, src.size), np.int32, order="F")
    ja[0] = dst[order]
    return ia, ja


def _kipf_graph(hub):
    n = 301
    ia, ja = random_graph(n, 900, seed=5, self_loops=True, isolated=3)
    ja = ja.copy(order="F")
    ja[1] = 0
    if hub:
        ia, ja = _add_hub(ia, ja, n, 700, 3)
        assert np.diff(ia).max() > 512 and np.bincount(ja[0] - 1, minlength=n).max() > 512
    else:
        assert np.diff(ia).max() <= 512
    assert not np.diff(ia)[-3:].any()
    return n, ia, ja


def _banded_graph():
    """a block-diagonal batch: 257 vertices, every neighbour within 17 rows, at most 8 entries per row AND per column, no empty row
    (finite coefficients): what banded_ok asks of both directions"""
    n, band, cap = 257, 17, 8
    rng = np.random.default_rng(17)
    deg = np.zeros(n, np.int64)
    pairs = []
    for v in range(n - 1):
        pairs.append((v, v + 1)); deg[v] += 1; deg[v + 1] += 1
    pairs.append((0, band))                                  # the band's edge is reached
    deg[0] += 1; deg[band] += 1
    for v in range(n):
        for u in rng.integers(v + 2, min(n, v + band + 1), 3) if v + 2 < n else []:
            if deg[v] < cap and deg[u] < cap:
                pairs.append((v, int(u))); deg[v] += 1; deg[u] += 1
    src = np.array([p[0] for p in pairs] + [p[1] for p in pairs], np.int64)
    dst = np.array([p[1] for p in pairs] + [p[0] for p in pairs], np.int64)
    order = np.lexsort((dst, src))
    ia = np.concatenate([[1], 1 + np.cumsum(np.bincount(src, minlength=n))]).astype(np.int32)
    ja = np.zeros((2, src.size), np.int32, order="F")
    ja[0] = dst[order] + 1
    assert np.diff(ia).max() <= cap and np.diff(ia).min() >= 1 and np.abs(src - dst).max() == band
    return n, ia, ja


def _kipf_case(kind, F):
    def build():
        from athena_amd import DeviceGraph

        n, ia, ja = {"hub": lambda: _kipf_graph(True), "plain": lambda: _kipf_graph(False), "banded": _banded_graph}[kind]()
        rng = np.random.default_rng(100 + F)
        return {"kind": kind, "n": n, "ia": ia, "ja": ja, "g": DeviceGraph(ia, ja, n_edge_cols=0), "F": F,
                "x": rng.uniform(-1, 1, (n, F)).astype(np.float32), "up": rng.uniform(-1, 1, (n, F)).astype(np.float32),
                "hub_rows": np.diff(ia) > 512, "hub_cols": np.bincount(ja[0] - 1, minlength=n) > 512}
    return cached(("kipf", kind, F), build)


def _fwd_ref(c, key="x"):
    o = o32()
    loose = c["hub_rows"] if c["hub_rows"].any() else None
    return exact(o.kipf_propagate(c[key], c["ia"], c["ja"]), loose, lambda: o64().kipf_propagate(c[key], c["ia"], c["ja"]))


def _bwd_ref(c, ex, key="up"):
    o = o32()
    loose = c["hub_cols"] if c["hub_cols"].any() else None
    return exact(o.kipf_propagate_bwd(c[key], c["ia"], c["ja"], exact=ex), loose,
                 lambda: o64().kipf_propagate_bwd(c[key], c["ia"], c["ja"], exact=ex))


def _plain_sum_ref(c, key="x"):
    """sum of the listed rows without a coefficient (duvenaud_propagate with no edge part)"""
    loose = c["hub_rows"] if c["hub_rows"].any() else None
    F = c[key].shape[1]
    e0 = np.zeros((1, 1), np.float32)
    return exact(np.ascontiguousarray(o32().duvenaud_propagate(c[key], e0, c["ia"], c["ja"])[:, :F]), loose,
                 lambda: o64().duvenaud_propagate(c[key], e0, c["ia"], c["ja"])[:, :F])


def _act_ref(c, act):
    r = _fwd_ref(c)
    if act == "relu":          # max(., 0) of the same bits
        return exact(o32().activation("relu", r.ref), r.loose, lambda: o64().activation("relu", r.f64()))
    return Ref(o32().activation(act, r.ref), "close", lambda: o64().activation(act, r.f64()))


KIPF = [
    Entry("kipf_fwd", "athena_mp_kipf_propagate_fwd", [G, "F", I("x"), O("y")], lambda c: {"y": _fwd_ref(c)}),
    Entry("kipf_act_relu", "athena_mp_kipf_propagate_act_fwd", [G, "F", I("x"), 1, O("y")], lambda c: {"y": _act_ref(c, "relu")}),
    Entry("kipf_act_tanh", "athena_mp_kipf_propagate_act_fwd", [G, "F", I("x"), 3, O("y")], lambda c: {"y": _act_ref(c, "tanh")}),
    Entry("kipf_bwd", "athena_mp_kipf_propagate_bwd", [G, "F", I("grad", "up"), O("dx"), 0], lambda c: {"dx": _bwd_ref(c, False)}),
    Entry("kipf_bwd_exact", "athena_mp_kipf_propagate_bwd", [G, "F", I("grad", "up"), O("dx"), 1], lambda c: {"dx": _bwd_ref(c, True)}),
    Entry("kipf_bwd_dual", "athena_mp_kipf_propagate_bwd_dual", [G, "F", I("grad", "up"), O("dx_plain"), O("dx_coef")],
          lambda c: {"dx_plain": _bwd_ref(c, False), "dx_coef": _bwd_ref(c, True)}),
    Entry("kipf_fwd_dual", "athena_mp_kipf_propagate_fwd_dual", [G, "F", I("x"), O("y_plain"), O("y_coef")],
          lambda c: {"y_plain": _plain_sum_ref(c), "y_coef": _fwd_ref(c)}),
    Entry("reverse_fwd", "athena_mp_reverse_kipf_propagate_fwd", [G, "F", I("a", "up"), O("c")], lambda c: {"c": _bwd_ref(c, False)}),
    Entry("reverse_partial", "athena_mp_reverse_kipf_propagate_partial", [G, "F", I("upstream", "x"), O("out")],
          lambda c: {"out": _fwd_ref(c)}),
    Entry("reverse_partial_val", "athena_mp_reverse_kipf_propagate_partial_val", [G, "F", I("upstream", "up"), O("out")],
          lambda c: {"out": _bwd_ref(c, False)}),
]


@pytest.mark.parametrize("F", [6, 7, 64, 128])
@pytest.mark.parametrize("entry,pl", cases(KIPF))
def test_kipf_gather(dev, entry, pl, F):
    """vec = 4 / 2 / 1 of the general gather (F = 6 at k = 2 is the one way into vec = 2), its segmented hub path and the partial
    buffer, the dual gather's two-pass route"""
    run(dev, entry, _kipf_case("hub", F), pl)


@pytest.mark.parametrize("F", [64, 128])
@pytest.mark.parametrize("entry,pl", cases(KIPF))
def test_kipf_gather_banded(dev, entry, pl, F):
    """the LDS-staged gather of a block-diagonal batch at k = 4, the general gather at k = 1, 2 (banded_ok)"""
    run(dev, entry, _kipf_case("banded", F), pl)


# =====================================================================================================================================
# the fused Kipf step
# =====================================================================================================================================
def _layer_case(kind, Fi, Fo):
    def build():
        c = dict(_kipf_case(kind, Fi))
        rng = np.random.default_rng(200 + Fi + Fo)
        n = c["n"]
        c.update({"Fi": Fi, "Fo": Fo, "W": (rng.standard_normal(Fo * Fi) * np.sqrt(2.0 / Fi)).astype(np.float32),
                  "bias": rng.standard_normal(Fo).astype(np.float32), "dZ": rng.uniform(-1, 1, (n, Fo)).astype(np.float32)})
        return c
    return cached(("layer", kind, Fi, Fo), build)


def _z_ref(c, act, bias):
    o, d = o32(), o64()
    ia, ja, w, x, b, Fo = c["ia"], c["ja"], c["W"], c["x"], c["bias"], c["Fo"]
    z = o.matmul(w, o.kipf_propagate(x, ia, ja), Fo)
    z64 = lambda: d.add_bias_rows(d.matmul(w, d.kipf_propagate(x, ia, ja), Fo), b) if bias else d.matmul(w, d.kipf_propagate(x, ia, ja), Fo)
    return Ref(o.activation(act, o.add_bias_rows(z, b) if bias else z), "close", lambda: d.activation(act, z64()))


def _dx_ref(c, ex):
    o, d = o32(), o64()
    ia, ja, w, dz, Fi = c["ia"], c["ja"], c["W"], c["dZ"], c["Fi"]
    return Ref(o.kipf_propagate_bwd(o.matmul_dx(w, dz, Fi), ia, ja, exact=ex), "close",
               lambda: d.kipf_propagate_bwd(d.matmul_dx(w, dz, Fi), ia, ja, exact=ex))


def _pull_ref(c, ex):
    """dX[v] = (sum over row v of [coef] dZ[col]) . W"""
    o, d = o32(), o64()
    ia, ja, w, dz, Fi = c["ia"], c["ja"], c["W"], c["dZ"], c["Fi"]
    e0 = np.zeros((1, 1), np.float32)
    agg = (lambda m: m.kipf_propagate(dz, ia, ja)) if ex else (lambda m: np.ascontiguousarray(m.duvenaud_propagate(dz, e0, ia, ja)[:, :dz.shape[1]]))
    return Ref(o.matmul_dx(w, agg(o), Fi), "close", lambda: d.matmul_dx(w, agg(d), Fi))


def _dw_ref(c):
    o, d = o32(), o64()
    ia, ja, x, dz = c["ia"], c["ja"], c["x"], c["dZ"]
    return Ref(o.matmul_dw(dz, o.kipf_propagate(x, ia, ja)).reshape(-1), "close", lambda: d.matmul_dw(dz, d.kipf_propagate(x, ia, ja)).reshape(-1))


LAYER = [
    Entry("layer_fwd_P_bias_tanh", "athena_mp_kipf_layer_fwd", [G, "Fi", "Fo", I("x"), I("W"), I("bias"), 3, O("P"), O("Z")],
          lambda c: {"P": _fwd_ref(c), "Z": _z_ref(c, "tanh", True)}),
    Entry("layer_fwd", "athena_mp_kipf_layer_fwd", [G, "Fi", "Fo", I("x"), I("W"), None, 0, None, O("Z")],
          lambda c: {"Z": _z_ref(c, "none", False)}),
    Entry("layer_bwd_x", "athena_mp_kipf_layer_bwd_x", [G, "Fi", "Fo", I("dZ"), I("W"), 0, O("dX")], lambda c: {"dX": _dx_ref(c, False)}),
    Entry("layer_bwd_x_exact", "athena_mp_kipf_layer_bwd_x", [G, "Fi", "Fo", I("dZ"), I("W"), 1, O("dX")], lambda c: {"dX": _dx_ref(c, True)}),
    Entry("pull_gemm", "athena_mp_pull_gemm", [G, "Fi", "Fo", I("dZ"), I("W"), 0, O("dX")], lambda c: {"dX": _pull_ref(c, False)}),
    Entry("pull_gemm_exact", "athena_mp_pull_gemm", [G, "Fi", "Fo", I("dZ"), I("W"), 1, O("dX")], lambda c: {"dX": _pull_ref(c, True)}),
    Entry("layer_bwd", "athena_mp_kipf_layer_bwd", [G, "Fi", "Fo", I("dZ"), I("W"), I("X", "x"), 0, O("dX"), O("dW")],
          lambda c: {"dX": _dx_ref(c, False), "dW": _dw_ref(c)}),
    Entry("layer_bwd_exact", "athena_mp_kipf_layer_bwd", [G, "Fi", "Fo", I("dZ"), I("W"), I("X", "x"), 1, O("dX"), O("dW")],
          lambda c: {"dX": _dx_ref(c, True), "dW": _dw_ref(c)}),
    Entry("layer_bwd_no_dx", "athena_mp_kipf_layer_bwd", [G, "Fi", "Fo", I("dZ"), I("W"), I("X", "x"), 0, None, O("dW")],
          lambda c: {"dW": _dw_ref(c)}),
]


@pytest.mark.parametrize("Fi,Fo", [(64, 64), (128, 128), (256, 256), (7, 7), (24, 16)])
@pytest.mark.parametrize("entry,pl", cases(LAYER))
def test_fused_kipf_step(dev, entry, pl, Fi, Fo):
    """the one-launch kernels (fused.hip, fused_dw.hip) at k = 4, the two-kernel route at k = 1, 2; 7 -> 7 on 301 rows: the second
    half of kipf_layer_bwd's workspace starts at an odd element"""
    run(dev, entry, _layer_case("plain", Fi, Fo), pl)


@pytest.mark.parametrize("Fi,Fo", [(64, 64), (128, 128)])
@pytest.mark.parametrize("entry,pl", cases(LAYER[:4]))
def test_fused_kipf_step_banded(dev, entry, pl, Fi, Fo):
    """banded_agg_gemm64 (64 -> 64, one launch) and the LDS-staged gather followed by the dense step"""
    run(dev, entry, _layer_case("banded", Fi, Fo), pl)


# =====================================================================================================================================
# dense contraction
# =====================================================================================================================================
def _dense_case(M, K, N):
    def build():
        rng = np.random.default_rng(M + K + N)
        c = {"M": M, "K": K, "N": N, "P": rng.uniform(-1, 1, (M, K)).astype(np.float32),
             "W": (rng.standard_normal(N * K) * np.sqrt(2.0 / K)).astype(np.float32), "bias": rng.standard_normal(N).astype(np.float32),
             "dZ": rng.uniform(-1, 1, (M, N)).astype(np.float32)}
        c["Wt"] = c["W"].reshape(K, N).astype(np.float64)
        return c
    return cached(("dense", M, K, N), build)


def _f64ref(a):
    """the float64 product as the reference, as test_gemm_family_vs_float64 holds the kernels to"""
    return Ref(np.ascontiguousarray(a, np.float64).astype(np.float32), "close", np.ascontiguousarray(a, np.float64))


DENSE = [
    Entry("matmul", "athena_mp_gemm_fwd", ["M", "K", "N", I("P"), I("W"), None, 0, O("Z")],
          lambda c: {"Z": _f64ref(c["P"].astype(np.float64) @ c["Wt"])}),
    Entry("matmul_bias_relu", "athena_mp_gemm_fwd", ["M", "K", "N", I("P"), I("W"), I("bias"), 1, O("Z")],
          lambda c: {"Z": _f64ref(np.maximum(c["P"].astype(np.float64) @ c["Wt"] + c["bias"], 0))}),
    Entry("matmul_dx", "athena_mp_gemm_dx", ["M", "K", "N", I("dZ"), I("W"), O("dP")],
          lambda c: {"dP": _f64ref(c["dZ"].astype(np.float64) @ c["Wt"].T)}),
    Entry("matmul_dw", "athena_mp_gemm_dw", ["M", "K", "N", I("P"), I("dZ"), O("dW")],
          lambda c: {"dW": _f64ref((c["P"].astype(np.float64).T @ c["dZ"]).reshape(-1))}),
]


@pytest.mark.parametrize("M,K,N", [(300, 64, 64), (100, 64, 64), (300, 128, 32), (300, 7, 6)])
@pytest.mark.parametrize("entry,pl", cases(DENSE))
def test_dense(dev, entry, pl, M, K, N):
    """the weight-resident MFMA kernels at k = 4; gemm_tiled without its vector loads (300 rows) and gemm_small_kernel (100 rows) at
    k = 1; 7 x 6: the VALU kernels at every k"""
    run(dev, entry, _dense_case(M, K, N), pl)


@pytest.mark.parametrize("M,K,N", [(200, 64, 64), (1000, 64, 64), (200, 128, 64), (1000, 128, 64), (4100, 256, 256)])
@pytest.mark.parametrize("entry,pl", cases(DENSE[3:]))
def test_dense_weight_gradient_routes(dev, entry, pl, M, K, N):
    """gemm_dw_dispatch: the register-resident kernel (64 / 128 wide) drops to gemm_dw_small_kernel with 4096 - 8192 outputs below
    256 rows and to gemm_atb_tiled from 256 rows when P or dZ is not 16-byte aligned; 256 x 256 from 4096 rows: the blocked route"""
    run(dev, entry, _dense_case(M, K, N), pl)


@pytest.mark.parametrize("entry,pl", cases(DENSE[2:3]))
def test_dense_wide_output(dev, entry, pl):
    """C[1100, 512] = A[1100, 64] . B^T: gemm_arow_kernel at k = 4, gemm_tiled at k = 1"""
    run(dev, entry, _dense_case(1100, 512, 64), pl)


# =====================================================================================================================================
# Duvenaud: a batch of molecule-like graphs (degrees 1 .. 4, every bond within 17 rows), n = 301 in 5 graphs; n = 1025 in 17 graphs
# for the entries whose MFMA routes start at 1024 rows (duv_use_mfma, athena_mp_duvenaud_readout_update_bwd)
# =====================================================================================================================================
def _molecules(n, n_graphs, seed):
    rng = np.random.default_rng(seed)
    sizes = np.full(n_graphs, n // n_graphs)
    sizes[: n - sizes.sum()] += 1
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    deg = np.zeros(n, np.int64)
    pairs = []
    for s in range(n_graphs):
        a, b = int(seg[s]), int(seg[s + 1])
        for v in range(a, b - 1):
            pairs.append((v + 1, v + 2)); deg[v] += 1; deg[v + 1] += 1
        for v in range(a, b - 2):
            u = int(rng.integers(v + 2, min(b, v + 18)))
            if deg[v] < 4 and deg[u] < 4 and rng.random() < 0.6:
                pairs.append((v + 1, u + 1)); deg[v] += 1; deg[u] += 1
    g = csr_from_index_list(n, np.array(pairs).T)
    assert np.diff(g.adj_ia).max() <= 4 and np.diff(g.adj_ia).min() >= 1
    return g.adj_ia, g.adj_ja, len(pairs), seg


def _duv_case(n, Fv, Fe, Fo, Oo):
    def build():
        from athena_amd import DeviceGraph

        o = o32()
        ia, ja, E, seg = _molecules(n, 5 if n < 1000 else 17, n + Fv)
        rng = np.random.default_rng(300 + n + Fv)
        mn, mx, Fi, S = 1, 4, Fv + Fe, seg.size - 1
        D = mx - mn + 1
        c = {"n": n, "ia": ia, "ja": ja, "E": E, "seg": seg, "S": S, "g": DeviceGraph(ia, ja, n_edge_cols=E), "Fv": Fv, "Fe": Fe, "Fi": Fi,
             "Fo": Fo, "O": Oo, "mn": mn, "mx": mx,
             "x": rng.uniform(0, 1, (n, Fv)).astype(np.float32), "e": rng.uniform(0, 1, (E, Fe)).astype(np.float32),
             "up_c": rng.uniform(-1, 1, (n, Fi)).astype(np.float32), "a": rng.uniform(0, 4, (n, Fi)).astype(np.float32),
             "w": (rng.standard_normal(Fo * Fi * D) * 0.3).astype(np.float32), "up_o": rng.uniform(-1, 1, (n, Fo)).astype(np.float32),
             "R": (rng.standard_normal(Oo * Fo) * 0.3).astype(np.float32), "gout": rng.standard_normal((S, Oo)).astype(np.float32),
             "dzn": rng.standard_normal((n, Fo)).astype(np.float32), "logits": (rng.standard_normal((n, Oo)) * 2).astype(np.float32),
             # the square step of athena_mp_duvenaud_readout_update_bwd: Fv + Fe -> Fv
             "w_sq": (rng.standard_normal(Fv * Fi * D) * 0.3).astype(np.float32), "R_sq": (rng.standard_normal(Oo * Fv) * 0.3).astype(np.float32),
             "dzn_sq": rng.standard_normal((n, Fv)).astype(np.float32)}
        c["a_x"], c["a_e"] = np.ascontiguousarray(c["a"][:, :Fv]), np.ascontiguousarray(c["a"][:, Fv:])
        c["z"] = o.activation("sigmoid", o.duvenaud_update(c["a"], c["w"], ia, mn, mx, Fo))
        c["p"] = o.softmax_cols(o.matmul(c["R"], c["z"], Oo))
        c["z_sq"] = o.activation("sigmoid", o.duvenaud_update(c["a"], c["w_sq"], ia, mn, mx, Fv))
        c["p_sq"] = o.softmax_cols(o.matmul(c["R_sq"], c["z_sq"], Oo))
        c["sizes"] = np.diff(seg)
        return c
    return cached(("duv", n, Fv, Fe, Fo, Oo), build)


def _small(c):
    return c["Fi"] < 16 or c["Fo"] < 16           # the VALU kernels in the reference's operation order: bit-exact


def _upd(m, c, w="w", Fo="Fo"):
    return m.duvenaud_update(c["a"], c[w], c["ia"], c["mn"], c["mx"], c[Fo])


def _upd_ref(c):
    r = _upd(o32(), c)
    return exact(r) if _small(c) else Ref(r, "close", lambda: _upd(o64(), c))


def _upd_act_ref(c):
    return Ref(o32().activation("sigmoid", _upd(o32(), c)), "close", lambda: o64().activation("sigmoid", _upd(o64(), c)))


def _p_ref(c):
    o, d = o32(), o64()
    return Ref(o.softmax_cols(o.matmul(c["R"], o.activation("sigmoid", _upd(o, c)), c["O"])), "close",
               lambda: d.softmax_cols(d.matmul(c["R"], d.activation("sigmoid", _upd(d, c)), c["O"])))


def _da_ref(c, cols=None, grad="up_o", w="w"):
    cut = (lambda a: np.ascontiguousarray(a[:, cols])) if cols is not None else (lambda a: a)
    f = lambda m: cut(m.duvenaud_update_bwd_a(c[grad], c[w], c["ia"], c["mn"], c["mx"], c["Fi"]))
    return exact(f(o32())) if _small(c) else Ref(f(o32()), "close", lambda: f(o64()))


def _dwd_ref(c, grad="up_o"):
    f = lambda m: m.duvenaud_update_bwd_w(c[grad], c["a"], c["ia"], c["mn"], c["mx"])
    return Ref(f(o32()), "close", lambda: f(o64()))


def _readout_refs(c):
    o, d = o32(), o64()
    po = o.softmax_cols(o.matmul(c["R"], c["z"], c["O"]))
    p64 = lambda: d.softmax_cols(d.matmul(c["R"], c["z"], c["O"]))
    return {"p": Ref(po, "close", p64), "out": Ref(o.segment_sum(po, c["seg"]), "close", lambda: d.segment_sum(p64(), c["seg"]))}


def _readout_bwd(m, c, z, R, p, dzn, act="sigmoid"):
    """(dc, dR, dl) of the readout's reverse through the message activation, the chain of test_gpu_ops.py"""
    Fv = z.shape[1]
    dl = m.softmax_cols_bwd(p, np.repeat(c["gout"], c["sizes"], axis=0))
    dz = m.matmul_dx(R, dl, Fv) + dzn
    return m.activation_bwd(act, z, dz), m.matmul_dw(dl, z).reshape(-1)


def _readout_bwd_refs(c):
    f = lambda m: _readout_bwd(m, c, c["z"], c["R"], c["p"], c["dzn"])
    return {"dc": Ref(f(o32())[0], "close", lambda: f(o64())[0]), "dR": Ref(f(o32())[1], "close", lambda: f(o64())[1])}


def _readout_update_bwd_refs(c):
    Fv = c["Fv"]

    def f(m):
        dc, dR = _readout_bwd(m, c, c["z_sq"], c["R_sq"], c["p_sq"], c["dzn_sq"])
        da = m.duvenaud_update_bwd_a(dc, c["w_sq"], c["ia"], c["mn"], c["mx"], c["Fi"])
        return (np.ascontiguousarray(da[:, :Fv]), np.ascontiguousarray(da[:, Fv:]), m.duvenaud_update_bwd_w(dc, c["a"], c["ia"], c["mn"], c["mx"]), dR)
    names = ("da_x", "da_e", "dW", "dR")
    got = f(o32())
    return {k: Ref(got[i], "close", (lambda i: lambda: f(o64())[i])(i)) for i, k in enumerate(names)}


def _prop(c):
    return o32().duvenaud_propagate(c["x"], c["e"], c["ia"], c["ja"])


DUV_GATHER = [
    Entry("duv_propagate", "athena_mp_duvenaud_propagate_fwd", [G, "Fv", "Fe", I("x"), I("e"), O("c")], lambda c: {"c": exact(_prop(c))}),
    Entry("duv_propagate_edges", "athena_mp_duvenaud_propagate_fwd", [G, 0, "Fe", None, I("e"), O("c")],
          lambda c: {"c": exact(np.ascontiguousarray(_prop(c)[:, c["Fv"]:]))}),
    Entry("neighbour_sum", "athena_mp_duvenaud_propagate_fwd", [G, "Fv", 0, I("x"), None, O("c")],
          lambda c: {"c": exact(np.ascontiguousarray(_prop(c)[:, :c["Fv"]]))}),
    Entry("duv_propagate_bwd_x", "athena_mp_duvenaud_propagate_bwd_x", [G, "Fv", "Fe", I("grad", "up_c"), O("dx")],
          lambda c: {"dx": exact(o32().duvenaud_propagate_bwd_x(c["up_c"], c["Fv"], c["ia"], c["ja"]))}),
    Entry("duv_propagate_bwd_e", "athena_mp_duvenaud_propagate_bwd_e", [G, "Fv", "Fe", I("grad", "up_c"), O("de")],
          lambda c: {"de": exact(o32().duvenaud_propagate_bwd_e(c["up_c"], c["Fv"], c["E"], c["ia"], c["ja"]))}),
    Entry("softmax_segsum", "athena_mp_softmax_segsum_fwd", ["O", "n", "S", I("seg"), I("logits"), O("p"), O("out"), 0],
          lambda c: {"p": Ref(o32().softmax_cols(c["logits"])), "out": Ref(o32().segment_sum(o32().softmax_cols(c["logits"]), c["seg"]))}),
    Entry("softmax_segsum_bwd", "athena_mp_softmax_segsum_bwd", ["O", "n", "S", I("seg"), I("p"), I("gout"), O("dlogits")],
          lambda c: {"dlogits": Ref(o32().softmax_cols_bwd(c["p"], np.repeat(c["gout"], c["sizes"], axis=0)))}),
    Entry("segment_sum", "athena_mp_segment_sum", ["O", "n", "S", I("seg"), I("p"), O("out"), 0],
          lambda c: {"out": Ref(o32().segment_sum(c["p"], c["seg"]), "close", lambda: o64().segment_sum(c["p"], c["seg"]))}),
    Entry("segment_sum_bwd", "athena_mp_segment_sum_bwd", ["O", "n", "S", I("seg"), I("gout"), O("dp")],
          lambda c: {"dp": exact(np.repeat(c["gout"], c["sizes"], axis=0))}),
]

DUV_UPDATE = [
    Entry("duv_update", "athena_mp_duvenaud_update_fwd", [G, "Fi", "Fo", "mn", "mx", I("a"), I("weight", "w"), O("c")],
          lambda c: {"c": _upd_ref(c)}),
    Entry("duv_update_act", "athena_mp_duvenaud_update_act_fwd", [G, "Fi", "Fo", "mn", "mx", I("a"), I("weight", "w"), 2, O("z")],
          lambda c: {"z": _upd_act_ref(c)}),
    Entry("duv_update_act_readout", "athena_mp_duvenaud_update_readout_fwd",
          [G, "Fi", "Fo", "mn", "mx", I("a"), I("weight", "w"), 2, O("z"), "O", I("R"), O("p")], lambda c: {"z": _upd_act_ref(c), "p": _p_ref(c)}),
    Entry("duv_update_act_readout_split", "athena_mp_duvenaud_update_readout_fwd_split",
          [G, "Fv", "Fe", "Fo", "mn", "mx", I("a_x"), I("a_e"), I("weight", "w"), 2, O("z"), "O", I("R"), O("p")],
          lambda c: {"z": _upd_act_ref(c), "p": _p_ref(c)}),
    Entry("duv_update_bwd_a", "athena_mp_duvenaud_update_bwd_a", [G, "Fi", "Fo", "mn", "mx", I("grad", "up_o"), I("weight", "w"), O("da")],
          lambda c: {"da": _da_ref(c)}),
    Entry("duv_update_bwd_w", "athena_mp_duvenaud_update_bwd_w", [G, "Fi", "Fo", "mn", "mx", I("grad", "up_o"), I("a"), O("dweight")],
          lambda c: {"dweight": _dwd_ref(c)}),
    Entry("duv_update_bwd", "athena_mp_duvenaud_update_bwd",
          [G, "Fi", "Fo", "mn", "mx", I("grad", "up_o"), I("a"), I("weight", "w"), O("da"), O("dweight")],
          lambda c: {"da": _da_ref(c), "dweight": _dwd_ref(c)}),
    Entry("duv_update_bwd_split", "athena_mp_duvenaud_update_bwd_split",
          [G, "Fv", "Fe", "Fo", "mn", "mx", I("grad", "up_o"), I("a"), I("weight", "w"), O("da_x"), O("da_e"), O("dweight")],
          lambda c: {"da_x": _da_ref(c, slice(0, c["Fv"])), "da_e": _da_ref(c, slice(c["Fv"], None)), "dweight": _dwd_ref(c)}),
    Entry("duv_readout", "athena_mp_duvenaud_readout_fwd", ["n", "Fo", "O", "S", I("seg"), I("z"), I("R"), O("p"), O("out"), 0], _readout_refs),
    Entry("duv_readout_bwd", "athena_mp_duvenaud_readout_bwd",
          ["n", "Fo", "O", "S", I("seg"), I("z"), I("R"), I("p"), I("gout"), I("dz_next", "dzn"), 2, O("dc"), O("dR"), 0], _readout_bwd_refs),
    Entry("duv_readout_update_bwd", "athena_mp_duvenaud_readout_update_bwd",
          [G, "Fv", "Fe", "mn", "mx", "O", "S", I("seg"), I("z", "z_sq"), I("R", "R_sq"), I("p", "p_sq"), I("gout"), I("dz_next", "dzn_sq"), 2,
           I("a"), I("weight", "w_sq"), O("da_x"), O("da_e"), O("dW"), O("dR"), 0, 0, None], _readout_update_bwd_refs),
    Entry("duv_readout_update_bwd_split_a", "athena_mp_duvenaud_readout_update_bwd",
          [G, "Fv", "Fe", "mn", "mx", "O", "S", I("seg"), I("z", "z_sq"), I("R", "R_sq"), I("p", "p_sq"), I("gout"), I("dz_next", "dzn_sq"), 2,
           I("a", "a_x"), I("weight", "w_sq"), O("da_x"), O("da_e"), O("dW"), O("dR"), 0, 0, I("a_e")], _readout_update_bwd_refs),
]

DUV_SHAPES = [(64, 8, 64, 10), (32, 4, 48, 3), (6, 1, 7, 2)]


@pytest.mark.parametrize("Fv,Fe,Fo,Oo", DUV_SHAPES)
@pytest.mark.parametrize("entry,pl", cases(DUV_GATHER))
def test_duvenaud_gathers_and_sums(dev, entry, pl, Fv, Fe, Fo, Oo):
    """gather_short_rows (whole packed rows, 16 bytes per lane) and the banded gather at k = 4, the general gather below"""
    run(dev, entry, _duv_case(301, Fv, Fe, Fo, Oo), pl)


@pytest.mark.parametrize("Fv,Fe,Fo,Oo", DUV_SHAPES)
@pytest.mark.parametrize("entry,pl", cases(DUV_UPDATE))
def test_duvenaud_update_and_readout(dev, entry, pl, Fv, Fe, Fo, Oo):
    """301 rows: the VALU update kernels; the one-launch readout (F_v = 64, O = 10) and its composed chain"""
    run(dev, entry, _duv_case(301, Fv, Fe, Fo, Oo), pl)


@pytest.mark.parametrize("Fv,Fe,Fo,Oo", DUV_SHAPES[:2])
@pytest.mark.parametrize("entry,pl", cases(DUV_UPDATE))
def test_duvenaud_update_and_readout_mfma_rows(dev, entry, pl, Fv, Fe, Fo, Oo):
    """1025 rows, the first size class of the bucketed MFMA kernels (duv_mfma.hip; 72 -> 64 the wide ones with the readout in the
    epilogue and the one-launch reverse, 36 -> 48 the any-shape ones): taken at k = 4, the tiled contraction per bucket at k = 1"""
    run(dev, entry, _duv_case(1025, Fv, Fe, Fo, Oo), pl)


# =====================================================================================================================================
# graph neural operator
# =====================================================================================================================================
def _gno_case(N, d, H, Fi, Fo):
    def build():
        import torch
        from athena_amd import DeviceGraph, _capi, ops

        o = o32()
        rng = np.random.default_rng(400 + N + d + H)
        pairs = [[i, i + 1] for i in range(1, N)] + [[1, N]]
        if N > 100:
            pairs += [[7, int(v)] for v in rng.choice(np.arange(9, N), 40, replace=False)]        # one row of more than 32 entries
            pairs += [[int(a), int(b)] for a, b in rng.integers(1, N + 1, (2 * N, 2)) if a != b]
        pairs = np.array(pairs).T
        g = csr_from_index_list(N, pairs)
        E = pairs.shape[1]
        deg = np.diff(g.adj_ia)
        assert N <= 100 or ((deg > 32).sum() == 1 and N % 32 != 0)
        c = {"N": N, "d": d, "H": H, "Fi": Fi, "Fo": Fo, "E": E, "ia": g.adj_ia, "ja": g.adj_ja, "g": DeviceGraph(g.adj_ia, g.adj_ja, n_edge_cols=E),
             "coords": rng.standard_normal((E, d)).astype(np.float32), "x": rng.uniform(-1, 1, (N, Fi)).astype(np.float32),
             "theta": (0.3 * rng.standard_normal(H * d + H + Fo * Fi * H + Fo * Fi)).astype(np.float32),
             "grad": rng.uniform(-1, 1, (N, Fo)).astype(np.float32)}
        c["kap"] = o.gno_kernel_eval(c["coords"], c["theta"], H, Fo * Fi)
        c["dk"] = o.gno_aggregate_bwd_k(c["grad"], c["x"], E, c["ia"], c["ja"])
        c["saved"] = ops.gno_saved_bytes(c["g"], d, H, Fi, Fo)
        if c["saved"]:        # the S an aligned forward pass keeps: an input of the reverse entries that stream it
            dev = torch.device("cuda:0")
            th, co, xd = (torch.from_numpy(c[k]).to(dev) for k in ("theta", "coords", "x"))
            _, s = ops.gno_aggregate_save(c["g"], th, co, xd, d, H, Fo)
            torch.cuda.synchronize()
            c["s_save"] = s.cpu().numpy()
        return c
    return cached(("gno", N, d, H, Fi, Fo), build)


def _gno_m(c):
    d = o64()
    return Ref(o32().gno_aggregate(c["x"], c["kap"], c["ia"], c["ja"], c["Fo"]), "close",
               lambda: d.gno_aggregate(c["x"], d.gno_kernel_eval(c["coords"], c["theta"], c["H"], c["Fo"] * c["Fi"]), c["ia"], c["ja"], c["Fo"]))


def _gno_dx(c):
    d = o64()
    return Ref(o32().gno_aggregate_bwd_x(c["grad"], c["kap"], c["ia"], c["ja"], c["Fi"]), "close",
               lambda: d.gno_aggregate_bwd_x(c["grad"], d.gno_kernel_eval(c["coords"], c["theta"], c["H"], c["Fo"] * c["Fi"]), c["ia"], c["ja"], c["Fi"]))


def _dk64(c):
    return o64().gno_aggregate_bwd_k(c["grad"], c["x"], c["E"], c["ia"], c["ja"])


def _gno_dth(c):
    return Ref(o32().gno_kernel_bwd_theta(c["coords"], c["theta"], c["dk"], c["H"]), "close",
               lambda: o64().gno_kernel_bwd_theta(c["coords"], c["theta"], _dk64(c), c["H"]))


def _gno_dco(c):
    return Ref(o32().gno_kernel_bwd_coords(c["coords"], c["theta"], c["dk"], c["H"]), "close",
               lambda: o64().gno_kernel_bwd_coords(c["coords"], c["theta"], _dk64(c), c["H"]))


def _fused_flag(c, state):
    state["fused"] = C.c_int32(-1)
    return C.byref(state["fused"])


def _fused_route(c, pl, state):
    """athena_mp_gno_aggregate_bwd says which route ran: the one-call kernels when x, grad, dx (and s_save) are 16-byte aligned at
    a shape that keeps S, the separate entry points otherwise"""
    want = int(bool(c["saved"]) and all(pl[n] == 4 for n in ("x", "grad", "dx", "s_save") if n in pl))
    assert state["fused"].value == want, f"fused = {state['fused'].value}, expected {want} at {pl}"


_GNO_HEAD = [G, "d", "H", "Fi", "Fo", I("theta"), I("coords")]
GNO = [
    Entry("gno_fwd", "athena_mp_gno_aggregate_fwd", _GNO_HEAD + [I("x"), O("m")], lambda c: {"m": _gno_m(c)}),
    Entry("gno_bwd_x", "athena_mp_gno_aggregate_bwd_x", _GNO_HEAD + [I("grad"), O("dx")], lambda c: {"dx": _gno_dx(c)}),
    # (a graph from csr_from_index_list lists both directions of a pair under one edge column: the pull over its own rows is the
    # same gradient)
    Entry("gno_bwd_x_pull", "athena_mp_gno_aggregate_bwd_x_pull", _GNO_HEAD + [I("grad_ext", "grad"), O("dx")], lambda c: {"dx": _gno_dx(c)}),
    Entry("gno_bwd_theta", "athena_mp_gno_aggregate_bwd_theta", _GNO_HEAD + [I("x"), I("grad"), O("dtheta")], lambda c: {"dtheta": _gno_dth(c)}),
    Entry("gno_bwd_coords", "athena_mp_gno_aggregate_bwd_coords", _GNO_HEAD + [I("x"), I("grad"), O("dcoords")], lambda c: {"dcoords": _gno_dco(c)}),
    Entry("gno_bwd", "athena_mp_gno_aggregate_bwd", _GNO_HEAD + [I("x"), I("grad"), None, O("dx"), O("dtheta"), O("dcoords"), _fused_flag],
          lambda c: {"dx": _gno_dx(c), "dtheta": _gno_dth(c), "dcoords": _gno_dco(c)}, route=_fused_route),
    Entry("gno_bwd_dx_only", "athena_mp_gno_aggregate_bwd", _GNO_HEAD + [I("x"), I("grad"), None, O("dx"), None, None, _fused_flag],
          lambda c: {"dx": _gno_dx(c)}, route=_fused_route),
]
GNO_SAVED = [
    Entry("gno_fwd_save", "athena_mp_gno_aggregate_fwd_save", _GNO_HEAD + [I("x"), O("m"), O("s_save")],
          lambda c: {"m": _gno_m(c), "s_save": Ref(c["s_save"], "scratch")},
          refuses=lambda pl: any(pl[n] != 4 for n in ("x", "m", "s_save"))),
    Entry("gno_bwd_theta_saved", "athena_mp_gno_aggregate_bwd_theta_saved", _GNO_HEAD + [I("x"), I("grad"), I("s_save"), O("dtheta")],
          lambda c: {"dtheta": _gno_dth(c)}),
    Entry("gno_bwd_saved", "athena_mp_gno_aggregate_bwd", _GNO_HEAD + [I("x"), I("grad"), I("s_save"), O("dx"), O("dtheta"), None, _fused_flag],
          lambda c: {"dx": _gno_dx(c), "dtheta": _gno_dth(c)}, route=_fused_route),
]


@pytest.mark.parametrize("N,d,H,Fi,Fo", [(301, 3, 64, 64, 64), (21, 1, 8, 3, 3), (21, 4, 64, 64, 64)])
@pytest.mark.parametrize("entry,pl", cases(GNO))
def test_gno(dev, entry, pl, N, d, H, Fi, Fo):
    """H = F = 64: the on-chip kernels of gno64.hip at k = 4 (d = 4: gno_fused_kernel, which reads V from theta 16 bytes per lane),
    the generic outer product + contraction and the tiled kernel-MLP reverse at k = 1, 2; 8 / 3 / 3: the generic route at every k"""
    run(dev, entry, _gno_case(N, d, H, Fi, Fo), pl)


@pytest.mark.parametrize("entry,pl", cases(GNO_SAVED))
def test_gno_training_pair(dev, entry, pl):
    """the pair that keeps S: fwd_save refuses x, m or s_save that are not 16-byte aligned (documented: S has one producer); the
    reverse entries rebuild S when they cannot stream it"""
    c = _gno_case(301, 3, 64, 64, 64)
    assert c["saved"] > 0
    run(dev, entry, c, pl)


# =====================================================================================================================================
# element-wise ops and the train step's tail
# =====================================================================================================================================
def _elem_case():
    def build():
        rng = np.random.default_rng(7)
        n = 70001
        c = {"n": n, "x": (rng.standard_normal(n) * 2).astype(np.float32), "g": rng.standard_normal(n).astype(np.float32),
             "y0": rng.standard_normal(n).astype(np.float32), "alpha": -0.05, "beta": 1.3}
        c["idx"] = rng.integers(0, 1001, 777).astype(np.int32)
        for F in (3, 14, 64):
            c[f"z{F}"] = (rng.standard_normal((1001, F)) * 3).astype(np.float32)
            c[f"g{F}"] = rng.standard_normal((1001, F)).astype(np.float32)
            c[f"y{F}"] = o32().softmax_cols(c[f"z{F}"])
        for k in ("none", "relu", "sigmoid", "tanh"):
            c["y_" + k] = o32().activation(k, c["x"])
        c["a"], c["b"] = np.ascontiguousarray(c["z14"]), np.ascontiguousarray(c["z3"])
        c["cat"] = o32().concat(c["a"], c["b"])
        return c
    return cached(("elem",), build)


def _attr(name, **attrs):
    from athena_amd import ops

    a = ops.actv_type(name, **attrs)
    code, scale, p0, p1 = ops._actp_args(a)
    return code, scale, p0, p1


def _attributed_entries():
    out = []
    for tag, name, attrs in [("leaky_relu", "leaky_relu", {"alpha": 0.2, "scale": 1.5}), ("selu", "selu", {}),
                             ("gaussian", "gaussian", {"sigma": 0.7, "mu": 0.3, "scale": 2.0}), ("piecewise", "piecewise", {"gradient": 0.25, "limit": 0.5})]:
        def args(c, s, name=name, attrs=attrs):
            return _attr(name, **attrs)
        sc = lambda i, args=args: (lambda c, s: args(c, s)[i])
        out.append(Entry(f"act_{tag}", "athena_mp_activation_param_fwd", [sc(0), "n", sc(1), sc(2), sc(3), I("x"), O("y")],
                         lambda c, name=name, attrs=attrs: {"y": Ref(o32().activation_param(name, c["x"], *_attr(name, **attrs)[1:]), rtol=2e-6)}))
        out.append(Entry(f"act_{tag}_bwd", "athena_mp_activation_param_bwd", [sc(0), "n", sc(1), sc(2), sc(3), I("x"), I("g"), O("dx")],
                         lambda c, name=name, attrs=attrs: {"dx": Ref(o32().activation_param_bwd(name, c["x"], c["g"], *_attr(name, **attrs)[1:]), rtol=2e-6)}))
    return out


def _plain_entries():
    out = []
    for code, k in enumerate(("none", "relu", "sigmoid", "tanh")):
        out.append(Entry(f"act_{k}", "athena_mp_activation_fwd", [code, "n", I("z", "x"), O("y")],
                         lambda c, k=k: {"y": Ref(o32().activation(k, c["x"]))}))
        out.append(Entry(f"act_{k}_bwd", "athena_mp_activation_bwd", [code, "n", I("y", "y_" + k), I("g"), O("dz")],
                         lambda c, k=k: {"dz": Ref(o32().activation_bwd(k, c["y_" + k], c["g"]))}))
    return out


def _softmax_entries():
    out = []
    for F in (3, 14, 64):
        out.append(Entry(f"softmax{F}", "athena_mp_softmax_fwd", [1001, F, I("z", f"z{F}"), O("y")],
                         lambda c, F=F: {"y": Ref(o32().softmax_cols(c[f"z{F}"]), rtol=2e-6)}))
        out.append(Entry(f"softmax{F}_bwd", "athena_mp_softmax_bwd", [1001, F, I("y", f"y{F}"), I("g", f"g{F}"), O("dz")],
                         lambda c, F=F: {"dz": Ref(o32().softmax_cols_bwd(c[f"y{F}"], c[f"g{F}"]), rtol=2e-6)}))
    return out


ELEMENTWISE = _plain_entries() + _attributed_entries() + _softmax_entries() + [
    Entry("swish", "athena_mp_swish_fwd", ["n", "beta", I("x"), O("y")], lambda c: {"y": Ref(o32().swish(c["x"], c["beta"]), rtol=1e-6)}),
    Entry("swish_bwd", "athena_mp_swish_bwd", ["n", "beta", I("x"), I("g"), O("dx")],
          lambda c: {"dx": Ref(o32().swish_bwd(c["x"], c["g"], c["beta"]), rtol=1e-6)}),
    Entry("concat", "athena_mp_concat_fwd", [1001, 14, 3, I("a"), I("b"), O("out")], lambda c: {"out": exact(c["cat"])}),
    Entry("concat_bwd", "athena_mp_concat_bwd", [1001, 14, 3, I("gout", "cat"), O("da"), O("db")], lambda c: {"da": exact(c["a"]), "db": exact(c["b"])}),
    Entry("concat_bwd_b_only", "athena_mp_concat_bwd", [1001, 14, 3, I("gout", "cat"), None, O("db")], lambda c: {"db": exact(c["b"])}),
    # y + fl(alpha x): one rounded multiply, one rounded add (the library is built without contraction)
    Entry("axpy", "athena_mp_axpy", ["n", "alpha", I("x"), IO("y", "y0")], lambda c: {"y": exact(c["y0"] + np.float32(c["alpha"]) * c["x"])}),
    Entry("gather_rows", "athena_mp_gather_rows", [777, 14, I("idx"), I("x", "z14"), O("out")], lambda c: {"out": exact(c["z14"][c["idx"]])}),
    Entry("gather_rows64", "athena_mp_gather_rows", [777, 64, I("idx"), I("x", "z64"), O("out")], lambda c: {"out": exact(c["z64"][c["idx"]])}),
    Entry("device_copy", "athena_mp_device_copy", [O("dst"), I("src", "x"), 4 * 70001], lambda c: {"dst": exact(c["x"])},
          refuses=lambda pl: any(k != 4 for k in pl.values())),
]


@pytest.mark.parametrize("entry,pl", cases(ELEMENTWISE))
def test_elementwise(dev, entry, pl):
    run(dev, entry, _elem_case(), pl)


def _train_case():
    def build():
        o = o32()
        rng = np.random.default_rng(3)
        n = 70001
        c = {"n": n, "p": rng.standard_normal(n).astype(np.float32), "g": rng.standard_normal(n).astype(np.float32),
             "v": (rng.standard_normal(n) * 0.1).astype(np.float32), "m": (rng.standard_normal(n) * 0.1).astype(np.float32),
             "v2": (rng.standard_normal(n) ** 2 * 0.1).astype(np.float32), "g3": (rng.standard_normal(n) * 3).astype(np.float32),
             "e": rng.standard_normal(n).astype(np.float32)}
        c["p"][:3] = [0.0, -0.0, 1e-30]
        c["sgd"] = o.sgd_step(c["p"], c["g"], c["v"], 0.05, 0.9, True, "l1l2", 0.02, 0.03)
        c["adam"] = o.adam_step(c["p"], c["g"], c["m"], c["v2"], 0.01, 3, reg="l2", l1=0.0, l2=0.03, decoupled=True)
        c["clamp"] = o.clip(c["g3"], -1.5, 2.0)
        g64 = c["g3"].astype(np.float64)
        c["norm"], c["norm64"] = o.clip(c["g3"], clip_norm=10.0), g64 * min(1.0, 10.0 / np.sqrt((g64 ** 2).sum()))
        lo, do = o.mse(c["p"], c["e"])
        c["loss"], c["dpred"] = np.array([lo], np.float32), do
        c["loss64"] = np.array([((c["p"].astype(np.float64) - c["e"]) ** 2).mean() / 2])
        return c
    return cached(("train",), build)


_HUGE = float(np.finfo(np.float32).max)
TRAIN = [
    Entry("sgd_step", "athena_mp_sgd_step", ["n", 0.05, 0.9, 1, 3, 0.02, 0.03, IO("param", "p"), IO("grad", "g"), IO("velocity", "v")],
          lambda c: {"param": exact(c["sgd"][0]), "grad": exact(c["sgd"][1]), "velocity": exact(c["sgd"][2])}),
    Entry("adam_step", "athena_mp_adam_step", ["n", 0.01, 0.9, 0.999, 1e-8, 3, 2, 0.0, 0.03, 1, IO("param", "p"), IO("grad", "g"), IO("m"), IO("v", "v2")],
          lambda c: {"param": exact(c["adam"][0]), "grad": Ref(c["adam"][1], "scratch"), "m": exact(c["adam"][2]), "v": exact(c["adam"][3])}),
    Entry("clip_min_max", "athena_mp_clip", ["n", IO("grad", "g3"), 1, -1.5, 2.0, 0, _HUGE], lambda c: {"grad": exact(c["clamp"])}),
    Entry("clip_norm", "athena_mp_clip", ["n", IO("grad", "g3"), 0, -_HUGE, _HUGE, 1, 10.0], lambda c: {"grad": Ref(c["norm"], "close", c["norm64"])}),
    Entry("mse_loss", "athena_mp_mse_loss", ["n", I("pred", "p"), I("expected", "e"), O("loss"), O("dpred")],
          lambda c: {"loss": Ref(c["loss"], "close", c["loss64"]), "dpred": exact(c["dpred"])}),
]


@pytest.mark.parametrize("entry,pl", cases(TRAIN))
def test_train_tail(dev, entry, pl):
    """what optim.py drives: the optimiser steps and the clamp bit for bit, the two reductions at 1e-5 anchored on float64"""
    run(dev, entry, _train_case(), pl)


# =====================================================================================================================================
# graph builders: the inputs and the output lists placed
# =====================================================================================================================================
def _radius_case():
    def build():
        from radius_reference import degree_radius, reference_pairs

        n, dim = 3000, 1                                   # the smallest cloud of test_radius_pairs_uniform_clouds
        p = np.random.Generator(np.random.PCG64(n + dim)).random((n, dim)).astype(np.float32)
        r = degree_radius(n, 6.0, dim)
        i, j, co = reference_pairs(p, r)
        pairs = np.ascontiguousarray(np.stack([i + 1, j + 1], axis=1).astype(np.int32))       # [E, 2] row-major = [2, E] column-major
        g = csr_from_index_list(n, pairs.T, self_loops=True)
        return {"n": n, "dim": dim, "points": p, "radius": r, "E": int(i.size), "pairs": pairs, "coords": co, "ia": g.adj_ia, "ja": g.adj_ja}
    return cached(("radius",), build)


def _count(c, state):
    state["count"] = C.c_int64(-1)
    return C.byref(state["count"])


def _count_is(key):
    def route(c, pl, state):
        assert state["count"].value == c[key]
    return route


RADIUS = [Entry("radius_pairs", "athena_mp_radius_pairs", ["n", "dim", I("points"), "radius", O("pairs"), O("coords"), "E", _count],
                lambda c: {"pairs": exact(c["pairs"]), "coords": exact(c["coords"])}, route=_count_is("E"))]


@pytest.mark.parametrize("entry,pl", cases(RADIUS))
def test_radius_pairs(dev, entry, pl):
    run(dev, entry, _radius_case(), pl)


@pytest.mark.parametrize("k", KS)
def test_handle_from_a_placed_device_edge_list(dev, k):
    """athena_mp_graph_create_from_edges_dev with the pair list at k: the adjacency it hands back and the handle's CSR against the
    host construction of the same list (graph_type.generate_adjacency + add_self_loops, numpy)"""
    import torch
    from athena_amd import DeviceGraph, _capi

    c = _radius_case()
    n, E = c["n"], c["E"]
    t = placed(c["pairs"], dev, k)
    ia = np.empty(n + 1, np.int32)
    ja = np.empty((2, 2 * E + n), np.int32, order="F")
    nnz, h = C.c_int64(), C.c_void_p()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _capi.use_torch_stream()
    _capi.call("athena_mp_graph_create_from_edges_dev", n, E, C.c_void_p(t.data_ptr()), 1, 1, vp(ia), vp(ja), ja.shape[1], C.byref(nnz), C.byref(h))
    try:
        torch.cuda.synchronize()
        got = DeviceGraph.borrow(h)
        assert np.array_equal(ia, c["ia"]) and np.array_equal(ja[:, :nnz.value], c["ja"])
        assert np.array_equal(got.export("rowptr"), c["ia"] - 1) and np.array_equal(got.export("col"), c["ja"][0] - 1)
        assert np.array_equal(got.export("eid"), c["ja"][1] - 1)
        assert np.array_equal(t.cpu().numpy(), c["pairs"])
    finally:
        _capi.call("athena_mp_graph_destroy", h)


def _periodic_case():
    def build():
        import periodic_reference as pr
        from test_gpu_periodic_graph import _fixture

        frac, lat, off = _fixture()                        # the fixture of test_fixture_equals_the_yardstick
        frac = np.ascontiguousarray(frac, np.float32).reshape(-1, 3)
        lat = np.ascontiguousarray(lat, np.float32).reshape(-1, 3, 3)
        off = np.ascontiguousarray(off, np.int32)
        want = pr.reference_edges(frac, lat, off, 0.5, 3.0)
        return {"B": lat.shape[0], "n": frac.shape[0], "off": off, "pbc": np.ones(3, np.int32), "frac": frac, "lat": lat, "want": want,
                "E": int(want["pairs"].shape[1])}
    return cached(("periodic",), build)


def _host(key):
    return lambda c, state: c[key].ctypes.data_as(C.c_void_p)


def _eoff(c, state):
    state["eoff"] = np.full(c["B"] + 1, -1, np.int64)
    return state["eoff"].ctypes.data_as(C.c_void_p)


def _periodic_route(c, pl, state):
    assert state["count"].value == c["E"] and np.array_equal(state["eoff"], c["want"]["edge_offsets"])


PERIODIC = [Entry("periodic_pairs", "athena_mp_periodic_pairs",
                  ["B", "n", _host("off"), I("frac"), I("lat"), _host("pbc"), 0.5, 3.0, O("pairs"), O("feature"), O("vec"), O("shift"), O("first_count"),
                   "E", _count, _eoff],
                  lambda c: {"pairs": exact(np.ascontiguousarray(c["want"]["pairs"].T)), "feature": exact(c["want"]["feature"]),
                             "vec": exact(c["want"]["vec"]), "shift": exact(c["want"]["shift"]), "first_count": exact(c["want"]["first_count"])},
                  route=_periodic_route)]


@pytest.mark.parametrize("entry,pl", cases(PERIODIC))
def test_periodic_pairs(dev, entry, pl):
    run(dev, entry, _periodic_case(), pl)


# =====================================================================================================================================
# two host-pointer entries with numpy views at an odd element offset
# =====================================================================================================================================
def _host_view(a, k):
    buf = np.full(a.size + 64, np.nan, np.float32)
    s = (-(buf.ctypes.data // 4)) % 4 + 16 + k             # k elements past a 16-byte boundary
    v = buf[s:s + a.size].reshape(a.shape)
    v[...] = a
    assert v.ctypes.data % 16 == (4 * k) % 16
    return buf, s, v


@pytest.mark.parametrize("k", [1, 3])
def test_host_pointer_entries_take_odd_offsets(dev, k):
    from athena_amd import _capi

    P_ = lambda a: a.ctypes.data_as(C.c_void_p)
    c = _kipf_case("hub", 7)
    _, _, x = _host_view(c["x"], k)
    ybuf, s, y = _host_view(np.zeros_like(c["x"]), k)
    ybuf[:] = np.nan
    _capi.call("athena_mp_kipf_propagate_fwd_host", c["g"].handle, 7, P_(x), P_(y))
    r = _fwd_ref(c)
    _compare(np.ascontiguousarray(y), r, "kipf_propagate_fwd_host")
    assert np.isnan(ybuf[:s]).all() and np.isnan(ybuf[s + y.size:]).all() and np.array_equal(x, c["x"])
    d = _dense_case(300, 7, 6)
    _, _, p = _host_view(d["P"], k)
    _, _, w = _host_view(d["W"], k)
    _, _, b = _host_view(d["bias"], k)
    zbuf, s, z = _host_view(np.zeros((300, 6), np.float32), k)
    zbuf[:] = np.nan
    _capi.call("athena_mp_gemm_fwd_host", 300, 7, 6, P_(p), P_(w), P_(b), 1, P_(z))
    _compare(np.ascontiguousarray(z), _f64ref(np.maximum(d["P"].astype(np.float64) @ d["Wt"] + d["bias"], 0)), "gemm_fwd_host")
    assert np.isnan(zbuf[:s]).all() and np.isnan(zbuf[s + z.size:]).all() and np.array_equal(p, d["P"]) and np.array_equal(w, d["W"])
