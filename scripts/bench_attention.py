#!/usr/bin/env python3
"""Times attention pooling over a two-set k-nearest-neighbour handle (athena_amd/csrc/attention.hip) on arrays that are resident in
HBM, on the MI355X: 1 000 000 queries against 1 000 000 sources, k = 16 in three dimensions, F = 64, H in (1, 4, 64) -- one weight
per edge, multi-head attention, vector attention.  Per launch -- softmax_fwd, gather_fwd, gather_edges_fwd, bwd_x, bwd_edges,
bwd_alpha in both forms, softmax_bwd: nine with the two gathers counted apart -- the time and the achieved bytes per second over the
ALGORITHMIC bytes, computed here from the shapes (E pairs, every array read or written once, 4 bytes per id):

  softmax_fwd       E * 4 for the edge ids + 4 H * 2 E                      (the kernel reads scores three times: the caches' business)
  gather_fwd        E * 8 for column and edge ids + 4 H * E for alpha + 4 F * (the distinct rows of x read + the rows of y written)
  gather_edges_fwd  E * 4 + 4 H * E + 4 F * (E rows of h read + the rows of y written)
  bwd_x             E * 8 + 4 H * E + 4 F * (the distinct rows of dy read + the rows of dx written)
  bwd_edges         E * 4 + 4 H * E + 4 F * (the distinct rows of dy read + E rows of dh written)
  bwd_alpha (x)     E * 8 + 4 H * E + 4 F * (the distinct rows of x and of dy read)
  bwd_alpha (h)     E * 4 + 4 H * E + 4 F * (E rows of h + the distinct rows of dy read)
  softmax_bwd       E * 4 + 4 H * 3 E

Beside them, in the same run and alternating with them:
  - the yardsticks, existing kernels that move the same rows on the same handle: athena_mp_interp_fwd beside gather_fwd at H = 1
    (E * 12 for ids and weights + 4 F * (rows read + rows written)) and athena_mp_pool_max_edges_fwd beside gather_edges_fwd
    (E * 8 + 4 F * (E + the rows of y and of arg written)); each yardstick is timed TWICE under two names, and the difference of the
    two medians is the run-to-run spread a difference between a gather and its yardstick has to exceed;
  - the route a user has without these entries, torch on the pair list: scatter_reduce_ amax, exp, index_add_, a division and an
    indexed multiply for the forward (vertex form); the indexed products, a sum over each head's columns and two index_add_ for the
    reverse.  Its sums are atomic: nothing that comes back is bit-defined.

A sample is --launches launches between two device events (torch: --torch-launches); after one warm-up sample, the median of
--repeats samples with min and max beside it.  There is no pass/fail time.

  python scripts/bench_attention.py [--repeats 5] [--launches 10] [--points 1000000] [--out profiles/attention.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                                  # bytes per second, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--torch-launches", type=int, default=2)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention.json"), help="'-': print only")
    a = ap.parse_args()

    import torch

    from athena_amd import DeviceGraph, _capi

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    _capi.use_torch_stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    k, F, records = 16, 64, []
    rng = np.random.Generator(np.random.PCG64(14))

    def sample(fn, launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(launches):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / launches                         # ms per launch

    def timed(fns):
        """{name: [ms per launch] * repeats}: one warm-up sample of each, then the samples alternating"""
        n_of = lambda n: a.torch_launches if n.startswith("torch") else a.launches
        for n, fn in fns.items():
            sample(fn, n_of(n))
        out = {n: [] for n in fns}
        for _ in range(a.repeats):
            for n, fn in fns.items():
                out[n].append(sample(fn, n_of(n)))
        return out

    def summary(ms, nbytes=None):
        med = statistics.median(ms)
        rec = {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
        if nbytes is not None:
            rate = nbytes / (med * 1e-3)
            rec.update({"algorithmic_bytes": int(nbytes), "bytes_per_second": round(rate), "share_of_8_TB_per_s": round(rate / HBM_PEAK, 3)})
        return rec

    q, s = rng.random((a.points, 3)).astype(np.float32), rng.random((a.points, 3)).astype(np.float32)
    g, coords, _ = DeviceGraph.from_point_sets_knn(q, s, k)
    del coords
    nq, ns, E = g.n_rows, g.n_cols, g.n_edge_cols
    rowptr, col, eid = g.export("rowptr"), g.export("col"), g.export("eid")
    entry_of_edge = np.empty(E, np.int64)
    entry_of_edge[eid] = np.arange(E)
    rows = np.repeat(np.arange(nq, dtype=np.int64), np.diff(rowptr))
    row_e, col_e = torch.from_numpy(rows[entry_of_edge]).to(dev), torch.from_numpy(col.astype(np.int64)[entry_of_edge]).to(dev)
    rows_used, cols_used = int((np.diff(rowptr) > 0).sum()), int(np.unique(col).size)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    x = torch.from_numpy(rng.standard_normal((ns, F)).astype(np.float32)).to(dev)
    dy = torch.from_numpy(rng.standard_normal((nq, F)).astype(np.float32)).to(dev)
    h = torch.randn((E, F), dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(14))
    y, yh, yi, yp = f32(nq, F), f32(nq, F), f32(nq, F), f32(nq, F)
    argp = torch.empty((nq, F), dtype=torch.int32, device=dev)
    dx, dh = f32(ns, F), f32(E, F)

    for H in (1, 4, 64):
        Cw = F // H
        scores = torch.from_numpy((3.0 * rng.standard_normal((E, H))).astype(np.float32)).to(dev)
        alpha, dalpha, dalpha_h, dscores = f32(E, H), f32(E, H), f32(E, H), f32(E, H)
        call = lambda entry, *args: _capi.call("athena_mp_" + entry, g.handle, *args)
        fns = {
            "softmax_fwd": lambda: call("attn_softmax_fwd", H, ptr(scores), ptr(alpha)),
            "gather_fwd": lambda: call("attn_gather_fwd", F, H, ptr(alpha), ptr(x), ptr(y)),
            "gather_edges_fwd": lambda: call("attn_gather_edges_fwd", F, H, ptr(alpha), ptr(h), ptr(yh)),
            "bwd_x": lambda: call("attn_gather_bwd_x", F, H, ptr(alpha), ptr(dy), ptr(dx)),
            "bwd_edges": lambda: call("attn_gather_bwd_edges", F, H, ptr(alpha), ptr(dy), ptr(dh)),
            "bwd_alpha_x": lambda: call("attn_gather_bwd_alpha", F, H, ptr(x), None, ptr(dy), ptr(dalpha)),
            "bwd_alpha_h": lambda: call("attn_gather_bwd_alpha", F, H, None, ptr(h), ptr(dy), ptr(dalpha_h)),
            "softmax_bwd": lambda: call("attn_softmax_bwd", H, ptr(alpha), ptr(dalpha), ptr(dscores)),
            "pool_max_edges_fwd": lambda: call("pool_max_edges_fwd", F, ptr(h), ptr(yp), ptr(argp)),
            "pool_max_edges_fwd_again": lambda: call("pool_max_edges_fwd", F, ptr(h), ptr(yp), ptr(argp)),
        }
        if H == 1:
            fns["interp_fwd"] = lambda: call("interp_fwd", F, ptr(alpha), ptr(x), ptr(yi))
            fns["interp_fwd_again"] = lambda: call("interp_fwd", F, ptr(alpha), ptr(x), ptr(yi))
        index = row_e[:, None].expand(-1, H)

        def torch_fwd():
            m = torch.full((nq, H), -np.inf, dtype=torch.float32, device=dev).scatter_reduce_(0, index, scores, "amax", include_self=True)
            p = torch.exp(scores - m[row_e])
            a_ = p / torch.zeros((nq, H), dtype=torch.float32, device=dev).index_add_(0, row_e, p)[row_e]
            out = torch.zeros((nq, F), dtype=torch.float32, device=dev).index_add_(0, row_e, a_.repeat_interleave(Cw, 1) * x[col_e])
            return a_, out

        def torch_bwd():
            v, gr = x[col_e], dy[row_e]
            tdx = torch.zeros((ns, F), dtype=torch.float32, device=dev).index_add_(0, col_e, alpha.repeat_interleave(Cw, 1) * gr)
            da = (gr * v).view(E, H, Cw).sum(2)
            dot = torch.zeros((nq, H), dtype=torch.float32, device=dev).index_add_(0, row_e, alpha * da)
            return tdx, alpha * (da - dot[row_e])

        fns["torch_fwd"], fns["torch_bwd"] = torch_fwd, torch_bwd
        for n in ("softmax_fwd", "gather_fwd", "bwd_x", "bwd_alpha_x", "softmax_bwd"):
            fns[n]()
        torch.cuda.synchronize()
        ta, ty = torch_fwd()
        tdx, tds = torch_bwd()
        filled = torch.from_numpy(np.diff(rowptr) > 0).to(dev)
        close = lambda u, w: float((u - w).abs().max() / w.abs().max().clamp_min(1e-30))
        agreement = {"alpha": close(ta, alpha), "y": close(ty[filled], y[filled]), "dx": close(tdx, dx), "dscores": close(tds, dscores)}
        del ta, ty, tdx, tds
        t = timed(fns)
        med = lambda n: statistics.median(t[n])
        nbytes = {"softmax_fwd": E * 4 + 4 * H * 2 * E, "gather_fwd": E * 8 + 4 * H * E + 4 * F * (cols_used + nq),
                  "gather_edges_fwd": E * 4 + 4 * H * E + 4 * F * (E + nq), "bwd_x": E * 8 + 4 * H * E + 4 * F * (rows_used + ns),
                  "bwd_edges": E * 4 + 4 * H * E + 4 * F * (rows_used + E), "bwd_alpha_x": E * 8 + 4 * H * E + 4 * F * (cols_used + rows_used),
                  "bwd_alpha_h": E * 4 + 4 * H * E + 4 * F * (E + rows_used), "softmax_bwd": E * 4 + 4 * H * 3 * E,
                  "pool_max_edges_fwd": E * 8 + 4 * F * (E + 2 * nq), "pool_max_edges_fwd_again": E * 8 + 4 * F * (E + 2 * nq),
                  "interp_fwd": E * 12 + 4 * F * (cols_used + nq), "interp_fwd_again": E * 12 + 4 * F * (cols_used + nq)}
        rec = {"queries": nq, "sources": ns, "k": k, "F": F, "H": H, "pairs": E, "distinct_sources_read": cols_used,
               "distinct_queries_read": rows_used}
        for n in fns:
            rec[n] = summary(t[n], nbytes.get(n))
        forward = med("softmax_fwd") + med("gather_fwd")
        reverse = med("bwd_x") + med("bwd_alpha_x") + med("softmax_bwd")
        rec.update({"forward_ms_x_form": round(forward, 4), "reverse_ms_x_form": round(reverse, 4),
                    "torch_vs_forward": round(med("torch_fwd") / forward, 2), "torch_vs_reverse": round(med("torch_bwd") / reverse, 2),
                    "gather_edges_fwd_vs_pool_max_edges_fwd": round(med("gather_edges_fwd") / med("pool_max_edges_fwd"), 3),
                    "pool_max_edges_fwd_spread": round(abs(med("pool_max_edges_fwd_again") / med("pool_max_edges_fwd") - 1), 4)})
        if H == 1:
            rec.update({"gather_fwd_vs_interp_fwd": round(med("gather_fwd") / med("interp_fwd"), 3),
                        "interp_fwd_spread": round(abs(med("interp_fwd_again") / med("interp_fwd") - 1), 4),
                        "gather_fwd_bytes_equal_interp_fwd": bool(torch.equal(y.view(torch.int32), yi.view(torch.int32)))})
        rec.update({"max_difference_from_torch_relative_to_the_largest_element": agreement, "launches_per_sample": a.launches,
                    "torch_launches_per_sample": a.torch_launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)})
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del scores, alpha, dalpha, dalpha_h, dscores, index, fns
    g.close()
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
