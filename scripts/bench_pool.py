#!/usr/bin/env python3
"""Times max pooling over a two-set k-nearest-neighbour handle (athena_amd/csrc/pool.hip) on arrays that are resident in HBM, on the
MI355X, at k = 8 in three dimensions, on the two rectangular cases of bench_interp.py:

  encoder   the 64^3 grid points (queries) against 1 000 000 mesh points (sources): a mesh onto a latent grid -- set abstraction;
  decoder   1 000 000 queries against the 64^3 points of a regular grid;

each at F = 64 and F = 128.  Per launch -- fwd, edges_fwd, bwd_x, bwd_edges -- the time and the achieved bytes per second over the
ALGORITHMIC bytes, computed here from the shapes and counted as bench_interp.py counts them:

  fwd         E * 4 for the column ids + 4 F * (the distinct rows of x read + the rows of y written + the rows of arg written)
  edges_fwd   E * 8 for column and edge ids + 4 F * (E rows of h read + the rows of y and of arg written)
  bwd_x       E * 4 for the row ids + 4 F * (the distinct rows of arg and of dy read + the rows of dx written)
  bwd_edges   E * 8 for column and edge ids + 4 F * (the distinct rows of arg and of dy read + E rows of dh written)

Beside them, in the same run and alternating with them:
  - athena_mp_interp_fwd / athena_mp_interp_bwd_x at the same shape (E * 12 for ids and weights + 4 F * (rows read + rows written)):
    the forward moves the same rows without weights, plus one arg row per output row;
  - the route a user has without these entries, torch index arithmetic on the pair list: x[col], then scatter_reduce_ with amax
    (atomics); for the reverse a comparison pass and index_add_ (a tie gets the gradient once per tied entry).

A sample is --launches launches between two device events; after one warm-up sample, the median of --repeats samples with min and
max beside it.  There is no pass/fail time.

  python scripts/bench_pool.py [--repeats 5] [--launches 20] [--points 1000000] [--only CASE] [--out profiles/pool.json]
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

CASES = ("encoder", "decoder")
HBM_PEAK = 8.0e12                                  # bytes per second, MI355X


def lattice(m):
    g = (np.arange(m, dtype=np.float64) + 0.5) / m
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--only", choices=CASES, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool.json"), help="'-': print only")
    a = ap.parse_args()

    import torch

    from athena_amd import DeviceGraph, _capi

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    _capi.use_torch_stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    k, dim, eps, records = 8, 3, 1e-16, []
    rng = np.random.Generator(np.random.PCG64(12))

    def sample(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.launches):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.launches                       # ms per launch

    def timed(fns):
        """{name: [ms per launch] * repeats}: one warm-up sample of each, then the samples alternating"""
        for fn in fns.values():
            sample(fn)
        out = {n: [] for n in fns}
        for _ in range(a.repeats):
            for n, fn in fns.items():
                out[n].append(sample(fn))
        return out

    def summary(ms, nbytes=None):
        med = statistics.median(ms)
        rec = {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
        if nbytes is not None:
            rate = nbytes / (med * 1e-3)
            rec.update({"algorithmic_bytes": int(nbytes), "bytes_per_second": round(rate), "share_of_8_TB_per_s": round(rate / HBM_PEAK, 3)})
        return rec

    for case in CASES:
        if a.only not in (None, case):
            continue
        cloud, grid = rng.random((a.points, 3)).astype(np.float32), lattice(a.grid)
        q, s = (cloud, grid) if case == "decoder" else (grid, cloud)
        g, coords, _ = DeviceGraph.from_point_sets_knn(q, s, k)
        nq, ns, E = g.n_rows, g.n_cols, g.n_edge_cols
        rowptr, col, eid = g.export("rowptr"), g.export("col"), g.export("eid")
        rows = np.repeat(np.arange(nq, dtype=np.int64), np.diff(rowptr))
        row_of, col_of = torch.from_numpy(rows).to(dev), torch.from_numpy(col.astype(np.int64)).to(dev)
        entry_of_edge = np.empty(E, np.int64)
        entry_of_edge[eid] = np.arange(E)
        rows_used, cols_used = int((np.diff(rowptr) > 0).sum()), int(np.unique(col).size)
        w = torch.empty((E,), dtype=torch.float32, device=dev)
        _capi.call("athena_mp_interp_weights", g.handle, dim, ptr(coords), eps, ptr(w), None)
        for F in (64, 128):
            x = torch.from_numpy(rng.standard_normal((ns, F)).astype(np.float32)).to(dev)
            dy = torch.from_numpy(rng.standard_normal((nq, F)).astype(np.float32)).to(dev)
            h = x[torch.from_numpy(col[entry_of_edge].astype(np.int64)).to(dev)].contiguous()       # h[e] = x[the source of edge e]
            y, yh, yi = (torch.empty((nq, F), dtype=torch.float32, device=dev) for _ in range(3))
            arg, argh = (torch.empty((nq, F), dtype=torch.int32, device=dev) for _ in range(2))
            dx, dxi = (torch.empty((ns, F), dtype=torch.float32, device=dev) for _ in range(2))
            dh = torch.empty((E, F), dtype=torch.float32, device=dev)
            index = row_of[:, None].expand(-1, F)

            def fwd():
                _capi.call("athena_mp_pool_max_fwd", g.handle, F, ptr(x), ptr(y), ptr(arg))

            def edges_fwd():
                _capi.call("athena_mp_pool_max_edges_fwd", g.handle, F, ptr(h), ptr(yh), ptr(argh))

            def bwd_x():
                _capi.call("athena_mp_pool_max_bwd_x", g.handle, F, ptr(arg), ptr(dy), ptr(dx))

            def bwd_edges():
                _capi.call("athena_mp_pool_max_bwd_edges", g.handle, F, ptr(argh), ptr(dy), ptr(dh))

            def interp_fwd():
                _capi.call("athena_mp_interp_fwd", g.handle, F, ptr(w), ptr(x), ptr(yi))

            def interp_bwd_x():
                _capi.call("athena_mp_interp_bwd_x", g.handle, F, ptr(w), ptr(dy), ptr(dxi))

            def torch_fwd():
                out = torch.empty((nq, F), dtype=torch.float32, device=dev)
                return out.scatter_reduce_(0, index, x[col_of], "amax", include_self=False)

            def torch_bwd_x():
                hit = x[col_of] == y[row_of]                                                          # the comparison pass
                return torch.zeros((ns, F), dtype=torch.float32, device=dev).index_add_(0, col_of, dy[row_of] * hit)

            fwd()
            edges_fwd()
            bwd_x()
            bwd_edges()
            torch.cuda.synchronize()
            filled = torch.from_numpy(np.diff(rowptr) > 0).to(dev)
            same_y = bool(torch.equal(torch_fwd()[filled], y[filled])) and bool(torch.equal(yh, y)) and bool(torch.equal(argh, arg))
            t = timed({"fwd": fwd, "interp_fwd": interp_fwd, "torch_fwd": torch_fwd, "edges_fwd": edges_fwd, "bwd_x": bwd_x,
                       "interp_bwd_x": interp_bwd_x, "torch_bwd_x": torch_bwd_x, "bwd_edges": bwd_edges})
            med = lambda n: statistics.median(t[n])
            rec = {"case": case, "queries": nq, "sources": ns, "k": k, "F": F, "pairs": E, "distinct_sources_read": cols_used,
                   "distinct_queries_read": rows_used,
                   "fwd": summary(t["fwd"], E * 4 + 4 * F * (cols_used + 2 * nq)),
                   "edges_fwd": summary(t["edges_fwd"], E * 8 + 4 * F * (E + 2 * nq)),
                   "bwd_x": summary(t["bwd_x"], E * 4 + 4 * F * (2 * rows_used + ns)),
                   "bwd_edges": summary(t["bwd_edges"], E * 8 + 4 * F * (2 * rows_used + E)),
                   "interp_fwd": summary(t["interp_fwd"], E * 12 + 4 * F * (cols_used + nq)),
                   "interp_bwd_x": summary(t["interp_bwd_x"], E * 12 + 4 * F * (rows_used + ns)),
                   "torch_fwd": summary(t["torch_fwd"]), "torch_bwd_x": summary(t["torch_bwd_x"]),
                   "fwd_vs_interp_fwd": round(med("fwd") / med("interp_fwd"), 2),
                   "bwd_x_vs_interp_bwd_x": round(med("bwd_x") / med("interp_bwd_x"), 2),
                   "torch_vs_fwd": round(med("torch_fwd") / med("fwd"), 2), "torch_vs_bwd_x": round(med("torch_bwd_x") / med("bwd_x"), 2),
                   "y_equals_torch_amax_and_the_edge_form": same_y, "launches_per_sample": a.launches, "repeats": a.repeats,
                   "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del x, dy, h, y, yh, yi, arg, argh, dx, dxi, dh, index
        g.close()
        del coords, w, row_of, col_of
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
