#!/usr/bin/env python3
"""Times inverse-distance interpolation over a two-set k-nearest-neighbour handle (athena_amd/csrc/interp.hip) on arrays that are
resident in HBM, on the MI355X, at k = 8 in three dimensions, on the two rectangular cases of bench_knn_bipartite.py:

  decoder   1 000 000 queries against the 64^3 points of a regular grid: a latent grid onto the points the user chooses;
  encoder   the 64^3 grid points (queries) against 1 000 000 mesh points (sources): a mesh onto a latent grid;

each at F = 64 and F = 128.  Per launch -- weights, fwd, bwd_x, bwd_coords -- the time and the achieved bytes per second over the
ALGORITHMIC bytes, computed here from the shapes:

  fwd / bwd_x   E * (8 + 4) for ids and weights + 4 F * (the distinct rows read + the rows written)
  weights       E * (4 + 4 dim + 4) for the edge id, coords and the weight written + 4 * n_rows for wsum
  bwd_coords    E * (8 + 4 + 4 dim + 4 dim) for ids, weight, coords and dcoords + 4 F * the distinct rows of x, y and dy read

Beside the gathers, in the same run and alternating with them, the route a user has without this entry: torch index arithmetic on the
pair list, x[col] * a[:, None] and index_add_ (atomics: results differ from run to run).

A sample is --launches launches between two device events; after one warm-up sample, the median of --repeats samples with min and
max beside it.  There is no pass/fail time.

  python scripts/bench_interp.py [--repeats 5] [--launches 20] [--points 1000000] [--only CASE] [--out profiles/interp.json]
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

CASES = ("decoder", "encoder")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp.json"), help="'-': print only")
    a = ap.parse_args()

    import torch

    from athena_amd import DeviceGraph, _capi

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    _capi.use_torch_stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    k, dim, eps, records = 8, 3, 1e-16, []
    rng = np.random.Generator(np.random.PCG64(11))

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
        rowptr, col = g.export("rowptr"), g.export("col")
        row_of = torch.from_numpy(np.repeat(np.arange(nq, dtype=np.int64), np.diff(rowptr))).to(dev)
        col_of = torch.from_numpy(col.astype(np.int64)).to(dev)
        rows_used, cols_used = int((np.diff(rowptr) > 0).sum()), int(np.unique(col).size)
        w = torch.empty((E,), dtype=torch.float32, device=dev)
        wsum = torch.empty((nq,), dtype=torch.float32, device=dev)
        dc = torch.empty((E, dim), dtype=torch.float32, device=dev)

        def weights():
            _capi.call("athena_mp_interp_weights", g.handle, dim, ptr(coords), eps, ptr(w), ptr(wsum))

        weights()
        for F in (64, 128):
            x = torch.from_numpy(rng.standard_normal((ns, F)).astype(np.float32)).to(dev)
            dy = torch.from_numpy(rng.standard_normal((nq, F)).astype(np.float32)).to(dev)
            y, dx = torch.empty((nq, F), dtype=torch.float32, device=dev), torch.empty((ns, F), dtype=torch.float32, device=dev)

            def fwd():
                _capi.call("athena_mp_interp_fwd", g.handle, F, ptr(w), ptr(x), ptr(y))

            def bwd_x():
                _capi.call("athena_mp_interp_bwd_x", g.handle, F, ptr(w), ptr(dy), ptr(dx))

            def bwd_coords():
                _capi.call("athena_mp_interp_bwd_coords", g.handle, dim, F, ptr(coords), eps, ptr(w), ptr(x), ptr(y), ptr(dy), ptr(dc))

            def torch_fwd():
                return torch.zeros((nq, F), dtype=torch.float32, device=dev).index_add_(0, row_of, x[col_of] * w[:, None])

            def torch_bwd_x():
                return torch.zeros((ns, F), dtype=torch.float32, device=dev).index_add_(0, col_of, dy[row_of] * w[:, None])

            fwd()
            bwd_x()
            worst = max(float((torch_fwd() - y).abs().max()), float((torch_bwd_x() - dx).abs().max()))
            t = timed({"weights": weights, "fwd": fwd, "torch_fwd": torch_fwd, "bwd_x": bwd_x, "torch_bwd_x": torch_bwd_x,
                       "bwd_coords": bwd_coords})
            b_fwd = E * 12 + 4 * F * (cols_used + nq)
            b_bwd = E * 12 + 4 * F * (rows_used + ns)
            rec = {"case": case, "queries": nq, "sources": ns, "k": k, "F": F, "pairs": E, "distinct_sources_read": cols_used,
                   "distinct_queries_read": rows_used,
                   "fwd": summary(t["fwd"], b_fwd), "bwd_x": summary(t["bwd_x"], b_bwd),
                   "weights": summary(t["weights"], E * (8 + 4 * dim) + 4 * nq),
                   "bwd_coords": summary(t["bwd_coords"], E * (12 + 8 * dim) + 4 * F * (cols_used + 2 * rows_used)),
                   "torch_fwd": summary(t["torch_fwd"]), "torch_bwd_x": summary(t["torch_bwd_x"]),
                   "torch_vs_fwd": round(statistics.median(t["torch_fwd"]) / statistics.median(t["fwd"]), 2),
                   "torch_vs_bwd_x": round(statistics.median(t["torch_bwd_x"]) / statistics.median(t["bwd_x"]), 2),
                   "worst_abs_difference_from_torch": worst, "launches_per_sample": a.launches, "repeats": a.repeats,
                   "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del x, dy, y, dx
        g.close()
        del coords, w, wsum, dc, row_of, col_of
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
