#!/usr/bin/env python3
"""Times the k-nearest-neighbour builder (athena_mp_knn_pairs_batched, athena_amd/csrc/knn_graph.hip) on points that are resident
in HBM, on the MI355X, at k = 8 and 16 (mode union, no cap), on three inputs:

  uniform   one cloud of 1 000 000 points uniform in the unit cube;
  graded    one cloud of 1 000 000 points with coordinates u^4, u uniform: the density varies by orders of magnitude, the case a
            fixed radius serves badly;
  batch     3 000 clouds of 4 to 29 points in the unit cube.

Beside each case, in the same run and alternating with it:

  radius    the radius builder (athena_mp_radius_pairs; athena_mp_radius_pairs_batched for the batch) at the radius that gives
            the same number of pairs, found by bisection on its size query; size query + fill, as its callers use it;
  host      the route without a device builder: points to the host, scipy cKDTree build + query (k + 1, all cores the process
            may use), the union pair list and p_i - p_j in numpy, pairs and coords uploaded.  Once per case.

After one warm-up build, the median of --repeats builds; host clock around a call that ends in a device synchronise.  One JSON
record per case with milliseconds per build, queries per second, candidates examined and cells visited per query (from
athena_mp_knn_stats) and the two other routes' times.  There is no pass/fail time.

  python scripts/bench_knn_graph.py [--repeats 5] [--points 1000000] [--only uniform|graded|batch] [--out profiles/knn_graph.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(only, n):
    rng = np.random.Generator(np.random.PCG64(8))
    if only in (None, "uniform"):
        yield "uniform", rng.random((n, 3)).astype(np.float32), np.array([0, n], np.int32), f"one cloud of {n} points uniform in the unit cube"
    if only in (None, "graded"):
        yield "graded", (rng.random((n, 3)) ** 4).astype(np.float32), np.array([0, n], np.int32), f"one cloud of {n} points, coordinates u^4"
    if only in (None, "batch"):
        off = np.concatenate([[0], np.cumsum(rng.integers(4, 30, 3000))]).astype(np.int32)
        yield "batch", rng.random((int(off[-1]), 3)).astype(np.float32), off, "3000 clouds of 4 to 29 points in the unit cube"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--only", choices=("uniform", "graded", "batch"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_graph.json"), help="'-': print only")
    a = ap.parse_args()

    import torch
    from scipy.spatial import cKDTree

    from athena_amd import _capi

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    _capi.use_torch_stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    workers = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1
    workers = min(workers, int(os.environ.get("OMP_NUM_THREADS", workers)))
    records = []

    for name, p, off, what in inputs(a.only, a.points):
        n, B = p.shape[0], off.size - 1
        pts = torch.from_numpy(p).to(dev)
        for k in (8, 16):
            T = n * k
            pairs = torch.empty((T, 2), dtype=torch.int32, device=dev)
            coords = torch.empty((T, 3), dtype=torch.float32, device=dev)
            eoff = np.empty(B + 1, np.int64)
            E = C.c_int64()

            def knn():
                t0 = time.perf_counter()
                _capi.call("athena_mp_knn_pairs_batched", B, n, vp(off), 3, ptr(pts), k, float("inf"), 0, None, ptr(pairs), ptr(coords), T,
                           vp(eoff), C.byref(E))
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            def radius_count(r):
                c = C.c_int64()
                if B == 1:
                    _capi.call("athena_mp_radius_pairs", n, 3, ptr(pts), float(r), None, None, 0, C.byref(c))
                else:
                    _capi.call("athena_mp_radius_pairs_batched", B, n, vp(off), 3, ptr(pts), float(r), None, None, 0, None, C.byref(c))
                return c.value

            knn()
            target = E.value
            stats = np.zeros(4, np.int64)
            _capi.call("athena_mp_knn_stats", vp(stats))
            # the radius with (as nearly as fp32 radii allow) the same number of pairs: grown from far below, so that no count pass
            # runs at a radius much above the one looked for (a count pass costs what it counts), then bisected
            def at_least(r):
                try:
                    return radius_count(r) >= target
                except _capi.AthenaMPError:                  # more pairs than a CSR holds
                    return True

            r = float((2.0 * target / n / (n / B) / (4.0 / 3.0 * np.pi)) ** (1.0 / 3.0)) / 1024.0    # 2^-10 of the uniform-density radius
            while not at_least(r):
                r *= 2.0
            lo, hi = 0.5 * r, r
            for _ in range(25):
                mid = 0.5 * (lo + hi)
                if at_least(mid):
                    hi = mid
                else:
                    lo = mid
            r = hi
            r_pairs = radius_count(r)
            rp = torch.empty((r_pairs, 2), dtype=torch.int32, device=dev)
            rc = torch.empty((r_pairs, 3), dtype=torch.float32, device=dev)

            def radius():
                t0 = time.perf_counter()
                c = C.c_int64()
                if B == 1:
                    _capi.call("athena_mp_radius_pairs", n, 3, ptr(pts), float(r), None, None, 0, C.byref(c))
                    _capi.call("athena_mp_radius_pairs", n, 3, ptr(pts), float(r), ptr(rp), ptr(rc), r_pairs, C.byref(c))
                else:
                    _capi.call("athena_mp_radius_pairs_batched", B, n, vp(off), 3, ptr(pts), float(r), None, None, 0, None, C.byref(c))
                    _capi.call("athena_mp_radius_pairs_batched", B, n, vp(off), 3, ptr(pts), float(r), ptr(rp), ptr(rc), r_pairs, None,
                               C.byref(c))
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            def host():
                t0 = time.perf_counter()
                ph = pts.cpu().numpy()
                p64 = ph.astype(np.float64)
                keys = []
                for b in range(B):
                    m = int(off[b + 1] - off[b])
                    if m < 2:
                        continue
                    q = p64[off[b]:off[b + 1]]
                    _, near = cKDTree(q).query(q, min(k, m - 1) + 1, workers=workers if B == 1 else 1)
                    i = np.repeat(np.arange(m, dtype=np.int64), near.shape[1] - 1) + off[b]
                    j = near[:, 1:].reshape(-1).astype(np.int64) + off[b]
                    keys.append(np.minimum(i, j) * n + np.maximum(i, j))
                key = np.unique(np.concatenate(keys))
                i, j = key // n, key % n
                hp = torch.from_numpy(np.stack([i + 1, j + 1], 1).astype(np.int32)).to(dev)
                hc = torch.from_numpy(ph[i] - ph[j]).to(dev)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, int(hp.shape[0])

            radius()
            t_knn, t_rad = [], []
            for _ in range(a.repeats):
                t_knn.append(knn())
                t_rad.append(radius())
            t_host, host_pairs = host()
            ms = statistics.median(t_knn) * 1e3
            rec = {"case": name, "what": what, "points": n, "clouds": B, "k": k, "mode": "union", "pairs": int(target),
                   "knn_ms_per_build": round(ms, 3), "knn_ms_min": round(min(t_knn) * 1e3, 3), "knn_ms_max": round(max(t_knn) * 1e3, 3),
                   "queries_per_second": round(n / (ms * 1e-3)), "candidates_per_query": round(float(stats[1]) / n, 2),
                   "cells_per_query": round(float(stats[2]) / n, 2), "largest_shell": int(stats[3]),
                   "radius_same_pairs": {"radius": r, "pairs": int(r_pairs), "ms_per_build": round(statistics.median(t_rad) * 1e3, 3),
                                         "what": "size query + fill"},
                   "host_ckdtree": {"pairs": host_pairs, "ms": round(t_host * 1e3, 1), "workers": workers if B == 1 else 1,
                                    "what": "points D2H + cKDTree build + query + union in numpy + pairs and coords H2D, once"},
                   "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del pairs, coords, rp, rc
        del pts
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
