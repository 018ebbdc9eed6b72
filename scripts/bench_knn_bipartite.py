#!/usr/bin/env python3
"""Times the two-set k-nearest-neighbour builder (athena_mp_knn_pairs_bipartite, athena_amd/csrc/knn_bipartite.hip) on points that
are resident in HBM, on the MI355X, at k = 8 in three dimensions, on four inputs:

  uniform   1 000 000 queries against 1 000 000 sources, both uniform in the unit cube;
  encoder   the 64^3 points of a regular grid (queries) against 1 000 000 mesh points (sources): a mesh onto a latent grid;
  decoder   1 000 000 queries against the 64^3 grid: a latent grid onto the points the user chooses;
  outside   1 000 000 queries uniform in [-0.25, 1.25]^3 against 1 000 000 sources in the unit cube, once without a cap -- the
            documented price of the one-axis stop rule: a query d cells outside the source box walks about d shells -- and once
            capped at the radius inside which a source has 8 others on average.

One search into buffers of n_queries * k pairs (pairs and coords), as DeviceGraph.from_point_sets_knn runs it.  Beside each case, in
the same run and alternating with it:

  one_set   athena_mp_knn_pairs on the same SOURCES at the same k (union, no cap): the search cost per query of the one-set
            builder, the figure the two-set search is read against;
  host      the route without a device builder: both sets to the host, scipy cKDTree of the sources, query of k (all cores the
            process may use), rows ordered by source index and q_i - p_j in numpy, pairs and coords uploaded.  Once per case.

After one warm-up build, the median of --repeats builds with min and max beside it; host clock around a call that ends in a device
synchronise.  One JSON record per case with milliseconds per build, candidates examined and cells visited per query and the largest
shell (athena_mp_knn_stats), and the two ratios.  There is no pass/fail time.

  python scripts/bench_knn_bipartite.py [--repeats 5] [--points 1000000] [--only CASE] [--out profiles/knn_bipartite.json]
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

CASES = ("uniform", "encoder", "decoder", "outside", "outside_capped")


def lattice(m):
    g = (np.arange(m, dtype=np.float64) + 0.5) / m
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def inputs(only, n):
    """(case, queries, sources, radius or None, description)"""
    rng = np.random.Generator(np.random.PCG64(9))
    cloud = lambda: rng.random((n, 3)).astype(np.float32)
    want = lambda c: only in (None, c)
    if want("uniform"):
        yield "uniform", cloud(), cloud(), None, f"{n} queries against {n} sources, both uniform in the unit cube"
    if want("encoder"):
        yield "encoder", lattice(64), cloud(), None, f"the 64^3 points of a regular grid against {n} mesh points"
    if want("decoder"):
        yield "decoder", cloud(), lattice(64), None, f"{n} queries against the 64^3 points of a regular grid"
    if want("outside") or want("outside_capped"):
        q, s = (rng.random((n, 3)) * 1.5 - 0.25).astype(np.float32), cloud()
        if want("outside"):
            yield "outside", q, s, None, f"{n} queries uniform in [-0.25, 1.25]^3 against {n} sources in the unit cube, no cap"
        if want("outside_capped"):
            r = float((8.0 / (n * 4.0 / 3.0 * np.pi)) ** (1.0 / 3.0))
            yield "outside_capped", q, s, r, f"the same, capped at radius {r:.5f}: 8 sources inside it on average"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--only", choices=CASES, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bipartite.json"), help="'-': print only")
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
    k, records = 8, []

    for name, q, s, r, what in inputs(a.only, a.points):
        nq, ns = q.shape[0], s.shape[0]
        qd, sd = torch.from_numpy(q).to(dev), torch.from_numpy(s).to(dev)
        qoff, soff = np.array([0, nq], np.int32), np.array([0, ns], np.int32)
        T, T1 = nq * k, ns * k
        pairs = torch.empty((T, 2), dtype=torch.int32, device=dev)
        coords = torch.empty((T, 3), dtype=torch.float32, device=dev)
        pairs1 = torch.empty((T1, 2), dtype=torch.int32, device=dev)
        coords1 = torch.empty((T1, 3), dtype=torch.float32, device=dev)
        E, E1 = C.c_int64(), C.c_int64()

        def two_sets():
            t0 = time.perf_counter()
            _capi.call("athena_mp_knn_pairs_bipartite", 1, nq, vp(qoff), ns, vp(soff), 3, ptr(qd), ptr(sd), k,
                       float("inf") if r is None else r, None, None, ptr(pairs), ptr(coords), T, None, None, C.byref(E))
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def one_set():
            t0 = time.perf_counter()
            _capi.call("athena_mp_knn_pairs", ns, 3, ptr(sd), k, float("inf"), 0, None, ptr(pairs1), ptr(coords1), T1, C.byref(E1))
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def host():
            t0 = time.perf_counter()
            qh, sh = qd.cpu().numpy(), sd.cpu().numpy()
            dist, near = cKDTree(sh.astype(np.float64)).query(qh.astype(np.float64), k, workers=workers,
                                                                **({} if r is None else {"distance_upper_bound": r}))
            near = np.sort(np.where(np.isfinite(dist), near, ns), axis=1)          # rows by source index; ns = no partner
            i = np.repeat(np.arange(nq, dtype=np.int64), k)
            j = near.reshape(-1).astype(np.int64)
            i, j = i[j < ns], j[j < ns]
            hp = torch.from_numpy(np.stack([i + 1, j + 1], 1).astype(np.int32)).to(dev)
            hc = torch.from_numpy(qh[i] - sh[j]).to(dev)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, int(hp.shape[0])

        two_sets()
        stats = np.zeros(4, np.int64)
        _capi.call("athena_mp_knn_stats", vp(stats))
        one_set()
        stats1 = np.zeros(4, np.int64)
        _capi.call("athena_mp_knn_stats", vp(stats1))
        t_two, t_one = [], []
        for _ in range(a.repeats):
            t_two.append(two_sets())
            t_one.append(one_set())
        t_host, host_pairs = host()
        ms, ms1 = statistics.median(t_two) * 1e3, statistics.median(t_one) * 1e3
        rec = {"case": name, "what": what, "queries": nq, "sources": ns, "k": k, "radius": r, "pairs": int(E.value),
               "ms_per_build": round(ms, 3), "ms_min": round(min(t_two) * 1e3, 3), "ms_max": round(max(t_two) * 1e3, 3),
               "queries_per_second": round(nq / (ms * 1e-3)), "candidates_per_query": round(float(stats[1]) / nq, 2),
               "cells_per_query": round(float(stats[2]) / nq, 2), "largest_shell": int(stats[3]),
               "one_set_same_sources": {"ms_per_build": round(ms1, 3), "ms_min": round(min(t_one) * 1e3, 3),
                                        "ms_max": round(max(t_one) * 1e3, 3), "pairs": int(E1.value),
                                        "candidates_per_query": round(float(stats1[1]) / ns, 2),
                                        "what": "athena_mp_knn_pairs on the sources, union, no cap"},
               "per_query_vs_one_set": round((ms / nq) / (ms1 / ns), 3),
               "host_ckdtree": {"pairs": host_pairs, "ms": round(t_host * 1e3, 1), "workers": workers,
                                "what": "both sets D2H + cKDTree of the sources + query + rows by index in numpy + pairs and coords H2D, once"},
               "host_vs_device": round(t_host * 1e3 / ms, 1), "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del pairs, coords, pairs1, coords1, qd, sd
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
