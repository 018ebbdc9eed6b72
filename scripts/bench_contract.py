#!/usr/bin/env python3
"""Times the graph contraction (athena_mp_contract_pairs, athena_amd/csrc/contract.hip) on pair lists that are resident in HBM, on
the MI355X:

  benchmark_graph   the pair list of the benchmark's graph (1 000 000 vertices, 4 500 000 uniform pairs, the draws of
                    synth.random_graph_csr) under a random map onto 65 536 clusters;
  knn_grid          the from_points_knn(k = 8) graph of one cloud of 1 000 000 uniform points under the cloud's own
                    from_grid_clusters map at 40 cells an axis, with the centroids as coarse positions.

Per case, after one warm-up call, the median of --repeats calls with min and max beside it, host clock around a call that ends in a
device synchronise, for each of: the size query, the fill (every output), the builder of the coarse handle, the builder of the
pooling handle; and for the torch route on the same input -- the relabelled keys, torch.unique(key, return_inverse=True,
return_counts=True) and a stable argsort of the inverse, which yields the coarse pairs, the counts and the members.  Beside the
times: the bytes the passes must move, from the shapes alone (12 B per edge and radix pass, 8 B per edge for the pair, 8 B for the
two gathers, and the outputs).  There is no pass/fail time.

  python scripts/bench_contract.py [--repeats 7] [--only CASE] [--out profiles/contract.json]
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

CASES = ("benchmark_graph", "knn_grid")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--only", choices=CASES)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contract.json"))
    a = ap.parse_args()
    import torch

    from athena_amd import DeviceGraph, _capi

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    _capi.use_torch_stream()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    want = lambda c: a.only in (None, c)
    records = []

    def timed(f, repeats):
        f()
        t = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return {"ms": round(statistics.median(t) * 1e3, 3), "ms_min": round(min(t) * 1e3, 3), "ms_max": round(max(t) * 1e3, 3)}

    def run(name, what, pairs, n, cluster, m, points):
        E = int(pairs.shape[0])
        dim = int(points.shape[1]) if points is not None else 0
        P, M = C.c_int64(), C.c_int64()
        head = (E, ptr(pairs), n, n, ptr(cluster), ptr(cluster), m, m, 0, dim, ptr(points), ptr(points))

        def query():
            _capi.call("athena_mp_contract_pairs", *head, 0, 0, None, None, None, None, None, None, C.byref(P), C.byref(M))

        t_query = timed(query, a.repeats)
        p, mm = int(P.value), int(M.value)
        coarse = torch.empty((p, 2), dtype=torch.int32, device=dev)
        rowptr = torch.empty((p + 1,), dtype=torch.int32, device=dev)
        members = torch.empty((mm, 2), dtype=torch.int32, device=dev)
        weights = torch.empty((mm,), dtype=torch.float32, device=dev)
        edge_pair = torch.empty((E,), dtype=torch.int32, device=dev)
        coords = torch.empty((p, dim), dtype=torch.float32, device=dev) if dim else None

        def fill():
            _capi.call("athena_mp_contract_pairs", *head, p, mm, ptr(coarse), ptr(rowptr), ptr(members), ptr(weights), ptr(edge_pair), ptr(coords),
                       C.byref(P), C.byref(M))

        t_fill = timed(fill, a.repeats)
        stats = np.zeros(4, np.int64)
        _capi.call("athena_mp_contract_stats", vp(stats))
        lib = _capi.load()

        def coarse_builder():
            h, nnz, ia = C.c_void_p(), C.c_int64(), np.empty(m + 1, np.int32)
            _capi.call("athena_mp_graph_create_from_edges_dev", m, p, ptr(coarse), 0, 1, vp(ia), None, 0, C.byref(nnz), C.byref(h))
            lib.athena_mp_graph_destroy(h)

        def pool_builder():
            h, ia = C.c_void_p(), np.empty(p + 1, np.int32)
            _capi.call("athena_mp_graph_create_bipartite_dev", p, E, mm, ptr(members), vp(ia), None, 0, C.byref(h))
            lib.athena_mp_graph_destroy(h)

        t_coarse, t_pool = timed(coarse_builder, a.repeats), timed(pool_builder, a.repeats)
        passes = 1 if stats[2] <= 8 else int((stats[2] + 7) // 8)
        moved = passes * 12 * E + 8 * E + 8 * E + 8 * p + 4 * (p + 1) + 8 * mm + 4 * mm + 4 * E + 4 * dim * p
        rec = {"case": name, "what": what, "vertices": n, "pairs": E, "clusters": m, "coarse_pairs": p, "members": mm, "key_bits": int(stats[2]),
               "radix_passes": passes, "largest_coarse_pair": int(stats[3]), "bytes_the_passes_must_move": int(moved),
               "size_query": t_query, "fill": t_fill, "coarse_handle_builder": t_coarse, "pool_handle_builder": t_pool,
               "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
        if not a.no_torch:
            cl0 = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), cluster.to(torch.int64)])

            def route():
                u, v = pairs[:, 0].to(torch.int64), pairs[:, 1].to(torch.int64)
                ca, cb = cl0[u], cl0[v]
                keep = (ca > 0) & (cb > 0) & (ca != cb)
                lo, hi = torch.minimum(ca, cb)[keep], torch.maximum(ca, cb)[keep]
                uniq, inverse, counts = torch.unique(lo * (m + 1) + hi, return_inverse=True, return_counts=True)
                order = torch.argsort(inverse, stable=True)
                return uniq, counts, order

            t_torch = timed(route, a.repeats)
            uniq, counts, order = route()
            same = bool(uniq.numel() == p and torch.equal(uniq, coarse[:, 0].to(torch.int64) * (m + 1) + coarse[:, 1].to(torch.int64))
                        and torch.equal(counts.to(torch.int32), rowptr[1:] - rowptr[:-1]))
            rec.update(torch_route=t_torch, torch_route_gives_the_same_coarse_pairs_and_counts=same)
        print(json.dumps(rec), flush=True)
        records.append(rec)

    n = a.points
    if want("benchmark_graph"):
        E = 4500000
        rng = np.random.Generator(np.random.PCG64(20260424))                   # synth.random_graph_csr's draws
        u = rng.integers(0, n, E, dtype=np.int64)
        v = rng.integers(0, n - 1, E, dtype=np.int64)
        v = v + (v >= u)
        pairs = torch.from_numpy(np.stack([u + 1, v + 1], axis=1).astype(np.int32)).to(dev)
        m = 65536
        cluster = torch.from_numpy(np.random.Generator(np.random.PCG64(18)).integers(1, m + 1, n).astype(np.int32)).to(dev)
        run("benchmark_graph", f"the benchmark's {n} vertices and {E} uniform pairs under a random map onto {m} clusters", pairs, n, cluster, m, None)
    if want("knn_grid"):
        pts = torch.from_numpy(np.random.Generator(np.random.PCG64(17)).random((n, 3)).astype(np.float32)).to(dev)
        fine = DeviceGraph.from_points_knn(pts, 8)[0]
        grid, centroid, coff, cluster, _ = DeviceGraph.from_grid_clusters(pts, 1.0 / 40)
        pairs = fine.pair_list()
        run("knn_grid", f"the k = 8 nearest-neighbour graph (union) of {n} uniform points under its voxel-grid map, 40 cells an axis", pairs, n,
            cluster, grid.n_rows, centroid)
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
