#!/usr/bin/env python3
"""Times the two-set radius builder (athena_mp_radius_pairs_bipartite + athena_mp_graph_create_bipartite_dev,
athena_amd/csrc/bipartite_graph.hip) on points that are resident in HBM, on the MI355X, on two inputs:

  uniform   1 000 000 sources and 1 000 000 queries uniform in the unit cube, the radius for a mean of about 8 partners per query;
  encoder   1 000 000 mesh points (uniform in the unit cube) onto a 64^3 regular grid of queries, radius 1.5 grid spacings: the
            first layer of a GNO / GINO model.

For each, in the same run and alternating:

  search    size query + fill (pairs, coords), as DeviceGraph.from_point_sets calls it;
  handle    athena_mp_graph_create_bipartite_dev on the pair list in HBM;
  both      DeviceGraph.from_point_sets, the two together;
  one_set   what a user without this builder does for the same graph: DeviceGraph.from_points-style search on the concatenated set
            [queries | sources] (athena_mp_radius_pairs, size query + fill), the pair list and coords to the host, the query-query
            and source-source pairs dropped and the rest renumbered in numpy, athena_mp_graph_create with explicit degrees.

After one warm-up of each, the median, minimum and maximum of --repeats runs; host clock around a call that ends in a device
synchronise.  One JSON record per input.  There is no pass/fail time.

  python scripts/bench_radius_bipartite.py [--repeats 5] [--points 1000000] [--only uniform|encoder] [--out profiles/radius_bipartite.json]
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
    rng = np.random.Generator(np.random.PCG64(9))
    if only in (None, "uniform"):
        r = float((8.0 / (n * 4.0 / 3.0 * np.pi)) ** (1.0 / 3.0))
        yield ("uniform", rng.random((n, 3)).astype(np.float32), rng.random((n, 3)).astype(np.float32), r,
               f"{n} queries and {n} sources uniform in the unit cube, about 8 partners per query")
    if only in (None, "encoder"):
        g = (np.arange(64, dtype=np.float32) + np.float32(0.5)) / np.float32(64)
        q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
        yield ("encoder", q, rng.random((n, 3)).astype(np.float32), 1.5 / 64,
               f"{n} mesh points onto a 64^3 grid of queries, radius 1.5 grid spacings")


def spread(t):
    return {"ms": round(statistics.median(t) * 1e3, 3), "ms_min": round(min(t) * 1e3, 3), "ms_max": round(max(t) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--only", choices=("uniform", "encoder"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_bipartite.json"), help="'-': print only")
    a = ap.parse_args()

    import torch

    from athena_amd import DeviceGraph, _capi

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    _capi.use_torch_stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    records = []

    for name, q, s, r, what in inputs(a.only, a.points):
        nq, ns = q.shape[0], s.shape[0]
        qd, sd = torch.from_numpy(q).to(dev), torch.from_numpy(s).to(dev)
        cat = torch.cat([qd, sd])
        qoff, soff = np.array([0, nq], np.int32), np.array([0, ns], np.int32)
        head = (1, nq, vp(qoff), ns, vp(soff), 3, ptr(qd), ptr(sd), float(r))
        E = C.c_int64()
        _capi.call("athena_mp_radius_pairs_bipartite", *head, None, None, 0, None, None, C.byref(E))
        pairs = torch.empty((E.value, 2), dtype=torch.int32, device=dev)
        coords = torch.empty((E.value, 3), dtype=torch.float32, device=dev)
        ia = np.empty(nq + 1, np.int32)

        def search():
            t0 = time.perf_counter()
            c = C.c_int64()
            _capi.call("athena_mp_radius_pairs_bipartite", *head, None, None, 0, None, None, C.byref(c))
            _capi.call("athena_mp_radius_pairs_bipartite", *head, ptr(pairs), ptr(coords), E.value, None, None, C.byref(c))
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def handle():
            h = C.c_void_p()
            t0 = time.perf_counter()
            _capi.call("athena_mp_graph_create_bipartite_dev", nq, ns, E.value, ptr(pairs), vp(ia), None, 0, C.byref(h))
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            _capi.call("athena_mp_graph_destroy", h)
            return t

        def both():
            t0 = time.perf_counter()
            g, c, _ = DeviceGraph.from_point_sets(qd, sd, r)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            g.close()
            return t

        def one_set():
            t0 = time.perf_counter()
            n = nq + ns
            c = C.c_int64()
            _capi.call("athena_mp_radius_pairs", n, 3, ptr(cat), float(r), None, None, 0, C.byref(c))
            p1 = torch.empty((c.value, 2), dtype=torch.int32, device=dev)
            c1 = torch.empty((c.value, 3), dtype=torch.float32, device=dev)
            _capi.call("athena_mp_radius_pairs", n, 3, ptr(cat), float(r), ptr(p1), ptr(c1), c.value, C.byref(c))
            ph, ch = p1.cpu().numpy(), c1.cpu().numpy()
            keep = (ph[:, 0] <= nq) & (ph[:, 1] > nq)            # i < j and the queries come first: a query with a source
            i, j = ph[keep, 0].astype(np.int64) - 1, ph[keep, 1].astype(np.int64) - 1 - nq
            hia = np.concatenate([[1], 1 + np.cumsum(np.bincount(i, minlength=nq))]).astype(np.int32)
            hja = np.asfortranarray(np.stack([j + 1, np.arange(1, i.size + 1)]).astype(np.int32))
            g = DeviceGraph(hia, hja, n_cols=ns, n_edge_cols=i.size, row_deg=np.bincount(i, minlength=nq),
                            col_deg=np.bincount(j, minlength=ns))
            hc = torch.from_numpy(np.ascontiguousarray(ch[keep])).to(dev)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            g.close()
            return t, int(c.value), int(i.size)

        search(); handle(); both()
        _, all_pairs, kept = one_set()
        assert kept == E.value, "the one-set route must end at the same graph"
        t = {"search": [], "handle": [], "both": [], "one_set": []}
        for _ in range(a.repeats):
            t["search"].append(search())
            t["handle"].append(handle())
            t["both"].append(both())
            t["one_set"].append(one_set()[0])
        rec = {"case": name, "what": what, "queries": nq, "sources": ns, "radius": r, "pairs": int(E.value),
               "partners_per_query": round(E.value / nq, 2), "search": spread(t["search"]), "handle": spread(t["handle"]),
               "both": spread(t["both"]),
               "one_set_route": dict(spread(t["one_set"]), pairs_of_the_concatenated_set=all_pairs,
                                     what="athena_mp_radius_pairs on [queries | sources] (size query + fill), pairs and coords D2H, "
                                          "filter and renumber in numpy, athena_mp_graph_create, coords H2D"),
               "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del pairs, coords, qd, sd, cat
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
