#!/usr/bin/env python3
"""Times the construction of BASELINE configs[3]'s radius graph (2 M points uniform in the unit cube, mean degree 15) from
points that are resident in HBM, two ways in ONE run on the MI355X:

  device   DeviceGraph.from_points: athena_mp_radius_pairs (size query + fill) and athena_mp_graph_create_from_edges_dev --
           the pair list never leaves HBM; result: handle + coords on the device;
  host     the best route without the device builder: the points copied to the host, a k-d tree pair search there
           (scipy cKDTree.query_pairs, what synth.radius_graph does), the differences p_i - p_j, then
           DeviceGraph.from_edges and the upload of coords; result: handle + coords on the device.

After one warm-up build of each, the median of --repeats builds, host clock around a call that ends in a device synchronise.
The two routes number the pairs differently (lexicographic against the tree's traversal order); the pair SETS are compared.

  python scripts/bench_radius_graph.py [--points 2000000] [--repeats 5] [--out profiles/radius_graph_build.txt]
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_radius_graph.py --device-only --repeats 2 --out -
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--degree", type=float, default=15.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device-only", action="store_true", help="skip the host route (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_graph_build.txt"), help="'-': print only")
    a = ap.parse_args()

    import torch

    from athena_amd import DeviceGraph, _capi

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    n = a.points
    p = np.random.Generator(np.random.PCG64(4)).random((n, 3)).astype(np.float32)
    r = float((a.degree / (n * 4.0 / 3.0 * np.pi)) ** (1.0 / 3.0))
    pts = torch.from_numpy(p).to(dev)
    torch.cuda.synchronize()

    def device_route():
        t0 = time.perf_counter()
        g, coords = DeviceGraph.from_points(pts, r)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, g, coords

    def host_route():
        from scipy.spatial import cKDTree

        t0 = time.perf_counter()
        ph = pts.cpu().numpy()
        t1 = time.perf_counter()
        pairs = cKDTree(ph.astype(np.float64)).query_pairs(r, output_type="ndarray")
        t2 = time.perf_counter()
        i, j = pairs[:, 0], pairs[:, 1]
        coords = torch.from_numpy(ph[i] - ph[j]).to(dev)
        idx = np.empty((2, i.size), np.int32, order="F")
        idx[0] = i + 1
        idx[1] = j + 1
        g = DeviceGraph.from_edges(n, idx)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return (t3 - t0, t1 - t0, t2 - t1, t3 - t2), g, coords, pairs

    lines = [f"# scripts/bench_radius_graph.py on {torch.cuda.get_device_name(0)}: {n} points uniform in the unit cube (PCG64(4), fp32), "
             f"radius {r:.6g} (mean degree {a.degree:g})",
             f"# warm-up build, then median of {a.repeats}; host clock around a call that ends in a device synchronise; seconds"]
    _, g, coords = device_route()
    E, nnz = int(coords.shape[0]), g.nnz
    dev_key = None
    if not a.device_only:
        ja = g.export("col").astype(np.int64)
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(g.export("rowptr")))
        dev_key = np.sort(rows[rows < ja] * n + ja[rows < ja])
    g.close()
    del coords
    td = []
    for _ in range(a.repeats):
        t, g, coords = device_route()
        td.append(t)
        g.close()
        del coords
    lines.append(f"pairs {E}  CSR entries {nnz}")
    lines.append(f"device route  DeviceGraph.from_points (points in HBM -> handle + coords in HBM)   median {statistics.median(td):.4f}   "
                 f"min {min(td):.4f}  max {max(td):.4f}")
    if not a.device_only:
        _, g, coords, pairs = host_route()
        lo, hi = pairs.min(1).astype(np.int64), pairs.max(1).astype(np.int64)
        host_key = np.sort(lo * n + hi)
        # the tree decides in float64 on the exact radius, the device in fp32: the sets may differ in borderline pairs only
        diff = np.setxor1d(host_key, dev_key, assume_unique=True).size
        g.close()
        del coords, pairs, host_key, dev_key
        th = []
        for _ in range(a.repeats):
            t, g, coords, _ = host_route()
            th.append(t)
            g.close()
            del coords
        tot = [t[0] for t in th]
        k = tot.index(sorted(tot)[len(tot) // 2])
        lines.append(f"host route    points D2H + cKDTree.query_pairs + DeviceGraph.from_edges + coords H2D      median {statistics.median(tot):.4f}   "
                     f"min {min(tot):.4f}  max {max(tot):.4f}")
        lines.append(f"              of the median run: D2H {th[k][1]:.4f}  pair search {th[k][2]:.4f}  differences + handle + upload {th[k][3]:.4f}")
        lines.append(f"pairs in one route's set and not the other's (float64 against fp32 on the bound): {diff}")
        lines.append(f"device route / host route = {statistics.median(td) / statistics.median(tot):.5f}")
        assert statistics.median(td) <= statistics.median(tot), "the device route is slower than the host route"
    text = "\n".join(lines)
    print(text)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
