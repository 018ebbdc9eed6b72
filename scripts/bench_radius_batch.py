#!/usr/bin/env python3
"""Times the construction of ONE block-diagonal radius graph from a batch of point clouds that are resident in HBM, three ways
in ONE run on the MI355X, alternating, on two datasets:

  meshes     2 000 clouds x 1 000 points uniform in the unit cube, radius for mean degree 15;
  molecules  130 000 clouds of 4 to 29 points (clip(round(N(18, 3)), 4, 29)) in the unit cube, radius for mean degree about 4.

  batched    DeviceGraph.from_point_clouds: athena_mp_radius_pairs_batched (size query + fill) and
             athena_mp_graph_create_from_edges_dev -- the pair list never leaves HBM; result: handle + coords on the device;
  per-cloud  the route without the batched entry that still searches on the device: DeviceGraph.from_points(want_adjacency=True)
             per cloud, the adjacencies downloaded, io.batch_graphs on the host, the batch uploaded (DeviceGraph), the coords
             concatenated on the device.  One call per cloud: on the molecules dataset it runs over the first --loop-clouds clouds
             only and the line says so (the time for all clouds is NOT measured; the line gives seconds per cloud);
  host       a host pair search per cloud (scipy cKDTree.query_pairs on the downloaded points), the differences p_i - p_j,
             DeviceGraph.from_edges and the upload of coords.

After one warm-up build of each, the median of --repeats builds, host clock around a call that ends in a device synchronise.
No threshold: the batched route is the only one that keeps the list in HBM and is kept whatever the others cost.

  python scripts/bench_radius_batch.py [--repeats 3] [--loop-clouds 4000] [--only meshes|molecules] [--out profiles/radius_batch_build.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def degree_radius(n, mean_degree):
    return float((mean_degree / (n * 4.0 / 3.0 * np.pi)) ** (1.0 / 3.0))


def datasets(only):
    rng = np.random.Generator(np.random.PCG64(4))
    out = []
    if only in (None, "meshes"):
        sizes = np.full(2000, 1000, np.int64)
        out.append(("meshes", sizes, degree_radius(1000, 15.0), "2000 clouds x 1000 points, radius for mean degree 15"))
    if only in (None, "molecules"):
        sizes = np.clip(np.rint(rng.normal(18.0, 3.0, 130_000)), 4, 29).astype(np.int64)
        out.append(("molecules", sizes, degree_radius(18, 4.0), "130000 clouds of 4 to 29 points, radius for mean degree about 4"))
    for name, sizes, r, what in out:
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        p = rng.random((int(off[-1]), 3)).astype(np.float32)
        yield name, off, p, r, what


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-clouds", type=int, default=4000, help="clouds the per-cloud route runs over when the dataset has more")
    ap.add_argument("--only", choices=("meshes", "molecules"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_batch_build.txt"), help="'-': print only")
    a = ap.parse_args()

    import torch
    from scipy.spatial import cKDTree

    from athena_amd import DeviceGraph, _capi, io
    from athena_amd.graph import graph_type

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    lines = [f"# scripts/bench_radius_batch.py on {torch.cuda.get_device_name(0)}: points uniform in the unit cube (PCG64(4), fp32), resident in HBM",
             f"# warm-up build of each route, then the routes alternating, median of {a.repeats}; host clock around a call that ends in a "
             "device synchronise; seconds"]

    for name, off, p, r, what in datasets(a.only):
        B, n = off.size - 1, p.shape[0]
        pts = torch.from_numpy(p).to(dev)
        torch.cuda.synchronize()
        K = min(B, a.loop_clouds)

        def batched():
            t0 = time.perf_counter()
            g, coords, _, _ = DeviceGraph.from_point_clouds(pts, off, r)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, g, coords

        def per_cloud():
            t0 = time.perf_counter()
            graphs, coords = [], []
            for b in range(K):
                h, c, ia, ja = DeviceGraph.from_points(pts[off[b]:off[b + 1]], r, want_adjacency=True)
                h.close()
                g = graph_type.from_csr(ia, ja, num_edges=int(c.shape[0]))
                g.vertex_features = np.zeros((g.num_vertices, 0), np.float32)
                g.edge_features = np.zeros((g.num_edges, 0), np.float32)
                graphs.append(g)
                coords.append(c)
            ia, ja, _, _, _ = io.batch_graphs(graphs)
            E = sum(g.num_edges for g in graphs)
            g = DeviceGraph(ia, ja, n_edge_cols=E)
            coords = torch.cat(coords)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, g, coords

        def host():
            t0 = time.perf_counter()
            ph = pts.cpu().numpy()
            p64 = ph.astype(np.float64)
            ii, jj = [], []
            for b in range(B):
                if off[b + 1] - off[b] < 2:
                    continue
                pr = cKDTree(p64[off[b]:off[b + 1]]).query_pairs(r, output_type="ndarray")
                ii.append(pr[:, 0] + off[b])
                jj.append(pr[:, 1] + off[b])
            i, j = np.concatenate(ii), np.concatenate(jj)
            coords = torch.from_numpy(ph[i] - ph[j]).to(dev)
            idx = np.empty((2, i.size), np.int32, order="F")
            idx[0] = i + 1
            idx[1] = j + 1
            g = DeviceGraph.from_edges(n, idx)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, g, coords

        routes = (("batched", batched), ("per-cloud", per_cloud), ("host", host))
        times = {k: [] for k, _ in routes}
        sizes = {}
        for rep in range(a.repeats + 1):
            for k, fn in routes:
                t, g, coords = fn()
                sizes[k] = (int(coords.shape[0]), g.nnz)
                g.close()
                del coords
                if rep:
                    times[k].append(t)
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append(f"{name}: {what}; {n} points, radius {r:.6g}")
        lines.append(f"  batched    DeviceGraph.from_point_clouds (points in HBM -> handle + coords in HBM)        median {med['batched']:.4f}   "
                     f"min {min(times['batched']):.4f}  max {max(times['batched']):.4f}   pairs {sizes['batched'][0]}  CSR entries {sizes['batched'][1]}")
        scope = "all clouds" if K == B else f"the FIRST {K} of {B} clouds only; all clouds not measured"
        lines.append(f"  per-cloud  from_points(want_adjacency) per cloud + io.batch_graphs + upload, {scope}   median {med['per-cloud']:.4f}   "
                     f"min {min(times['per-cloud']):.4f}  max {max(times['per-cloud']):.4f}   {med['per-cloud'] / K * 1e3:.4f} ms per cloud   pairs {sizes['per-cloud'][0]}")
        lines.append(f"  host       points D2H + cKDTree.query_pairs per cloud + DeviceGraph.from_edges + coords H2D   median {med['host']:.4f}   "
                     f"min {min(times['host']):.4f}  max {max(times['host']):.4f}   pairs {sizes['host'][0]} (float64 on the bound against fp32)")
        del pts
    text = "\n".join(lines)
    print(text)
    if a.out != "-":
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
