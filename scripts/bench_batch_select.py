#!/usr/bin/env python3
"""Times what one training step pays to get its mini-batch out of a BASELINE configs[2]-shaped dataset (130 k periodic structures of
8 - 30 atoms, scripts/bench_periodic_graph.py's generator) whose graph was built on the device, for batches of 2 000 and 32 000
structures, three ways in ONE run on the MI355X, alternating, a new random selection every repetition (the same one for all routes):

  (a) select   DeviceDataset.select (athena_mp_batch_select) + the three gathers a step needs (x [n, 6], feature [E], vec [E, 3]);
  (b) rebuild  the device route without the selection: the selected coordinates gathered on the device, then
               DeviceGraph.from_structures on them (neighbour search, sort, CSR build again) + the gather of x;
  (c) host     the host route without it: the dataset's pair list sliced and renumbered in numpy, DeviceGraph.from_edges, and the
               upload of the batch's x, feature and vec.

Separately: the forward pass of the example's Duvenaud layer (F_v 6, F_e 1, T = 4, degrees 1 .. 10, 10 outputs) on a FRESH child
-- where the lazily built degree buckets and tiles show -- and the second forward pass on the same child.

Medians of --repeats (at least 20) repetitions after a warm-up of each route; host clock around work that ends in a device
synchronise.  (a) and (c) give the same handle arrays, (b) the same too: compared once per batch size.

  python scripts/bench_batch_select.py [--structures 130000] [--repeats 20] [--out profiles/batch_select.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=130_000)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 32000])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_select.txt"), help="'-': print only")
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats must be at least 20")

    import torch

    import batch_reference as br
    from athena_amd import DeviceDataset, DeviceGraph, _capi
    from athena_amd.layers import duvenaud_msgpass_layer_type
    from bench_periodic_graph import make_batch

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    B, cmin, cmax, Fv = a.structures, 0.5, 3.0, 6
    frac, lat, off = make_batch(B)
    n = int(off[-1])
    fd, ld = torch.from_numpy(frac).to(dev), torch.from_numpy(lat).to(dev)
    t0 = time.perf_counter()
    handle, feature, vec, voff, eoff = DeviceGraph.from_structures(fd, ld, off, cmin, cmax)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    ds = DeviceDataset(handle, voff, eoff)
    torch.cuda.synchronize()
    t_plan = time.perf_counter() - t0
    E = int(eoff[-1])
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).uniform(-1, 1, (n, Fv)).astype(np.float32)).to(dev)
    # what the host route holds: the dataset's pair list and per-edge / per-vertex arrays on the host
    pairs = br.pairs_of_arrays({k: handle.export(k) for k in ("e_rowptr", "e_row", "e_entry", "col")}, E).astype(np.int64)
    feature_h, vec_h, x_h = feature.cpu().numpy(), vec.cpu().numpy(), x.cpu().numpy()
    off64, sizes, esizes = off.astype(np.int64), np.diff(off).astype(np.int64), np.diff(eoff)

    def ranges(start, count):
        """concatenated aranges [start[k], start[k] + count[k]) and the base of each in the concatenation"""
        base = np.concatenate([[0], np.cumsum(count)])
        return np.repeat(start - base[:-1], count) + np.arange(base[-1]), base

    def route_select(sel):
        t0 = time.perf_counter()
        b = ds.select(sel)
        out = (b.take_vertices(x), b.take_edges(feature), b.take_edges(vec))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, b.handle, out

    def route_rebuild(sel):
        t0 = time.perf_counter()
        rows, base = ranges(off64[sel], sizes[sel])
        rows_d = torch.from_numpy(rows).to(dev)
        sel_d = torch.from_numpy(sel.astype(np.int64)).to(dev)
        g, f_b, v_b, _, _ = DeviceGraph.from_structures(fd.index_select(0, rows_d), ld.index_select(0, sel_d), base.astype(np.int32), cmin, cmax)
        out = (x.index_select(0, rows_d), f_b, v_b)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, g, out

    def route_host(sel):
        t0 = time.perf_counter()
        rows, base = ranges(off64[sel], sizes[sel])
        cols, _ = ranges(eoff[sel], esizes[sel])
        shift = np.repeat(base[:-1] - off64[sel], esizes[sel])
        cp = np.asfortranarray((pairs[:, cols] + shift).astype(np.int32))
        g = DeviceGraph.from_edges(int(base[-1]), cp)
        out = (torch.from_numpy(x_h[rows]).to(dev), torch.from_numpy(feature_h[cols]).to(dev), torch.from_numpy(vec_h[cols]).to(dev))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, g, out

    routes = (("(a) select + 3 gathers", route_select), ("(b) from_structures on the selection", route_rebuild),
              ("(c) numpy slice + from_edges + uploads", route_host))
    layer = duvenaud_msgpass_layer_type(num_vertex_features=[Fv], num_edge_features=[1], num_time_steps=4, max_vertex_degree=10,
                                        num_outputs=10, min_vertex_degree=1, seed=3)
    lines = [f"# scripts/bench_batch_select.py on {torch.cuda.get_device_name(0)}: dataset of {B} structures of 8 - 30 atoms ({n} atoms, {E} edges, "
             f"{handle.nnz} CSR entries), cutoffs {cmin:g} / {cmax:g}",
             f"# warm-up of each route, then medians of {a.repeats} repetitions, the routes alternating, a new shuffled selection per repetition; "
             "host clock around work that ends in a device synchronise; milliseconds",
             f"once per dataset: DeviceGraph.from_structures {1e3 * t_build:.2f}   DeviceDataset (plan: check kernel + tables) {1e3 * t_plan:.2f}"]
    for m in a.batches:
        m = min(m, B)
        rng = np.random.default_rng(m)
        sel = rng.permutation(B)[:m].astype(np.int32)
        built = [fn(sel) for _, fn in routes]                               # warm-up, and the three results compared
        for k in ("rowptr", "col", "eid", "t_src", "e_entry"):
            ref = built[0][1].export(k)
            assert all(np.array_equal(ref, r[1].export(k)) for r in built[1:]), f"the routes built different handles ({k})"
        for i in range(3):
            assert all(torch.equal(built[0][2][i], r[2][i]) for r in built[1:]), "the routes gathered different tensors"
        for r in built:
            r[1].close()
        del built
        times = [[] for _ in routes]
        first, second = [], []
        for rep in range(a.repeats):
            sel = rng.permutation(B)[:m].astype(np.int32)
            for k, (_, fn) in enumerate(routes):
                t, g, out = fn(sel)
                times[k].append(t)
                if k == 0:                                                   # the layer's first and second forward pass on the fresh child
                    vo = np.concatenate([[0], np.cumsum(sizes[sel])]).astype(np.int32)
                    e = out[1][:, None].contiguous()
                    torch.cuda.synchronize()
                    for acc in (first, second):
                        t0 = time.perf_counter()
                        layer.set_graph_handle(g, vo)
                        layer.forward(out[0], e)
                        torch.cuda.synchronize()
                        acc.append(time.perf_counter() - t0)
                g.close()
                del out
        med = [statistics.median(t) for t in times]
        lines.append(f"batch of {m} structures")
        for (name, _), t, md in zip(routes, times, med):
            lines.append(f"  {name:<42s} median {1e3 * md:9.3f}   min {1e3 * min(t):9.3f}   max {1e3 * max(t):9.3f}")
        lines.append(f"  (a) / (b) = {med[0] / med[1]:.4f}   (a) / (c) = {med[0] / med[2]:.4f}")
        lines.append(f"  Duvenaud layer forward (T = 4) on the fresh child: first pass median {1e3 * statistics.median(first):.3f}   "
                     f"second pass median {1e3 * statistics.median(second):.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
