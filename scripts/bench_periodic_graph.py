#!/usr/bin/env python3
"""Times the construction of the neighbour graphs of a BASELINE configs[2]-shaped batch -- 130 k periodic structures of 8 - 30
atoms, half in cubic and half in skewed cells, cutoffs 0.5 / 3.0 as in get_graph_from_basis -- two ways in ONE run on the MI355X:

  device   DeviceGraph.from_structures: athena_mp_periodic_pairs (size query + fill) and athena_mp_graph_create_from_edges_dev --
           the pair list never leaves HBM; result: one block-diagonal handle + feature + vec on the device;
  host     the best route without the device builder: the pair-and-image search on the host (the vectorised numpy yardstick of
           tests/periodic_reference.py over the sufficient shift range, structure by structure), the batch's pair list assembled,
           then DeviceGraph.from_edges and the upload of feature and vec; result: the same handle and tensors.

After one warm-up build of each, the median of --repeats (device) / --host-repeats (host) builds, host clock around a call that ends
in a device synchronise.  The two routes use one definition: the arrays are compared for equality.

The large-cell leg (--large-cells: that leg alone, appended to --out) times athena_mp_periodic_pairs (size query + fill of every
output) on single cubic structures of 128 ... 32 768 atoms at the density of 4096 atoms in a cell of edge 38.4 (the edge grows
with the cube root of the atom count) and on a batch of 64 structures of 1000 atoms, with ATHENA_MP_PERIODIC_ROUTE = walk and
= grid pinned in turn, alternating in one process; the arrays of the two routes are compared, and athena_mp_periodic_stats of
each build is printed.  It is what kGridAtoms of periodic_graph.hip, the automatic threshold between the routes, rests on.

  python scripts/bench_periodic_graph.py [--structures 130000] [--repeats 5] [--host-repeats 1] [--out profiles/periodic_graph_build.txt]
  python scripts/bench_periodic_graph.py --large-cells [--repeats 5]         (appends to --out)
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_periodic_graph.py --device-only --repeats 2 --out -
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_batch(B, seed=2):
    """B structures of 8 - 30 atoms: even ones in cubic cells (edge 4.3 - 8), odd ones in sheared cells of the same volume range"""
    rng = np.random.Generator(np.random.PCG64(seed))
    sizes = rng.integers(8, 31, B)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    frac = rng.random((int(off[-1]), 3)).astype(np.float32)
    edge = rng.uniform(4.3, 8.0, B)
    lat = np.zeros((B, 3, 3))
    lat[:, 0, 0] = lat[:, 1, 1] = lat[:, 2, 2] = edge
    shear = rng.uniform(-0.6, 0.6, (B, 3)) * edge[:, None]
    odd = np.arange(B) % 2 == 1
    lat[odd, 1, 0], lat[odd, 2, 0], lat[odd, 2, 1] = shear[odd, 0], shear[odd, 1], shear[odd, 2]
    return frac, lat.astype(np.float32), off


LARGE_SIZES = (128, 256, 512, 1024, 4096, 32768)


def large_cells(a):
    """single large cells and a batch of 64 x 1000 atoms, walk against grid; returns the lines of the report"""
    import ctypes as C

    import torch

    from athena_amd import _capi
    from athena_amd.graph import periodic_stats

    dev = torch.device("cuda:0")
    cmin, cmax = 0.5, 3.0
    density = 4096 / 38.4 ** 3
    rng = np.random.Generator(np.random.PCG64(9))
    cases = []
    for m in LARGE_SIZES:
        edge = (m / density) ** (1.0 / 3.0)
        cases.append((f"1 x {m} atoms, edge {edge:.2f}", rng.random((m, 3)).astype(np.float32),
                      (np.eye(3) * edge).astype(np.float32)[None], np.array([0, m], np.int32)))
    edge = (1000 / density) ** (1.0 / 3.0)
    cases.append((f"64 x 1000 atoms, edge {edge:.2f}", rng.random((64000, 3)).astype(np.float32),
                  np.tile((np.eye(3) * edge).astype(np.float32), (64, 1, 1)), (np.arange(65) * 1000).astype(np.int32)))
    pbc = np.ones(3, np.int32)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def build(route, fd, ld, off):
        """size query, allocation of the outputs, fill: seconds, the output tensors, the stats"""
        os.environ["ATHENA_MP_PERIODIC_ROUTE"] = route
        B, n = ld.shape[0], fd.shape[0]
        head = (B, n, vp(off), ptr(fd), ptr(ld), vp(pbc), cmin, cmax)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E = C.c_int64()
        _capi.call("athena_mp_periodic_pairs", *head, None, None, None, None, None, 0, C.byref(E), None)
        pairs = torch.empty((E.value, 2), dtype=torch.int32, device=dev)
        feature = torch.empty((E.value,), dtype=torch.float32, device=dev)
        vec = torch.empty((E.value, 3), dtype=torch.float32, device=dev)
        shift = torch.empty((E.value, 3), dtype=torch.int32, device=dev)
        first = torch.empty((n,), dtype=torch.int32, device=dev)
        eoff = np.zeros(B + 1, np.int64)
        _capi.call("athena_mp_periodic_pairs", *head, ptr(pairs), ptr(feature), ptr(vec), ptr(shift), ptr(first), E.value, C.byref(E),
                   vp(eoff))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, (pairs, feature, vec, shift, first), periodic_stats()

    lines = [f"# large cells, scripts/bench_periodic_graph.py --large-cells on {torch.cuda.get_device_name(0)}: athena_mp_periodic_pairs, size "
             f"query + fill of every output, cutoffs {cmin:g} / {cmax:g}, random atoms at {density:.4f} per cubic unit",
             f"# the route pinned with ATHENA_MP_PERIODIC_ROUTE, walk and grid alternating in one process; one warm-up build of each, then "
             f"median (min - max) of {a.repeats}; host clock around calls that end in a device synchronise; seconds"]
    old = os.environ.get("ATHENA_MP_PERIODIC_ROUTE")
    try:
        for name, frac, lat, off in cases:
            fd, ld = torch.from_numpy(frac).to(dev), torch.from_numpy(lat).to(dev)
            _, walk, sw = build("walk", fd, ld, off)
            _, grid, sg = build("grid", fd, ld, off)
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(walk, grid)), f"{name}: the routes differ"
            E = int(walk[1].shape[0])
            del walk, grid
            tw, tg = [], []
            for _ in range(a.repeats):
                tw.append(build("walk", fd, ld, off)[0])
                tg.append(build("grid", fd, ld, off)[0])
            mw, mg = statistics.median(tw), statistics.median(tg)
            lines.append(f"{name:32s} edges {E:9d}  walk {mw:.5f} ({min(tw):.5f} - {max(tw):.5f})  grid {mg:.5f} ({min(tg):.5f} - {max(tg):.5f})  "
                         f"walk / grid {mw / mg:7.2f}  walk pairs {sw['walk_pairs']}  grid pairs {sg['grid_pairs']}  "
                         f"grid structures {sg['structures_grid']}  identical arrays")
    finally:
        if old is None:
            os.environ.pop("ATHENA_MP_PERIODIC_ROUTE", None)
        else:
            os.environ["ATHENA_MP_PERIODIC_ROUTE"] = old
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large-cells", action="store_true", help="only the large-cell leg (walk against grid), appended to --out")
    ap.add_argument("--structures", type=int, default=130_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--device-only", action="store_true", help="skip the host route (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodic_graph_build.txt"), help="'-': print only")
    a = ap.parse_args()

    import torch

    import periodic_reference as pr
    from athena_amd import DeviceGraph, _capi

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    if a.large_cells:
        text = "\n".join(large_cells(a))
        print(text)
        if a.out != "-":
            with open(a.out, "a") as f:
                f.write(text + "\n")
        return
    dev = torch.device("cuda:0")
    B = a.structures
    cmin, cmax = 0.5, 3.0
    frac, lat, off = make_batch(B)
    n = int(off[-1])
    fd, ld = torch.from_numpy(frac).to(dev), torch.from_numpy(lat).to(dev)
    torch.cuda.synchronize()

    def device_route():
        t0 = time.perf_counter()
        g, feature, vec, _, _ = DeviceGraph.from_structures(fd, ld, off, cmin, cmax)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, g, feature, vec

    def host_route():
        t0 = time.perf_counter()
        fh, lh = fd.cpu().numpy(), ld.cpu().numpy()
        t1 = time.perf_counter()
        per = [pr.structure_edges(fh[off[s]:off[s + 1]], lh[s], cmin, cmax, extra=0) for s in range(B)]
        arrays = pr.assemble(per, off, cmax)
        t2 = time.perf_counter()
        g = DeviceGraph.from_edges(n, arrays["pairs"])
        feature, vec = torch.from_numpy(arrays["feature"]).to(dev), torch.from_numpy(arrays["vec"]).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return (t3 - t0, t1 - t0, t2 - t1, t3 - t2), g, feature, vec

    lines = [f"# scripts/bench_periodic_graph.py on {torch.cuda.get_device_name(0)}: {B} structures of 8 - 30 atoms ({n} atoms), cubic and "
             f"sheared cells of edge 4.3 - 8, cutoffs {cmin:g} / {cmax:g}",
             f"# warm-up build, then median of {a.repeats} (device) / {a.host_repeats} (host); host clock around a call that ends in a "
             "device synchronise; seconds"]
    _, g, feature, vec = device_route()
    E, nnz = int(feature.shape[0]), g.nnz
    keep = (feature.cpu().numpy(), vec.cpu().numpy(), g.export("col"), g.export("eid")) if not a.device_only else None
    g.close()
    del feature, vec
    td = []
    for _ in range(a.repeats):
        t, g, feature, vec = device_route()
        td.append(t)
        g.close()
        del feature, vec
    lines.append(f"edges {E}  CSR entries {nnz}")
    lines.append(f"device route  DeviceGraph.from_structures (structures in HBM -> handle + feature + vec in HBM)   median {statistics.median(td):.4f}   "
                 f"min {min(td):.4f}  max {max(td):.4f}")
    if not a.device_only:
        _, g, feature, vec = host_route()
        same = (np.array_equal(feature.cpu().numpy(), keep[0]) and np.array_equal(vec.cpu().numpy(), keep[1])
                and np.array_equal(g.export("col"), keep[2]) and np.array_equal(g.export("eid"), keep[3]))
        assert same, "the two routes built different graphs"
        g.close()
        del feature, vec, keep
        th = []
        for _ in range(a.host_repeats):
            t, g, feature, vec = host_route()
            th.append(t)
            g.close()
            del feature, vec
        tot = [t[0] for t in th]
        k = tot.index(sorted(tot)[len(tot) // 2])
        lines.append(f"host route    structures D2H + numpy pair-and-image search + DeviceGraph.from_edges + uploads           median {statistics.median(tot):.4f}   "
                     f"min {min(tot):.4f}  max {max(tot):.4f}")
        lines.append(f"              of the median run: D2H {th[k][1]:.4f}  search + assembly {th[k][2]:.4f}  handle + uploads {th[k][3]:.4f}")
        lines.append("the two routes' feature, vec and CSR arrays are equal")
        lines.append(f"device route / host route = {statistics.median(td) / statistics.median(tot):.5f}")
    text = "\n".join(lines)
    print(text)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
