#!/usr/bin/env python3
"""Times the step from a per-edge gradient back to the atoms and the cell on the BASELINE configs[2]-shaped batch of
scripts/bench_periodic_graph.py (130 k periodic structures of 8 - 30 atoms, cubic and sheared cells, cutoffs 0.5 / 3.0), two ways
in ONE run on the MI355X.  Inputs in HBM: the handle, vec [E, 3] and a gradient de [E, fe_cols] with respect to the edge feature
(what duvenaud_msgpass_layer_type.backward(need_edge_grad=True) returns).  Outputs in HBM: dcart, dfrac [n, 3], virial, dlat [B, 3, 3].

  device   athena_amd.structures_grad: one gather launch (dcart with dfrac as its epilogue), the virial's two launches;
  host     the best route without it: download de and vec, form gx in numpy, scatter with np.add.at (dcart), per-structure sums
           with np.add.reduceat (virial), dfrac and dlat in numpy, upload the four results.

After one warm-up of each, the median of --repeats (device) / --host-repeats (host) runs, host clock around a call that ends in a
device synchronise.  The host route sums in another order: the results are compared within 1e-5 of their term magnitudes.

  python scripts/bench_geometry_grad.py [--structures 130000] [--fe-cols 8] [--repeats 20] [--host-repeats 3] [--out profiles/geometry_grad.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=130_000)
    ap.add_argument("--fe-cols", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--device-only", action="store_true", help="skip the host route (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_grad.txt"), help="'-': print only")
    a = ap.parse_args()

    import torch

    from athena_amd import DeviceGraph, _capi, structures_grad
    from bench_periodic_graph import make_batch

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    B, cmin, cmax = a.structures, 0.5, 3.0
    frac, lat, off = make_batch(B)
    n = int(off[-1])
    handle, feature, vec, voff, eoff = DeviceGraph.from_structures(frac, lat, off, cmin, cmax)
    E = int(vec.shape[0])
    lat_d = torch.from_numpy(lat).to(dev)
    de = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).uniform(-1, 1, (E, a.fe_cols)).astype(np.float32)).to(dev)
    pairs_i = np.repeat(np.arange(n), np.diff(handle.export("rowptr")))      # the edge ends, once, outside the timed region:
    col, eid = handle.export("col"), handle.export("eid")                    # the host route's own index arrays
    first = (eid >= 0) & (pairs_i < col)
    ei, ej, ee = pairs_i[first], col[first], eid[first]
    sid = np.repeat(np.arange(B), np.diff(off))
    inv_t = np.linalg.inv(lat.astype(np.float64)).transpose(0, 2, 1)
    torch.cuda.synchronize()

    def device_route():
        t0 = time.perf_counter()
        out = structures_grad(handle, lat_d, voff, eoff, vec, cmax, dfeature=de)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def host_route():
        t0 = time.perf_counter()
        deh, x = de.cpu().numpy(), vec.cpu().numpy()
        t1 = time.perf_counter()
        r = np.sqrt((x * x).sum(1))
        gx = (deh.sum(1) / np.float32(cmax) / r)[:, None] * x
        cart = np.zeros((n, 3), np.float32)
        np.add.at(cart, ei, gx[ee])
        np.subtract.at(cart, ej, gx[ee])
        dfrac = np.einsum("nkc,nc->nk", lat[sid], cart)
        outer = x[:, :, None] * gx[:, None, :]
        virial = np.zeros((B, 3, 3), np.float32)
        has = np.diff(eoff) > 0
        virial[has] = np.add.reduceat(outer, eoff[:-1][has], axis=0)
        dlat = (inv_t @ virial).astype(np.float32)
        t2 = time.perf_counter()
        out = {k: torch.from_numpy(v).to(dev) for k, v in (("cart", cart), ("frac", dfrac), ("virial", virial), ("lat", dlat))}
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return (t3 - t0, t1 - t0, t2 - t1, t3 - t2), out

    lines = [f"# scripts/bench_geometry_grad.py on {torch.cuda.get_device_name(0)}: {B} structures of 8 - 30 atoms ({n} atoms, {E} edges), "
             f"de [E, {a.fe_cols}] -> dcart, dfrac, virial, dlat",
             f"# warm-up, then median of {a.repeats} (device) / {a.host_repeats} (host); host clock around a call that ends in a device "
             "synchronise; seconds"]
    _, ref = device_route()
    td = [device_route()[0] for _ in range(a.repeats)]
    lines.append(f"device route  structures_grad (de, vec in HBM -> four outputs in HBM)                     median {statistics.median(td):.6f}   "
                 f"min {min(td):.6f}  max {max(td):.6f}")
    if not a.device_only:
        _, got = host_route()
        x = vec.cpu().numpy().astype(np.float64)
        mag = np.zeros((n, 3))
        gmag = np.abs(de.cpu().numpy().astype(np.float64)).sum(1)[:, None] / cmax * np.abs(x) / np.sqrt((x * x).sum(1))[:, None]
        np.add.at(mag, ei, gmag[ee])
        np.add.at(mag, ej, gmag[ee])
        worst = float((np.abs(got["cart"].cpu().numpy().astype(np.float64) - ref["cart"].cpu().numpy()) / np.maximum(mag, 1e-30)).max())
        assert worst <= 1e-5, f"the two routes' dcart differ by {worst:.2e} of their term magnitudes"
        th = [host_route()[0] for _ in range(a.host_repeats)]
        tot = [t[0] for t in th]
        k = tot.index(sorted(tot)[len(tot) // 2])
        lines.append(f"host route    de, vec D2H + numpy (np.add.at, np.add.reduceat) + four uploads                   median {statistics.median(tot):.6f}   "
                     f"min {min(tot):.6f}  max {max(tot):.6f}")
        lines.append(f"              of the median run: D2H {th[k][1]:.6f}  numpy {th[k][2]:.6f}  uploads {th[k][3]:.6f}")
        lines.append(f"the two routes' dcart agree within {worst:.1e} of their term magnitudes")
        lines.append(f"device route / host route = {statistics.median(td) / statistics.median(tot):.6f}")
    text = "\n".join(lines)
    print(text)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(text + "\n")
    handle.close()


if __name__ == "__main__":
    main()
