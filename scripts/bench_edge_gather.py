#!/usr/bin/env python3
"""Times the gather that makes the edge MLP's input, and its reverse (athena_amd/csrc/edge_gather.hip), on arrays that are resident in
HBM, on the MI355X, at k = 8 in three dimensions, on the two rectangular cases of bench_pool.py:

  encoder   the 64^3 grid points (queries) against 1 000 000 mesh points (sources): a mesh onto a latent grid -- set abstraction;
  decoder   1 000 000 queries against the 64^3 points of a regular grid;

each at (Fs, dim) = (64, 3) and (128, 3) with no query block, at the pitch ld = W and at ld padded to a multiple of 4, and once
(Fs = 64, padded) with relative and Fq = Fs; then four forward-only variants at Fs = 64 (ANATOMY below) that show what the
padded forward's time is made of.  Per call -- fwd, and bwd with every output the widths allow -- the time and the achieved
bytes per second over the ALGORITHMIC bytes, computed here from the shapes and counted as bench_pool.py counts them:

  fwd   E * 8 for column and edge ids + 4 * (Fs * the distinct rows of xs read + Fq * the distinct rows of xq read + dim * E of coords
        + W * E of h written)
  bwd   E * 4 of ids for each of dxs and dxq + 4 * (W * E of dh, counted once + Fs * n_sources + Fq * n_queries + dim * E written)

Beside them, in the same run and alternating with them:
  - athena_mp_pool_max_bwd_edges at F = Fs (E * 8 + 4 F * (the distinct rows of arg and dy read + E rows of dh written)): the launch
    that also streams E rows out once, the yardstick of the forward;
  - the route a user has without these entries, torch index arithmetic on the pair list: torch.cat of indexed rows for the forward,
    index_add_ (atomics) and a strided copy for the reverse.

A sample is --launches calls between two device events; after one warm-up sample, the median of --repeats samples with min and max
beside it.  There is no pass/fail time.

  python scripts/bench_edge_gather.py [--repeats 5] [--launches 20] [--points 1000000] [--only CASE] [--out profiles/edge_gather.json]
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

CASES = ("encoder", "decoder")
HBM_PEAK = 8.0e12                                  # bytes per second, MI355X
# (Fs, Fq, dim, relative, ld)
RUNS = ((64, 0, 3, 0, 67), (64, 0, 3, 0, 68), (128, 0, 3, 0, 131), (128, 0, 3, 0, 132), (64, 64, 3, 1, 132))
# what the padded forward's time is made of, Fs = 64: rows of 256 bytes at a 256-byte pitch and no tail; the same rows at the
# 272-byte pitch; a tail of four words, which leaves no word of the pitch unwritten (coords: random [E, 4]); the tail alone
ANATOMY = ((64, 0, 0, 0, 64), (64, 0, 0, 0, 68), (64, 0, 4, 0, 68), (0, 0, 3, 0, 68))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_gather.json"), help="'-': print only")
    a = ap.parse_args()

    import torch

    from athena_amd import DeviceGraph, _capi

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    _capi.use_torch_stream()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    k, records = 8, []
    rng = np.random.Generator(np.random.PCG64(13))

    def sample(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.launches):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.launches                       # ms per call

    def timed(fns):
        """{name: [ms per call] * repeats}: one warm-up sample of each, then the samples alternating"""
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
        rowptr, col, eid = g.export("rowptr"), g.export("col"), g.export("eid")
        rows = np.repeat(np.arange(nq, dtype=np.int64), np.diff(rowptr))
        entry_of_edge = np.empty(E, np.int64)
        entry_of_edge[eid] = np.arange(E)
        row_e = torch.from_numpy(rows[entry_of_edge]).to(dev)                                     # the query and the source of edge e
        col_e = torch.from_numpy(col[entry_of_edge].astype(np.int64)).to(dev)
        rows_used, cols_used = int((np.diff(rowptr) > 0).sum()), int(np.unique(col).size)
        for Fs, Fq, dim, rel, ld in RUNS + ANATOMY:
            W = Fs + Fq + dim
            if (Fs, Fq, dim, rel, ld) in ANATOMY:
                xs = torch.randn((ns, Fs), dtype=torch.float32, device=dev) if Fs else None
                co = coords if dim == 3 else torch.randn((E, dim), dtype=torch.float32, device=dev) if dim else None
                h = torch.zeros((E, ld), dtype=torch.float32, device=dev)
                fn = lambda: _capi.call("athena_mp_edge_gather_fwd", g.handle, Fs, ptr(xs), 0, None, dim, ptr(co), 0, ld, ptr(h))
                rec = {"case": case, "anatomy": True, "Fs": Fs, "dim": dim, "W": W, "ld": ld, "pairs": E,
                       "fwd": summary(timed({"fwd": fn})["fwd"], E * 8 + 4 * (Fs * cols_used + dim * E + W * E))}
                print(json.dumps(rec), flush=True)
                records.append(rec)
                del xs, co, h
                continue
            xs = torch.from_numpy(rng.standard_normal((ns, Fs)).astype(np.float32)).to(dev)
            xq = torch.from_numpy(rng.standard_normal((nq, Fq)).astype(np.float32)).to(dev) if Fq else None
            h = torch.zeros((E, ld), dtype=torch.float32, device=dev)
            dh = torch.randn((E, ld), dtype=torch.float32, device=dev)
            dxs = torch.empty((ns, Fs), dtype=torch.float32, device=dev)
            dxq = torch.empty((nq, Fq), dtype=torch.float32, device=dev) if Fq else None
            dco = torch.empty((E, dim), dtype=torch.float32, device=dev)
            # the yardstick launch's operands: arg from a forward over random edge values, so that it names real columns
            hp = torch.randn((E, Fs), dtype=torch.float32, device=dev)
            yp, dyp = torch.empty((nq, Fs), dtype=torch.float32, device=dev), torch.randn((nq, Fs), dtype=torch.float32, device=dev)
            argp = torch.empty((nq, Fs), dtype=torch.int32, device=dev)
            _capi.call("athena_mp_pool_max_edges_fwd", g.handle, Fs, ptr(hp), ptr(yp), ptr(argp))

            def fwd():
                _capi.call("athena_mp_edge_gather_fwd", g.handle, Fs, ptr(xs), Fq, ptr(xq), dim, ptr(coords), rel, ld, ptr(h))

            def bwd():
                _capi.call("athena_mp_edge_gather_bwd", g.handle, Fs, Fq, dim, rel, ld, ptr(dh), ptr(dxs), ptr(dxq), ptr(dco))

            def pool_bwd_edges():
                _capi.call("athena_mp_pool_max_bwd_edges", g.handle, Fs, ptr(argp), ptr(dyp), ptr(hp))

            def torch_fwd():
                if rel:
                    mine = xq[row_e]
                    return torch.cat([xs[col_e] - mine, mine, coords], 1)
                return torch.cat([xs[col_e], coords], 1)

            def torch_bwd():
                out = [torch.zeros((ns, Fs), dtype=torch.float32, device=dev).index_add_(0, col_e, dh[:, :Fs])]
                if Fq:
                    out.append(torch.zeros((nq, Fq), dtype=torch.float32, device=dev).index_add_(0, row_e, dh[:, Fs:Fs + Fq] - dh[:, :Fs]))
                return out + [dh[:, Fs + Fq:W].contiguous()]

            fwd()
            bwd()
            torch.cuda.synchronize()
            same_h = bool(torch.equal(torch_fwd().view(torch.int32), h[:, :W].view(torch.int32)))
            same_dc = bool(torch.equal(torch_bwd()[-1].view(torch.int32), dco.view(torch.int32)))
            t = timed({"fwd": fwd, "pool_bwd_edges": pool_bwd_edges, "torch_fwd": torch_fwd, "bwd": bwd, "torch_bwd": torch_bwd})
            med = lambda n: statistics.median(t[n])
            fwd_bytes = E * 8 + 4 * (Fs * cols_used + Fq * rows_used + dim * E + W * E)
            bwd_bytes = E * 4 * (1 + (Fq > 0)) + 4 * (W * E + Fs * ns + Fq * nq + dim * E)
            rec = {"case": case, "queries": nq, "sources": ns, "k": k, "Fs": Fs, "Fq": Fq, "dim": dim, "relative": rel, "W": W, "ld": ld,
                   "pairs": E, "distinct_sources_read": cols_used, "distinct_queries_read": rows_used,
                   "fwd": summary(t["fwd"], fwd_bytes), "bwd": summary(t["bwd"], bwd_bytes),
                   "pool_bwd_edges": summary(t["pool_bwd_edges"], E * 8 + 4 * Fs * (2 * rows_used + E)),
                   "torch_fwd": summary(t["torch_fwd"]), "torch_bwd": summary(t["torch_bwd"]),
                   "torch_vs_fwd": round(med("torch_fwd") / med("fwd"), 2), "torch_vs_bwd": round(med("torch_bwd") / med("bwd"), 2),
                   "h_equals_torch_cat_bit_for_bit": same_h, "dcoords_equals_the_slice": same_dc,
                   "launches_per_sample": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del xs, xq, h, dh, dxs, dxq, dco, hp, yp, dyp, argp
            torch.cuda.empty_cache()
        g.close()
        del coords, row_e, col_e
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
