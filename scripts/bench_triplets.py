#!/usr/bin/env python3
"""Times the bond-angle triplets of a neighbour graph (athena_amd/csrc/triplets.hip) on the MI355X: a batch of periodic structures
of 100 atoms in cubic cells of edge 12, about 1 000 000 atoms in all, at two cutoffs that give roughly 12 and roughly 40 entries per
row (3.67 and 5.48 at this density).  Per cutoff:

  build     athena_mp_triplet_pairs as a size query, the same as a fill, and athena_mp_graph_create_bipartite_dev on the list, each
            between host clocks around a device synchronisation (the entries wait for the device themselves); the handle builder's
            share of the three is recorded beside them, with athena_mp_triplet_stats
  forward   athena_mp_entry_vectors_fwd and athena_mp_triplet_cos_fwd, between device events
  reverse   athena_mp_triplet_cos_bwd and athena_mp_entry_vectors_bwd: dcos -> dvec

Beside them the route a user has without these entries, torch on the same device, written out below: the row of every entry, every
entry repeated over its row's length by repeat_interleave, the partner from the position inside the run, a mask for k != k', the
indexed entry vectors for the cosine, and index_add_ for the reverse (its sums are atomic: nothing that comes back is bit-defined).
Where torch runs out of memory that is what is recorded.

A sample is --launches launches between two device events; after one warm-up sample, the median of --repeats samples with min and
max beside it.  There is no pass/fail time.

  python scripts/bench_triplets.py [--atoms 1000000] [--cutoffs 3.67 5.48] [--repeats 5] [--launches 5] [--out profiles/triplets.json]
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

PER_STRUCTURE, EDGE = 100, 12.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=1_000_000)
    ap.add_argument("--cutoffs", type=float, nargs="+", default=[3.67, 5.48])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triplets.json"), help="'-': print only")
    a = ap.parse_args()

    import torch

    from athena_amd import DeviceGraph, _capi
    from athena_amd.geometry import triplet_stats

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    _capi.use_torch_stream()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    rng = np.random.Generator(np.random.PCG64(15))
    B = max(a.atoms // PER_STRUCTURE, 1)
    n = B * PER_STRUCTURE
    frac = rng.random((n, 3)).astype(np.float32)
    lat = np.tile((np.eye(3) * EDGE).astype(np.float32), (B, 1, 1))
    off = (np.arange(B + 1) * PER_STRUCTURE).astype(np.int32)
    records = []

    def sample(fn, launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(launches):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / launches                         # ms per launch

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def summary(ms):
        return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}

    for cutoff in a.cutoffs:
        g, _, vec, _, _ = DeviceGraph.from_structures(frac, lat, off, 0.0, cutoff)
        nnz, E = g.nnz, g.n_edge_cols
        inf = float("inf")
        T = C.c_int64()

        def query():
            _capi.call("athena_mp_triplet_pairs", g.handle, 3, ptr(vec), inf, None, 0, None, C.byref(T))

        query()
        pairs = torch.empty((T.value, 2), dtype=torch.int32, device=dev)
        ia = np.empty(nnz + 1, np.int32)

        def fill():
            _capi.call("athena_mp_triplet_pairs", g.handle, 3, ptr(vec), inf, ptr(pairs), T.value, None, C.byref(T))

        def handle():
            h = C.c_void_p()
            _capi.call("athena_mp_graph_create_bipartite_dev", nnz, nnz, T.value, ptr(pairs), ia.ctypes.data_as(C.c_void_p), None, 0,
                       C.byref(h))
            return h

        fill()
        t_query, t_fill, t_handle = [], [], []
        tg = None
        for _ in range(a.repeats):
            t_query.append(wall(query)[0])
            t_fill.append(wall(fill)[0])
            if tg is not None:
                _capi.load().athena_mp_graph_destroy(tg)
            ms, tg = wall(handle)
            t_handle.append(ms)
        stats = triplet_stats()
        Tn = int(T.value)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        dirs, cosv, ddir, dvec = f32(nnz, 3), f32(Tn), f32(nnz, 3), f32(E, 3)
        dcos = torch.randn((Tn,), dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(15))
        fns = {
            "entry_vectors_fwd": lambda: _capi.call("athena_mp_entry_vectors_fwd", g.handle, 3, ptr(vec), ptr(dirs)),
            "triplet_cos_fwd": lambda: _capi.call("athena_mp_triplet_cos_fwd", tg, 3, ptr(dirs), ptr(cosv)),
            "triplet_cos_bwd": lambda: _capi.call("athena_mp_triplet_cos_bwd", tg, 3, ptr(dirs), ptr(cosv), ptr(dcos), ptr(ddir)),
            "entry_vectors_bwd": lambda: _capi.call("athena_mp_entry_vectors_bwd", g.handle, 3, ptr(ddir), ptr(dvec)),
        }
        times = {}
        for name, fn in fns.items():
            sample(fn, a.launches)
            times[name] = [sample(fn, a.launches) for _ in range(a.repeats)]
        med = lambda name: statistics.median(times[name])
        build = statistics.median(t_query) + statistics.median(t_fill) + statistics.median(t_handle)
        rec = {"atoms": n, "structures": B, "cutoff": cutoff, "edges": E, "entries": nnz, "entries_per_row": round(nnz / n, 2),
               "triplets": Tn, "triplet_stats": {"triplets": stats[0], "participants": stats[1], "longest_run": stats[2]},
               "size_query": summary(t_query), "fill": summary(t_fill), "handle_builder": summary(t_handle), "build_ms": round(build, 3),
               "handle_builder_share_of_build": round(statistics.median(t_handle) / build, 3)}
        for name in fns:
            rec[name] = summary(times[name])
        rec["forward_ms"] = round(med("entry_vectors_fwd") + med("triplet_cos_fwd"), 4)
        rec["reverse_ms"] = round(med("triplet_cos_bwd") + med("entry_vectors_bwd"), 4)

        if not a.no_torch:
            rowptr = torch.from_numpy(g.export("rowptr").astype(np.int64)).to(dev)
            col = torch.from_numpy(g.export("col").astype(np.int64)).to(dev)
            eid = torch.from_numpy(g.export("eid").astype(np.int64)).to(dev)

            def torch_build():
                deg = rowptr[1:] - rowptr[:-1]
                row = torch.repeat_interleave(torch.arange(n, device=dev), deg)
                first = torch.repeat_interleave(torch.arange(nnz, device=dev), deg[row])         # every entry over its row's length
                run = torch.cumsum(deg[row], 0) - deg[row]
                second = rowptr[row[first]] + (torch.arange(first.numel(), device=dev) - run[first])
                keep = first != second
                return row, first[keep], second[keep]

            def torch_forward(row, first, second):
                sign = torch.where(row <= col, -1.0, 1.0).to(torch.float32)
                d = vec[eid] * sign[:, None]
                va, vb = d[first], d[second]
                den = va.norm(dim=1) * vb.norm(dim=1)
                return d, va, vb, den, (va * vb).sum(1) / den, sign

            def torch_reverse(d, va, vb, den, cs, sign, first, second):
                w = dcos[:, None]
                ga = vb / den[:, None] - cs[:, None] * va / (va * va).sum(1, keepdim=True)
                gb = va / den[:, None] - cs[:, None] * vb / (vb * vb).sum(1, keepdim=True)
                dd = torch.zeros_like(d).index_add_(0, first, w * ga).index_add_(0, second, w * gb)
                return torch.zeros((E, 3), dtype=torch.float32, device=dev).index_add_(0, eid, dd * sign[:, None])

            try:
                ms_b, (row, first, second) = wall(torch_build)                                    # warm-up
                tb = []
                for _ in range(a.repeats):
                    del row, first, second
                    ms_b, (row, first, second) = wall(torch_build)
                    tb.append(ms_b)
                fwd = torch_forward(row, first, second)
                same_list = bool(torch.equal(first.to(torch.int32) + 1, pairs[:, 0]) and torch.equal(second.to(torch.int32) + 1, pairs[:, 1]))
                tdv = torch_reverse(*fwd, first, second)
                fns["entry_vectors_fwd"](); fns["triplet_cos_fwd"](); fns["triplet_cos_bwd"](); fns["entry_vectors_bwd"]()
                torch.cuda.synchronize()
                close = lambda u, w: float((u - w).abs().max() / w.abs().max().clamp_min(1e-30))
                agreement = {"cos": close(fwd[4], cosv), "dvec": close(tdv, dvec)}
                del tdv
                tf = [sample(lambda: torch_forward(row, first, second), 1) for _ in range(a.repeats + 1)][1:]
                tr_ = [sample(lambda: torch_reverse(*fwd, first, second), 1) for _ in range(a.repeats + 1)][1:]
                rec.update({"torch_build": summary(tb), "torch_forward": summary(tf), "torch_reverse": summary(tr_),
                            "torch_pair_list_equal": same_list, "torch_vs_build": round(statistics.median(tb) / build, 2),
                            "torch_vs_forward": round(statistics.median(tf) / rec["forward_ms"], 2),
                            "torch_vs_reverse": round(statistics.median(tr_) / rec["reverse_ms"], 2),
                            "max_difference_from_torch_relative_to_the_largest_element": agreement})
                del row, first, second, fwd
            except torch.cuda.OutOfMemoryError as err:
                rec["torch"] = "out of memory: " + str(err).split("\n")[0][:160]
            del rowptr, col, eid
            torch.cuda.empty_cache()
        rec.update({"launches_per_sample": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)})
        print(json.dumps(rec), flush=True)
        records.append(rec)
        _capi.load().athena_mp_graph_destroy(tg)
        del pairs, dirs, cosv, ddir, dvec, dcos, vec
        g.close()
        torch.cuda.empty_cache()
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
