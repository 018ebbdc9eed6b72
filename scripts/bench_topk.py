#!/usr/bin/env python3
"""Times the top-k vertex selection (athena_mp_topk_vertices, athena_amd/csrc/topk_select.hip) and its gated rows
(athena_mp_select_rows_fwd / _bwd) on scores that are resident in HBM, on the MI355X:

  one_graph      one graph of 1 000 000 vertices                          (sort route, 33 key bits)
  many_large     1 024 graphs x 4 096 vertices                            (sort route, 42 key bits)
  molecules      32 768 graphs x 30 vertices                              (wave route)

all at ratio = 0.5 on standard-normal scores, and on the selection of many_large the gated forward and reverse at F = 64 and 128.
Each is timed against the torch route on the same device: a stable torch.sort on the composite 64-bit key (graph << 32 | the
descending score bits) plus the rank mask and a scatter for the map; for the rows an indexed multiply and an index_add_-free
scatter.  The torch route's map is compared with the library's (finite scores without -0: there the two agree).

Per measurement, after a warm-up of both routes, --repeats samples that alternate the two routes; a sample is the host clock around
--inner calls that end in a device synchronise, divided by --inner; the median with min and max beside it.  There is no pass/fail
time.

  python scripts/bench_topk.py [--repeats 7] [--inner 10] [--only CASE] [--out profiles/topk.json]
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

CASES = {"one_graph": (1, 1000000), "many_large": (1024, 4096), "molecules": (32768, 30)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", choices=tuple(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk.json"))
    a = ap.parse_args()
    import torch

    from athena_amd import _capi
    from athena_amd.geometry import topk_stats

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    _capi.use_torch_stream()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    records = []

    def window(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.inner

    def timed_pair(ours, theirs):
        """both warmed, then alternating samples -> two records of ms"""
        ours(), theirs()
        t = ([], [])
        for _ in range(a.repeats):
            t[0].append(window(ours))
            t[1].append(window(theirs))
        rec = lambda s: {"ms": round(statistics.median(s) * 1e3, 4), "ms_min": round(min(s) * 1e3, 4), "ms_max": round(max(s) * 1e3, 4)}
        return rec(t[0]), rec(t[1])

    for name, (B, each) in CASES.items():
        if a.only not in (None, name):
            continue
        n = B * each
        off = (np.arange(B + 1, dtype=np.int64) * each).astype(np.int32)
        kk = np.full(B, (each + 1) // 2, np.int32)
        room = int(kk.sum())
        score = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).standard_normal(n).astype(np.float32)).to(dev)
        cluster = torch.empty((n,), dtype=torch.int32, device=dev)
        selected = torch.empty((room,), dtype=torch.int32, device=dev)
        soff, count = np.zeros(B + 1, np.int32), C.c_int64()

        def ours():
            _capi.call("athena_mp_topk_vertices", B, n, vp(off), ptr(score), 0, vp(kk), 0, 0.0, ptr(cluster), ptr(selected), None, vp(soff),
                       C.byref(count))

        batch = torch.arange(n, device=dev, dtype=torch.int64) // each            # the block-diagonal layout, the user's part
        start = torch.from_numpy(off[:-1].astype(np.int64)).to(dev)
        k_dev = torch.from_numpy(kk.astype(np.int64)).to(dev)
        slot = torch.arange(n, device=dev, dtype=torch.int64)

        def theirs():
            b = score.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
            asc = torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)
            perm = torch.sort((batch << 32) | (0xFFFFFFFF - asc), stable=True).indices
            g = batch[perm]
            keep = (slot - start[g]) < k_dev[g]
            chosen = torch.sort(perm[keep]).values
            cl = torch.zeros(n, dtype=torch.int32, device=dev)
            cl[chosen] = torch.arange(1, chosen.numel() + 1, dtype=torch.int32, device=dev)
            return cl, chosen

        t_ours, t_torch = timed_pair(ours, theirs)
        ours()
        cl, chosen = theirs()
        stats = topk_stats()
        rec = {"case": name, "graphs": B, "vertices_per_graph": each, "vertices": n, "ratio": 0.5, "kept": int(count.value),
               "graphs_on_wave_route": stats[0], "graphs_on_sort_route": stats[1], "key_bits": stats[2], "radix_passes": stats[3],
               "topk_vertices": t_ours, "torch_route": t_torch,
               "torch_route_gives_the_same_map": bool(torch.equal(cl, cluster) and chosen.numel() == count.value),
               "repeats": a.repeats, "calls_per_sample": a.inner, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        if name != "many_large":
            continue
        m = int(count.value)
        sel64 = (selected[:m] - 1).to(torch.int64)
        gate = torch.tanh(score)
        for F in (64, 128):
            x = torch.randn((n, F), dtype=torch.float32, device=dev)
            dy = torch.randn((m, F), dtype=torch.float32, device=dev)
            y = torch.empty((m, F), dtype=torch.float32, device=dev)
            dx = torch.empty((n, F), dtype=torch.float32, device=dev)
            dgate = torch.empty((n,), dtype=torch.float32, device=dev)

            def fwd():
                _capi.call("athena_mp_select_rows_fwd", n, m, F, ptr(selected), ptr(x), ptr(gate), ptr(y))

            def fwd_torch():
                return x[sel64] * gate[sel64, None]

            def bwd():
                _capi.call("athena_mp_select_rows_bwd", n, m, F, ptr(cluster), ptr(dy), ptr(x), ptr(gate), ptr(dx), ptr(dgate))

            def bwd_torch():
                tx = torch.zeros((n, F), dtype=torch.float32, device=dev)
                tx[sel64] = dy * gate[sel64, None]
                tg = torch.zeros((n,), dtype=torch.float32, device=dev)
                tg[sel64] = (dy * x[sel64]).sum(dim=1)
                return tx, tg

            t_fwd, t_fwd_torch = timed_pair(fwd, fwd_torch)
            t_bwd, t_bwd_torch = timed_pair(bwd, bwd_torch)
            fwd(), bwd()
            tx, tg = bwd_torch()
            rec = {"case": f"gated_rows_F{F}", "on": name, "vertices": n, "kept": m, "F": F,
                   "bytes_forward": 4 * (2 * m * F + 2 * m), "bytes_reverse": 4 * (3 * m * F + n * F + 4 * n),
                   "select_rows_fwd": t_fwd, "torch_forward": t_fwd_torch, "select_rows_bwd": t_bwd, "torch_reverse": t_bwd_torch,
                   "forward_equals_torch": bool(torch.equal(y, fwd_torch())), "dx_equals_torch": bool(torch.equal(dx, tx)),
                   "dgate_max_difference_from_torch": float((dgate - tg).abs().max()),
                   "repeats": a.repeats, "calls_per_sample": a.inner, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del x, dy, y, dx, dgate, tx, tg
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
