#!/usr/bin/env python3
"""Times neighbour-sampled mini-batches (NeighborSampler, athena_amd/csrc/neighbor_sample.hip) of the benchmark's own graph --
synth.random_graph_csr(1 000 000, 4 500 000): 1 M vertices, 10 M entries -- resident in HBM, on the MI355X:

  seeds_1024_10_10, seeds_1024_15_10_5, seeds_8192_10_10, seeds_8192_15_10_5
                     that many random seed vertices at those fan-outs (hop 0 around the seeds first);
  hub_1024_10_10     the same graph with 100 000 more entries in the row of vertex 0, which is among the seeds.

Per case, after one warm-up, the median of --repeats samples with min and max beside it (host clock around a sample, which ends
synchronised, the blocks closed outside the window): the device route; the time of its hops split into count, draw, relabel and
handle (athena_mp_sample_stats, summed over the hops of the median run's last sample); the share of 64-entry steps the draw kernel
skipped; and the HOST route on the same seeds -- the CSR on the host, the selection of tests/sampling_reference.py vectorised in
numpy, the upload and athena_mp_graph_create per hop.  Both routes give the same arrays (checked on vertex_map and the entry counts).
Beside them: a Kipf forward + reverse step at 128 -> 128 features over the blocks (one step per block, outermost first, features
gathered by take_vertices), and the same step on the whole graph.  There is no pass/fail time.

  python scripts/bench_neighbor_sampling.py [--repeats 5] [--only CASE] [--out profiles/neighbor_sampling.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"seeds_1024_10_10": (1024, (10, 10), False), "seeds_1024_15_10_5": (1024, (15, 10, 5), False),
         "seeds_8192_10_10": (8192, (10, 10), False), "seeds_8192_15_10_5": (8192, (15, 10, 5), False),
         "hub_1024_10_10": (1024, (10, 10), True)}
HUB_EXTRA = 100000


def with_hub(ia, ja, rng):
    """the same CSR with HUB_EXTRA more entries (uniform columns, no edge ids) at the end of row 0"""
    n = ia.size - 1
    extra = np.zeros((2, HUB_EXTRA), np.int32, order="F")
    extra[0] = rng.integers(1, n + 1, HUB_EXTRA)
    end = int(ia[1]) - 1
    ja2 = np.asfortranarray(np.concatenate([ja[:, :end], extra, ja[:, end:]], axis=1))
    ia2 = ia.copy()
    ia2[1:] += HUB_EXTRA
    return ia2, ja2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=1000000)
    ap.add_argument("--pairs", type=int, default=4500000)
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--only", choices=sorted(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbor_sampling.json"))
    a = ap.parse_args()
    import torch

    import sampling_reference as sr
    from athena_amd import DeviceGraph, NeighborSampler, _capi, ops, synth

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    rng = np.random.Generator(np.random.PCG64(23))
    n, F = a.nodes, a.feat
    ia, ja = synth.random_graph_csr(n, a.pairs)
    ja[1] = 0                                                          # a Kipf handle: no edge columns
    x = torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)).to(dev)
    W = torch.from_numpy((rng.standard_normal(F * F) / np.sqrt(F)).astype(np.float32)).to(dev)
    records = []

    def timed(f, repeats, after=lambda r: None):
        after(f())
        t = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
            after(r)
        return round(statistics.median(t) * 1e3, 3), round(min(t) * 1e3, 3), round(max(t) * 1e3, 3)

    def kipf_step(handles, x0):
        """forward through the handles in order, reverse back through them (dX and dW of every step).  A square handle takes the
        one-call reverse pass; a block, which is rectangular, keeps P and takes kipf_layer_bwd_x + matmul_dw"""
        acts, kept = [x0], []
        for g in handles:
            P, Z = ops.kipf_layer_fwd(g, acts[-1], W, F, keep_P=g.n_rows != g.n_cols)
            acts.append(Z)
            kept.append(P)
        dz = acts[-1]
        for g, xin, P in zip(handles[::-1], acts[-2::-1], kept[::-1]):
            if P is None:
                dz, _ = ops.kipf_layer_bwd(g, dz, W, xin)
            else:
                ops.matmul_dw(P, dz)
                dz = ops.kipf_layer_bwd_x(g, dz, W, F)

    graphs = {}
    for name, (m, fanouts, hub) in CASES.items():
        if a.only not in (None, name):
            continue
        if hub not in graphs:
            gia, gja = with_hub(ia, ja, rng) if hub else (ia, ja)
            g = DeviceGraph(gia, gja, n_edge_cols=0)
            graphs[hub] = (gia, gja, g, NeighborSampler(g)) + sr.parent_csr(gia, gja)[:2]
        gia, gja, g, sampler, rowptr, col = graphs[hub]
        seeds = rng.permutation(n)[:m].astype(np.int32)
        if hub:
            seeds[0] = 0
        epoch = 5

        close = lambda blocks: [b.close() for b in blocks]
        dev_ms = timed(lambda: sampler.sample(seeds, fanouts, seed=epoch), a.repeats, close)
        blocks = sampler.sample(seeds, fanouts, seed=epoch)
        hops = np.array(sampler.hop_stats)
        split = {k: round(float(hops[:, 4 + i].sum()) / 1e3, 3) for i, k in enumerate(("count_ms", "draw_ms", "relabel_ms", "handle_ms"))}
        steps, skipped = int(hops[:, 2].sum()), int(hops[:, 3].sum())

        def host_route():
            out, s = [], seeds
            for h, k in enumerate(fanouts):
                b = sr.sample_hop_vectorised(rowptr, col, None, s, k, sr.hop_seed(epoch, h))
                out.append((b, DeviceGraph(b["adj_ia"], b["adj_ja"], n_cols=b["n_cols"], n_edge_cols=0, row_deg=b["row_deg"], col_deg=b["col_deg"])))
                s = b["vertex_map"]
            return out[::-1]

        closeh = lambda pairs: [p[1].close() for p in pairs]
        host_ms = timed(host_route, a.host_repeats, closeh)
        ref = host_route()
        same = all(np.array_equal(b.vertex_map.cpu().numpy(), r[0]["vertex_map"]) and b.handle.nnz == r[0]["nnz"] for b, r in zip(blocks, ref))
        closeh(ref)

        handles = [b.handle for b in blocks]
        x0 = blocks[0].take_vertices(x)
        step_ms = timed(lambda: kipf_step(handles, x0), a.repeats)
        gather_ms = timed(lambda: blocks[0].take_vertices(x), a.repeats)
        full_ms = timed(lambda: kipf_step([g], x), a.repeats)
        rec = {"case": name, "vertices": n, "entries": int(gja.shape[1]), "seeds": m, "fanouts": list(fanouts), "hub_row_entries": int(gia[1] - gia[0]),
               "block_rows": [b.handle.n_rows for b in blocks], "block_cols": [b.handle.n_cols for b in blocks],
               "block_entries": [int(b.handle.nnz) for b in blocks], "device_ms": dev_ms[0], "device_ms_min": dev_ms[1], "device_ms_max": dev_ms[2],
               **split, "rows_drawn": int(hops[:, 0].sum()), "rows_whole": int(hops[:, 1].sum()), "draw_steps": steps, "draw_steps_skipped": skipped,
               "skip_share": round(skipped / steps, 4) if steps else None, "hop0_steps": int(hops[0, 2]), "hop0_skipped": int(hops[0, 3]),
               "host_ms": host_ms[0], "host_ms_min": host_ms[1], "host_ms_max": host_ms[2], "host_over_device": round(host_ms[0] / dev_ms[0], 2),
               "same_arrays": bool(same), "kipf_blocks_fwd_bwd_ms": step_ms[0], "take_vertices_ms": gather_ms[0],
               "kipf_full_graph_fwd_bwd_ms": full_ms[0], "feat": F, "repeats": a.repeats, "host_repeats": a.host_repeats,
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        close(blocks)
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
