#!/usr/bin/env python3
"""Times the Duvenaud degree-bucket plan of a FRESH mini-batch child, built on the host (the route every earlier commit had) and on
the device (athena_amd/csrc/bucket_plan.hip), in ONE run on the MI355X.  The dataset is scripts/bench_batch_select.py's: a
configs[2]-shaped set of periodic structures of 8 - 30 atoms whose graph was built on the device; children of 2 000 and 32 000
structures are drawn with DeviceDataset.select, a new shuffled selection every repetition, and ATHENA_MP_BUCKET_PLAN alternates
between host and device from one repetition to the next.  Per repetition, on a child that has no plan yet:

  call     host wall time of DeviceGraph.plan_duvenaud(1, 10) alone (what the training loop's thread is held for);
  stream   time between two events recorded on the stream around that call (under `host` this contains the blocking uploads);
  forward  host wall time from the call to the completion of the first forward pass of a Duvenaud layer at configs[2]'s widths
           (F_v 64, F_e 8, T = 4, degrees 1 .. 10, 10 outputs) on that child -- the figure a training step sees.

Min and median of --repeats (at least 5) repetitions per route after one warm-up of each, APPENDED to --out.

  python scripts/bench_bucket_plan.py [--structures 130000] [--batches 2000 32000] [--repeats 7] [--out profiles/bucket_plan.txt]
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
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 32000])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bucket_plan.txt"), help="'-': print only")
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")

    import torch

    from athena_amd import DeviceDataset, DeviceGraph, _capi, duvenaud_plan_stats
    from athena_amd.layers import duvenaud_msgpass_layer_type
    from bench_periodic_graph import make_batch

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    B, cmin, cmax, Fv, Fe, lo, hi = a.structures, 0.5, 3.0, 64, 8, 1, 10
    frac, lat, off = make_batch(B)
    n = int(off[-1])
    handle, _, _, voff, eoff = DeviceGraph.from_structures(torch.from_numpy(frac).to(dev), torch.from_numpy(lat).to(dev), off, cmin, cmax)
    ds = DeviceDataset(handle, voff, eoff)
    E = int(eoff[-1])
    rng = np.random.Generator(np.random.PCG64(5))
    x = torch.from_numpy(rng.uniform(-1, 1, (n, Fv)).astype(np.float32)).to(dev)
    e = torch.from_numpy(rng.uniform(-1, 1, (E, Fe)).astype(np.float32)).to(dev)
    layer = duvenaud_msgpass_layer_type(num_vertex_features=[Fv], num_edge_features=[Fe], num_time_steps=4, max_vertex_degree=hi,
                                        num_outputs=10, min_vertex_degree=lo, seed=3)
    old = os.environ.get("ATHENA_MP_BUCKET_PLAN")

    def one(sel, mode):
        """(call, stream, forward) in seconds on a fresh child of sel, the plan built by `mode`"""
        b = ds.select(sel)
        x_b, e_b = b.take_vertices(x), b.take_edges(e)
        layer.set_graph_handle(b.handle, b.vertex_offsets)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        before = duvenaud_plan_stats()
        os.environ["ATHENA_MP_BUCKET_PLAN"] = mode
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev0.record()
        b.handle.plan_duvenaud(lo, hi)
        t_call = time.perf_counter() - t0
        ev1.record()
        layer.forward(x_b, e_b)
        torch.cuda.synchronize()
        t_fwd = time.perf_counter() - t0
        now = duvenaud_plan_stats()
        assert now[mode + "_builds"] == before[mode + "_builds"] + 1 and now["reused"] > before["reused"], "the child was not planned as pinned"
        t_stream = 1e-3 * ev0.elapsed_time(ev1)
        rows = b.handle.n_rows
        b.close()
        return (t_call, t_stream, t_fwd), rows

    lines = [f"# scripts/bench_bucket_plan.py on {torch.cuda.get_device_name(0)}: dataset of {B} structures of 8 - 30 atoms ({n} atoms, {E} edges, "
             f"{handle.nnz} CSR entries); plan of degrees {lo} .. {hi}; layer F_v {Fv}, F_e {Fe}, T = 4, 10 outputs",
             f"# one warm-up of each route, then {a.repeats} repetitions each, the pin alternating, a new shuffled selection per repetition; milliseconds"]
    try:
        for m in a.batches:
            m = min(m, B)
            rng = np.random.default_rng(m)
            times = {"host": [], "device": []}
            rows = 0
            for rep in range(-1, a.repeats):                                    # repetition -1 is the warm-up
                for mode in (("host", "device") if rep % 2 == 0 else ("device", "host")):
                    sel = rng.permutation(B)[:m].astype(np.int32)
                    t, rows = one(sel, mode)
                    if rep >= 0:
                        times[mode].append(t)
            lines.append(f"batch of {m} structures (about {rows} vertices)")
            for mode in ("host", "device"):
                for k, what in enumerate(("plan call, host wall", "plan, stream (events)", "call to end of 1st forward")):
                    v = [1e3 * t[k] for t in times[mode]]
                    lines.append(f"  {mode:<6s} {what:<28s} min {min(v):9.3f}   median {statistics.median(v):9.3f}")
            med = {mode: statistics.median(t[2] for t in times[mode]) for mode in times}
            lines.append(f"  call to end of 1st forward, median: device / host = {med['device'] / med['host']:.4f}")
    finally:
        if old is None:
            os.environ.pop("ATHENA_MP_BUCKET_PLAN", None)
        else:
            os.environ["ATHENA_MP_BUCKET_PLAN"] = old
    text = "\n".join(lines)
    print(text)
    if a.out != "-":
        with open(a.out, "a") as f:
            f.write(text + "\n")
    ds.close()
    handle.close()


if __name__ == "__main__":
    main()
