#!/usr/bin/env python3
"""Times the voxel-grid clusters (athena_mp_grid_clusters, athena_amd/csrc/grid_clusters.hip) on points that are resident in HBM, on
the MI355X, in three dimensions, every output asked for:

  uniform_4096 / uniform_65536   one cloud of 1 000 000 uniform points (the generator of scripts/bench_fps.py), the cell size chosen
                                 so that about 4 096 / about 65 536 clusters result;
  graded_4096 / graded_65536     the same size, strongly graded (every coordinate the fourth power of a uniform number); the size is
                                 found by bisection on the host;
  batch                          1 024 clouds of 4 096 uniform points, 64 cells each;
  wide_key                       the uniform cloud at size 2^-11: 2049^3 cells, keys of more than 32 bits.

After one warm-up call, the median of --repeats calls with min and max beside it; host clock around a call that ends in a device
synchronise.  Beside each case: the farthest-point sampler at the same number of coarse points where profiles/fps.json has one, and
a torch transcription on the device -- torch.unique(keys, return_inverse=True) + index_add_ + a division -- with its time, whether
its centroids are the same bytes in every run, and how far they lie from this library's.  There is no pass/fail time.

The per-launch times come from a run of their own under the profiler, one case at a time, merged afterwards:

  python scripts/bench_grid_clusters.py [--repeats 7] [--only CASE] [--out profiles/grid_clusters.json]
  rocprofv3 --kernel-trace --stats -f csv -d DIR/CASE -- python scripts/bench_grid_clusters.py --only CASE --repeats 3 --no-torch --out -
  python scripts/bench_grid_clusters.py --merge DIR --out profiles/grid_clusters.json      (DIR/CASE/**/*kernel_stats.csv)
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("uniform_4096", "uniform_65536", "graded_4096", "graded_65536", "batch", "wide_key")
FPS_BESIDE = {"uniform_4096": "stream_uniform", "graded_4096": "stream_graded", "batch": "batch"}


def cells_on_host(p, size):
    """the clusters of one cloud at this size: the cell function in numpy float32"""
    inv = np.float32(1) / np.float32(size)
    lo = p.min(axis=0) + np.float32(0)
    c = ((p - lo) * inv).astype(np.int64)
    nc = c.max(axis=0) + 1
    return np.unique((c[:, 2] * nc[1] + c[:, 1]) * nc[0] + c[:, 0]).size


def size_for(p, target):
    """a size at which about `target` clusters result, by bisection (the count falls as the size grows)"""
    small, large = 1e-4, 2.0
    for _ in range(30):
        mid = float(np.sqrt(small * large))
        if cells_on_host(p, mid) > target:
            small = mid
        else:
            large = mid
    return float(np.float32(large))


def merge(directory, out):
    """the kernel statistics of the profiled runs into the records of `out`: per kernel its launches per call and mean microseconds"""
    records = json.load(open(out))
    for rec in records:
        files = glob.glob(os.path.join(directory, rec["case"], "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            continue
        calls_per_run = None
        launches = []
        for row in csv.DictReader(open(files[0])):
            name = row["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            launches.append({"kernel": name, "launches": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 2),
                             "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1)})
            if "gc_key_kernel" in name:
                calls_per_run = int(row["Calls"])
        own = [l for l in launches if any(t in l["kernel"] for t in ("gc_", "radix", "scan64", "rg_", "rgb_", "bip_rowptr"))]
        if calls_per_run:
            for l in own:
                l["launches_per_call"] = round(l["launches"] / calls_per_run, 2)
                l["us_per_call"] = round(l["total_us"] / calls_per_run, 1)
        rec["launches"] = sorted(own, key=lambda l: -l["total_us"])
        rec["kernel_us_per_call"] = round(sum(l.get("us_per_call", 0.0) for l in own), 1)
    with open(out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--only", choices=CASES)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch transcription (profiled runs)")
    ap.add_argument("--merge", metavar="DIR", help="merge the profiler's kernel statistics under DIR/CASE into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_clusters.json"))
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    import torch

    from athena_amd import _capi

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    _capi.use_torch_stream()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    want = lambda c: a.only in (None, c)
    rng = np.random.Generator(np.random.PCG64(17))
    fps = {}
    fps_path = os.path.join(ROOT, "profiles", "fps.json")
    if os.path.exists(fps_path):
        fps = {r["case"]: r for r in json.load(open(fps_path))}
    records = []

    def timed(f, repeats):
        f()
        t = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return round(statistics.median(t) * 1e3, 3), round(min(t) * 1e3, 3), round(max(t) * 1e3, 3)

    def run(name, what, p, off, size):
        B, n = off.size - 1, p.shape[0]
        pd = torch.from_numpy(p).to(dev)
        cluster = torch.empty((n,), dtype=torch.int32, device=dev)
        pairs = torch.empty((n, 2), dtype=torch.int32, device=dev)
        rowptr = torch.empty((n + 1,), dtype=torch.int32, device=dev)
        weights = torch.empty((n,), dtype=torch.float32, device=dev)
        centroid = torch.empty((n, 3), dtype=torch.float32, device=dev)
        nearest = torch.empty((n,), dtype=torch.int32, device=dev)
        cell = torch.empty((n, 3), dtype=torch.int32, device=dev)
        coff, m = np.zeros(B + 1, np.int32), C.c_int64()

        def once():
            _capi.call("athena_mp_grid_clusters", B, n, vp(off), 3, ptr(pd), float(size), None, n, ptr(cluster), ptr(pairs), ptr(rowptr),
                       ptr(weights), ptr(centroid), ptr(nearest), ptr(cell), vp(coff), None, C.byref(m))

        ms, ms_min, ms_max = timed(once, a.repeats)
        stats = np.zeros(4, np.int64)
        _capi.call("athena_mp_grid_clusters_stats", vp(stats))
        rec = {"case": name, "what": what, "clouds": B, "points": n, "size": float(size), "clusters": int(m.value), "key_bits": int(stats[1]),
               "radix_passes": int(stats[2]), "largest_cluster": int(stats[3]), "ms_per_call": ms, "ms_min": ms_min, "ms_max": ms_max,
               "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
        beside = fps.get(FPS_BESIDE.get(name))
        if beside:
            rec["farthest_points_ms"] = beside["ms_per_call"]
            rec["farthest_points_samples"] = beside["samples"]
        if not a.no_torch:
            cloud = torch.from_numpy(np.repeat(np.arange(B), np.diff(off))).to(dev)
            inv = float(np.float32(1) / np.float32(size))

            def transcription():
                lo = torch.full((B, 3), float("inf"), device=dev).scatter_reduce_(0, cloud[:, None].expand(-1, 3), pd, "amin")
                c = ((pd - lo[cloud]) * inv).floor().to(torch.int64)
                nc = c.max(dim=0).values + 1
                keys = ((cloud * nc[2] + c[:, 2]) * nc[1] + c[:, 1]) * nc[0] + c[:, 0]
                uniq, inverse = torch.unique(keys, return_inverse=True)
                sums = torch.zeros((uniq.numel(), 3), device=dev).index_add_(0, inverse, pd)
                return sums / torch.bincount(inverse, minlength=uniq.numel())[:, None]

            t_ms, t_min, t_max = timed(transcription, a.repeats)
            runs = [transcription().cpu().numpy() for _ in range(3)]
            ours = centroid[:m.value].cpu().numpy()
            rec.update(torch_ms=t_ms, torch_ms_min=t_min, torch_ms_max=t_max, torch_clusters=int(runs[0].shape[0]),
                       torch_centroids_reproducible=bool(all(r.tobytes() == runs[0].tobytes() for r in runs[1:])),
                       torch_runs_max_abs_difference=float(max(np.abs(r - runs[0]).max() for r in runs[1:])),
                       torch_vs_library_max_abs_difference=float(np.abs(runs[0] - ours).max()) if runs[0].shape == ours.shape else None)
        print(json.dumps(rec), flush=True)
        records.append(rec)

    n = a.points
    one = np.array([0, n], np.int32)
    # the order of the draws is that of scripts/bench_fps.py: the batch first, then the uniform cloud, then the graded one
    batch = rng.random((1024 * 4096, 3)).astype(np.float32)
    uniform = rng.random((n, 3)).astype(np.float32)
    graded = (rng.random((n, 3)) ** 4).astype(np.float32)
    if want("uniform_4096"):
        run("uniform_4096", f"one cloud of {n} uniform points, 16 cells an axis", uniform, one, 1.0 / 16)
    if want("uniform_65536"):
        run("uniform_65536", f"one cloud of {n} uniform points, 40 cells an axis", uniform, one, 1.0 / 40)
    for target in (4096, 65536):
        if want(f"graded_{target}"):
            run(f"graded_{target}", f"one cloud of {n} points, every coordinate u^4 of a uniform u, the size bisected for {target} clusters",
                graded, one, size_for(graded, target))
    if want("batch"):
        run("batch", "1024 clouds of 4096 uniform points, 4 cells an axis", batch, (np.arange(1025) * 4096).astype(np.int32), 0.25)
    if want("wide_key"):
        run("wide_key", f"one cloud of {n} uniform points at size 2^-11: 2049^3 cells", uniform, one, 2.0 ** -11)
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
