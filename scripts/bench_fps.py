#!/usr/bin/env python3
"""Times farthest-point sampling (athena_mp_farthest_points, athena_amd/csrc/fps.hip) on points that are resident in HBM, on the
MI355X, in three dimensions:

  batch            1 024 clouds of 4 096 uniform points, 256 samples each: the register route, one workgroup per cloud;
  stream_uniform   one cloud of 1 000 000 uniform points, 4 096 samples: the stream route, on ONE compute unit;
  stream_graded    the same size, strongly graded (every coordinate the fourth power of a uniform number: the density varies by
                   orders of magnitude);
  stream_unpruned  stream_uniform through a library built for this run with -DATHENA_MP_FPS_NO_PRUNE (every chunk that holds an
                   unchosen point is read at every step): what the exact pruning saves;
  host             the route without a device sampler: the points to the host, the numpy loop of the yardstick (one pass over the
                   cloud per sample), the samples uploaded.  Run at --host-samples samples (default 256) of the 1 000 000-point
                   cloud, the size that finishes, once; the device at that size beside it.

After one warm-up call, the median of --repeats calls with min and max beside it; host clock around a call that ends in a device
synchronise.  One JSON record per case, the stream cases with the skipped share of the chunk tests (athena_mp_fps_stats).  There is
no pass/fail time.

  python scripts/bench_fps.py [--repeats 5] [--points 1000000] [--only CASE] [--out profiles/fps.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ("batch", "stream_uniform", "stream_graded", "stream_unpruned", "host")
UNPRUNED = os.path.join(ROOT, "athena_amd", "libathena_mp_fps_noprune.so")


def unpruned_library():
    """fps.hip alone with the build flag, beside the product library (whose error plumbing and stream it uses), built when it is
    missing or older than its source; -Bsymbolic: its entry calls its own kernels, whatever was loaded before it"""
    src = os.path.join(ROOT, "athena_amd", "csrc", "fps.hip")
    if not os.path.exists(UNPRUNED) or os.path.getmtime(UNPRUNED) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                               "-DATHENA_MP_FPS_NO_PRUNE", "-shared", src, "-o", UNPRUNED, "-L" + os.path.join(ROOT, "athena_amd"),
                               "-lathena_mp", "-Wl,-Bsymbolic", "-Wl,-rpath,$ORIGIN"])
    lib = C.CDLL(UNPRUNED)
    lib.athena_mp_farthest_points.restype = C.c_int
    lib.athena_mp_fps_stats.restype = C.c_int
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--host-samples", type=int, default=256)
    ap.add_argument("--only", choices=CASES)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps.json"))
    a = ap.parse_args()
    import torch

    import fps_reference as fr
    from athena_amd import _capi

    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    _capi.init(0)
    dev = torch.device("cuda:0")
    _capi.use_torch_stream()
    lib = _capi.load()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    want = lambda c: a.only in (None, c)
    rng = np.random.Generator(np.random.PCG64(17))
    records = []

    def run(name, what, p, off, soff, library=lib, repeats=a.repeats):
        B, n, m = off.size - 1, p.shape[0], int(soff[-1])
        pd = torch.from_numpy(p).to(dev)
        sample = torch.empty((m,), dtype=torch.int32, device=dev)
        sp = torch.empty((m, 3), dtype=torch.float32, device=dev)
        sq = torch.empty((m,), dtype=torch.float32, device=dev)
        cover = torch.empty((B,), dtype=torch.float32, device=dev)

        def once():
            t0 = time.perf_counter()
            rc = library.athena_mp_farthest_points(C.c_int32(B), C.c_int32(n), vp(off), C.c_int32(3), ptr(pd), C.c_int32(m), vp(soff), None,
                                                   ptr(sample), ptr(sp), ptr(sq), ptr(cover))
            _capi.check(rc, "athena_mp_farthest_points")
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        once()
        stats = np.zeros(4, np.int64)
        library.athena_mp_fps_stats(vp(stats))
        t = [once() for _ in range(repeats)]
        ms = statistics.median(t) * 1e3
        rec = {"case": name, "what": what, "clouds": B, "points": n, "samples": m, "ms_per_call": round(ms, 3),
               "ms_min": round(min(t) * 1e3, 3), "ms_max": round(max(t) * 1e3, 3), "us_per_step": round(ms * 1e3 / max(int(np.diff(soff).max()), 1), 3),
               "clouds_on_the_stream_route": int(stats[3]), "chunk_tests": int(stats[1]), "chunks_skipped": int(stats[2]),
               "skipped_share": round(float(stats[2]) / float(stats[1]), 4) if stats[1] else None,
               "cover_radius_max": float(np.sqrt(cover.cpu().numpy().max())), "repeats": repeats, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        return pd, sample

    if want("batch"):
        B, n, m = 1024, 4096, 256
        run("batch", f"{B} clouds of {n} uniform points, {m} samples each (register route)", rng.random((B * n, 3)).astype(np.float32),
            fr.offsets_of([n] * B), fr.offsets_of([m] * B))
    n = a.points
    uniform = rng.random((n, 3)).astype(np.float32)
    off = fr.offsets_of([n])
    if want("stream_uniform"):
        run("stream_uniform", f"one cloud of {n} uniform points, {a.samples} samples (stream route, one compute unit)", uniform, off,
            fr.offsets_of([a.samples]))
    if want("stream_graded"):
        run("stream_graded", f"one cloud of {n} points, every coordinate u^4 of a uniform u, {a.samples} samples",
            (rng.random((n, 3)) ** 4).astype(np.float32), off, fr.offsets_of([a.samples]))
    if want("stream_unpruned"):
        run("stream_unpruned", "stream_uniform built with -DATHENA_MP_FPS_NO_PRUNE: no chunk with an unchosen point is skipped", uniform,
            off, fr.offsets_of([a.samples]), library=unpruned_library(), repeats=min(a.repeats, 3))
    if want("host"):
        mh = a.host_samples
        pd, sample = run("device_at_the_host_size", f"one cloud of {n} uniform points, {mh} samples: the device beside the host route",
                         uniform, off, fr.offsets_of([mh]))
        t0 = time.perf_counter()
        ph = pd.cpu().numpy()
        hs, hp, _, _ = fr.brute_force(ph, fr.offsets_of([mh]))
        up = torch.from_numpy(hs).to(dev), torch.from_numpy(hp).to(dev)
        torch.cuda.synchronize()
        t_host = time.perf_counter() - t0
        assert np.array_equal(hs, sample.cpu().numpy()), "the host loop and the device disagree"
        rec = {"case": "host", "what": f"points D2H + the numpy loop of tests/fps_reference.py + samples H2D, {n} points, {mh} samples, once",
               "points": n, "samples": mh, "ms": round(t_host * 1e3, 1), "host_vs_device": round(t_host * 1e3 / records[-1]["ms_per_call"], 1)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del up
    if a.out != "-":
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
