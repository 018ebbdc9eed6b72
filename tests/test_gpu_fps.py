"""GPU: athena_mp_farthest_points (athena_amd/csrc/fps.hip) against the brute-force transcription of the definition
(tests/fps_reference.py).  Every output is compared with np.array_equal, the floats by their int32 view, on every shape class of
tests/test_fps.py, under each route the cloud fits (ATHENA_MP_FPS_ROUTE), and the routes against each other byte for byte."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import fps_reference as fr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "fps_run")
vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
CASES = fr.shape_cases()
ROUTED = [(c, route) for c in range(len(CASES)) for route in ("auto", "registers", "stream")
          if route != "registers" or np.diff(CASES[c][2]).max() <= fr.CAPACITY]


@functools.lru_cache(None)
def _brute(c):
    name, p, off, soff, start = CASES[c]
    return fr.brute_force(p, soff, off, start)


def _device(dev, p, soff, off=None, start=None):
    """(sample, sample_points, sample_sqdist, cover_sqdist) of the device, into buffers that show an entry left unwritten"""
    import torch
    from athena_amd import _capi

    _capi.use_torch_stream()
    off = fr.offsets_of([p.shape[0]]) if off is None else off
    B, n, dim, m = off.size - 1, p.shape[0], p.shape[1], int(soff[-1])
    pd = torch.from_numpy(p).to(dev)
    sample = torch.full((m,), -1, dtype=torch.int32, device=dev)
    sp = torch.full((m, dim), float("nan"), dtype=torch.float32, device=dev)
    sq = torch.full((m,), float("nan"), dtype=torch.float32, device=dev)
    cover = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    _capi.call("athena_mp_farthest_points", B, n, vp(off), dim, ptr(pd), m, vp(soff), vp(start), ptr(sample), ptr(sp), ptr(sq), ptr(cover))
    torch.cuda.synchronize()
    return sample.cpu().numpy(), sp.cpu().numpy(), sq.cpu().numpy(), cover.cpu().numpy()


def _stats():
    from athena_amd import _capi

    out = np.zeros(4, np.int64)
    _capi.call("athena_mp_fps_stats", vp(out))
    return out


def _assert_same(got, want, what=""):
    for g, w, name in zip(got, want, ("sample", "sample_points", "sample_sqdist", "cover_sqdist")):
        assert g.shape == w.shape and np.array_equal(g.view(np.int32), w.view(np.int32)), f"{what}: {name} differs"


@pytest.mark.parametrize("c,route", ROUTED, ids=[f"{CASES[c][0]}-{route}" for c, route in ROUTED])
def test_the_shape_classes_of_the_cpu_tests(dev, monkeypatch, c, route):
    name, p, off, soff, start = CASES[c]
    monkeypatch.setenv("ATHENA_MP_FPS_ROUTE", route)
    got = _device(dev, p, soff, off, start)
    want = _brute(c)
    _assert_same(got, want, f"{name} ({route})")
    streamed = _stats()[3]
    if route == "registers":
        assert streamed == 0
    if route == "stream":
        assert streamed == int(((np.diff(soff) > 0) & (np.diff(off) > 0)).sum())
    if "3e38" in name:
        assert np.isinf(want[2][1:]).any(), "the case must hold a squared distance that overflows"


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_a_stream_cloud_of_more_than_one_group_per_wave(dev, dim):
    """64 chunks a group, 16 waves: beyond 65536 points a wave owns a second group"""
    n = 64 * 64 * 16 + 64 * 70 + 5
    p = np.concatenate([fr.clustered(n - 20000, dim, 61 + dim, spread=0.01), fr._rng(62).random((20000, dim)).astype(np.float32)])
    soff = fr.offsets_of([24])
    _assert_same(_device(dev, p, soff, start=np.array([n], np.int32)), fr.brute_force(p, soff, start=np.array([n], np.int32)))
    st = _stats()
    assert st[0] == 24 and st[3] == 1 and st[1] == 24 * ((n + 63) // 64) and 0 < st[2] < st[1]


def test_a_clustered_stream_cloud_skips_chunks(dev):
    p = fr.clustered(6000, 3, 63)
    soff = fr.offsets_of([64])
    _assert_same(_device(dev, p, soff), fr.brute_force(p, soff))
    st = _stats()
    assert st[3] == 1 and st[2] > 0, "no chunk was skipped"


def test_both_routes_in_one_call_and_the_single_calls_shifted(dev):
    sizes, m = [5000, 0, 300, fr.CAPACITY + 1, 10, fr.CAPACITY], [20, 0, 300, 0, 10, 7]
    p = fr._rng(64).random((sum(sizes), 2)).astype(np.float32)
    off, soff = fr.offsets_of(sizes), fr.offsets_of(m)
    got = _device(dev, p, soff, off)
    assert _stats()[3] == 1
    _assert_same(got, fr.brute_force(p, soff, off))
    assert got[3][1] == 0 and np.isinf(got[3][3])
    for b in range(len(sizes)):
        if m[b] == 0:
            continue
        one = _device(dev, np.ascontiguousarray(p[off[b]:off[b + 1]]), fr.offsets_of([m[b]]))
        assert np.array_equal(one[0] + off[b], got[0][soff[b]:soff[b + 1]])
        assert np.array_equal(one[2].view(np.int32), got[2][soff[b]:soff[b + 1]].view(np.int32)) and one[3][0] == got[3][b]


@pytest.mark.parametrize("n", [3000, 9000])
def test_fewer_samples_are_the_prefix(dev, n):
    p = fr._rng(65).random((n, 3)).astype(np.float32)
    full = _device(dev, p, fr.offsets_of([50]))
    assert np.isinf(full[2][0]) and (np.diff(full[2][1:]) <= 0).all() and full[3][0] <= full[2][-1]
    for m in (1, 17, 49):
        part = _device(dev, p, fr.offsets_of([m]))
        assert np.array_equal(part[0], full[0][:m]) and np.array_equal(part[2].view(np.int32), full[2][:m].view(np.int32))
        assert part[3][0] == full[2][m], "the cover of a prefix is the dmin of the next choice"


def test_two_calls_are_byte_identical_and_each_output_may_be_null_alone(dev):
    import torch
    from athena_amd import _capi

    p, off, soff = fr.mixed_batch()
    first, again = _device(dev, p, soff, off), _device(dev, p, soff, off)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    B, n, m = off.size - 1, p.shape[0], int(soff[-1])
    pd = torch.from_numpy(p).to(dev)
    for keep in range(4):
        outs = [torch.full((m,), -1, dtype=torch.int32, device=dev), torch.full((m, 3), float("nan"), dtype=torch.float32, device=dev),
                torch.full((m,), float("nan"), dtype=torch.float32, device=dev), torch.full((B,), float("nan"), dtype=torch.float32, device=dev)]
        args = [ptr(t) if i == keep else None for i, t in enumerate(outs)]
        _capi.call("athena_mp_farthest_points", B, n, vp(off), 3, ptr(pd), m, vp(soff), None, *args)
        torch.cuda.synchronize()
        assert np.array_equal(outs[keep].cpu().numpy().view(np.int32), first[keep].view(np.int32))
    _capi.call("athena_mp_farthest_points", B, n, vp(off), 3, ptr(pd), m, vp(soff), None, None, None, None, None)


def test_refusals_leave_the_library_usable(dev, monkeypatch):
    import torch
    from athena_amd import _capi
    from athena_amd._capi import AthenaMPError

    _capi.use_torch_stream()
    p, off, soff = fr.mixed_batch()
    want = fr.brute_force(p, soff, off)
    B, n, m = off.size - 1, p.shape[0], int(soff[-1])
    pd = torch.from_numpy(p).to(dev)
    sample = torch.empty((m,), dtype=torch.int32, device=dev)

    def call(B=B, n=n, off=off, dim=3, pd=pd, m=m, soff=soff, start=None):
        _capi.call("athena_mp_farthest_points", B, n, vp(off), dim, ptr(pd), m, vp(soff), vp(start), ptr(sample), None, None, None)

    def refused(match, **kw):
        with pytest.raises(AthenaMPError, match=match):
            call(**kw)
        sample.fill_(-1)
        call()                                             # the library stays usable
        assert np.array_equal(sample.cpu().numpy(), want[0])

    refused(r"dim = 4 outside \[1,3\]", dim=4)
    refused(r"dim = 0 outside \[1,3\]", dim=0)
    refused(r"n_clouds = -1 is negative", B=-1)
    bad = off.copy(); bad[0] = 1
    refused(r"offsets\(1\) = 1, not 0", off=bad)
    bad = off.copy(); bad[5] = bad[4] - 1
    refused(rf"cloud 5: offsets descend from {off[4]} to {off[4] - 1}", off=bad)
    refused(rf"offsets end at {n}, the batch has {n + 1} points", n=n + 1)
    bad = soff.copy(); bad[0] = 2
    refused(r"sample_offsets\(1\) = 2, not 0", soff=bad)
    bad = soff.copy(); bad[3] = bad[2] - 1
    refused(rf"cloud 3: sample_offsets descend from {soff[2]} to {soff[2] - 1}", soff=bad)
    refused(rf"sample_offsets end at {m}, the batch has {m - 1} samples", m=m - 1)
    bad = soff.copy(); bad[3:] += 1                        # cloud 3 has one point and is asked for two
    refused(r"cloud 3: 2 samples asked of 1 points", soff=bad, m=m + 1)
    start = np.zeros(B, np.int32); start[4] = off[5] + 1
    refused(rf"cloud 5: start = {off[5] + 1} outside its points {off[4] + 1} \.\. {off[5]}", start=start)
    start = np.zeros(B, np.int32); start[0] = -3
    refused(r"cloud 1: start = -3 outside its points", start=start)
    i = int(off[3]) + 2
    bad_p = p.copy(); bad_p[i, 1] = np.nan
    refused(rf"cloud 4: points\(2,{i + 1}\) = nan is not finite", pd=torch.from_numpy(bad_p).to(dev))
    j = int(off[6])
    bad_p = p.copy(); bad_p[j, 2] = -np.inf
    refused(rf"cloud 7: points\(3,{j + 1}\) = -inf is not finite", pd=torch.from_numpy(bad_p).to(dev))
    # the register route pinned on a cloud it cannot hold
    big = fr._rng(66).random((fr.CAPACITY + 1, 3)).astype(np.float32)
    monkeypatch.setenv("ATHENA_MP_FPS_ROUTE", "registers")
    with pytest.raises(AthenaMPError, match=rf"cloud 1: ATHENA_MP_FPS_ROUTE = registers holds {fr.CAPACITY} points, the cloud has {fr.CAPACITY + 1}"):
        _device(dev, big, fr.offsets_of([4]))
    monkeypatch.setenv("ATHENA_MP_FPS_ROUTE", "sideways")
    with pytest.raises(AthenaMPError, match=r'ATHENA_MP_FPS_ROUTE = "sideways" is none of auto, registers, stream'):
        call()
    monkeypatch.setenv("ATHENA_MP_FPS_ROUTE", "auto")
    sample.fill_(-1)
    call()
    assert np.array_equal(sample.cpu().numpy(), want[0])


def test_the_host_form_agrees_with_the_device_form(dev):
    from athena_amd import _capi

    for c in (len(CASES) - 1, [x[0] for x in CASES].index(f"n = {fr.CAPACITY + 1}, m = 32")):
        name, p, off, soff, start = CASES[c]
        B, n, dim, m = off.size - 1, p.shape[0], p.shape[1], int(soff[-1])
        out = np.full(m, -1, np.int32), np.full((m, dim), np.nan, np.float32), np.full(m, np.nan, np.float32), np.full(B, np.nan, np.float32)
        _capi.call("athena_mp_farthest_points_host", B, n, vp(off), dim, vp(p), m, vp(soff), vp(start), *(vp(a) for a in out))
        _assert_same(out, _device(dev, p, soff, off, start), name)
        _assert_same(out, _brute(c), name)


@pytest.mark.parametrize("has_start", [0, 1])
def test_fortran_program_writes_the_arrays_of_the_yardstick(dev, tmp_path, has_start):
    if not os.path.exists(RUNNER):
        pytest.fail("fps_run is not built: __graft_entry__.build() compiles the Fortran host side")
    c = len(CASES) - 1 if has_start else len(CASES) - 2
    name, p, off, soff, start = CASES[c]
    assert (start is not None) == bool(has_start)
    B, n, m = off.size - 1, p.shape[0], int(soff[-1])
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        np.array([B, n, 3, m, has_start], np.int32).tofile(f)
        off.tofile(f); soff.tofile(f); (start if has_start else np.zeros(B, np.int32)).tofile(f); p.tofile(f)
    out = subprocess.run([RUNNER, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"fps_run failed ({out.returncode}): {out.stdout[-1000:]} {out.stderr[-2000:]}"
    raw = open(res, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a

    got = take(np.int32, m), take(np.float32, 3 * m).reshape(m, 3), take(np.float32, m), take(np.float32, B)
    _assert_same(got, _brute(c), name)
    assert take(np.int64, 4).tolist() == [m, 0, 0, 0] and at == len(raw)


def test_the_samples_are_the_queries_of_a_graph_that_covers_every_point(dev):
    """the pipeline the sampler exists for: samples -> cover_radius -> from_point_sets over their own cloud, every source column
    of the handle has an entry; from_point_sets_knn(k = 1) takes the same arrays"""
    from athena_amd import DeviceGraph
    from athena_amd.geometry import cover_radius, farthest_points

    sizes = [5000, 0, 700, 1]
    p = np.concatenate([fr.clustered(5000, 3, 67, spread=0.02), fr._rng(68).random((701, 3)).astype(np.float32)])
    off = fr.offsets_of(sizes)
    sample, coarse, soff, cover, sqd = farthest_points(p, off, ratio=0.03, want_sqdist=True)
    assert np.diff(soff).tolist() == [150, 0, 21, 1]
    want = fr.brute_force(p, soff, off)
    _assert_same((sample.cpu().numpy(), coarse.cpu().numpy(), sqd.cpu().numpy(), cover.cpu().numpy()), want)
    r = cover_radius(cover)
    below = np.nextafter(np.float32(r), np.float32(0))
    assert np.float32(r) * np.float32(r) >= want[3].max() and below * below < want[3].max()
    handle, coords, eoff, ia, ja = DeviceGraph.from_point_sets(coarse, p, r, query_offsets=soff, source_offsets=off, want_adjacency=True)
    assert handle.n_rows == int(soff[-1]) and handle.n_cols == p.shape[0]
    assert np.unique(ja[0]).size == p.shape[0], "a point is left without a sample inside the covering radius"
    one, _, _ = DeviceGraph.from_point_sets_knn(coarse, p, 1, query_offsets=soff, source_offsets=off)
    assert one.nnz == int(soff[-1])             # every cloud that has samples has sources: one pair per sample
    per_cloud = farthest_points(p, off, n_samples=[3, 0, 2, 1])
    assert np.array_equal(per_cloud[2], [0, 3, 3, 5, 6]) and np.array_equal(per_cloud[0].cpu().numpy()[:3], want[0][:3])
    with pytest.raises(ValueError, match="exactly one of n_samples and ratio"):
        farthest_points(p, off)
