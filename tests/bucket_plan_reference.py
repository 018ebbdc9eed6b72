"""The Duvenaud degree-bucket plan in numpy: a transcription of the definition in include/athena_mp.h (athena_mp_duvenaud_plan), the
yardstick of tests/test_bucket_plan.py and tests/test_gpu_bucket_plan.py.  The sort is numpy's stable argsort; nothing here is shared
with the library's builders."""
import numpy as np

NAMES = ("bucket_perm", "btile_start", "btile_info", "btile_rows", "btile_off_dev", "bucket_off", "btile_off")


def plan_reference(deg, min_deg, max_deg):
    """dict of the seven arrays for the degrees deg [n]: bucket_perm [n], btile_start [nt], btile_info [nt], btile_rows [4, 16 nt],
    btile_off_dev [nb + 1] (int32), bucket_off [nb + 1] (int64), btile_off [nb + 1] (int32)"""
    deg = np.asarray(deg, dtype=np.int64).reshape(-1)
    if not min_deg <= max_deg:
        raise ValueError("min_deg must not exceed max_deg")
    nb = max_deg - min_deg + 1
    bucket = np.clip(deg, min_deg, max_deg) - min_deg
    perm = np.argsort(bucket, kind="stable").astype(np.int32)
    bucket_off = np.concatenate([[0], np.cumsum(np.bincount(bucket, minlength=nb))]).astype(np.int64)
    start, info, tile_off = [], [], [0]
    for b in range(nb):
        for i in range(int(bucket_off[b]), int(bucket_off[b + 1]), 16):
            start.append(i)
            info.append((b << 8) | min(16, int(bucket_off[b + 1]) - i))
        tile_off.append(len(start))
    nt = len(start)
    rows = np.zeros((4, 16 * nt), np.int32)
    for t in range(nt):
        count = info[t] & 255
        for i in range(16):
            v = int(perm[start[t] + (i if i < count else 0)])
            sv = v if i < count else ~v
            tp = 4 * (i & 3) + (i >> 2)
            rows[0, 16 * t + i] = sv
            rows[1, 16 * t + i] = v
            rows[2, 16 * t + tp] = v
            rows[3, 16 * t + tp] = sv
    toff = np.asarray(tile_off, np.int32)
    return {"bucket_perm": perm, "btile_start": np.asarray(start, np.int32).reshape(-1), "btile_info": np.asarray(info, np.int32).reshape(-1),
            "btile_rows": rows, "btile_off_dev": toff, "bucket_off": bucket_off, "btile_off": toff.copy()}


def same(a, b):
    """byte equality of two plans, array by array: the name of the first array that differs, or None"""
    for k in NAMES:
        if not (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()):
            return k
    return None
