"""Shared test utilities: seeded graphs in athena's CSR convention and an INDEPENDENT float64
dense-matrix formulation of each op (from the layer documentation, not from the oracle's loops)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)


def csr_from_index_list(n, index_list, self_loops=False):
    from athena_amd.graph import graph_type

    g = graph_type()
    g.set_num_vertices(n, 0)
    g.generate_adjacency(np.asarray(index_list))
    if self_loops:
        g.add_self_loops()
    return g


def random_graph(n, n_pairs, seed, self_loops=True, isolated=0):
    """random multigraph; `isolated` trailing vertices get no entries at all (zero-degree rows)."""
    from athena_amd import synth

    m = n - isolated
    ia, ja = synth.random_graph_csr(m, n_pairs, seed=seed, self_loops=self_loops)
    if isolated:
        ia = np.concatenate([ia, np.full(isolated, ia[-1], np.int32)])
    return ia, ja


def dense_adjacency(ia, ja, n_cols=None):
    """A[v,u] = multiplicity of u in row v (float64)"""
    n = ia.size - 1
    A = np.zeros((n, n_cols or n), np.float64)
    for v in range(n):
        for w in range(ia[v] - 1, ia[v + 1] - 1):
            A[v, ja[0, w] - 1] += 1.0
    return A


def kipf_dense(ia, ja, x):
    """D^-1/2 A D^-1/2 X with D = CSR row length (docs/source/layers/msgpass/kipf_msgpass_layer.rst)"""
    A = dense_adjacency(ia, ja)
    deg = np.diff(ia).astype(np.float64)
    with np.errstate(divide="ignore"):
        dinv = np.where(deg > 0, deg ** -0.5, 0.0)
    return (dinv[:, None] * A * dinv[None, :]) @ x.astype(np.float64)


def rel_err(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def assert_close(a, b, rtol=1e-5, what="", f64=None):
    """north-star tolerance: 1e-5 relative fp32 (relative to the tensor's scale) against the fp32 oracle `b`.

    f64 (an array, or a callable evaluated only when needed): the SAME reference formulas evaluated in float64
    (oracle/oracle64.py).  Chains of fp32 roundings (a reduction over thousands of vertices, several layers in a row) can
    put the fp32 oracle itself more than 1e-5 from exact arithmetic; the device result then passes when it is no further
    from the float64 value than the oracle is, plus rtol:  |a - f64| <= |b - f64| + rtol * scale.  A device result that is
    simply wrong fails both tests."""
    e = rel_err(a, b)
    if e <= rtol:
        return
    if f64 is not None:
        ref = np.asarray(f64() if callable(f64) else f64, np.float64)
        scale = max(np.abs(ref).max(), 1e-30)
        e_dev = float(np.abs(np.asarray(a, np.float64) - ref).max() / scale)
        e_orc = float(np.abs(np.asarray(b, np.float64) - ref).max() / scale)
        assert e_dev <= e_orc + rtol, (f"{what}: {e:.3e} from the fp32 oracle; {e_dev:.3e} from float64 where the oracle "
                                       f"itself is {e_orc:.3e} (allowed: oracle's distance + {rtol})")
        return
    assert e <= rtol, f"{what}: rel err {e:.3e} > {rtol}"


def assert_close_elementwise(a, b, scale, rtol=1e-5, what=""):
    """element-wise check for sums: |a - b| <= rtol * scale element by element, where `scale` is the sum of the
    MAGNITUDES of the terms of each element (the quantity fp32 summation error is relative to; an element whose terms
    cancel is not held to a relative error of its tiny value, and is not excused by the tensor's maximum either)."""
    a, b, scale = (np.asarray(t, np.float64) for t in (a, b, scale))
    bad = np.abs(a - b) > rtol * scale + 1e-30
    assert not bad.any(), f"{what}: {int(bad.sum())} element(s) beyond {rtol} of their term magnitudes; worst {float((np.abs(a - b) / np.maximum(scale, 1e-30)).max()):.3e}"


def elementwise_worst(a, b, scale):
    """max over the elements of |a - b| / scale, scale = the sum of the MAGNITUDES of each element's terms (the oracle run on
    |operands|): the strongest element-wise statement fp32 sums allow -- an element whose terms cancel is held to the size of
    what was added, not to its tiny value, and no element hides behind the tensor's maximum"""
    a, b, scale = (np.asarray(t, np.float64) for t in (a, b, scale))
    return float((np.abs(a - b) / np.maximum(scale, 1e-30)).max()) if a.size else 0.0


# ---- graphs with chosen row lengths and column counts (tests/test_segment_reference.py, tests/test_gpu_hub_rows.py) ---------------
# every length at which the hub route of agg.hip changes: empty, one entry, either side of kLongRow = 512 (512 is still a short
# row, 513 has a second segment of ONE entry), either side of two and three full segments, and a six-segment row
HUB_LENGTHS = (0, 1, 511, 512, 513, 1023, 1024, 1025, 1536, 1537, 2600)


def hub_length_layout(n, rng, fill=3):
    """lengths [n] holding HUB_LENGTHS where position matters: a hub as row 0 beside an empty row, 513 / 1023 / 1024 / 1025 as
    adjacent rows, a hub between two empty rows in the middle, a hub as the last row; every other row has 1..fill entries, but
    for some empty ones"""
    assert n >= 64
    lens = rng.integers(1, fill + 1, n).astype(np.int64)
    lens[rng.choice(np.arange(16, n // 2 - 2), 24, replace=False)] = 0
    lens[:9] = [2600, 0, 1, 511, 512, 513, 1023, 1024, 1025]
    lens[n // 2 - 1:n // 2 + 2] = [0, 1536, 0]
    lens[n - 1] = 1537
    assert set(HUB_LENGTHS) <= set(lens.tolist())
    return lens


def spread_lengths(total, where):
    """lengths over the positions where `where` holds that add up to total, as even as they can be"""
    where = np.asarray(where, bool)
    m = int(where.sum())
    out = np.zeros(where.size, np.int64)
    out[where] = total // m
    out[np.nonzero(where)[0][:total % m]] += 1
    return out


def graph_from_lengths(row_len, col_len, rng, edge_cols=0):
    """(adj_ia, adj_ja) of a multigraph whose row r has row_len[r] entries and whose column u is listed col_len[u] times (the two
    add up to the same): the columns are a random permutation of the multiset.  edge_cols > 0: every entry carries a random edge
    column 1..edge_cols, about one in eight none (0)"""
    row_len, col_len = np.asarray(row_len, np.int64), np.asarray(col_len, np.int64)
    assert row_len.sum() == col_len.sum()
    ia = np.concatenate([[1], 1 + np.cumsum(row_len)]).astype(np.int32)
    ja = np.zeros((2, int(row_len.sum())), np.int32, order="F")
    ja[0] = rng.permutation(np.repeat(np.arange(1, col_len.size + 1), col_len))
    if edge_cols:
        ja[1] = np.where(rng.integers(0, 8, ja.shape[1]) == 0, 0, rng.integers(1, edge_cols + 1, ja.shape[1]))
    return ia, ja


# ---- operands at chosen alignments, between guards (tests/test_gpu_unaligned.py) ---------------------------------------------------
# A torch allocation starts on a 256-byte boundary and is rounded up to 512 bytes, so a fresh tensor never shows what a kernel does
# with a pointer that is only 4- or 8-byte aligned, nor a store a few elements past the end.  placed / placed_out put an operand k
# elements past a 512-byte boundary inside a larger buffer filled with a sentinel:
#   k = 1   4-byte aligned
#   k = 2   8-byte aligned
#   k = 4   16-byte aligned, but 16 bytes off every 32-byte (and 256-, 512-byte) boundary, flush against its guards
SENTINEL = {"float32": 0x7FC0ABCD, "int32": 0x5A5A5A5A}   # a quiet NaN with a payload / a pattern no index or count takes


def _placed_raw(n, dtype, dev, k, guard):
    """(raw int32 buffer filled with the sentinel of dtype, index of the operand's first element)"""
    import torch

    name = str(dtype).replace("torch.", "")
    assert name in SENTINEL and k >= 0 and guard >= 0
    lead = 128 * ((guard + 127) // 128)                    # whole 512-byte blocks that hold the front guard
    raw = torch.full((127 + lead + k + n + guard,), SENTINEL[name], dtype=torch.int32, device=dev)
    assert raw.data_ptr() % 4 == 0
    first = (-(raw.data_ptr() // 4)) % 128                 # elements up to the next 512-byte boundary, whatever the allocator returned
    return raw, first + lead + k


def placed(array, dev, k, guard=256):
    """`array` (numpy float32 / int32) on the device, its first element k elements past a 512-byte boundary, `guard` sentinel
    elements on both sides; returns the contiguous view"""
    import torch

    a = np.ascontiguousarray(array)
    t = torch.from_numpy(a)
    raw, s = _placed_raw(a.size, t.dtype, dev, k, guard)
    view = raw[s:s + a.size].view(t.dtype).reshape(a.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * k) % 16 and (view.data_ptr() - 4 * k) % 512 == 0
    return view


def placed_out(shape, dtype, dev, k, guard=256, init=None):
    """an output of this shape placed like `placed`, pre-filled with the sentinel (init: the contents of an in-place operand
    instead); returns (view, check): check() asserts, word for word, that no guard element on either side was written"""
    import torch

    n = int(np.prod(shape))
    raw, s = _placed_raw(n, dtype, dev, k, guard)
    view = raw[s:s + n].view(dtype).reshape(tuple(shape))
    if init is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(init)))
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * k) % 16 and (view.data_ptr() - 4 * k) % 512 == 0
    word = SENTINEL[str(dtype).replace("torch.", "")]

    def check(what=""):
        torch.cuda.synchronize()
        front, back = raw[s - guard:s], raw[s + n:s + n + guard]
        for side, part in (("before", front), ("after", back)):
            bad = torch.nonzero(part != word).flatten()
            assert bad.numel() == 0, (f"{what}: {bad.numel()} guard word(s) {side} the output overwritten, the first at element "
                                      f"{int(bad[0]) - (guard if side == 'before' else 0)} relative to that end")

    return view, check


def unwritten(view):
    """number of elements of an output from placed_out that still hold the sentinel (compared as words: a NaN equals nothing)"""
    import torch

    word = SENTINEL[str(view.dtype).replace("torch.", "")]
    return int((view.reshape(-1).view(torch.int32) == word).sum())
