"""CPU: host-side logic and the C-ABI library surface (no compute calls without a GPU)."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import csr_from_index_list, golden


def test_library_loads_and_exports_every_declared_symbol():
    from athena_amd import _capi

    assert os.path.exists(_capi.LIB_PATH), "build with __graft_entry__.build()"
    lib = _capi.load()
    declared = _capi.declared_symbols()
    assert len(declared) >= 30
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, missing
    # every declared function has a ctypes prototype (so the binding cannot drift from the header)
    unbound = [s for s in declared if s not in _capi._PROTOS and s != "athena_mp_last_error"]
    assert not unbound, unbound
    assert lib.athena_mp_version() >= 100


def test_graph_type_matches_reference_test_graph():
    t = golden("reference_test_topologies.json")["kipf_layer_6v8e"]
    g = csr_from_index_list(6, t["index_list"])
    assert g.adj_ia.tolist() == [1, 3, 6, 9, 12, 15, 17]          # degrees 2,3,3,3,3,2
    assert g.nnz == 16 and g.adj_ja.shape == (2, 16)
    # each undirected edge id appears exactly twice, with mirrored endpoints
    rows = np.repeat(np.arange(1, 7), np.diff(g.adj_ia))
    for e in range(1, 9):
        w = np.nonzero(g.adj_ja[1] == e)[0]
        assert w.size == 2
        assert {(rows[w[0]], g.adj_ja[0, w[0]]), (rows[w[1]], g.adj_ja[0, w[1]])} == \
            {(t["index_list"][0][e - 1], t["index_list"][1][e - 1]), (t["index_list"][1][e - 1], t["index_list"][0][e - 1])}
    g.add_self_loops()
    assert g.nnz == 22 and np.diff(g.adj_ia).tolist() == [3, 4, 4, 4, 4, 3]
    rows = np.repeat(np.arange(1, 7), np.diff(g.adj_ia))
    loops = g.adj_ja[0] == rows
    assert loops.sum() == 6 and np.all(g.adj_ja[1, loops] == 0)
    g.add_self_loops()  # idempotent
    assert g.nnz == 22


def test_synth_generator_is_seeded_and_well_formed():
    from athena_amd import synth

    ia, ja = synth.random_graph_csr(1000, 4500)
    ia2, ja2 = synth.random_graph_csr(1000, 4500)
    assert np.array_equal(ia, ia2) and np.array_equal(ja, ja2)
    assert ia[0] == 1 and ia[-1] - 1 == ja.shape[1] == 10000
    rows = np.repeat(np.arange(1, 1001), np.diff(ia))
    assert np.all(ja[0, ia[:-1] - 1] == np.arange(1, 1001))       # self loop first in each row
    assert np.all((ja[1] == 0) == (ja[0] == rows))
    assert ja[0].min() >= 1 and ja[0].max() <= 1000


def test_all_graphs_text_format_round_trip(tmp_path):
    """the reference's graph interchange file (example/msgpass_chemical/src/main.f90:353-396): the committed
    fixture parses to the graphs its generator built, and write -> read is bit-identical (ES16.8E2 keeps
    9 significant digits, enough for float32)"""
    from athena_amd import io
    from athena_amd.graph import graph_type

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "all_graphs_small.txt")
    graphs, labels = io.read_all_graphs(path)
    assert [g.num_vertices for g in graphs] == [3, 5, 4, 6] and [g.num_edges for g in graphs] == [2, 5, 3, 6]
    assert all(g.num_vertex_features == 6 and g.num_edge_features == 1 for g in graphs)
    g0 = graphs[0]                       # path 1-2-3 with self loops: loops first (edge id 0), then by edge id
    assert g0.adj_ia.tolist() == [1, 3, 6, 8]
    assert g0.adj_ja.T.tolist() == [[1, 0], [2, 1], [2, 0], [1, 1], [3, 2], [3, 0], [2, 2]]
    ref = graph_type(); ref.set_num_vertices(5, 6)
    ref.generate_adjacency(np.array([[1, 2], [2, 3], [3, 4], [4, 5], [5, 1]]).T); ref.add_self_loops()
    assert np.array_equal(graphs[1].adj_ia, ref.adj_ia) and np.array_equal(graphs[1].adj_ja, ref.adj_ja)
    out = tmp_path / "again.txt"
    io.write_all_graphs(out, graphs, labels)
    assert open(out).read() == open(path).read()
    g2, l2 = io.read_all_graphs(out)
    assert np.array_equal(l2, labels)
    for a, b in zip(graphs, g2):
        assert np.array_equal(a.vertex_features, b.vertex_features) and np.array_equal(a.edge_features, b.edge_features)
        assert np.array_equal(a.adj_ja, b.adj_ja)
    # block-diagonal batch: offsets, shifted ids, self-loop id 0 untouched
    ia, ja, voff, x, e = io.batch_graphs(graphs)
    assert voff.tolist() == [0, 3, 8, 12, 18] and ia.size == 19 and ja.shape[1] == sum(g.nnz for g in graphs)
    assert x.shape == (18, 6) and e.shape == (16, 1)
    w0 = graphs[0].nnz
    assert np.array_equal(ja[0, w0:w0 + graphs[1].nnz], graphs[1].adj_ja[0] + 3)
    assert np.array_equal(ja[1, w0:w0 + graphs[1].nnz], np.where(graphs[1].adj_ja[1] > 0, graphs[1].adj_ja[1] + 2, 0))
    # a truncated file is an error, not a silent short read
    bad = tmp_path / "bad.txt"
    bad.write_text(" ".join(open(path).read().split()[:40]))
    with pytest.raises(ValueError, match="ended early|span"):
        io.read_all_graphs(bad)


def test_fortran_e16_8e2_field_formatting():
    """'(5(E16.8E2))' as the reference writes weights (athena_kipf_msgpass_layer.f90:430-433): 0.d mantissa of
    eight digits, two-digit exponent, 16 columns -- of the STORED float32 value"""
    from athena_amd.io import _e16, parse_layer_card

    assert _e16(1.0) == "  0.10000000E+01" and _e16(-1.0) == " -0.10000000E+01" and _e16(0.0) == "  0.00000000E+00"
    assert _e16(np.float32(0.3)) == "  0.30000001E+00"           # float32(0.3) = 0.300000011920929
    assert _e16(-9.87654321e-5) == " -0.98765432E-04" and _e16(0.999999999) == "  0.10000000E+01"
    assert all(len(_e16(v)) == 16 for v in (3.4e38, -1.17e-38, 123456.789))
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kipf_layer_card.txt")).read()
    name, hp, w = parse_layer_card(text)
    assert name == "kipf" and hp["NUM_VERTEX_FEATURES"] == "2 3 1" and hp["activation_name"] == "relu"
    assert w.tolist() == [0.5, -0.25, 0.125, -0.75, 1.5, 2.0, 1.5, -0.03125, 0.125]
    with pytest.raises(ValueError, match="Unrecognised line"):
        parse_layer_card(text.replace("   NUM_TIME_STEPS = 2", "   what is this"))


def test_e16_field_is_the_eight_digit_rounding_of_the_value_property():
    """hypothesis: for any finite float32, the E16.8E2 field is 16 columns, parses back to within half a unit of
    the eighth significant digit, re-prints identically (idempotent), and the mantissa is normalised 0.1 <= m < 1"""
    from hypothesis import given, settings, strategies as st

    from athena_amd.io import _e16

    @settings(max_examples=400, deadline=None)
    @given(st.floats(width=32, allow_nan=False, allow_infinity=False))
    def check(v):
        f = _e16(np.float32(v))
        assert len(f) == 16
        back = float(f)
        if v == 0.0:
            assert back == 0.0
            return
        assert abs(back - v) <= 0.5000001e-8 * 10.0 ** (np.floor(np.log10(abs(v))) + 1)
        assert _e16(back) == f
        m = f.strip().lstrip("-")
        assert m.startswith("0.") and m[2] != "0"

    check()


def test_activation_objects_and_their_card_blocks():
    """ops.actv_type mirrors base_actv_type: reset_* defaults, `apply_scaling` only beyond 1e-6 of one, unknown
    attributes rejected; the ACTIVATION block lists name, scale, then the activation's own attributes as
    adjustl(F10.6) in export_attributes_* order (athena_activation_{relu,leaky_relu,selu,gaussian,piecewise,swish}.f90)
    and reads back to an equal object"""
    from athena_amd import ops
    from athena_amd.io import _activation_block, activation_from_card

    assert ops.resolve_activation(ops.actv_type("relu")) == "relu"
    assert ops.resolve_activation(ops.actv_type("tanh", scale=1.0000005)) == "tanh"
    a = ops.resolve_activation(ops.actv_type("relu", threshold=0.1))
    assert isinstance(a, ops.actv_type) and a.p == [0.1, 0.0] and ops.needs_input(a) and not ops.needs_input("relu")
    assert ops.actv_type("selu").p == [1.67326, 1.0507] and ops.actv_type("selu", **{"lambda": 2.0}).p[1] == 2.0
    assert ops.actv_type("gaussian").p == [1.5, 0.0] and ops.actv_type("piecewise").p == [0.1, 1.0]
    assert ops.actv_type("leaky_relu").p[0] == 0.01
    with pytest.raises(ValueError, match="no attribute"):
        ops.actv_type("sigmoid", alpha=1.0)
    with pytest.raises(ValueError, match="unknown activation"):
        ops.actv_type("gelu")
    assert _activation_block("relu") == ["   ACTIVATION", "      name = relu", "      scale = 1.000000",
                                         "      threshold = 0.000000", "   END ACTIVATION"]
    blk = _activation_block(ops.actv_type("selu", scale=2.0), identifier="MESSAGE")
    assert blk == ["   ACTIVATION: MESSAGE", "      name = selu", "      scale = 2.000000", "      alpha = 1.673260",
                   "      lambda = 1.050700", "   END ACTIVATION"]
    assert _activation_block(ops.actv_type("swish", beta=0.5))[3] == "      beta = 0.500000"
    for a in (ops.actv_type("gaussian", sigma=0.7, mu=0.25), ops.actv_type("piecewise", gradient=0.3), ops.actv_type("swish", beta=2.0)):
        hp = {}
        for line in _activation_block(a)[1:-1]:
            k, v = (s.strip() for s in line.split("=", 1))
            hp["activation_" + k] = v
        b = activation_from_card(hp)
        assert (b.name, b.scale, b.p, b.beta) == (a.name, a.scale, a.p, a.beta)


def test_fortran_host_side_is_built():
    """__graft_entry__.build() compiles the Fortran host side (interface module, layer types, the boundary test and
    the case runner); the runner's usage path exits 2 without touching a GPU"""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runner = os.path.join(root, "athena_amd", "fortran", "athena_mp_layer_run")
    if not os.path.exists(runner):
        pytest.skip("Fortran host side not built here (run __graft_entry__.build())")
    r = subprocess.run([runner], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


def test_graph_key_is_a_content_key():
    """athena_mp_graph_key (host only, no device call): what a cached handle is valid for.  Equal content -> equal key;
    same vertex and entry counts with another adjacency -> another key (round 2's Fortran shim keyed on nnz alone);
    in-place edits of a mini-batch graph are always seen; above 2^18 entries head, tail and the strided sample are."""
    import ctypes as C

    from athena_amd import _capi

    def key(ia, ja):
        ia = np.ascontiguousarray(ia, np.int32)
        ja = np.asfortranarray(ja, np.int32)
        k = C.c_uint64(0)
        _capi.call("athena_mp_graph_key", ia.size - 1, ja.shape[1], ia.ctypes.data, ja.ctypes.data, C.byref(k))
        return k.value

    g = csr_from_index_list(6, golden("reference_test_topologies.json")["kipf_layer_6v8e"]["index_list"])
    k0 = key(g.adj_ia, g.adj_ja)
    assert k0 == key(g.adj_ia.copy(), g.adj_ja.copy())
    perm = np.array([2, 1, 3, 4, 5, 6])                      # rename two vertices: same counts, other adjacency
    idx = perm[np.asarray(golden("reference_test_topologies.json")["kipf_layer_6v8e"]["index_list"]) - 1]
    h = csr_from_index_list(6, idx)
    assert h.nnz == g.nnz and h.num_vertices == g.num_vertices
    assert key(h.adj_ia, h.adj_ja) != k0
    ja = np.array(g.adj_ja, order="F")
    for w in range(ja.shape[1]):                             # any single in-place change is seen
        for r in range(2):
            old = ja[r, w]
            ja[r, w] = old + 1
            assert key(g.adj_ia, ja) != k0
            ja[r, w] = old
    assert key(g.adj_ia, ja) == k0
    # a large graph: EVERY word enters the key by default (the reference re-copies the CSR per set_graph and is always
    # current) -- positions between the old sample points, chunk borders of the threaded hash, row pointers
    n, nnz = 300_000, (1 << 21) + 12345
    rng = np.random.default_rng(0)
    ia = np.concatenate([[1], 1 + np.sort(rng.integers(0, nnz + 1, n - 1)), [nnz + 1]]).astype(np.int32)
    jb = np.asfortranarray(rng.integers(1, n + 1, (2, nnz)).astype(np.int32))
    kb = key(ia, jb)
    st = nnz // 4096
    for w in (0, 1023, 1500, st * 7, st * 7 + 1, st * 7 + st // 2, (1 << 19) - 1, 1 << 19, (1 << 19) + 1, nnz - 1025, nnz - 1,
              *rng.integers(0, nnz, 40).tolist()):
        for r in range(2):
            old = jb[r, w]
            jb[r, w] = old % n + 1
            assert key(ia, jb) != kb, (r, w)
            jb[r, w] = old
    for i in (1, 1500, n // 2, n - 2):                        # two rows trade one entry: same nnz, other row pointers
        ia[i] += 1
        assert key(ia, jb) != kb, i
        ia[i] -= 1
    assert key(ia, jb) == kb
    assert key(ia[:-1], jb[:, : ia[-2] - 1]) != kb
    # the ADVICE reproduction: rewire everything BETWEEN the sampled positions of the opt-in key
    jc = np.array(jb, order="F")
    keep = np.zeros(nnz, bool)
    keep[:1024] = keep[-1024:] = True
    keep[::st] = True
    jc[0, ~keep] = jc[0, ~keep] % n + 1
    assert key(ia, jc) != kb


def test_graph_key_does_not_depend_on_the_thread_count_and_sampling_is_opt_in():
    """the key of a large CSR is folded from fixed 2^20-value chunks in chunk order: 1 thread and 8 threads agree; the
    sampled key exists only behind ATHENA_MP_GRAPH_KEY_SAMPLED=1 (and then misses an edit between its samples -- which
    is why it is not the default)."""
    import subprocess
    import sys

    prog = r'''
import ctypes as C, numpy as np, sys, os
if os.environ.get("KEY_TEST_ONE_CORE"):
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})     # std::thread::hardware_concurrency follows the mask
sys.path.insert(0, %r)
from athena_amd import _capi
n, nnz = 200_000, (1 << 22) + 77
rng = np.random.default_rng(3)
ia = np.concatenate([[1], 1 + np.sort(rng.integers(0, nnz + 1, n - 1)), [nnz + 1]]).astype(np.int32)
ja = np.asfortranarray(rng.integers(1, n + 1, (2, nnz)).astype(np.int32))
def key():
    k = C.c_uint64(0)
    _capi.call("athena_mp_graph_key", n, nnz, ia.ctypes.data, ja.ctypes.data, C.byref(k))
    return k.value
k0 = key()
w = (nnz // 4096) * 9 + 5          # between two sample positions
ja[0, w] = ja[0, w] %% n + 1
print(k0, key())
''' % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    def run(env):
        e = dict(os.environ)
        e.update(env)
        out = subprocess.run([sys.executable, "-c", prog], env=e, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        return [int(t) for t in out.stdout.split()]

    a = run({"KEY_TEST_ONE_CORE": "1"})      # affinity mask of one core: the key's chunks are hashed by one thread
    b = run({})                              # ... and by up to eight
    assert a == b and a[0] != a[1]
    s = run({"ATHENA_MP_GRAPH_KEY_SAMPLED": "1"})
    assert s[0] == s[1] and s[0] != a[0]


def _control_plane_worker(rank, world, port, q):
    import importlib.util

    import torch.distributed as dist

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for k in ("ATHENA_MP_BENCH_CONTROL", "ATHENA_MP_BENCH_BACKEND", "ATHENA_MP_COMM_TRANSPORT"):
        os.environ.pop(k, None)
    spec = importlib.util.spec_from_file_location("bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    control = bench.init_control_plane(None, one_device=(rank >= 0 and world == 2))
    import torch
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.barrier()
    q.put((rank, control, dist.get_backend(), os.environ.get("ATHENA_MP_COMM_TRANSPORT"), t.item(), bench.control_plane_note(control)))
    dist.destroy_process_group()


def test_bench_control_plane_is_gloo_so_that_rccl_holds_one_communicator_per_rank():
    """bench.py --gpus N: barriers / the max of the step time / scalar agreement / the communicator id broadcast run on a gloo
    group unless ATHENA_MP_BENCH_CONTROL=nccl opts into torch's RCCL group; the data plane's transport is never inferred from
    that backend (dist.c_comm: RCCL unless named otherwise or the ranks of a node outnumber its devices)"""
    import multiprocessing as mp
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_control_plane_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, control, backend, transport, mx, note in got:
        assert control == "gloo" and backend == "gloo" and mx == 2.0
        assert transport == "shm"                      # the one-device dry run names the test transport itself
        assert note.startswith("gloo") and "two communicators" not in note
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "athena_amd", "dist.py")).read()
    body = src[src.index("def c_comm("):src.index("def c_comm_stats(")] if "def c_comm_stats(" in src else src[src.index("def c_comm("):]
    assert "get_backend" not in body.split("_COMM.handle")[0]


def test_bench_line_refuses_the_test_transport_outside_the_dry_run():
    """a typo'd backend on a real node must not "scale" through /dev/shm files: bench.py marks such a line ok = false
    and exits non-zero unless the one-device dry-run switch is set"""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.transport_error("rccl", False) is None
    assert bench.transport_error("shm (test transport: host-staged files, not RCCL)", True) is None
    assert "not RCCL" in bench.transport_error("shm (test transport: host-staged files, not RCCL)", False)
    assert bench.transport_error("torch.distributed point-to-point (python plan) -- FALLBACK, the C-ABI path failed: x", False)


def test_bench_checks_and_extra_measurements_wait_for_full(monkeypatch):
    """a plain `bench.py --gpus 1 --steps N --warmup W` does only what its headline needs; parity, the CPU baseline, the
    relu epilogue, the secondary block and the breakdown run with --full, which is off by default"""
    import importlib.util
    import sys

    spec = importlib.util.spec_from_file_location("bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse_args()
    assert args.full is False and (args.steps, args.warmup, args.gpus) == (7, 2, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--cpu-runs", "1", "--secondary", "c3"])
    args = bench.parse_args()
    assert args.full is True and args.cpu_runs == 1 and args.secondary == "c3"


def test_watchdog_ends_a_stalled_rank_with_a_message_and_exit_code_3():
    """athena_amd.dist.Watchdog (bench.py's guard around every wait for a peer): a phase that outlives its deadline ends the
    PROCESS -- one json line {"ok": false, "error": "rank r stalled in <phase> ..."} on stdout, exit code 3, no cleanup that
    could block; a phase that finishes in time leaves nothing behind; nested phases report the innermost."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = r'''
import sys, time
sys.path.insert(0, %r)
from athena_amd.dist import Watchdog
wd = Watchdog(5, timeout_s=0.6)
with wd.phase("quick phase"):
    time.sleep(0.05)
print("still here", flush=True)
with wd.phase("outer phase", factor=50.0):
    with wd.phase("halo exchange of the forward rows"):
        time.sleep(30)
print("never printed", flush=True)
''' % root
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr[-500:])
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "still here" and "never printed" not in r.stdout
    msg = json.loads(lines[-1])
    assert msg["ok"] is False and "rank 5 stalled in halo exchange of the forward rows" in msg["error"]
    # an OUTER phase's earlier deadline is enforced while an inner phase with a longer leash is active
    prog2 = r'''
import sys, time
sys.path.insert(0, %r)
from athena_amd.dist import Watchdog
wd = Watchdog(2, timeout_s=0.5)
with wd.phase("timed loop"):
    with wd.phase("shard build inside it", factor=100.0):
        time.sleep(30)
''' % root
    r = subprocess.run([sys.executable, "-c", prog2], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr[-500:])
    assert "rank 2 stalled in timed loop" in json.loads(r.stdout.strip().splitlines()[-1])["error"]


def test_frozen_graph_keeps_its_content_key_and_refuses_in_place_edits():
    """graph_type.freeze(): read-only adjacency arrays -> topology_key() may memoise the full content key (set_graph before every
    forward then costs a tuple compare); an in-place edit raises instead of going unseen; an assignment re-keys"""
    from athena_amd import synth
    from athena_amd.graph import graph_type

    ia, ja = synth.random_graph_csr(2000, 9000)
    g = graph_type.from_csr(ia, ja)
    k0 = g.topology_key()
    assert g.topology_key() == k0 and getattr(g, "_key_memo", None) is None      # writable arrays: hashed every time
    g.adj_ja[0, 5] = g.adj_ja[0, 5] % 2000 + 1                                     # ... so an in-place edit is seen
    assert g.topology_key()[4] != k0[4] or ja[0, 5] == g.adj_ja[0, 5]
    g.freeze()
    k1 = g.topology_key()
    assert g._key_memo is not None and g.topology_key() is k1
    with pytest.raises(ValueError):
        g.adj_ja[0, 0] = 3
    with pytest.raises(ValueError):
        g.adj_ia[1] = 7
    with pytest.raises(ValueError):                                                # ... and it cannot be un-frozen behind the memo
        g.adj_ja.flags.writeable = True
    # read-only arrays that merely OWN their data (they could be made writeable again) are never memoised
    h = graph_type.from_csr(ia, ja)
    a, b = np.array(h.adj_ia), np.asfortranarray(np.array(h.adj_ja))
    a.flags.writeable = b.flags.writeable = False
    h.adj_ia, h.adj_ja = a, b
    kh = h.topology_key()
    assert getattr(h, "_key_memo", None) is None
    b.flags.writeable = True
    b[0, 7] = b[0, 7] % 2000 + 1
    b.flags.writeable = False
    assert h.topology_key()[4] != kh[4] or ja[0, 7] == b[0, 7]
    ja2 = np.asfortranarray(np.array(g.adj_ja))
    ja2[0, 0] = ja2[0, 0] % 2000 + 1
    g.adj_ja = ja2                                                                 # assignment: version bump, memo dropped
    k2 = g.topology_key()
    assert k2[1] != k1[1] and k2[4] != k1[4]


def test_product_source_has_no_compatibility_layers_and_never_reaches_for_the_oracle():
    """north_star: "no CUDA-compat shims, no dual CUDA/HIP paths and no Triton"; the oracle is test infrastructure.  The product
    sources (athena_amd/: HIP, C++, Fortran, Python; include/) contain no hipcub / rocprim / thrust / cub include (round 5's graph
    builder sorted through hipcub: gone since round 6, radix_sort.h), no CUDA dual-path macro, no hipify residue, no BLAS / Triton,
    and nothing that imports, links or opens anything under oracle/ (comments may name it)."""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    banned = [r"#\s*include\s*<\s*(hipcub|rocprim|thrust|cub)/", r"__HIP_PLATFORM_(AMD|NVIDIA)__", r"__CUDACC__|__CUDA_ARCH__", r"\bcuda[A-Z]\w+\(",
              r"hipify", r"#\s*include\s*<\s*(rocblas|hipblas|hipblaslt)", r"\bimport\s+triton\b|\btriton\.jit\b"]
    oracle_use = [r"^\s*(from|import)\s+oracle\b", r"liboracle", r"oracle/\w+\.(so|py|c)\b"]
    seen = 0
    for base in ("athena_amd", "include"):
        for dirpath, _, files in os.walk(os.path.join(root, base)):
            if "__pycache__" in dirpath:
                continue
            for f in files:
                if not f.endswith((".hip", ".h", ".cpp", ".f90", ".py", ".sh")):
                    continue
                seen += 1
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                for pat in banned:
                    assert not re.search(pat, text), f"{os.path.join(dirpath, f)}: {pat}"
                code = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith(("#", "//", "!", "*", "/*")))
                for pat in oracle_use:
                    assert not re.search(pat, code, re.M), f"{os.path.join(dirpath, f)} reaches for the oracle: {pat}"
    assert seen > 40
