"""GPU: geometry gradients on the device (athena_amd/csrc/geometry_grad.hip; athena_mp_edge_grad_to_points, athena_mp_periodic_grad,
their *_host entries and the Python / Fortran mirrors) against the yardstick of tests/geometry_reference.py run on the handle's
exported CSR.  The gathers are defined to the bit: dpoints, dcart and dfrac are compared with np.array_equal.  The virial's summation
order is free: it is held to 1e-5 of its term magnitudes against the float64 twin; dlat to one fp32 rounding of L^-T virial."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import geometry_reference as gr
from helpers import assert_close_elementwise, placed, placed_out, unwritten
from radius_reference import degree_radius
from test_gpu_periodic_graph import _batch, _fixture, _sizes, _structures

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "athena_amd", "fortran", "geometry_grad_run")
CMAX = 3.0


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _csr(handle):
    return handle.export("rowptr"), handle.export("col"), handle.export("eid")


def _up(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- points mode ------------------------------------------------------------------------------------------------------------------

def _cloud(dev, p, radius, loops, seed=1):
    """handle of the cloud, its CSR, a random dcoords (numpy) and the yardstick's dpoints"""
    from athena_amd import DeviceGraph

    handle, coords = DeviceGraph.from_points(np.ascontiguousarray(p, np.float32), radius, add_self_loops=loops)
    dc = _rng(seed).uniform(-1, 1, tuple(coords.shape)).astype(np.float32)
    csr = _csr(handle)
    want, _ = gr.points_grad(*csr, dc, np.float32)
    return handle, csr, dc, want


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_points_uniform_cloud_equals_the_yardstick(dev, dim, loops):
    from athena_amd import points_grad

    n = 3000
    p = _rng(10 + dim).random((n, dim)).astype(np.float32)
    handle, csr, dc, want = _cloud(dev, p, degree_radius(n, 14.0, dim), loops)
    assert dc.shape[0] > 4 * n and (csr[2] < 0).sum() == (n if loops else 0)
    got = points_grad(handle, _up(dc, dev))
    assert got.shape == (n, dim) and np.array_equal(got.cpu().numpy(), want)
    assert np.abs(want).max() > 0
    handle.close()


def test_points_hub_rows_and_isolated_points(dev):
    """a cluster of 700 near-coincident points (rows of 699 entries: many rounds of the lane group) among isolated points"""
    from athena_amd import points_grad

    rng = _rng(21)
    grid = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    cluster = (np.float32(2.5) + rng.random((700, 3)) * 1e-3).astype(np.float32)
    p = np.concatenate([grid[:100], cluster, grid[100:]])
    handle, csr, dc, want = _cloud(dev, p, 0.01, False)
    lens = np.diff(csr[0])
    assert lens.max() > 512 and (lens == 0).sum() == 216 and dc.shape[0] == 700 * 699 // 2
    got = points_grad(handle, _up(dc, dev))
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.all(want[:100] == 0) and np.all(np.signbit(got.cpu().numpy()[:100]) == False)      # a row without entries: +0
    handle.close()


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("which", ["dcoords", "out"])
def test_points_operands_at_four_byte_addresses_between_guards(dev, dim, which):
    import torch
    from athena_amd import points_grad

    n = 900
    p = _rng(30 + dim).random((n, dim)).astype(np.float32)
    handle, csr, dc, want = _cloud(dev, p, degree_radius(n, 12.0, dim), True)
    dcd = placed(dc, dev, 1) if which == "dcoords" else _up(dc, dev)
    out, check = placed_out((n, dim), torch.float32, dev, 1 if which == "out" else 4)
    assert unwritten(out) == n * dim
    points_grad(handle, dcd, out=out)
    check(f"dpoints, {which} at a 4-byte address")
    assert unwritten(out) == 0 and np.array_equal(out.cpu().numpy(), want)
    handle.close()


def test_points_without_vertices_and_without_edges(dev):
    import torch
    from athena_amd import DeviceGraph, points_grad

    handle, coords = DeviceGraph.from_points(np.zeros((0, 3), np.float32), 0.1)
    assert coords.shape == (0, 3)
    assert points_grad(handle, coords).shape == (0, 3)
    handle.close()
    for loops in (False, True):                                            # points too far apart for any pair
        p = (np.arange(50, dtype=np.float32)[:, None] * np.ones(2, np.float32)).astype(np.float32)
        handle, coords = DeviceGraph.from_points(p, 0.1, add_self_loops=loops)
        assert coords.shape == (0, 2) and handle.n_edge_cols == 0
        out, check = placed_out((50, 2), torch.float32, dev, 1)
        points_grad(handle, coords, out=out)
        check("E = 0")
        assert unwritten(out) == 0 and torch.all(out == 0)
        handle.close()


# ---- periodic mode ----------------------------------------------------------------------------------------------------------------

class _Case:
    """a batch through DeviceGraph.from_structures, with random per-edge gradients"""

    def __init__(self, dev, frac, lat, off, cmin, loops=False, seed=2):
        from athena_amd import DeviceGraph

        self.dev, self.lat, self.off = dev, np.ascontiguousarray(lat, np.float32), np.ascontiguousarray(off, np.int32)
        self.handle, self.feature, self.vec, self.voff, self.eoff = DeviceGraph.from_structures(frac, lat, off, cmin, CMAX, add_self_loops=loops)
        self.csr = _csr(self.handle)
        self.vec_h = self.vec.cpu().numpy()
        self.E, self.n, self.B = self.vec_h.shape[0], int(off[-1]), self.lat.shape[0]
        rng = _rng(seed)
        self.de = {k: rng.uniform(-1, 1, (self.E, k)).astype(np.float32) for k in (1, 8)}
        self.dv = rng.uniform(-1, 1, (self.E, 3)).astype(np.float32)
        self.lat_d = _up(self.lat, dev)

    def operands(self, mode):
        """mode: (fe_cols or 0, with dvec) -> (dfeature, dvec) numpy or None"""
        return (self.de[mode[0]] if mode[0] else None), (self.dv if mode[1] else None)

    def reference(self, mode, dtype, cell=True, lat=None):
        de, dv = self.operands(mode)
        return gr.structures_grad(*self.csr, self.lat if lat is None else lat, self.off, self.eoff, self.vec_h, CMAX, de, dv, dtype, cell=cell)

    def run(self, mode, want=("cart", "frac", "virial", "lat"), out=None, lat=None, vec=None, de=None, dv=None):
        from athena_amd import structures_grad

        hde, hdv = self.operands(mode)
        de = de if de is not None else (_up(hde, self.dev) if hde is not None else None)
        dv = dv if dv is not None else (_up(hdv, self.dev) if hdv is not None else None)
        return structures_grad(self.handle, self.lat_d if lat is None else lat, self.voff, self.eoff, self.vec if vec is None else vec, CMAX,
                               dfeature=de, dvec=dv, want=want, out=out)

    def check(self, got, mode, what=""):
        """every output in `got` against the yardstick / the twin; returns the twin"""
        a = self.reference(mode, np.float32, cell=False)
        b = self.reference(mode, np.float64)
        g = {k: v.cpu().numpy() for k, v in got.items()}
        for k in ("cart", "frac"):
            if k in g:
                assert g[k].dtype == np.float32 and g[k].shape == a[k].shape
                assert np.array_equal(g[k], a[k]), f"{what}: d{k} differs from the yardstick"
        if "virial" in g:
            assert_close_elementwise(g["virial"], b["virial"], b["virial_mag"], 1e-5, f"{what}: virial")
            empty = np.diff(self.eoff) == 0
            assert np.all(g["virial"][empty] == 0)
        if "lat" in g and "virial" in g:
            inv_t = np.linalg.inv(self.lat.astype(np.float64)).transpose(0, 2, 1)
            want = inv_t @ g["virial"].astype(np.float64)
            scale = np.abs(inv_t) @ np.abs(g["virial"].astype(np.float64))
            assert_close_elementwise(g["lat"], want, scale, 1e-6, f"{what}: dlat")
        return b


MODES = [(1, False), (0, True), (8, True)]                                 # dfeature only, dvec only, both (8 columns)


def _check_all(case, what):
    """every mode with all outputs together; each output alone and a second run, byte for byte the first"""
    import torch

    for mode in MODES:
        got = case.run(mode)
        b = case.check(got, mode, f"{what}, mode {mode}")
        if mode[1]:
            assert np.abs(b["virial"] - np.swapaxes(b["virial"], 1, 2)).max() > 0      # dvec: not symmetric
        assert case.E == 0 or np.abs(b["virial"]).max() > 0
    mode = MODES[2]
    again = case.run(mode)
    for k in got:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), f"{what}: two runs differ in {k}"
        alone = case.run(mode, want=(k,))
        assert list(alone) == [k] and torch.equal(got[k].view(torch.int32), alone[k].view(torch.int32)), f"{what}: {k} alone"
    got1 = case.run((1, True))                                             # one column with dvec
    case.check(got1, (1, True), f"{what}, mode (1, True)")


def test_periodic_fixture_equals_the_yardstick(dev):
    frac, lat, off = _fixture()
    case = _Case(dev, frac, lat, off, 0.5)
    assert case.E == 1849
    _check_all(case, "fixture")
    case.handle.close()


@pytest.mark.parametrize("kind", ["cubic", "skewed", "small"])
@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_periodic_random_batches_equal_the_yardstick(dev, kind, B):
    rng = _rng(B * 11 + len(kind))
    distinct = _structures(rng, kind, _sizes(rng, B) if B > 1 else [int(rng.integers(8, 31))])
    order = list(range(B))
    if B > 1:
        order[B // 2] = None                                               # an empty structure in the middle
        order[-1] = None                                                   # ... and one at the end
    frac, lat, off = _batch(distinct, order)
    case = _Case(dev, frac, lat, off, 0.5 if kind != "small" else 0.0, loops=(B % 2 == 0))
    print(f"{kind}, {B} structures, {case.n} atoms, {case.E} edges")
    assert case.E > 0
    if B > 1:
        assert np.any(np.diff(off) == 1) and np.any(np.diff(off) == 0)
    if kind == "small":
        rows = np.repeat(np.arange(case.n), np.diff(case.csr[0]))
        assert np.any((case.csr[1] == rows) & (case.csr[2] >= 0))           # self-image edges: skipped by the gather, in the virial
    _check_all(case, f"{kind} x {B}")
    case.handle.close()


def test_periodic_structure_of_several_work_items_between_small_ones(dev):
    rng = _rng(41)
    distinct = _structures(rng, "cubic", [12, 9, 10])
    distinct.insert(1, (rng.random((600, 3)).astype(np.float32), (np.eye(3) * 12.0).astype(np.float32)))
    frac, lat, off = _batch(distinct, [0, 1, None, 2, 3])
    case = _Case(dev, frac, lat, off, 0.5)
    assert case.eoff[2] - case.eoff[1] > 8192                              # at least three work items of 4096 edges
    _check_all(case, "600 atoms")
    case.handle.close()


@pytest.mark.parametrize("which", ["lat", "vec", "dfeature", "dvec", "outputs"])
def test_periodic_operands_at_four_byte_addresses_between_guards(dev, which):
    import torch

    rng = _rng(51)
    distinct = _structures(rng, ("cubic", "small", "skewed"), _sizes(rng, 20), max_range=8)
    order = list(range(20)); order[7] = None
    frac, lat, off = _batch(distinct, order)
    case = _Case(dev, frac, lat, off, 0.5, loops=True)
    mode = (8, True)
    ref = case.run(mode)
    case.check(ref, mode, "aligned")
    kw, checks = {}, []
    if which == "lat":
        kw["lat"] = placed(case.lat, dev, 1)
    elif which == "vec":
        kw["vec"] = placed(case.vec_h, dev, 1)
    elif which == "dfeature":
        kw["de"] = placed(case.de[8], dev, 1)
    elif which == "dvec":
        kw["dv"] = placed(case.dv, dev, 1)
    out = {}
    for k, shape in (("cart", (case.n, 3)), ("frac", (case.n, 3)), ("virial", (case.B, 3, 3)), ("lat", (case.B, 3, 3))):
        out[k], chk = placed_out(shape, torch.float32, dev, 1 if which == "outputs" else 4)
        checks.append((k, chk))
    got = case.run(mode, out=out, **kw)
    for k, chk in checks:
        chk(f"{k}, {which} at a 4-byte address")
        assert got[k] is out[k] and unwritten(out[k]) == 0, k
        assert torch.equal(out[k].view(torch.int32), ref[k].view(torch.int32)), k
    case.handle.close()


def test_periodic_without_atoms_and_without_edges(dev):
    import torch
    from athena_amd import DeviceGraph, structures_grad

    lat = np.tile((np.eye(3) * 9.0).astype(np.float32), (3, 1, 1))
    for frac, off in ((np.zeros((0, 3), np.float32), [0, 0, 0, 0]), (np.full((2, 3), 0.25, np.float32), [0, 1, 1, 2])):
        handle, feature, vec, voff, eoff = DeviceGraph.from_structures(frac, lat, off, 0.5, CMAX)
        assert vec.shape == (0, 3) and eoff[-1] == 0
        got = structures_grad(handle, lat, voff, eoff, vec, CMAX, dfeature=feature[:, None].contiguous())
        n = len(frac)
        assert got["cart"].shape == (n, 3) and got["virial"].shape == (3, 3, 3)
        for k in got:
            assert torch.all(got[k] == 0), k
        handle.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def test_duvenaud_edge_gradient_back_to_atoms_and_cell(dev):
    """from_structures -> duvenaud layer forward / backward(need_edge_grad) -> structures_grad(dfeature = de): the yardstick applied
    to the downloaded de, bit for bit; and no net force on any structure"""
    import torch
    from athena_amd.layers import duvenaud_msgpass_layer_type

    rng = _rng(61)
    B, Fv, Fe, T, O = 200, 6, 1, 2, 10
    distinct = _structures(rng, ("cubic", "cubic", "small"), _sizes(rng, 60))
    order = [int(k) for k in rng.integers(0, 60, B)]
    order[B // 2] = None
    frac, lat, off = _batch(distinct, order)
    case = _Case(dev, frac, lat, off, 0.5)
    layer = duvenaud_msgpass_layer_type(num_vertex_features=[Fv], num_edge_features=[Fe], num_time_steps=T, max_vertex_degree=10,
                                        num_outputs=O, min_vertex_degree=1, seed=3)
    layer.set_graph_handle(case.handle, case.voff)
    x = _up(rng.uniform(-1, 1, (case.n, Fv)).astype(np.float32), dev)
    up = _up(rng.uniform(-1, 1, (B, O)).astype(np.float32), dev)
    layer.forward(x, case.feature[:, None].contiguous())
    _, de = layer.backward(up, need_input_grad=True, need_edge_grad=True)
    de = de.clone()
    assert de.shape == (case.E, Fe) and de.abs().max() > 0
    case.de[1] = de.cpu().numpy()
    got = case.run((1, False), de=de)
    b = case.check(got, (1, False), "duvenaud")
    cart = got["cart"].cpu().numpy().astype(np.float64)
    for s in range(B):
        rows = slice(off[s], off[s + 1])
        assert np.all(np.abs(cart[rows].sum(0)) <= 1e-5 * b["cart_mag"][rows].sum(0) + 1e-30), f"structure {s}: a net force"
    assert np.abs(cart).max() > 0
    case.handle.close()


def test_gno_coordinate_gradient_back_to_points(dev):
    import torch
    from athena_amd import DeviceGraph, points_grad
    from athena_amd.layers import graph_nop_layer_type

    n, Fi, Fo, d, H = 2000, 64, 64, 3, 64
    rng = _rng(71)
    p = rng.random((n, d)).astype(np.float32)
    handle, coords = DeviceGraph.from_points(p, degree_radius(n, 12.0, d))
    layer = graph_nop_layer_type(num_outputs=Fo, coord_dim=d, kernel_hidden=H, num_inputs=Fi, use_bias=True, activation="relu", seed=5)
    layer.set_params(layer.get_params() + _rng(1).standard_normal(layer.get_num_params()).astype(np.float32) * 0.05)
    layer.set_graph_handle(handle)
    layer.forward(_up(rng.uniform(-1, 1, (n, Fi)).astype(np.float32), dev), coords)
    _, dc = layer.backward(_up(rng.uniform(-1, 1, (n, Fo)).astype(np.float32), dev), need_coord_grad=True)
    dc = dc.clone()
    got = points_grad(handle, dc)
    want, mag = gr.points_grad(*_csr(handle), dc.cpu().numpy(), np.float32)
    assert np.array_equal(got.cpu().numpy(), want) and np.abs(want).max() > 0
    total = got.cpu().numpy().astype(np.float64).sum(0)
    assert np.all(np.abs(total) <= 1e-5 * mag.sum(0))                      # translation invariance
    handle.close()


# ---- refusals and the Fortran runner ----------------------------------------------------------------------------------------------

def test_refusals_say_why_and_leave_the_library_usable(dev):
    import torch
    from athena_amd import DeviceGraph, _capi, points_grad, structures_grad
    from athena_amd import synth

    rng = _rng(81)
    distinct = _structures(rng, "cubic", _sizes(rng, 10))
    frac, lat, off = _batch(distinct, list(range(10)))
    case = _Case(dev, frac, lat, off, 0.5)
    de, dv = _up(case.de[1], dev), _up(case.dv, dev)
    call = lambda **kw: structures_grad(kw.get("handle", case.handle), kw.get("lat", case.lat_d), kw.get("off", case.voff),
                                        kw.get("eoff", case.eoff), case.vec, kw.get("cmax", CMAX), dfeature=kw.get("de", de),
                                        dvec=kw.get("dv", dv), want=kw.get("want", ("cart", "frac", "virial", "lat")))
    ia, ja = synth.random_graph_csr(case.n, 5 * case.n, seed=1)
    kipf = DeviceGraph(ia, ja, n_edge_cols=0)
    with pytest.raises(_capi.AthenaMPError, match=r"periodic_grad: the handle has no edge columns"):
        call(handle=kipf)
    with pytest.raises(_capi.AthenaMPError, match=r"edge_grad_to_points: the handle has no edge columns"):
        _capi.call("athena_mp_edge_grad_to_points", kipf.handle, 3, C.c_void_p(dv.data_ptr()), C.c_void_p(dv.data_ptr()))
    kipf.close()
    other = _Case(dev, frac[:off[9]], lat[:9], off[:10], 0.5)              # one structure fewer: other rows, other edge columns
    with pytest.raises(_capi.AthenaMPError, match=r"n_atoms = %d, the handle has %d rows" % (case.n, other.n)):
        call(handle=other.handle)
    other.handle.close()
    bad = case.eoff.copy(); bad[-1] -= 1
    with pytest.raises(_capi.AthenaMPError, match=r"edge_offsets end at %d, the handle has %d edge columns" % (bad[-1], case.E)):
        call(eoff=bad)
    bad = case.voff.copy(); bad[4] = bad[3] - 1
    with pytest.raises(_capi.AthenaMPError, match=r"structure 4: offsets descend from %d to %d" % (bad[3], bad[4])):
        call(off=bad)
    bad = case.voff.copy(); bad[0] = 1
    with pytest.raises(_capi.AthenaMPError, match=r"offsets\(1\) = 1, not 0"):
        call(off=bad)
    bad = case.eoff.copy(); bad[0] = 2
    with pytest.raises(_capi.AthenaMPError, match=r"edge_offsets\(1\) = 2, not 0"):
        call(eoff=bad)
    bad = case.eoff.copy(); bad[6] = bad[5] - 3
    with pytest.raises(_capi.AthenaMPError, match=r"structure 6: edge_offsets descend from %d to %d" % (bad[5], bad[6])):
        call(eoff=bad)
    for dim in (0, 4):
        with pytest.raises(_capi.AthenaMPError, match=r"dim = %d is outside 1\.\.3" % dim):
            _capi.call("athena_mp_edge_grad_to_points", case.handle.handle, dim, C.c_void_p(dv.data_ptr()), C.c_void_p(dv.data_ptr()))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with pytest.raises(_capi.AthenaMPError, match=r"fe_cols = 0 with a dfeature"):
        _capi.call("athena_mp_periodic_grad", case.handle.handle, case.B, case.n, case.voff.ctypes.data_as(C.c_void_p),
                   case.eoff.ctypes.data_as(C.c_void_p), ptr(case.lat_d), CMAX, ptr(case.vec), ptr(de), 0, None, ptr(dv), None, None, None)
    with pytest.raises(_capi.AthenaMPError, match=r"dfeature and dvec are both null"):
        call(de=None, dv=None)
    for cmax in (np.inf, np.nan, 0.0, -3.0):
        with pytest.raises(_capi.AthenaMPError, match=r"cutoff_max = .*: need a finite value above 0"):
            call(cmax=cmax)
    L = case.lat.copy(); L[5, 2] = L[5, 0] + L[5, 1]; L[5, 1] = 2 * L[5, 0]       # coplanar: no inverse
    with pytest.raises(_capi.AthenaMPError, match=r"structure 6: det\(lat\) is zero or not finite: dlat needs the inverse"):
        call(lat=_up(L, dev))
    got = call(lat=_up(L, dev), want=("cart", "frac", "virial"))           # ... which the virial alone does not need
    b = case.reference((1, True), np.float64, lat=L.astype(np.float64))
    assert_close_elementwise(got["virial"].cpu().numpy(), b["virial"], b["virial_mag"], 1e-5, "virial with a singular lattice")
    case.check(call(), (1, True), "after the refusals")                   # the library is usable afterwards
    case.handle.close()


def test_host_entries_and_the_fortran_program_write_the_arrays_of_the_python_mirror(dev, tmp_path):
    import torch
    from athena_amd import DeviceGraph, _capi, structures_grad_host
    from athena_amd.graph import graph_type

    if not os.path.exists(RUNNER):
        pytest.fail("geometry_grad_run is not built: __graft_entry__.build() compiles the Fortran host side")
    rng = _rng(91)
    distinct = _structures(rng, ("cubic", "small", "skewed"), _sizes(rng, 50), max_range=8)
    order = list(range(50)); order[20] = None
    frac, lat, off = _batch(distinct, order)
    B, n, loops, fe = lat.shape[0], frac.shape[0], 1, 8
    case = _Case(dev, frac, lat, off, 0.5, loops=True)
    mode = (fe, True)
    dev_res = case.run(mode)
    case.check(dev_res, mode, "device route")
    host_res = structures_grad_host(case.handle, lat, case.voff, case.eoff, case.vec_h, CMAX, dfeature=case.de[fe], dvec=case.dv)
    for k in dev_res:
        assert host_res[k].dtype == np.float32 and np.array_equal(host_res[k].view(np.int32), dev_res[k].cpu().numpy().view(np.int32)), k
    # points mode through its host entry
    p = rng.random((500, 2)).astype(np.float32)
    ph, coords = DeviceGraph.from_points(p, degree_radius(500, 10.0, 2))
    dc = rng.uniform(-1, 1, tuple(coords.shape)).astype(np.float32)
    dp = np.full((500, 2), np.nan, np.float32)
    _capi.call("athena_mp_edge_grad_to_points_host", ph.handle, 2, dc.ctypes.data_as(C.c_void_p), dp.ctypes.data_as(C.c_void_p))
    assert np.array_equal(dp, gr.points_grad(*_csr(ph), dc, np.float32)[0])
    ph.close()
    # the Fortran program: builds the graphs itself, takes the handle of that CSR, writes the four outputs
    case_file, res_file = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(case_file, "wb") as f:
        f.write(np.asarray([B, n, loops, 1, 1, 1, fe, 1], np.int32).tobytes() + np.asarray([0.5, CMAX], np.float32).tobytes() + off.tobytes()
                + frac.tobytes() + lat.tobytes() + np.asarray([case.E], np.int32).tobytes() + case.de[fe].tobytes() + case.dv.tobytes())
    out = subprocess.run([RUNNER, case_file, res_file], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"geometry_grad_run failed ({out.returncode}): {out.stderr[-2000:]}"
    b = open(res_file, "rb").read()
    assert tuple(np.frombuffer(b, np.int32, 3)) == (B, n, case.E)
    o = 12
    for k, count in (("cart", 3 * n), ("frac", 3 * n), ("virial", 9 * B), ("lat", 9 * B)):
        got = np.frombuffer(b, np.int32, count, o); o += 4 * count
        assert np.array_equal(got, host_res[k].view(np.int32).ravel()), f"geometry_grad_run: {k} differs from the Python mirror"
    assert o == len(b)
    case.handle.close()
