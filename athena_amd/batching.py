"""Mini-batches drawn from a dataset graph that stays on the device (athena_amd/csrc/batch_select.hip; the definition is in
include/athena_mp.h): what network%train does with get_sample(input_graph, i0, i1) under shuffle_batches, without assembling the
batch on the host and without searching its neighbours again.

    handle, feature, vec, voff, eoff = DeviceGraph.from_structures(...)        # once
    ds = DeviceDataset(handle, voff, eoff)
    for b in ds.batches(2000, seed=epoch):
        layer.set_graph_handle(b.handle, b.vertex_offsets)
        out = layer.forward(b.take_vertices(x), b.take_edges(feature)[:, None]) ...
        g = structures_grad(b.handle, b.take_structures(lat), b.vertex_offsets, b.edge_offsets, b.take_edges(vec), cutoff_max, dfeature=de)

ONE large graph (a citation or product graph, a mesh, a point cloud joined by from_points_knn) is not a dataset of structures:
NeighborSampler draws neighbour-sampled mini-batches of its vertices instead (athena_amd/csrc/neighbor_sample.hip).

    sampler = NeighborSampler(handle)                                          # once
    for blocks in sampler.batches(1024, (10, 10), seed=epoch):                 # outermost block first
        h = blocks[0].take_vertices(x)
        for layer, b in zip(layers, blocks):
            layer.set_graph_handle(b.handle)
            h = layer.forward(h) ...                                           # [b.handle.n_cols, F] -> [b.n_seeds, F]

A batch's handle is a deep copy: it outlives the dataset and is closed like any DeviceGraph.  Gradients come back in batch order (a
batch's forces are compared with the batch's gathered targets); scattering them to dataset order is not part of this module."""
import ctypes as C

import numpy as np

from . import _capi
from .graph import DeviceGraph


class Batch:
    """One selection of a DeviceDataset: handle (a DeviceGraph that owns the child), vertex_offsets (int32) and edge_offsets (int64)
    numpy [m + 1], vertex_map / edge_map (int32 device tensors: the dataset row of every vertex / edge column of the batch) and
    ids (the selected structures, int32 numpy)."""

    def __init__(self, handle, vertex_offsets, edge_offsets, vertex_map, edge_map, ids, dataset_rows):
        self.handle, self.vertex_offsets, self.edge_offsets = handle, vertex_offsets, edge_offsets
        self.vertex_map, self.edge_map, self.ids = vertex_map, edge_map, ids
        self._rows = dataset_rows                                              # the dataset's (vertices, edge columns, structures)
        self._ids_dev = None

    @staticmethod
    def _take(t, idx, rows, what):
        """rows idx of a float32 device tensor [rows, ...] through ops.gather_rows (a 1-d tensor is taken as one column)"""
        import torch

        from . import ops

        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() >= 1):
            raise ValueError(f"{what}: expect a contiguous float32 device tensor")
        if t.shape[0] != rows:
            raise ValueError(f"{what}: the tensor holds {t.shape[0]} rows, the dataset has {rows}")
        tail = tuple(t.shape[1:])
        F = int(np.prod(tail)) if tail else 1
        if F < 1:
            raise ValueError(f"{what}: rows of no elements")
        out = ops.gather_rows(t.reshape(rows, F), idx)
        return out.reshape((idx.numel(),) + tail)

    def take_vertices(self, t):
        """the batch's rows of a per-vertex tensor of the dataset, [n, ...] -> [n_batch, ...]"""
        return self._take(t, self.vertex_map, self._rows[0], "take_vertices")

    def take_edges(self, t):
        """the batch's rows of a per-edge tensor of the dataset (feature [E], vec [E, 3], ...)"""
        return self._take(t, self.edge_map, self._rows[1], "take_edges")

    def take_structures(self, t):
        """the batch's rows of a per-structure tensor of the dataset (lat [B, 3, 3], targets [B, ...])"""
        import torch

        if self._ids_dev is None:
            self._ids_dev = torch.from_numpy(self.ids).to(self.vertex_map.device)
        return self._take(t, self._ids_dev, self._rows[2], "take_structures")

    def close(self):
        self.handle.close()


class DeviceDataset:
    """A block-diagonal dataset handle (DeviceGraph.from_structures, a layer's batched graph, io.batch_graphs) cut into structures
    by vertex_offsets [B + 1] (int32) and edge_offsets [B + 1] (int64; None for a handle without edge columns).  Owns the batch plan
    (athena_mp_batch_plan_create: the block-diagonal check on the device and the per-structure tables) and keeps the handle alive."""

    def __init__(self, handle, vertex_offsets, edge_offsets=None):
        self.handle = handle
        self.vertex_offsets = np.ascontiguousarray(vertex_offsets, dtype=np.int32).copy()
        self.edge_offsets = None if edge_offsets is None else np.ascontiguousarray(edge_offsets, dtype=np.int64).copy()
        if self.vertex_offsets.ndim != 1 or self.vertex_offsets.size < 1:
            raise ValueError("vertex_offsets must be [B + 1]")
        if self.edge_offsets is not None and self.edge_offsets.shape != self.vertex_offsets.shape:
            raise ValueError("edge_offsets must be [B + 1] like vertex_offsets")
        self.num_structures = int(self.vertex_offsets.size - 1)
        _capi.use_torch_stream()
        plan = C.c_void_p()
        _capi.call("athena_mp_batch_plan_create", handle.handle, self.num_structures, self.vertex_offsets.ctypes.data_as(C.c_void_p),
                   self.edge_offsets.ctypes.data_as(C.c_void_p) if self.edge_offsets is not None else None, C.byref(plan))
        self._plan = plan

    def __len__(self):
        return self.num_structures

    def sizes(self, ids):
        """(vertex_offsets, edge_offsets) of the batch `ids` would give: the size query, nothing is built"""
        if self._plan is None:
            raise ValueError("the dataset is closed")
        sel = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        voff = np.empty(sel.size + 1, np.int32)
        eoff = np.empty(sel.size + 1, np.int64)
        _capi.call("athena_mp_batch_select", self._plan, sel.size, sel.ctypes.data_as(C.c_void_p), None, voff.ctypes.data_as(C.c_void_p),
                   eoff.ctypes.data_as(C.c_void_p), None, None)
        return voff, eoff

    def select(self, ids, vertex_map=None, edge_map=None, plan_degrees=None):
        """The batch of the structures `ids` (0-based, any order, repeats allowed) as a Batch.  vertex_map / edge_map: contiguous int32
        device tensors of the batch's vertex / edge-column count to write the maps into.  plan_degrees = (min_deg, max_deg): the
        child's Duvenaud degree-bucket plan is built behind the select, on the same stream (DeviceGraph.plan_duvenaud), so the first
        layer call on the batch does not stop to build it."""
        import torch

        if self._plan is None:
            raise ValueError("the dataset is closed")
        sel = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        voff, eoff = self.sizes(sel)
        dev = torch.device("cuda", torch.cuda.current_device())
        maps = []
        for given, count, what in ((vertex_map, int(voff[-1]), "vertex_map"), (edge_map, int(eoff[-1]), "edge_map")):
            if given is None:
                given = torch.empty(count, dtype=torch.int32, device=dev)
            elif not (given.is_cuda and given.dtype == torch.int32 and given.is_contiguous() and tuple(given.shape) == (count,)):
                raise ValueError(f"{what} must be a contiguous int32 device tensor [{count}]")
            maps.append(given)
        _capi.use_torch_stream()
        child = C.c_void_p()
        _capi.call("athena_mp_batch_select", self._plan, sel.size, sel.ctypes.data_as(C.c_void_p), C.byref(child),
                   voff.ctypes.data_as(C.c_void_p), eoff.ctypes.data_as(C.c_void_p), C.c_void_p(maps[0].data_ptr()),
                   C.c_void_p(maps[1].data_ptr()))
        rows = (int(self.vertex_offsets[-1]), int(self.edge_offsets[-1]) if self.edge_offsets is not None else 0, self.num_structures)
        b = Batch(DeviceGraph.borrow(child), voff, eoff, maps[0], maps[1], sel.copy(), rows)
        b.handle._borrowed = False                                             # the batch owns its child: close() destroys it
        if plan_degrees is not None:
            b.handle.plan_duvenaud(*plan_degrees)
        return b

    def batches(self, batch_size, shuffle=True, seed=0, drop_last=False):
        """The Batches of one epoch, batch_size structures each (the last one smaller unless drop_last).  With shuffle the order is
        numpy.random.default_rng(seed).permutation(B): pass the epoch as the seed for a new order every epoch.  The reference's own
        shuffle order (network%train under shuffle_batches) is not pinned anywhere and is not reproduced."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        B = self.num_structures
        order = np.random.default_rng(seed).permutation(B).astype(np.int32) if shuffle else np.arange(B, dtype=np.int32)
        for i0 in range(0, B, batch_size):
            ids = order[i0:i0 + batch_size]
            if drop_last and ids.size < batch_size:
                break
            yield self.select(ids)

    def close(self):
        """destroys the plan; the dataset handle is the caller's, batches already drawn stay valid"""
        if getattr(self, "_plan", None):
            _capi.load().athena_mp_batch_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_HOP = 0xD1B54A32D192ED03
_DEGREES = {"block": 0, "parent": 1}


class Block:
    """One hop of a NeighborSampler: handle (a DeviceGraph that owns the rectangular block: row s is seed s, its columns are the seeds
    first, then the other sampled vertices ascending by id), n_seeds, and the int32 device tensors vertex_map [n_cols] (the parent
    vertex of every column; vertex_map[:n_seeds] are the seeds), entry_map [nnz] (the parent CSR position of every entry) and
    edge_map [nnz] (the parent edge column of every entry, -1 for an entry without one; None when the parent has no edge columns).
    All three are 0-based, as Batch.vertex_map: the C ABI's are 1-based, like `sample` of geometry.farthest_points."""

    def __init__(self, handle, n_seeds, vertex_map, entry_map, edge_map, parent_rows, vertex_ids):
        self.handle, self.n_seeds = handle, n_seeds
        self.vertex_map, self.entry_map, self.edge_map = vertex_map, entry_map, edge_map
        self._rows = parent_rows                                               # the parent's (vertices, edge columns, entries)
        self._vertex_ids = vertex_ids                                          # vertex_map 1-based: the next hop's seeds as they are

    def take_vertices(self, t):
        """the block's columns of a per-vertex tensor of the parent, [n, ...] -> [n_cols, ...]; its first n_seeds rows are the seeds'"""
        return Batch._take(t, self.vertex_map, self._rows[0], "take_vertices")

    def take_edges(self, t):
        """the block's entries of a per-edge tensor of the parent (feature [E], coords [E, 3], ...), one row per entry, which is the
        block's edge column; an entry without an edge column (edge_map < 0) takes row 0"""
        if self.edge_map is None:
            raise ValueError("take_edges: the parent has no edge columns")
        return Batch._take(t, self.edge_map.clamp(min=0), self._rows[1], "take_edges")

    def take_entries(self, t):
        """the block's entries of a per-entry tensor of the parent (one row per CSR position), [nnz_parent, ...] -> [nnz, ...]"""
        return Batch._take(t, self.entry_map, self._rows[2], "take_entries")

    def close(self):
        self.handle.close()


class NeighborSampler:
    """Neighbour-sampled mini-batches of one square handle that stays on the device (athena_mp_sampler_create; the definition is in
    include/athena_mp.h).  Owns the sampler plan and keeps the handle alive; one sample at a time."""

    def __init__(self, handle):
        if handle.n_rows != handle.n_cols:
            raise ValueError(f"a rectangular handle ({handle.n_rows} x {handle.n_cols}) has no vertices to walk on")
        self.handle = handle
        self.num_vertices = int(handle.n_rows)
        _capi.use_torch_stream()
        plan = C.c_void_p()
        _capi.call("athena_mp_sampler_create", handle.handle, C.byref(plan))
        self._plan = plan
        self.hop_stats = []                                                    # stats() of every hop of the last sample()

    def __len__(self):
        return self.num_vertices

    def _hop(self, seeds1, k, seed, mode):
        import torch

        dev = seeds1.device
        m, n = int(seeds1.numel()), self.num_vertices
        _capi.use_torch_stream()
        if k > 0:
            cap = m * k                                                        # rows have min(L, k) entries
        else:
            nnz = C.c_int64()
            _capi.call("athena_mp_sample_count", self._plan, m, C.c_void_p(seeds1.data_ptr()), k, None, C.byref(nnz))
            cap = nnz.value
        vcap = min(n, m + cap)
        has_edges = self.handle.n_edge_cols > 0
        vm = torch.empty(vcap, dtype=torch.int32, device=dev)
        em = torch.empty(cap, dtype=torch.int32, device=dev)
        ed = torch.empty(cap, dtype=torch.int32, device=dev) if has_edges else None
        n_cols, nnz, block = C.c_int32(), C.c_int64(), C.c_void_p()
        _capi.call("athena_mp_sample_neighbors", self._plan, m, C.c_void_p(seeds1.data_ptr()), k, C.c_uint64(seed), mode,
                   C.c_void_p(vm.data_ptr()), vcap, C.c_void_p(em.data_ptr()), cap, C.c_void_p(ed.data_ptr()) if has_edges else None, cap,
                   C.byref(n_cols), C.byref(nnz), C.byref(block))
        g = DeviceGraph.borrow(block)
        g._borrowed = False                                                    # the block owns its handle: close() destroys it
        vm = vm[:n_cols.value]
        rows = (n, self.handle.n_edge_cols, int(self.handle.nnz))
        return Block(g, m, vm - 1, em[:nnz.value].sub_(1), ed[:nnz.value].sub_(1) if has_edges else None, rows, vm)

    def sample(self, seeds, fanouts, seed=0, degrees="block"):
        """The blocks of the vertices `seeds` (0-based, distinct, any order: a sequence, a numpy array or an int32 device tensor), one
        per fan-out: hop h draws fanouts[h] entries per row, hop 0 around the seeds, each further hop around the previous hop's whole
        vertex_map.  A fan-out is 1..64, or 0 for every entry.  Returned outermost first, the order the layers apply them: blocks[0] is
        fed with blocks[0].take_vertices(x), blocks[-1] has the seeds as its rows, and blocks[i].vertex_map[:blocks[i].n_seeds] equals
        blocks[i + 1].vertex_map.  degrees: "block" (row lengths and column counts of the block) or "parent" (the parent's degrees
        of the same vertices: with fan-out 0 a Kipf step on the block is the parent's step on the seed rows).  The same (seed, vertex)
        draws the same neighbours whatever else is in the batch; pass the epoch as the seed."""
        import torch

        if self._plan is None:
            raise ValueError("the sampler is closed")
        if degrees not in _DEGREES:
            raise ValueError('degrees must be "block" or "parent"')
        fanouts = [int(k) for k in fanouts]
        if not fanouts or any(k < 0 or k > 64 for k in fanouts):
            raise ValueError("fanouts: at least one, each in 0..64 (0: every entry)")
        dev = torch.device("cuda", torch.cuda.current_device())
        if isinstance(seeds, torch.Tensor):
            s1 = seeds.to(dev, torch.int32).reshape(-1) + 1
        else:
            s1 = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1) + np.int32(1)).to(dev)
        blocks, self.hop_stats = [], []
        for h, k in enumerate(fanouts):
            b = self._hop(s1, k, (int(seed) + _HOP * (h + 1)) % 2 ** 64, _DEGREES[degrees])
            blocks.append(b)
            self.hop_stats.append(self.stats())                               # per hop, in hop order
            s1 = b._vertex_ids
        return blocks[::-1]

    def batches(self, batch_size, fanouts, ids=None, shuffle=True, seed=0, drop_last=False):
        """The block lists of one epoch, batch_size seed vertices each (the last one smaller unless drop_last), over the vertices `ids`
        (None: all of them).  With shuffle the order is numpy.random.default_rng(seed).permutation, as DeviceDataset.batches: pass
        the epoch as the seed for a new order and new neighbours every epoch."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        ids = np.arange(self.num_vertices, dtype=np.int32) if ids is None else np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        order = ids[np.random.default_rng(seed).permutation(ids.size)] if shuffle else ids
        for i0 in range(0, order.size, batch_size):
            part = order[i0:i0 + batch_size]
            if drop_last and part.size < batch_size:
                break
            yield self.sample(part, fanouts, seed=seed)

    def stats(self):
        """of the last hop sampled: rows drawn by key, rows copied whole, 64-entry steps, steps skipped, and the microseconds of the
        count stretch, the draw kernel, the relabelling and the handle (athena_mp_sample_stats)"""
        out = np.zeros(8, np.int64)
        _capi.call("athena_mp_sample_stats", out.ctypes.data_as(C.c_void_p))
        return out

    def close(self):
        """destroys the plan; the parent handle is the caller's, blocks already drawn stay valid"""
        if getattr(self, "_plan", None):
            _capi.load().athena_mp_sampler_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
