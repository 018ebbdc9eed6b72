"""Mini-batches drawn from a dataset graph that stays on the device (athena_amd/csrc/batch_select.hip; the definition is in
include/athena_mp.h): what network%train does with get_sample(input_graph, i0, i1) under shuffle_batches, without assembling the
batch on the host and without searching its neighbours again.

    handle, feature, vec, voff, eoff = DeviceGraph.from_structures(...)        # once
    ds = DeviceDataset(handle, voff, eoff)
    for b in ds.batches(2000, seed=epoch):
        layer.set_graph_handle(b.handle, b.vertex_offsets)
        out = layer.forward(b.take_vertices(x), b.take_edges(feature)[:, None]) ...
        g = structures_grad(b.handle, b.take_structures(lat), b.vertex_offsets, b.edge_offsets, b.take_edges(vec), cutoff_max, dfeature=de)

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
