"""Host-side mirror of graphstruc's `graph_type` as athena's msgpass layers see it, plus the
device graph handle.

The reference reads only `adj_ia`, `adj_ja`, vertex/edge feature arrays and the counts from
`graph_type` (call sites athena_kipf_msgpass_layer.f90:943-946,
athena_msgpass_layer_sub.f90:144-174).  Conventions are kept Fortran-like so tests read like the
reference's:
  adj_ia : int32 [num_vertices+1], 1-based row pointers
  adj_ja : int32 [2, nnz]; adj_ja[0, w] = neighbour (1-based), adj_ja[1, w] = undirected edge id
           (1-based; 0 for a self-loop entry, as in test/test_diffstruc_extd_kipf.f90:29-31)
  vertex_features : float32 [num_vertex_features, num_vertices] (Fortran shape) -- stored here
           transposed as C-contiguous [num_vertices, F], which is the same memory.
"""
import ctypes as C

import numpy as np

from . import _capi


def _knn_radius(radius):
    """the cap of the k-nearest-neighbour builders: None = +infinity = no cap"""
    return float("inf") if radius is None else float(radius)


def _knn_mode(mode):
    if mode not in ("union", "mutual", 0, 1):
        raise ValueError('mode must be "union" or "mutual"')
    return {"union": 0, "mutual": 1}.get(mode, mode)


def _two_sets_on_device(queries, sources, query_offsets, source_offsets, device):
    """the inputs of the two-set builders as the C ABI takes them: (device, queries, sources) float32 [n, dim] on the device and
    query_offsets / source_offsets [B + 1] int32 on the host (both None: one cloud); the torch stream is the library's"""
    import torch

    _capi.init(device)
    dev = torch.device("cuda", device)

    def on_device(p, what):
        if isinstance(p, torch.Tensor):
            t = p.to(dev, torch.float32).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).to(dev)
        if t.dim() != 2:
            raise ValueError(f"{what} must be [n, dim]")
        return t

    q, s = on_device(queries, "queries"), on_device(sources, "sources")
    if q.shape[1] != s.shape[1]:
        raise ValueError(f"queries have {q.shape[1]} components, sources {s.shape[1]}")
    if (query_offsets is None) != (source_offsets is None):
        raise ValueError("query_offsets and source_offsets must be given together")
    qoff = np.ascontiguousarray([0, q.shape[0]] if query_offsets is None else query_offsets, dtype=np.int32)
    soff = np.ascontiguousarray([0, s.shape[0]] if source_offsets is None else source_offsets, dtype=np.int32)
    if qoff.ndim != 1 or qoff.size < 1 or soff.shape != qoff.shape:
        raise ValueError("query_offsets and source_offsets must both be [B + 1]")
    _capi.use_torch_stream()
    return dev, q, s, qoff, soff


def _structure_arrays(frac, lat, offsets, pbc):
    """the inputs of the periodic builders as the C ABI takes them: frac [n, 3] / lat [B, 3, 3] float32, offsets [B + 1] and
    pbc [3] int32 on the host"""
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    pbc3 = np.ascontiguousarray([1 if p else 0 for p in pbc], dtype=np.int32)
    if not (off.ndim == 1 and off.size >= 1 and pbc3.size == 3):
        raise ValueError("offsets must be [B + 1] and pbc three flags")
    if isinstance(frac, np.ndarray) or not hasattr(frac, "data_ptr"):
        frac = np.ascontiguousarray(frac, dtype=np.float32).reshape(-1, 3)
    if isinstance(lat, np.ndarray) or not hasattr(lat, "data_ptr"):
        lat = np.ascontiguousarray(lat, dtype=np.float32).reshape(-1, 3, 3)
    if not (lat.shape[0] == off.size - 1 and tuple(lat.shape[1:]) == (3, 3) and frac.shape[-1] == 3 and len(frac.shape) == 2):
        raise ValueError("frac must be [n, 3] and lat [B, 3, 3] with B + 1 offsets")
    return frac, lat, off, pbc3


PERIODIC_STATS = ("structures_walked", "structures_grid", "walk_pairs", "grid_pairs", "grid_fallbacks")


def periodic_stats():
    """What the most recent periodic build of the process did (athena_mp_periodic_stats), as a dict: structures that took the
    walk over every pair / the cell grid, atom pairs i <= j each route examined, and structures that qualified for the grid but
    took the walk (a fractional coordinate beyond +-64, lattice vectors too long for the cutoff, or no periodic axis)."""
    out = (C.c_int64 * 5)()
    _capi.call("athena_mp_periodic_stats", out)
    return dict(zip(PERIODIC_STATS, (int(v) for v in out)))


def duvenaud_plan_stats():
    """Degree-bucket plans this process built on the host / on the device, and requests served by a plan the handle already held
    (athena_mp_duvenaud_plan_stats), as a dict."""
    h, d, r = C.c_int64(), C.c_int64(), C.c_int64()
    _capi.call("athena_mp_duvenaud_plan_stats", C.byref(h), C.byref(d), C.byref(r))
    return {"host_builds": int(h.value), "device_builds": int(d.value), "reused": int(r.value)}


class graph_type:
    """Undirected sparse graph in athena's CSR convention."""

    def __init__(self):
        self._version = 0
        self.num_vertices = 0
        self.num_edges = 0
        self.num_vertex_features = 0
        self.num_edge_features = 0
        self.adj_ia = np.ones(1, np.int32)
        self.adj_ja = np.zeros((2, 0), np.int32, order="F")
        self.vertex_features = None  # [num_vertices, Fv]
        self.edge_features = None    # [num_edges, Fe]
        self.is_sparse = True

    # adjacency arrays: assigning either one (generate_adjacency, add_self_loops, from_csr, user code) bumps a version
    # counter that the layers' device-handle cache keys on
    @property
    def adj_ia(self):
        return self._adj_ia

    @adj_ia.setter
    def adj_ia(self, a):
        self._adj_ia = a
        self._version += 1

    @property
    def adj_ja(self):
        return self._adj_ja

    @adj_ja.setter
    def adj_ja(self, a):
        self._adj_ja = a
        self._version += 1

    def topology_key(self):
        """what a cached device handle of this graph is valid for: the object, its version (bumped by every assignment
        of adj_ia / adj_ja), the sizes and the C ABI's content key of the arrays (athena_mp_graph_key: EVERY word of
        both arrays, hashed by a few host threads -- an in-place edit is always seen, as in the reference, which
        re-copies the CSR on every set_graph.  Only under ATHENA_MP_GRAPH_KEY_SAMPLED=1 does a graph of 2^18 entries
        or more get the cheap sampled key; then an in-place edit needs touch(), which also evicts the stale handle
        from the library's cache)."""
        import ctypes as C

        from . import _capi

        # A FROZEN graph (freeze(): both arrays read-only, so an in-place edit raises instead of going unseen) keeps its key
        # for as long as the arrays and the version stay what they were: set_graph before every forward then costs a tuple
        # compare, not a pass over every word of the CSR (1.5 ms per 84 MB, per layer, per step).
        memo = getattr(self, "_key_memo", None)
        if memo is not None:
            ia0, ja0 = self._adj_ia, self._adj_ja
            if (memo[0] == (self._version, id(ia0), id(ja0), ia0.ctypes.data, ja0.ctypes.data, ia0.size, ja0.size)
                    and not ia0.flags.writeable and not ja0.flags.writeable):
                return memo[1]
        ia = np.ascontiguousarray(self._adj_ia, dtype=np.int32)
        ja = np.asfortranarray(self._adj_ja, dtype=np.int32)
        key = C.c_uint64(0)
        _capi.call("athena_mp_graph_key", int(ia.size - 1), int(ja.shape[1]), ia.ctypes.data, ja.ctypes.data, C.byref(key))
        out = (id(self), self._version, int(self.num_vertices), int(ja.shape[1]), int(key.value))
        # memoised ONLY for the arrays freeze() made: views of immutable bytes objects, which numpy refuses to make writeable
        # again -- a read-only array that owns its data could be un-frozen, edited and re-frozen behind the memo
        ia0, ja0 = self._adj_ia, self._adj_ja
        if getattr(self, "_frozen", None) == (id(ia0), id(ja0)) and not ia0.flags.writeable and not ja0.flags.writeable:
            self._key_memo = ((self._version, id(ia0), id(ja0), ia0.ctypes.data, ja0.ctypes.data, ia0.size, ja0.size), out)
        else:
            self._key_memo = None
        return out

    def freeze(self):
        """Make adj_ia / adj_ja IMMUTABLE arrays (int32, contiguous / Fortran order, views of bytes objects: an in-place edit
        raises, and so does setting flags.writeable back to True), so topology_key() may memoise the content key -- nothing can
        change under it without an assignment (which bumps the version and drops the memo).  Returns self."""
        ia_src = np.ascontiguousarray(self._adj_ia, dtype=np.int32)
        ja_src = np.asfortranarray(self._adj_ja, dtype=np.int32)
        ia = np.frombuffer(ia_src.tobytes(order="C"), dtype=np.int32)
        ja = np.frombuffer(ja_src.tobytes(order="F"), dtype=np.int32).reshape(ja_src.shape, order="F")
        self._adj_ia, self._adj_ja = ia, ja
        self._version += 1
        self._key_memo = None
        self._frozen = (id(ia), id(ja))
        return self

    def touch(self):
        """the adjacency arrays were edited in place: cached device handles of this graph are stale"""
        self._version += 1

    # -- graphstruc API used by the reference's tests (test_kipf_msgpass_layer.f90:71-100) -------
    def set_num_vertices(self, n, num_features=0):
        self.num_vertices = int(n)
        self.num_vertex_features = int(num_features)
        self.vertex_features = np.zeros((self.num_vertices, self.num_vertex_features), np.float32)

    def set_num_edges(self, n, num_features=0):
        self.num_edges = int(n)
        self.num_edge_features = int(num_features)
        self.edge_features = np.zeros((self.num_edges, self.num_edge_features), np.float32)

    def generate_adjacency(self, index_list):
        """index_list [2, num_edges], 1-based vertex pairs; edge e = column e (1-based id).

        Each undirected edge contributes two CSR entries sharing the same edge id.  Within a row,
        entries are ordered by edge id (graphstruc's internal order is not visible from the
        reference and only affects fp32 summation order)."""
        idx = np.asarray(index_list, dtype=np.int64)
        if not (idx.ndim == 2 and idx.shape[0] == 2):
            raise ValueError('expected: idx.ndim == 2 and idx.shape[0] == 2')
        E = idx.shape[1]
        if self.num_edges == 0:
            self.num_edges = E
        src = np.concatenate([idx[0], idx[1]])
        dst = np.concatenate([idx[1], idx[0]])
        eid = np.concatenate([np.arange(1, E + 1), np.arange(1, E + 1)])
        loops = idx[0] == idx[1]
        if loops.any():  # a self edge is a single CSR entry
            keep = np.concatenate([np.ones(E, bool), ~loops])
            src, dst, eid = src[keep], dst[keep], eid[keep]
        self._from_entries(src, dst, eid)

    def generate_adjacency_device(self, index_list, add_self_loops=False):
        """generate_adjacency (+ add_self_loops) on the GPU: same arrays as the host methods, built by one radix sort
        (athena_mp_csr_from_edges); for edge lists of millions of pairs"""
        idx = np.asfortranarray(np.asarray(index_list, dtype=np.int32))
        if not (idx.ndim == 2 and idx.shape[0] == 2):
            raise ValueError('expected: idx.ndim == 2 and idx.shape[0] == 2')
        E = idx.shape[1]
        if self.num_edges == 0:
            self.num_edges = E
        _capi.init(0)
        ia = np.empty(self.num_vertices + 1, np.int32)
        nnz = C.c_int64()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _capi.call("athena_mp_csr_from_edges", self.num_vertices, E, vp(idx), int(add_self_loops), vp(ia), None, 0, C.byref(nnz))
        ja = np.empty((2, nnz.value), np.int32, order="F")
        _capi.call("athena_mp_csr_from_edges", self.num_vertices, E, vp(idx), int(add_self_loops), vp(ia), vp(ja), nnz.value,
                   C.byref(nnz))
        self.adj_ia, self.adj_ja = ia, ja

    def generate_radius_adjacency_device(self, points, radius, add_self_loops=False):
        """The radius graph of a point cloud, built on the GPU (athena_mp_radius_graph_host): points [n, dim] float32, dim 1..3;
        i < j are joined iff the fp32 sum of the squared fp32 differences is <= fl(radius * radius); edge ids follow the
        lexicographic order of (i, j).  Sets num_vertices (when unset), num_edges, adj_ia, adj_ja -- the arrays
        generate_adjacency (+ add_self_loops) makes of that pair list -- and returns coords [num_edges, dim] = p_i - p_j
        (numpy), graph_nop_layer_type's edge input.  The sibling of generate_adjacency_device."""
        pts = np.ascontiguousarray(points, dtype=np.float32)
        if pts.ndim != 2:
            raise ValueError("points must be [n, dim]")
        n, dim = pts.shape
        if self.num_vertices == 0:
            self.num_vertices = n
        if n != self.num_vertices:
            raise ValueError("points must hold one row per vertex")
        _capi.init(0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        nnz, E = C.c_int64(), C.c_int64()
        _capi.call("athena_mp_radius_graph_host", n, dim, vp(pts), float(radius), int(bool(add_self_loops)), None, None, 0,
                   C.byref(nnz), None, 0, C.byref(E))
        ia = np.empty(n + 1, np.int32)
        ja = np.empty((2, nnz.value), np.int32, order="F")
        coords = np.empty((E.value, dim), np.float32)
        _capi.call("athena_mp_radius_graph_host", n, dim, vp(pts), float(radius), int(bool(add_self_loops)), vp(ia), vp(ja),
                   nnz.value, C.byref(nnz), vp(coords), E.value, C.byref(E))
        self.num_edges = int(E.value)
        self.adj_ia, self.adj_ja = ia, ja
        return coords

    def generate_radius_batch_adjacency_device(self, points, offsets, radius, add_self_loops=False):
        """The radius graphs of a batch of point clouds as ONE block-diagonal graph, built on the GPU
        (athena_mp_radius_graph_batched_host; the definition is in include/athena_mp.h): points [n, dim] float32, dim 1..3,
        offsets [B + 1] 0-based; cloud b is the rows offsets[b] .. offsets[b+1]-1.  Sets num_vertices (when unset), num_edges,
        adj_ia, adj_ja -- what generate_radius_adjacency_device makes of every cloud, edge ids running over the batch -- and
        returns (coords [num_edges, dim] = p_i - p_j, edge_offsets [B + 1] int64) as numpy.  The host-array sibling of
        DeviceGraph.from_point_clouds."""
        pts = np.ascontiguousarray(points, dtype=np.float32)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        if pts.ndim != 2 or off.ndim != 1 or off.size < 1:
            raise ValueError("points must be [n, dim] and offsets [B + 1]")
        n, dim = pts.shape
        B = off.size - 1
        if self.num_vertices == 0:
            self.num_vertices = n
        if n != self.num_vertices:
            raise ValueError("points must hold one row per vertex")
        _capi.init(0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        nnz, E = C.c_int64(), C.c_int64()
        head = (B, n, vp(off), dim, vp(pts), float(radius), int(bool(add_self_loops)))
        _capi.call("athena_mp_radius_graph_batched_host", *head, None, None, 0, C.byref(nnz), None, 0, C.byref(E), None)
        ia = np.empty(n + 1, np.int32)
        ja = np.empty((2, nnz.value), np.int32, order="F")
        coords = np.empty((E.value, dim), np.float32)
        eoff = np.empty(B + 1, np.int64)
        _capi.call("athena_mp_radius_graph_batched_host", *head, vp(ia), vp(ja), nnz.value, C.byref(nnz), vp(coords), E.value,
                   C.byref(E), vp(eoff))
        self.num_edges = int(E.value)
        self.adj_ia, self.adj_ja = ia, ja
        return coords, eoff

    def generate_knn_batch_adjacency_device(self, points, offsets, k, radius=None, mode="union", add_self_loops=False):
        """The k-nearest-neighbour graphs of a batch of point clouds as ONE block-diagonal graph, built on the GPU
        (athena_mp_knn_graph_batched_host; the definition is in include/athena_mp.h): every point is joined to the first k others
        of its cloud in the order (fp32 squared distance, index), inside radius when one is given; mode "union" keeps a pair
        either end chose, "mutual" one both chose.  Sets num_vertices (when unset), num_edges, adj_ia, adj_ja and returns
        (coords [num_edges, dim] = p_i - p_j, edge_offsets [B + 1] int64) as numpy.  The host-array sibling of
        DeviceGraph.from_point_clouds_knn."""
        pts = np.ascontiguousarray(points, dtype=np.float32)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        if pts.ndim != 2 or off.ndim != 1 or off.size < 1:
            raise ValueError("points must be [n, dim] and offsets [B + 1]")
        n, dim = pts.shape
        B = off.size - 1
        if self.num_vertices == 0:
            self.num_vertices = n
        if n != self.num_vertices:
            raise ValueError("points must hold one row per vertex")
        _capi.init(0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        nnz, E = C.c_int64(), C.c_int64()
        head = (B, n, vp(off), dim, vp(pts), int(k), _knn_radius(radius), _knn_mode(mode), int(bool(add_self_loops)))
        _capi.call("athena_mp_knn_graph_batched_host", *head, None, None, 0, C.byref(nnz), None, 0, C.byref(E), None)
        ia = np.empty(n + 1, np.int32)
        ja = np.empty((2, nnz.value), np.int32, order="F")
        coords = np.empty((E.value, dim), np.float32)
        eoff = np.empty(B + 1, np.int64)
        _capi.call("athena_mp_knn_graph_batched_host", *head, vp(ia), vp(ja), nnz.value, C.byref(nnz), vp(coords), E.value,
                   C.byref(E), vp(eoff))
        self.num_edges = int(E.value)
        self.adj_ia, self.adj_ja = ia, ja
        return coords, eoff

    def generate_knn_adjacency_device(self, points, k, radius=None, mode="union", add_self_loops=False):
        """generate_knn_batch_adjacency_device for one cloud; returns coords [num_edges, dim]."""
        pts = np.ascontiguousarray(points, dtype=np.float32)
        if pts.ndim != 2:
            raise ValueError("points must be [n, dim]")
        return self.generate_knn_batch_adjacency_device(pts, [0, pts.shape[0]], k, radius, mode, add_self_loops)[0]

    def generate_periodic_adjacency_device(self, frac, lat, offsets, cutoff_min, cutoff_max, pbc=(1, 1, 1), add_self_loops=False):
        """The neighbour graphs of a batch of periodic structures as ONE block-diagonal graph, built on the GPU
        (athena_mp_periodic_graph_host; the definition is in include/athena_mp.h): frac [n, 3] float32 fractional coordinates,
        lat [B, 3, 3] float32 (row a = lattice vector a), offsets [B + 1] 0-based.  What get_graph_from_basis + generate_adjacency
        (+ add_self_loops) make of every structure, edge ids running over the batch.  Sets num_vertices (when unset), num_edges,
        adj_ia, adj_ja and returns (feature [E] = r / cutoff_max, vec [E, 3], first_count [n], edge_offsets [B + 1]) as numpy.
        The host-array sibling of DeviceGraph.from_structures."""
        frac, lat, off, pbc3 = _structure_arrays(frac, lat, offsets, pbc)
        n, B = frac.shape[0], lat.shape[0]
        if self.num_vertices == 0:
            self.num_vertices = n
        if n != self.num_vertices:
            raise ValueError("frac must hold one row per vertex")
        _capi.init(0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        nnz, E = C.c_int64(), C.c_int64()
        head = (B, n, vp(off), vp(frac), vp(lat), vp(pbc3), float(cutoff_min), float(cutoff_max), int(bool(add_self_loops)))
        _capi.call("athena_mp_periodic_graph_host", *head, None, None, 0, C.byref(nnz), None, None, None, 0, C.byref(E), None)
        ia = np.empty(n + 1, np.int32)
        ja = np.empty((2, nnz.value), np.int32, order="F")
        feature = np.empty(E.value, np.float32)
        vec = np.empty((E.value, 3), np.float32)
        first = np.empty(n, np.int32)
        eoff = np.empty(B + 1, np.int64)
        _capi.call("athena_mp_periodic_graph_host", *head, vp(ia), vp(ja), nnz.value, C.byref(nnz), vp(feature), vp(vec), vp(first),
                   E.value, C.byref(E), vp(eoff))
        self.num_edges = int(E.value)
        self.adj_ia, self.adj_ja = ia, ja
        return feature, vec, first, eoff

    def add_self_loops(self):
        """A~ = A + I: one entry (v, v) with edge id 0 per vertex that has none."""
        rows = np.repeat(np.arange(1, self.num_vertices + 1), np.diff(self.adj_ia))
        has = np.zeros(self.num_vertices + 1, bool)
        has[rows[self.adj_ja[0] == rows]] = True
        add = np.nonzero(~has[1:])[0] + 1
        src = np.concatenate([rows, add])
        dst = np.concatenate([self.adj_ja[0], add])
        eid = np.concatenate([self.adj_ja[1], np.zeros(add.size, np.int64)])
        self._from_entries(src, dst, eid, self_loops_first=True)

    def _from_entries(self, src, dst, eid, self_loops_first=False):
        n = self.num_vertices
        key = eid.astype(np.int64)
        if self_loops_first:
            key = np.where(eid == 0, -1, key)
        order = np.lexsort((key, src))
        src, dst, eid = src[order], dst[order], eid[order]
        counts = np.bincount(src - 1, minlength=n)
        self.adj_ia = np.concatenate([[1], 1 + np.cumsum(counts)]).astype(np.int32)
        ja = np.empty((2, src.size), np.int32, order="F")
        ja[0] = dst
        ja[1] = eid
        self.adj_ja = ja

    @property
    def nnz(self):
        return int(self.adj_ja.shape[1])

    @classmethod
    def from_csr(cls, adj_ia, adj_ja, num_edges=None):
        g = cls()
        g.adj_ia = np.ascontiguousarray(adj_ia, np.int32)
        g.adj_ja = np.asfortranarray(adj_ja, np.int32)
        g.num_vertices = g.adj_ia.size - 1
        g.num_edges = int(g.adj_ja[1].max()) if (num_edges is None and g.adj_ja.shape[1]) else int(num_edges or 0)
        return g


class DeviceGraph:
    """Owns an `athena_mp_graph*` (device CSR + transposed CSR + coefficients).

    Built once and reused: the reference re-copies the CSR on every forward
    (athena_network_sub.f90:2727-2730); the handle is what `set_graph` caches."""

    def __init__(self, adj_ia, adj_ja, n_cols=None, n_edge_cols=None, row_deg=None, col_deg=None, device=0, shared=False):
        """shared=True (square graph, degrees = row lengths): the handle comes from the library's content-keyed cache
        (athena_mp_graph_acquire) -- every layer of a network that is given the same graph gets the same device arrays,
        and close() releases a reference instead of freeing them"""
        _capi.init(device)
        ia = np.ascontiguousarray(adj_ia, np.int32)
        ja = np.asfortranarray(adj_ja, np.int32)
        if not (ja.ndim == 2 and ja.shape[0] == 2):
            raise ValueError("adj_ja must be [2, nnz]")
        self.n_rows = ia.size - 1
        self.n_cols = self.n_rows if n_cols is None else int(n_cols)
        self.nnz = int(ja.shape[1])
        if n_edge_cols is None:
            n_edge_cols = int(ja[1].max()) if self.nnz else 0
        elif n_edge_cols == 0 and self.nnz and ja[1].any():
            ja = ja.copy(order="F")  # edge ids not needed (Kipf): drop them, skip the edge index
            ja[1] = 0
        self.n_edge_cols = int(n_edge_cols)
        rd = cd = None
        if row_deg is not None:
            rd = np.ascontiguousarray(row_deg, np.int32)
            cd = np.ascontiguousarray(col_deg, np.int32)
            if not (rd.size == self.n_rows and cd.size == self.n_cols):
                raise ValueError('expected: rd.size == self.n_rows and cd.size == self.n_cols')
        h = C.c_void_p()
        if shared and rd is None and self.n_cols == self.n_rows:
            _capi.call("athena_mp_graph_acquire", self.n_rows, self.nnz, ia.ctypes.data_as(C.c_void_p),
                       ja.ctypes.data_as(C.c_void_p), self.n_edge_cols, C.byref(h))
        else:
            _capi.call(
                "athena_mp_graph_create", self.n_rows, self.n_cols, self.nnz,
                ia.ctypes.data_as(C.c_void_p), ja.ctypes.data_as(C.c_void_p), self.n_edge_cols,
                rd.ctypes.data_as(C.c_void_p) if rd is not None else None,
                cd.ctypes.data_as(C.c_void_p) if cd is not None else None, C.byref(h))
        self.handle = h

    _ARRAYS = {"rowptr": (0, np.int32), "col": (1, np.int32), "eid": (2, np.int32), "coef": (3, np.float32),
               "t_rowptr": (4, np.int32), "t_src": (5, np.int32), "t_eid": (6, np.int32), "t_coef": (7, np.float32),
               "e_rowptr": (8, np.int32), "e_row": (9, np.int32), "e_entry": (10, np.int32),
               "deg_row": (11, np.int32), "deg_col": (12, np.int32)}

    def export(self, name):
        """one array of the device handle as numpy (0-based indices)"""
        which, dt = self._ARRAYS[name]
        n = C.c_int64()
        _capi.call("athena_mp_graph_export", self.handle, which, None, 0, C.byref(n))
        out = np.empty(n.value, dt)
        _capi.call("athena_mp_graph_export", self.handle, which, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
        return out

    _PLAN_ARRAYS = {"bucket_perm": (0, np.int32), "btile_start": (1, np.int32), "btile_info": (2, np.int32),
                    "btile_rows": (3, np.int32), "btile_off_dev": (4, np.int32), "bucket_off": (5, np.int64),
                    "btile_off": (6, np.int32)}

    def plan_duvenaud(self, min_deg, max_deg):
        """Build the Duvenaud degree-bucket plan of (min_deg, max_deg) now, on torch's current stream (athena_mp_duvenaud_plan; the
        definition is in include/athena_mp.h): the first layer call on this handle then finds it.  A no-op when the handle already
        holds that plan.  Returns self."""
        _capi.use_torch_stream()
        _capi.call("athena_mp_duvenaud_plan", self.handle, int(min_deg), int(max_deg))
        return self

    def export_duvenaud_plan(self):
        """the seven arrays of the handle's degree-bucket plan as numpy (athena_mp_duvenaud_plan_export): bucket_perm, btile_start,
        btile_info, btile_rows [4, 16 nt], btile_off_dev, and the host tables bucket_off (int64) and btile_off"""
        _capi.use_torch_stream()
        out = {}
        for name, (which, dt) in self._PLAN_ARRAYS.items():
            n = C.c_int64()
            _capi.call("athena_mp_duvenaud_plan_export", self.handle, which, None, 0, C.byref(n))
            a = np.empty(n.value, dt)
            _capi.call("athena_mp_duvenaud_plan_export", self.handle, which, a.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
            out[name] = a
        out["btile_rows"] = out["btile_rows"].reshape(4, -1)
        return out

    @classmethod
    def from_edges(cls, num_vertices, index_list, add_self_loops=False, with_edge_ids=True, want_adjacency=False, device=0):
        """edge list -> device handle in one call (athena_mp_graph_create_from_edges): generate_adjacency
        [+ add_self_loops] and set_graph with the CSR entries staying in HBM in between.  Returns the handle, or
        (handle, adj_ia, adj_ja) with want_adjacency (adj_ia is produced either way)."""
        _capi.init(device)
        idx = np.asfortranarray(np.asarray(index_list, dtype=np.int32))
        if not (idx.ndim == 2 and idx.shape[0] == 2):
            raise ValueError('expected: idx.ndim == 2 and idx.shape[0] == 2')
        n, E = int(num_vertices), idx.shape[1]
        self = cls.__new__(cls)
        ia = np.empty(n + 1, np.int32)
        nnz = C.c_int64()
        h = C.c_void_p()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        ja = None
        if want_adjacency:
            cap = 2 * E + n
            ja = np.empty((2, cap), np.int32, order="F")
        _capi.call("athena_mp_graph_create_from_edges", n, E, vp(idx), int(bool(add_self_loops)), int(bool(with_edge_ids)),
                   vp(ia), vp(ja) if ja is not None else None, ja.shape[1] if ja is not None else 0, C.byref(nnz), C.byref(h))
        self.handle = h
        self.n_rows = self.n_cols = n
        self.nnz = int(nnz.value)
        self.n_edge_cols = E if with_edge_ids else 0
        if want_adjacency:
            return self, ia, np.asfortranarray(ja[:, :self.nnz])
        return self

    @classmethod
    def from_points(cls, points, radius, add_self_loops=False, want_adjacency=False, device=0):
        """points -> radius graph -> device handle without the pair list leaving HBM (athena_mp_radius_pairs, then
        athena_mp_graph_create_from_edges_dev).  points [n, dim] float32, dim 1..3: a numpy array, or a torch tensor that is
        already on the device (then only adj_ia crosses PCIe, unless the adjacency is asked for).  Returns
        (handle, coords) or (handle, coords, adj_ia, adj_ja); coords is a device tensor [num_edges, dim] = p_i - p_j, i < j,
        rows in lexicographic order of (i, j): graph_nop_layer_type's edge input for this handle."""
        import torch

        _capi.init(device)
        dev = torch.device("cuda", device)
        if isinstance(points, torch.Tensor):
            pts = points.to(dev, torch.float32).contiguous()
        else:
            pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev)
        if pts.dim() != 2:
            raise ValueError("points must be [n, dim]")
        n, dim = int(pts.shape[0]), int(pts.shape[1])
        _capi.use_torch_stream()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        E = C.c_int64()
        _capi.call("athena_mp_radius_pairs", n, dim, ptr(pts), float(radius), None, None, 0, C.byref(E))
        pairs = torch.empty((E.value, 2), dtype=torch.int32, device=dev)       # the memory of a column-major [2, E]
        coords = torch.empty((E.value, dim), dtype=torch.float32, device=dev)
        _capi.call("athena_mp_radius_pairs", n, dim, ptr(pts), float(radius), ptr(pairs), ptr(coords), E.value, C.byref(E))
        self = cls.__new__(cls)
        ia = np.empty(n + 1, np.int32)
        nnz = C.c_int64()
        h = C.c_void_p()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        ja = np.empty((2, 2 * E.value + n), np.int32, order="F") if want_adjacency else None
        _capi.call("athena_mp_graph_create_from_edges_dev", n, E.value, ptr(pairs), int(bool(add_self_loops)), 1, vp(ia),
                   vp(ja) if ja is not None else None, ja.shape[1] if ja is not None else 0, C.byref(nnz), C.byref(h))
        self.handle = h
        self.n_rows = self.n_cols = n
        self.nnz = int(nnz.value)
        self.n_edge_cols = int(E.value)
        if want_adjacency:
            return self, coords, ia, np.asfortranarray(ja[:, :self.nnz])
        return self, coords

    @classmethod
    def from_point_clouds(cls, points, offsets, radius, add_self_loops=False, want_adjacency=False, device=0):
        """A batch of point clouds -> one block-diagonal device handle without the pair list leaving HBM
        (athena_mp_radius_pairs_batched, then athena_mp_graph_create_from_edges_dev): what from_points makes of every cloud, edge
        ids running over the batch.  points [n, dim] float32, dim 1..3: a numpy array, or a torch tensor already on the device
        (then only offsets, the clouds' bounding boxes, edge_offsets and adj_ia cross PCIe, unless the adjacency is asked for);
        offsets [B + 1] 0-based on the host, cloud b = rows offsets[b] .. offsets[b+1]-1, empty clouds allowed; one radius for all.
        The definition of the pairs (fp32, term by term) is in include/athena_mp.h.  Returns (handle, coords, vertex_offsets,
        edge_offsets) or, with want_adjacency, (..., adj_ia, adj_ja): coords is a device tensor [num_edges, dim] = p_i - p_j,
        i < j, rows in edge-id order; vertex_offsets (int32) and edge_offsets (int64) are numpy [B + 1] -- what
        DeviceDataset(handle, vertex_offsets, edge_offsets) and graph_nop_layer_type.set_graph_handle(handle, vertex_offsets)
        cut the batch by."""
        import torch

        _capi.init(device)
        dev = torch.device("cuda", device)
        if isinstance(points, torch.Tensor):
            pts = points.to(dev, torch.float32).contiguous()
        else:
            pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        if pts.dim() != 2 or off.ndim != 1 or off.size < 1:
            raise ValueError("points must be [n, dim] and offsets [B + 1]")
        n, dim, B = int(pts.shape[0]), int(pts.shape[1]), int(off.size - 1)
        _capi.use_torch_stream()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        E = C.c_int64()
        eoff = np.empty(B + 1, np.int64)
        head = (B, n, vp(off), dim, ptr(pts), float(radius))
        _capi.call("athena_mp_radius_pairs_batched", *head, None, None, 0, vp(eoff), C.byref(E))
        pairs = torch.empty((E.value, 2), dtype=torch.int32, device=dev)       # the memory of a column-major [2, E]
        coords = torch.empty((E.value, dim), dtype=torch.float32, device=dev)
        _capi.call("athena_mp_radius_pairs_batched", *head, ptr(pairs), ptr(coords), E.value, vp(eoff), C.byref(E))
        self = cls.__new__(cls)
        ia = np.empty(n + 1, np.int32)
        nnz = C.c_int64()
        h = C.c_void_p()
        ja = np.empty((2, 2 * E.value + n), np.int32, order="F") if want_adjacency else None
        _capi.call("athena_mp_graph_create_from_edges_dev", n, E.value, ptr(pairs), int(bool(add_self_loops)), 1, vp(ia),
                   vp(ja) if ja is not None else None, ja.shape[1] if ja is not None else 0, C.byref(nnz), C.byref(h))
        self.handle = h
        self.n_rows = self.n_cols = n
        self.nnz = int(nnz.value)
        self.n_edge_cols = int(E.value)
        if want_adjacency:
            return self, coords, off.copy(), eoff, ia, np.asfortranarray(ja[:, :self.nnz])
        return self, coords, off.copy(), eoff

    @classmethod
    def from_point_sets(cls, queries, sources, radius, query_offsets=None, source_offsets=None, want_adjacency=False, device=0):
        """Two point sets -> the directed, rectangular device handle that joins every query to the sources of its cloud inside
        the radius, without the pair list leaving HBM (athena_mp_radius_pairs_bipartite, then
        athena_mp_graph_create_bipartite_dev): the graph graph_nop_layer_type(local_term=False) integrates over when its output
        points are not its input points.  queries [n_queries, dim] and sources [n_sources, dim] float32, dim 1..3: numpy arrays,
        or torch tensors already on the device; query_offsets / source_offsets [B + 1] 0-based on the host (both or neither:
        without them the sets are one cloud), empty slices allowed; one radius for all.  The definition of the pairs (fp32, term
        by term; no self-pair rule) is in include/athena_mp.h.  Returns (handle, coords, edge_offsets) or, with want_adjacency,
        (..., adj_ia, adj_ja): handle.n_rows = n_queries, handle.n_cols = n_sources, one CSR entry and one edge column per pair;
        coords is a device tensor [num_edges, dim] = q_i - p_j, rows in lexicographic order of (i, j); edge_offsets (int64) is
        numpy [B + 1]."""
        import torch

        dev, q, s, qoff, soff = _two_sets_on_device(queries, sources, query_offsets, source_offsets, device)
        nq, ns, dim, B = int(q.shape[0]), int(s.shape[0]), int(q.shape[1]), int(qoff.size - 1)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        E = C.c_int64()
        eoff = np.empty(B + 1, np.int64)
        head = (B, nq, vp(qoff), ns, vp(soff), dim, ptr(q), ptr(s), float(radius))
        _capi.call("athena_mp_radius_pairs_bipartite", *head, None, None, 0, None, vp(eoff), C.byref(E))
        pairs = torch.empty((E.value, 2), dtype=torch.int32, device=dev)       # the memory of a column-major [2, E]
        coords = torch.empty((E.value, dim), dtype=torch.float32, device=dev)
        _capi.call("athena_mp_radius_pairs_bipartite", *head, ptr(pairs), ptr(coords), E.value, None, vp(eoff), C.byref(E))
        self = cls.__new__(cls)
        ia = np.empty(nq + 1, np.int32)
        h = C.c_void_p()
        ja = np.empty((2, E.value), np.int32, order="F") if want_adjacency else None
        _capi.call("athena_mp_graph_create_bipartite_dev", nq, ns, E.value, ptr(pairs), vp(ia), vp(ja) if ja is not None else None,
                   E.value if ja is not None else 0, C.byref(h))
        self.handle = h
        self.n_rows, self.n_cols = nq, ns
        self.nnz = int(E.value)
        self.n_edge_cols = int(E.value)
        if want_adjacency:
            return self, coords, eoff, ia, ja
        return self, coords, eoff

    @classmethod
    def from_point_sets_knn(cls, queries, sources, k, radius=None, query_offsets=None, source_offsets=None, want_adjacency=False,
                            want_neighbours=False, device=0):
        """Two point sets -> the directed, rectangular device handle that joins every query to the first k sources of its cloud
        in the order (fp32 squared distance, source index) -- inside radius when one is given --, without the pair list leaving
        HBM (athena_mp_knn_pairs_bipartite, then athena_mp_graph_create_bipartite_dev): from_point_sets for queries that may lie
        where the sources are sparse or dense, or outside them altogether.  Arguments as in from_point_sets; 1 <= k <= 64; the
        definition is in include/athena_mp.h.  One search into buffers of n_queries * k pairs, narrowed afterwards.  Returns
        what from_point_sets returns -- (handle, coords, edge_offsets) or, with want_adjacency, (..., adj_ia, adj_ja) -- and,
        with want_neighbours, nbr and sqdist last: device tensors [n_queries, k], row i = the chosen sources of query i as
        1-based global ids in key order padded with 0 (int32), and their squared distances padded with +inf (float32).  Without
        a cap a query far outside its sources walks their whole grid: give a radius where queries may lie far away."""
        import torch

        dev, q, s, qoff, soff = _two_sets_on_device(queries, sources, query_offsets, source_offsets, device)
        nq, ns, dim, B = int(q.shape[0]), int(s.shape[0]), int(q.shape[1]), int(qoff.size - 1)
        k = int(k)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        E = C.c_int64()
        eoff = np.empty(B + 1, np.int64)
        kk = max(min(k, 64), 1)                  # a k outside 1..64 is the library's to refuse
        cap = nq * kk
        pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)           # the memory of a column-major [2, cap]
        coords = torch.empty((cap, dim), dtype=torch.float32, device=dev)
        nbr = torch.empty((nq, kk), dtype=torch.int32, device=dev) if want_neighbours else None
        sqdist = torch.empty((nq, kk), dtype=torch.float32, device=dev) if want_neighbours else None
        _capi.call("athena_mp_knn_pairs_bipartite", B, nq, vp(qoff), ns, vp(soff), dim, ptr(q), ptr(s), k, _knn_radius(radius), ptr(nbr),
                   ptr(sqdist), ptr(pairs), ptr(coords), cap, None, vp(eoff), C.byref(E))
        pairs, coords = pairs[:E.value].clone(), coords[:E.value].clone()      # narrowed: the n_queries * k buffers go back
        self = cls.__new__(cls)
        ia = np.empty(nq + 1, np.int32)
        h = C.c_void_p()
        ja = np.empty((2, E.value), np.int32, order="F") if want_adjacency else None
        _capi.call("athena_mp_graph_create_bipartite_dev", nq, ns, E.value, ptr(pairs), vp(ia), vp(ja) if ja is not None else None,
                   E.value if ja is not None else 0, C.byref(h))
        self.handle = h
        self.n_rows, self.n_cols = nq, ns
        self.nnz = int(E.value)
        self.n_edge_cols = int(E.value)
        out = (self, coords, eoff)
        if want_adjacency:
            out += (ia, ja)
        if want_neighbours:
            out += (nbr, sqdist)
        return out

    @classmethod
    def from_grid_clusters(cls, points, size, offsets=None, origin=None, want_nearest=False, want_cells=False, device=0):
        """A batch of point clouds -> its voxel-grid clusters and the directed, rectangular device handle of their membership,
        without the list leaving HBM (athena_mp_grid_clusters, then athena_mp_graph_create_bipartite_dev): every non-empty cubic
        cell of edge `size` of a cloud is one row, its points the row's columns in index order; the definition is in
        include/athena_mp.h.  points [n, dim] float32, dim 1..3: a numpy array, or a torch tensor already on the device; offsets
        [B + 1] 0-based on the host (None: one cloud), empty clouds allowed; origin [dim]: the grid's corner for every cloud
        (None: each cloud's own lower corner).  One call into buffers of n clusters, narrowed afterwards.  Returns (handle,
        centroid, cluster_offsets, cluster, weights) and, when asked for, nearest and cells last: handle.n_rows = m clusters,
        n_cols = n, edge e = pair e; centroid [m, dim] float32, cluster [n] int32 (1-based) and weights [n] float32 (1 / the
        members of the pair's cluster) on the device; cluster_offsets numpy int32 [B + 1], what the query_offsets= /
        source_offsets= arguments of from_point_sets / from_point_sets_knn take for the centroids; nearest [m] int32, the member
        nearest each centroid as a 1-based global point id; cells [m, dim] int32.  pool_max(handle, x=x) is max pooling over the
        clusters, interpolate(handle, weights, x) mean pooling.  The handle keeps rowptr [m + 1] int32 on the device as
        handle.cluster_rowptr: geometry.grid_clusters_grad takes the handle."""
        import torch

        _capi.init(device)
        dev = torch.device("cuda", device)
        if isinstance(points, torch.Tensor):
            pts = points.to(dev, torch.float32).contiguous()
        else:
            pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev)
        if pts.dim() != 2:
            raise ValueError("points must be [n, dim]")
        n, dim = int(pts.shape[0]), int(pts.shape[1])
        off = np.array([0, n], np.int32) if offsets is None else np.ascontiguousarray(offsets, dtype=np.int32)
        if off.ndim != 1 or off.size < 1:
            raise ValueError("offsets must be [B + 1]")
        B = int(off.size - 1)
        org = None
        if origin is not None:
            org = np.ascontiguousarray(origin, dtype=np.float32)
            if org.shape != (dim,):
                raise ValueError("origin must hold one coordinate per axis")
        _capi.use_torch_stream()
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        cluster = torch.empty((n,), dtype=torch.int32, device=dev)
        pairs = torch.empty((n, 2), dtype=torch.int32, device=dev)             # the memory of a column-major [2, n]
        rowptr = torch.empty((n + 1,), dtype=torch.int32, device=dev)
        weights = torch.empty((n,), dtype=torch.float32, device=dev)
        centroid = torch.empty((n, max(dim, 1)), dtype=torch.float32, device=dev)
        nearest = torch.empty((n,), dtype=torch.int32, device=dev) if want_nearest else None
        cells = torch.empty((n, max(dim, 1)), dtype=torch.int32, device=dev) if want_cells else None
        coff = np.empty(B + 1, np.int32)
        m = C.c_int64()
        _capi.call("athena_mp_grid_clusters", B, n, vp(off), dim, ptr(pts), float(size), vp(org), n, ptr(cluster), ptr(pairs), ptr(rowptr),
                   ptr(weights), ptr(centroid), ptr(nearest), ptr(cells), vp(coff), None, C.byref(m))
        m = int(m.value)
        centroid = centroid[:m, :dim].clone()                                  # narrowed: the buffers of n clusters go back
        self = cls.__new__(cls)
        ia = np.empty(m + 1, np.int32)
        h = C.c_void_p()
        _capi.call("athena_mp_graph_create_bipartite_dev", m, n, n, ptr(pairs), vp(ia), None, 0, C.byref(h))
        self.handle = h
        self.n_rows, self.n_cols = m, n
        self.nnz = n
        self.n_edge_cols = n
        self.cluster_rowptr = rowptr[:m + 1].clone()
        out = (self, centroid, coff, cluster, weights)
        if want_nearest:
            out += (nearest[:m].clone(),)
        if want_cells:
            out += (cells[:m, :dim].clone(),)
        return out

    def pair_list(self):
        """The handle's pair list written on the device (athena_mp_graph_pairs): an int32 tensor [n_edge_cols, 2], the memory of a
        column-major [2, n_edge_cols], 1-based; edge column e holds (row, column) of the first CSR entry that carries it -- (min,
        max) of input pair e on a from_edges handle, the pair itself on a rectangular one -- and (0, 0) where no entry does."""
        import torch

        _capi.use_torch_stream()
        E = int(self.n_edge_cols)
        pairs = torch.empty((E, 2), dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
        _capi.call("athena_mp_graph_pairs", self.handle, C.c_void_p(pairs.data_ptr()), E)
        return pairs

    @classmethod
    def from_contraction(cls, graph, cluster, n_clusters, col_cluster=None, n_col_clusters=None, points=None, col_points=None,
                         add_self_loops=False, want_pool=True, n_vertices=None, n_col_vertices=None, device=0):
        """A graph contracted over a cluster map -> the coarse device handle that keeps the fine graph's adjacency, and the handle
        that pools per-edge features, without a list leaving HBM (athena_mp_graph_pairs, athena_mp_contract_pairs, then
        athena_mp_graph_create_from_edges_dev or athena_mp_graph_create_bipartite_dev): every fine pair is relabelled through the
        map, the distinct results are the coarse pairs in lexicographic order, their fine edges the members in edge-id order; the
        definition is in include/athena_mp.h.  graph: a DeviceGraph with edge columns, or a device int32 tensor [E, 2] (the memory
        of a column-major [2, E], 1-based, 0 = no such edge) together with n_vertices= (and n_col_vertices= for a two-set list).
        cluster [n_rows] int32 on the device or numpy, values 0 .. n_clusters, 0 drops the vertex: what from_grid_clusters
        returns, as it is, and what geometry.topk_vertices returns for a selection by scores -- score -> topk_vertices ->
        from_contraction(handle, cluster, m) is the induced subgraph of the kept vertices, geometry.select_rows(selected, x, gate)
        their gated features and geometry.unpool(cluster, y) the way back up; None: the identity (n_clusters must be n_rows),
        which merges duplicate pairs.  The mode follows the
        graph: square and no col_cluster is undirected (self pairs of clusters go, pairs are (min, max)); n_cols != n_rows or a
        col_cluster given (with n_col_clusters) is directed, two sets.  points [n_clusters, dim] (and col_points
        [n_col_clusters, dim] in the directed mode) float32, dim 1..3: the coarse positions, e.g. the centroids.  One size query
        and one call.  Returns (coarse_handle, coarse_pairs, pool_handle, weights, edge_pair) and, with points, coords last:
        coarse_pairs int32 [P, 2] on the device; pool_handle (None without want_pool) has n_rows = P coarse pairs, n_cols = E fine
        edges, one entry per member: pool_max(pool_handle, x=h) is max pooling of fine edge features h [E, F],
        interpolate(pool_handle, weights, h) mean pooling; weights float32 [M]; edge_pair int32 [E], the coarse pair of each fine
        edge, 0 where it takes no part (unpooling is h_coarse[edge_pair - 1]); coords float32 [P, dim] = points[a] - points[b],
        the coarse handle's GNO edge input."""
        import torch

        if isinstance(graph, DeviceGraph):
            if n_vertices is not None or n_col_vertices is not None:
                raise ValueError("n_vertices belongs to a pair list; a DeviceGraph knows its own")
            if graph.n_edge_cols <= 0:
                raise ValueError("the handle has no edge columns: there is no pair list to contract")
            n_rows, n_cols = int(graph.n_rows), int(graph.n_cols)
            pairs = None
        else:
            if not (isinstance(graph, torch.Tensor) and graph.dtype == torch.int32 and graph.dim() == 2 and graph.shape[1] == 2):
                raise ValueError("graph must be a DeviceGraph or a device int32 tensor [E, 2]")
            if n_vertices is None:
                raise ValueError("a pair list needs n_vertices")
            n_rows = int(n_vertices)
            n_cols = n_rows if n_col_vertices is None else int(n_col_vertices)
            pairs = graph
        mode = 1 if (n_cols != n_rows or col_cluster is not None) else 0
        if mode == 1 and cluster is not None and col_cluster is None:
            raise ValueError("a two-set graph needs col_cluster beside cluster")
        if mode == 1 and points is not None and col_points is None:
            raise ValueError("a two-set graph needs col_points beside points")
        if mode == 0 and (col_points is not None or n_col_clusters is not None):
            raise ValueError("col_points and n_col_clusters belong to the two-set mode: give col_cluster")
        m_rows = int(n_clusters)
        m_cols = m_rows if mode == 0 else int(n_col_clusters if n_col_clusters is not None else (n_cols if col_cluster is None else -1))
        if m_cols < 0:
            raise ValueError("col_cluster needs n_col_clusters")
        for a, what, rows in ((cluster, "cluster", n_rows), (col_cluster, "col_cluster", n_cols), (points, "points", m_rows),
                              (col_points, "col_points", m_cols)):
            if a is not None and int(a.shape[0]) != rows:
                raise ValueError(f"{what} must have {rows} rows, not {int(a.shape[0])}")
        _capi.init(device)
        dev = torch.device("cuda", device)
        if pairs is not None:
            pairs = pairs.to(dev).contiguous()

        def on_device(a, dt, what, rows):
            if a is None:
                return None
            if isinstance(a, torch.Tensor):
                return a.to(dev, dt).contiguous()
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32 if dt == torch.int32 else np.float32)).to(dev)

        rc = on_device(cluster, torch.int32, "cluster", n_rows)
        cc = rc if mode == 0 else on_device(col_cluster, torch.int32, "col_cluster", n_cols)
        rp = on_device(points, torch.float32, "points", m_rows)
        cp = rp if mode == 0 else on_device(col_points, torch.float32, "col_points", m_cols)
        dim = 0
        if rp is not None:
            if rp.dim() != 2 or cp.dim() != 2 or rp.shape[1] != cp.shape[1]:
                raise ValueError("points must be [n_clusters, dim], the same dim on both sides")
            dim = int(rp.shape[1])
        _capi.use_torch_stream()
        if pairs is None:
            pairs = graph.pair_list()
        E = int(pairs.shape[0])
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        P, M = C.c_int64(), C.c_int64()
        head = (E, ptr(pairs), n_rows, n_cols, ptr(rc), ptr(cc), m_rows, m_cols, mode, dim, ptr(rp), ptr(cp))
        _capi.call("athena_mp_contract_pairs", *head, 0, 0, None, None, None, None, None, None, C.byref(P), C.byref(M))
        P, M = int(P.value), int(M.value)
        coarse_pairs = torch.empty((P, 2), dtype=torch.int32, device=dev)      # the memory of a column-major [2, P]
        members = torch.empty((M, 2), dtype=torch.int32, device=dev) if want_pool else None
        weights = torch.empty((M,), dtype=torch.float32, device=dev)
        edge_pair = torch.empty((E,), dtype=torch.int32, device=dev)
        coords = torch.empty((P, dim), dtype=torch.float32, device=dev) if rp is not None else None
        P2, M2 = C.c_int64(), C.c_int64()
        _capi.call("athena_mp_contract_pairs", *head, P, M, ptr(coarse_pairs), None, ptr(members), ptr(weights), ptr(edge_pair), ptr(coords),
                   C.byref(P2), C.byref(M2))
        self = cls.__new__(cls)
        h = C.c_void_p()
        ia = np.empty(m_rows + 1, np.int32)
        if mode == 0:
            nnz = C.c_int64()
            _capi.call("athena_mp_graph_create_from_edges_dev", m_rows, P, ptr(coarse_pairs), int(bool(add_self_loops)), 1, vp(ia), None, 0,
                       C.byref(nnz), C.byref(h))
            self.nnz = int(nnz.value)
        else:
            _capi.call("athena_mp_graph_create_bipartite_dev", m_rows, m_cols, P, ptr(coarse_pairs), vp(ia), None, 0, C.byref(h))
            self.nnz = P
        self.handle = h
        self.n_rows, self.n_cols = m_rows, m_cols
        self.n_edge_cols = P
        pool = None
        if want_pool:
            pool = cls.__new__(cls)
            hp = C.c_void_p()
            pia = np.empty(P + 1, np.int32)
            _capi.call("athena_mp_graph_create_bipartite_dev", P, E, M, ptr(members), vp(pia), None, 0, C.byref(hp))
            pool.handle = hp
            pool.n_rows, pool.n_cols = P, E
            pool.nnz = M
            pool.n_edge_cols = M
        out = (self, coarse_pairs, pool, weights, edge_pair)
        if coords is not None:
            out += (coords,)
        return out

    _CELLS = {1: (2, 1), 2: (3, 3), 3: (4, 4), 4: (4, 6), "segment": 1, "triangle": 2, "quadrilateral": 3, "tetrahedron": 4}

    @classmethod
    def from_mesh(cls, cells, n_vertices, cell_type, points=None, add_self_loops=False, want_pool=True, device=0):
        """Mesh elements -> the device handle of the mesh's edge graph, without a list leaving HBM (athena_mp_cell_pairs, then
        from_contraction with the identity map): a graph neural operator dataset that arrives as elements.  cells [n_cells, nv]
        int32, 1-based: a numpy array, or a torch tensor already on the device; cell_type 1 / "segment" (nv = 2), 2 / "triangle"
        (3), 3 / "quadrilateral" (4, its ring) or 4 / "tetrahedron" (4, all six pairs); points [n_vertices, dim] float32, dim
        1..3.  Returns what from_contraction returns -- (handle, edges, pool_handle, weights, edge_pair) and, with points, coords
        last --: edges int32 [P, 2] are the mesh's distinct edges (a < b) in lexicographic order; pool_handle maps the n_cells * ne
        element-edge slots (slot c * ne + l = local pair l of cell c) onto them, so 1 / weights counts the elements on an edge (1
        on the boundary of a triangle mesh); edge_pair [n_cells * ne] is the edge of each slot, 0 for the pair of a repeated
        vertex; coords [P, dim] = points[a] - points[b]."""
        import torch

        ct = cls._CELLS.get(cell_type, cell_type) if isinstance(cell_type, str) else cell_type
        if ct not in (1, 2, 3, 4):
            raise ValueError("cell_type must be 1..4 or one of segment, triangle, quadrilateral, tetrahedron")
        nv, ne = cls._CELLS[ct]
        if len(cells.shape) != 2 or cells.shape[1] != nv:
            raise ValueError(f"cells must be [n_cells, {nv}] for cell_type {ct}")
        if points is not None and int(points.shape[0]) != int(n_vertices):
            raise ValueError(f"points must have {int(n_vertices)} rows, not {int(points.shape[0])}")
        _capi.init(device)
        dev = torch.device("cuda", device)
        if isinstance(cells, torch.Tensor):
            cd = cells.to(dev, torch.int32).contiguous()
        else:
            cd = torch.from_numpy(np.ascontiguousarray(cells, dtype=np.int32)).to(dev)
        n_cells = int(cd.shape[0])
        _capi.use_torch_stream()
        pairs = torch.empty((n_cells * ne, 2), dtype=torch.int32, device=dev)  # the memory of a column-major [2, n_cells * ne]
        count = C.c_int64()
        _capi.call("athena_mp_cell_pairs", int(n_vertices), n_cells, ct, C.c_void_p(cd.data_ptr()), C.c_void_p(pairs.data_ptr()),
                   n_cells * ne, C.byref(count))
        return cls.from_contraction(pairs, None, int(n_vertices), points=points, add_self_loops=add_self_loops, want_pool=want_pool,
                                    n_vertices=int(n_vertices), device=device)

    @classmethod
    def from_point_clouds_knn(cls, points, offsets, k, radius=None, mode="union", add_self_loops=False, want_adjacency=False,
                              want_neighbours=False, device=0):
        """A batch of point clouds -> one block-diagonal k-nearest-neighbour device handle without the pair list leaving HBM
        (athena_mp_knn_pairs_batched, then athena_mp_graph_create_from_edges_dev).  Every point is joined to the first k others
        of its cloud in the order (fp32 squared distance, index) -- inside radius when one is given --; mode "union" keeps a pair
        either end chose, "mutual" one both chose (the definition is in include/athena_mp.h).  points and offsets as in
        from_point_clouds.  One search into buffers of n * k pairs, narrowed afterwards.  Returns what from_point_clouds returns
        -- (handle, coords, vertex_offsets, edge_offsets) or, with want_adjacency, (..., adj_ia, adj_ja) -- and, with
        want_neighbours, nbr last: a device tensor [n, k] int32, row i = the chosen neighbours of i as 1-based global ids in key
        order, padded with 0."""
        import torch

        _capi.init(device)
        dev = torch.device("cuda", device)
        if isinstance(points, torch.Tensor):
            pts = points.to(dev, torch.float32).contiguous()
        else:
            pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        if pts.dim() != 2 or off.ndim != 1 or off.size < 1:
            raise ValueError("points must be [n, dim] and offsets [B + 1]")
        n, dim, B, k = int(pts.shape[0]), int(pts.shape[1]), int(off.size - 1), int(k)
        _capi.use_torch_stream()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        E = C.c_int64()
        eoff = np.empty(B + 1, np.int64)
        cap = n * max(min(k, 64), 1)             # a k outside 1..64 is the library's to refuse
        pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)           # the memory of a column-major [2, cap]
        coords = torch.empty((cap, dim), dtype=torch.float32, device=dev)
        nbr = torch.empty((n, max(min(k, 64), 1)), dtype=torch.int32, device=dev) if want_neighbours else None
        _capi.call("athena_mp_knn_pairs_batched", B, n, vp(off), dim, ptr(pts), k, _knn_radius(radius), _knn_mode(mode),
                   ptr(nbr) if nbr is not None else None, ptr(pairs), ptr(coords), cap, vp(eoff), C.byref(E))
        pairs, coords = pairs[:E.value].clone(), coords[:E.value].clone()      # narrowed: the n * k buffers go back
        self = cls.__new__(cls)
        ia = np.empty(n + 1, np.int32)
        nnz = C.c_int64()
        h = C.c_void_p()
        ja = np.empty((2, 2 * E.value + n), np.int32, order="F") if want_adjacency else None
        _capi.call("athena_mp_graph_create_from_edges_dev", n, E.value, ptr(pairs), int(bool(add_self_loops)), 1, vp(ia),
                   vp(ja) if ja is not None else None, ja.shape[1] if ja is not None else 0, C.byref(nnz), C.byref(h))
        self.handle = h
        self.n_rows = self.n_cols = n
        self.nnz = int(nnz.value)
        self.n_edge_cols = int(E.value)
        out = (self, coords, off.copy(), eoff)
        if want_adjacency:
            out += (ia, np.asfortranarray(ja[:, :self.nnz]))
        if want_neighbours:
            out += (nbr,)
        return out

    @classmethod
    def from_points_knn(cls, points, k, radius=None, mode="union", add_self_loops=False, want_adjacency=False,
                        want_neighbours=False, device=0):
        """from_point_clouds_knn for one cloud.  Returns what from_points returns -- (handle, coords) or (handle, coords, adj_ia,
        adj_ja) -- with nbr added last when want_neighbours."""
        n = int(points.shape[0])
        out = cls.from_point_clouds_knn(points, [0, n], k, radius, mode, add_self_loops, want_adjacency, want_neighbours, device)
        return out[:2] + out[4:]

    @classmethod
    def from_structures(cls, frac, lat, offsets, cutoff_min, cutoff_max, pbc=(1, 1, 1), add_self_loops=False, want_adjacency=False,
                        device=0):
        """A batch of periodic structures -> one block-diagonal device handle without the pair list leaving HBM
        (athena_mp_periodic_pairs, then athena_mp_graph_create_from_edges_dev): what the reference's get_graph_from_basis +
        generate_adjacency (+ add_self_loops) make of every structure, on the host, one at a time.  frac [n, 3] fractional
        coordinates and lat [B, 3, 3] (row a = lattice vector a): float32 numpy arrays, or torch tensors already on the device;
        offsets [B + 1] 0-based on the host; pbc: an axis with 0 is neither wrapped nor imaged.  The definition of the edges
        (fp32, term by term) is in include/athena_mp.h.  Returns (handle, feature, vec, vertex_offsets, edge_offsets) or, with
        want_adjacency, (..., adj_ia, adj_ja): feature [E] = r / cutoff_max and vec [E, 3] = atom i minus the image of atom j
        are device tensors, rows in edge-id order; vertex_offsets (int32) and edge_offsets (int64) are numpy [B + 1] -- what
        msgpass_layer_type.set_graph_handle(handle, vertex_offsets) cuts the batch by."""
        import torch

        _capi.init(device)
        dev = torch.device("cuda", device)
        frac, lat, off, pbc3 = _structure_arrays(frac, lat, offsets, pbc)
        on_dev = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(a)).to(dev, torch.float32).contiguous()
        frac, lat = on_dev(frac), on_dev(lat)
        n, B = int(frac.shape[0]), int(lat.shape[0])
        _capi.use_torch_stream()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        E = C.c_int64()
        head = (B, n, vp(off), ptr(frac), ptr(lat), vp(pbc3), float(cutoff_min), float(cutoff_max))
        _capi.call("athena_mp_periodic_pairs", *head, None, None, None, None, None, 0, C.byref(E), None)
        pairs = torch.empty((E.value, 2), dtype=torch.int32, device=dev)       # the memory of a column-major [2, E]
        feature = torch.empty(E.value, dtype=torch.float32, device=dev)
        vec = torch.empty((E.value, 3), dtype=torch.float32, device=dev)
        eoff = np.empty(B + 1, np.int64)
        _capi.call("athena_mp_periodic_pairs", *head, ptr(pairs), ptr(feature), ptr(vec), None, None, E.value, C.byref(E), vp(eoff))
        self = cls.__new__(cls)
        ia = np.empty(n + 1, np.int32)
        nnz = C.c_int64()
        h = C.c_void_p()
        ja = np.empty((2, 2 * E.value + n), np.int32, order="F") if want_adjacency else None
        _capi.call("athena_mp_graph_create_from_edges_dev", n, E.value, ptr(pairs), int(bool(add_self_loops)), 1, vp(ia),
                   vp(ja) if ja is not None else None, ja.shape[1] if ja is not None else 0, C.byref(nnz), C.byref(h))
        self.handle = h
        self.n_rows = self.n_cols = n
        self.nnz = int(nnz.value)
        self.n_edge_cols = int(E.value)
        if want_adjacency:
            return self, feature, vec, off.copy(), eoff, ia, np.asfortranarray(ja[:, :self.nnz])
        return self, feature, vec, off.copy(), eoff

    @classmethod
    def from_triplets(cls, handle, vec=None, cutoff=None, device=0):
        """A square handle with edge columns -> the handle over its bond-angle triplets, without the pair list leaving HBM
        (athena_mp_triplet_pairs, then athena_mp_graph_create_bipartite_dev): every ordered pair (k, k') of distinct CSR entries of
        one vertex row is a triplet, numbered in lexicographic order; the definition is in include/athena_mp.h.  handle: from
        from_structures, from_points, from_point_clouds[_knn] or from_edges (with edge ids); vec [E, dim] float32 as its builder
        returned it, a numpy array or a torch tensor already on the device; cutoff: the shorter three-body cutoff -- only entries
        with |vec| < cutoff take part (None: every entry with an edge id; vec may then be None too).  One size query, then one
        fill.  Returns (thandle, dir), or (thandle, None) without vec: thandle.n_rows = thandle.n_cols = handle.nnz, one CSR entry
        and one edge column per triplet (thandle.n_edge_cols = T), so per-entry messages are its vertex values and per-triplet
        values its edge values; dir [nnz, dim] is geometry.entry_vectors(handle, vec), what geometry.triplet_cos takes."""
        import torch

        _capi.init(device)
        dev = torch.device("cuda", device)
        if vec is not None:
            if isinstance(vec, torch.Tensor):
                vec = vec.to(dev, torch.float32).contiguous()
            else:
                vec = torch.from_numpy(np.ascontiguousarray(vec, dtype=np.float32)).to(dev)
            if vec.dim() != 2 or int(vec.shape[0]) != handle.n_edge_cols:
                raise ValueError(f"vec must be [{handle.n_edge_cols}, dim]")
        elif cutoff is not None:
            raise ValueError("a cutoff needs vec")
        dim = int(vec.shape[1]) if vec is not None else 3
        cutoff3 = float("inf") if cutoff is None else float(cutoff)
        _capi.use_torch_stream()
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        T = C.c_int64()
        _capi.call("athena_mp_triplet_pairs", handle.handle, dim, ptr(vec), cutoff3, None, 0, None, C.byref(T))
        pairs = torch.empty((T.value, 2), dtype=torch.int32, device=dev)       # the memory of a column-major [2, T]
        _capi.call("athena_mp_triplet_pairs", handle.handle, dim, ptr(vec), cutoff3, ptr(pairs), T.value, None, C.byref(T))
        self = cls.__new__(cls)
        nnz = handle.nnz
        ia = np.empty(nnz + 1, np.int32)
        h = C.c_void_p()
        _capi.call("athena_mp_graph_create_bipartite_dev", nnz, nnz, T.value, ptr(pairs), ia.ctypes.data_as(C.c_void_p), None, 0,
                   C.byref(h))
        self.handle = h
        self.n_rows = self.n_cols = nnz
        self.nnz = int(T.value)
        self.n_edge_cols = int(T.value)
        if vec is None:
            return self, None
        from . import geometry

        return self, geometry.entry_vectors(handle, vec)

    @classmethod
    def borrow(cls, handle, owner=None):
        """wrap a handle somebody else owns (the row blocks of an athena_mp_shard): never destroyed from here"""
        self = cls.__new__(cls)
        self.handle, self._borrowed, self._owner = handle, True, owner
        nr, nc, nnz, ne = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        _capi.call("athena_mp_graph_dims", handle, C.byref(nr), C.byref(nc), C.byref(nnz), C.byref(ne))
        self.n_rows, self.n_cols, self.nnz, self.n_edge_cols = nr.value, nc.value, nnz.value, ne.value
        return self

    @classmethod
    def from_graph(cls, g, device=0):
        return cls(g.adj_ia, g.adj_ja, n_edge_cols=max(g.num_edges, int(g.adj_ja[1].max()) if g.nnz else 0),
                   device=device)

    def evict(self):
        """close(), and the library's handle cache forgets this handle (athena_mp_graph_evict): the next acquire of the
        same key builds from the arrays.  What a layer does with its old handle after graph_type.touch()."""
        if getattr(self, "handle", None):
            if not getattr(self, "_borrowed", False):
                _capi.call("athena_mp_graph_evict", self.handle)
            self.handle = None

    def close(self):
        if getattr(self, "handle", None):
            if not getattr(self, "_borrowed", False):
                _capi.load().athena_mp_graph_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
