"""Geometry gradients: a layer's per-edge gradient carried back to the points, the atoms and the cell, on the device
(athena_amd/csrc/geometry_grad.hip; the definition, term by term in fp32, is in include/athena_mp.h).

    handle, coords = DeviceGraph.from_points(points, radius)            # coords[e] = p_i - p_j
    ... graph_nop_layer_type.backward(need_coord_grad=True) -> dcoords [E, d]
    dpoints = points_grad(handle, dcoords)                              # [n, d]

    handle, feature, vec, voff, eoff = DeviceGraph.from_structures(frac, lat, offsets, cutoff_min, cutoff_max)
    ... duvenaud_msgpass_layer_type.backward(need_edge_grad=True) -> de [E, F_e]
    g = structures_grad(handle, lat, voff, eoff, vec, cutoff_max, dfeature=de)
    forces = -g["cart"];  g["frac"], g["virial"], g["lat"]

    handle, coords, eoff = DeviceGraph.from_point_sets(queries, sources, radius)    # coords[e] = q_i - p_j
    ... graph_nop_layer_type(local_term=False).backward(need_coord_grad=True) -> dcoords [E, d]
    g = point_sets_grad(handle, dcoords);  g["queries"] [n_queries, d], g["sources"] [n_sources, d]

There is no autograd wrapper: these are the reverse steps themselves, to be called where the chain needs them.

Also the step that MAKES the second point set of from_point_sets / from_point_sets_knn (athena_amd/csrc/fps.hip):

    sample, coarse, sample_offsets, cover = farthest_points(points, offsets, ratio=0.05)
    handle, coords, eoff = DeviceGraph.from_point_sets(coarse, points, cover_radius(cover), sample_offsets, offsets)

And the way back, coarse to fine (athena_amd/csrc/interp.hip): inverse-distance interpolation of the coarse set's features onto the
fine points, and its reverse steps down to both point sets:

    sample, coarse, sample_offsets, cover = farthest_points(points, offsets, ratio=0.05)
    handle, coords, eoff = DeviceGraph.from_point_sets_knn(points, coarse, k=3, query_offsets=offsets, source_offsets=sample_offsets)
    weights, wsum = interp_weights(handle, coords)                      # [E], [n_points]
    y = interpolate(handle, weights, x_coarse)                          # [n_points, F]
    ... the layers above return dy [n_points, F]
    g = interpolate_grad(handle, coords, weights, x_coarse, y, dy)      # g["x"] [n_coarse, F], g["coords"] [E, d]
    p = point_sets_grad(handle, g["coords"]);  p["queries"], p["sources"]

interpolate and interpolate_grad(want=("x",)) take ANY weights [E]: mean pooling and quadrature-weighted transfer are the same calls.

And the way down, fine to coarse (athena_amd/csrc/pool.hip): the set-abstraction step -- an MLP on every (sample, neighbour) pair, then
the maximum over each sample's neighbourhood, with the arg-max that the reverse step needs:

    sample, coarse, sample_offsets, cover = farthest_points(points, offsets, ratio=0.05)
    handle, coords, eoff = DeviceGraph.from_point_sets_knn(coarse, points, k=16, query_offsets=sample_offsets, source_offsets=offsets)
    m = edge_features(handle, x_sources=x, coords=coords, pad_to=4)     # [E, F_x + d]: the edge MLP's input (edge_gather.hip)
    ... the edge MLP on m returns h [E, F]
    y, arg = pool_max(handle, edges=h)                                  # [n_coarse, F], [n_coarse, F] int32
    ... the layers above return dy [n_coarse, F]
    dh = pool_max_grad(handle, arg, dy, to="edges")                     # [E, F]
    ... the edge MLP's reverse returns dm [E, F_x + d]
    g = edge_features_grad(handle, dm, widths=(F_x, 0, d))              # g["sources"] [n_points, F_x], g["coords"] [E, d]
    p = point_sets_grad(handle, g["coords"]);  p["queries"], p["sources"]

pool_max(handle, x=...) takes per-vertex values instead (on any handle, square ones too) and pool_max_grad(..., to="x") is its
reverse.  edge_features(..., x_queries=..., relative=True) makes EdgeConv's input (x_j - x_i, x_i).

The third reduction over the same neighbourhoods is attention (athena_amd/csrc/attention.hip): a softmax over each row's entries, per
head, and the weighted sum with the weight chosen per head -- edge_features -> MLP -> attention_weights -> attend:

    m = edge_features(handle, x_sources=x, x_queries=x_coarse, coords=coords, relative=True, pad_to=4)
    ... the edge MLPs on m return scores [E, H] and values h [E, F], F a multiple of H (H = F: vector attention)
    alpha = attention_weights(handle, scores)                           # [E, H]: each row's entries add up to 1, per head
    y = attend(handle, alpha, edges=h)                                  # [n_coarse, F]; or attend(handle, alpha, x=x) over vertex values
    ... the layers above return dy [n_coarse, F]
    g = attend_grad(handle, alpha, dy, edges=h)                         # g["values"] [E, F] (dh; dx [n_points, F] with x=), g["scores"] [E, H]

For LARGE clouds the coarse set comes from a voxel grid instead (athena_amd/csrc/grid_clusters.hip): O(n), no dependent steps, one
coarse point -- the centroid -- per non-empty cubic cell, and the membership as the pooling handle:

    handle, centroid, cluster_offsets, cluster, weights = DeviceGraph.from_grid_clusters(points, size, offsets)
    y, arg = pool_max(handle, x=x)                                      # [n_clusters, F]: max pooling; or the mean:
    y = interpolate(handle, weights, x)                                 # weights[e] = 1 / the members of the pair's cluster
    ... the coarse level works on (centroid, y)
    up, coords, eoff = DeviceGraph.from_point_sets_knn(points, centroid, k=3, query_offsets=offsets, source_offsets=cluster_offsets)
    w, wsum = interp_weights(up, coords);  z = interpolate(up, w, y_coarse)             # the way up, [n_points, F]
    ... the reverse pass returns dcentroid [n_clusters, dim]
    dpoints = grid_clusters_grad(cluster, handle, dcentroid)            # [n_points, dim]

Three-body terms (athena_amd/csrc/triplets.hip): the pairs of bonds that meet at an atom and the angle between them, as a handle over
the CSR entries of the neighbour graph, so that the row kernels above run on it over per-bond messages and per-triplet values:

    handle, feature, vec, voff, eoff = DeviceGraph.from_structures(frac, lat, offsets, cutoff_min, cutoff_max)
    thandle, dir = DeviceGraph.from_triplets(handle, vec, cutoff=cutoff3)   # rows = columns = CSR entries, one edge per triplet
    cos = triplet_cos(thandle, dir)                                     # [T]
    ... edge_features(thandle, x_sources=m, ...) -> MLP -> attend / interpolate / pool_max on thandle ... return dcos [T]
    ddir = triplet_cos_grad(thandle, dir, cos, dcos)                    # [nnz, 3]
    dvec = entry_vectors_grad(handle, ddir)                             # [E, 3]
    g = structures_grad(handle, lat, voff, eoff, vec, cutoff_max, dvec=dvec)

Graphs WITHOUT coordinates (citation graphs, bond lists) coarsen by learned scores instead (athena_amd/csrc/topk_select.hip): the k
best-scored vertices of every graph, the induced subgraph through from_contraction, and the kept rows gated by the score:

    score = ... any layer with one output feature (a Kipf layer for SAGPool, a projection for TopKPooling) ... [n]
    cluster, selected, sel_offsets = topk_vertices(score, offsets, ratio=0.5)
    coarse, coarse_pairs, pool, w, edge_pair = DeviceGraph.from_contraction(handle, cluster, len(selected))
    gate = ops.activation("tanh", score)
    y = select_rows(selected, x, gate)                                  # [m, F]; sel_offsets are the pooled batch's vertex offsets
    ... the coarse level works on (coarse, y) and returns z [m, F]; on the way up: unpool(cluster, z) [n, F]
    g = select_rows_grad(cluster, dy, x=x, gate=gate)                   # g["x"] [n, F], g["gate"] [n]
    dscore = ops.activation_bwd("tanh", gate, g["gate"])"""
import ctypes as C

import numpy as np

from . import _capi

WANT = ("cart", "frac", "virial", "lat")


def points_grad(handle, dcoords, out=None):
    """The reverse of DeviceGraph.from_points (athena_mp_edge_grad_to_points): dcoords [E, dim] float32 on the device, the gradient
    with respect to coords[e] = p_i - p_j -> dpoints [n, dim], the gradient with respect to the points.  Row i is the signed sum
    over the handle's row i in CSR order (+ where i is the smaller index of the edge, - where it is the larger); bit for bit the
    sequential sum.  out: a contiguous float32 device tensor [n, dim] to write into."""
    import torch

    if not (isinstance(dcoords, torch.Tensor) and dcoords.is_cuda and dcoords.dtype == torch.float32 and dcoords.dim() == 2
            and dcoords.is_contiguous()):
        raise ValueError("dcoords must be a contiguous float32 device tensor [E, dim]")
    E, dim = int(dcoords.shape[0]), int(dcoords.shape[1])
    if E != handle.n_edge_cols:
        raise ValueError(f"dcoords holds {E} rows, the handle has {handle.n_edge_cols} edge columns")
    n = handle.n_rows
    if out is None:
        out = torch.empty((n, dim), dtype=torch.float32, device=dcoords.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n, dim) and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 device tensor [{n}, {dim}]")
    _capi.use_torch_stream()
    _capi.call("athena_mp_edge_grad_to_points", handle.handle, dim, C.c_void_p(dcoords.data_ptr()), C.c_void_p(out.data_ptr()))
    return out


def point_sets_grad(handle, dcoords, want=("queries", "sources"), out=None):
    """The reverse of DeviceGraph.from_point_sets (athena_mp_edge_grad_to_point_sets): dcoords [E, dim] float32 on the device, the
    gradient with respect to coords[e] = q_i - p_j -> a dict of device tensors for the names in `want`: "queries" [n_queries, dim],
    row i = the sum of dcoords over the handle's row i in CSR order; "sources" [n_sources, dim], row j = minus the sum over the
    handle's column j, queries ascending; bit for bit the sequential sums.  out: a dict of contiguous float32 device tensors to
    write into, by the same names."""
    import torch

    if not (isinstance(dcoords, torch.Tensor) and dcoords.is_cuda and dcoords.dtype == torch.float32 and dcoords.dim() == 2
            and dcoords.is_contiguous()):
        raise ValueError("dcoords must be a contiguous float32 device tensor [E, dim]")
    E, dim = int(dcoords.shape[0]), int(dcoords.shape[1])
    if E != handle.n_edge_cols:
        raise ValueError(f"dcoords holds {E} rows, the handle has {handle.n_edge_cols} edge columns")
    want = tuple(want)
    if not want or any(w not in ("queries", "sources") for w in want):
        raise ValueError('want must name some of ("queries", "sources")')
    shapes = {"queries": (handle.n_rows, dim), "sources": (handle.n_cols, dim)}
    res = {}
    for w in want:
        t = None if out is None else out.get(w)
        if t is None:
            t = torch.empty(shapes[w], dtype=torch.float32, device=dcoords.device)
        elif not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shapes[w] and t.is_contiguous()):
            raise ValueError(f"out[{w!r}] must be a contiguous float32 device tensor {shapes[w]}")
        res[w] = t
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _capi.use_torch_stream()
    _capi.call("athena_mp_edge_grad_to_point_sets", handle.handle, dim, ptr(dcoords), ptr(res.get("queries")), ptr(res.get("sources")))
    return res


def _device_f32(t, shape, what):
    """t is a contiguous float32 device tensor of this shape (None in a place: any size), or ValueError"""
    import torch

    ok = isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == len(shape)
    if not (ok and all(want is None or int(have) == want for have, want in zip(t.shape, shape))):
        raise ValueError(f"{what} must be a contiguous float32 device tensor [{', '.join('*' if s is None else str(s) for s in shape)}]")
    return t


def _device_i32(t, shape, what):
    """the same for a contiguous int32 device tensor"""
    import torch

    ok = isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)
    if not ok:
        raise ValueError(f"{what} must be a contiguous int32 device tensor [{', '.join(str(s) for s in shape)}]")
    return t


def interp_weights(handle, coords, eps=1e-16, out=None):
    """Inverse-squared-distance weights over a two-set handle (athena_mp_interp_weights; the definition, term by term in fp32, is in
    include/athena_mp.h): handle and coords [E, dim] as DeviceGraph.from_point_sets / from_point_sets_knn returned them.  Returns
    (weights [E], wsum [n_queries]) float32 on the device: w_e = 1 / max(|coords[e]|^2, eps), wsum[i] = the sum of w over row i in
    CSR order, weights[e] = w_e / wsum[i] (0 along a row whose sum is 0): each non-empty row's weights add up to 1 but for rounding.
    eps: finite, at least 2^-60.  out: a (weights, wsum) pair of contiguous float32 device tensors to write into."""
    import torch

    E, n = handle.n_edge_cols, handle.n_rows
    coords = _device_f32(coords, (E, None), "coords")
    dim = int(coords.shape[1])
    if out is None:
        out = (torch.empty((E,), dtype=torch.float32, device=coords.device), torch.empty((n,), dtype=torch.float32, device=coords.device))
    weights, wsum = _device_f32(out[0], (E,), "out[0]"), _device_f32(out[1], (n,), "out[1]")
    _capi.use_torch_stream()
    _capi.call("athena_mp_interp_weights", handle.handle, dim, C.c_void_p(coords.data_ptr()), float(eps), C.c_void_p(weights.data_ptr()),
               C.c_void_p(wsum.data_ptr()))
    return weights, wsum


def interpolate(handle, weights, x, out=None):
    """y [n_queries, F] = the weighted sum over each row of the handle (athena_mp_interp_fwd): y[i] = sum over the entries (j, e) of
    row i in CSR order of weights[e] * x[j], bit for bit the sequential fp32 sum; an empty row gives 0.  weights [E] and x
    [n_sources, F]: contiguous float32 device tensors; any weights, not only interp_weights'.  out: a contiguous float32 device
    tensor [n_queries, F] to write into."""
    import torch

    weights = _device_f32(weights, (handle.n_edge_cols,), "weights")
    x = _device_f32(x, (handle.n_cols, None), "x")
    F = int(x.shape[1])
    if out is None:
        out = torch.empty((handle.n_rows, F), dtype=torch.float32, device=x.device)
    out = _device_f32(out, (handle.n_rows, F), "out")
    _capi.use_torch_stream()
    _capi.call("athena_mp_interp_fwd", handle.handle, F, C.c_void_p(weights.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()))
    return out


def interpolate_grad(handle, coords, weights, x, y, dy, eps=1e-16, want=("x", "coords"), out=None):
    """The reverse of interpolate, and of interp_weights under it (athena_mp_interp_bwd_x, athena_mp_interp_bwd_coords): dy
    [n_queries, F] -> a dict of device tensors for the names in `want`: "x" [n_sources, F], row j = the sum over the handle's column
    j, queries ascending, of weights[e] * dy[i], bit for bit the sequential sum; "coords" [E, dim], the gradient with respect to
    coords through the weights of interp_weights(handle, coords, eps) -- exactly 0 where the clamp held --, which point_sets_grad
    takes as it is.  coords, weights, x and y as the forward calls took and returned them ("x" alone needs only weights and dy:
    coords, x and y may then be None).  out: a dict of contiguous float32 device tensors to write into, by the same names."""
    import torch

    want = tuple(want)
    if not want or any(w not in ("x", "coords") for w in want):
        raise ValueError('want must name some of ("x", "coords")')
    E, nq, ns = handle.n_edge_cols, handle.n_rows, handle.n_cols
    weights = _device_f32(weights, (E,), "weights")
    dy = _device_f32(dy, (nq, None), "dy")
    F = int(dy.shape[1])
    dim = None
    if "coords" in want:
        coords = _device_f32(coords, (E, None), "coords")
        dim = int(coords.shape[1])
        x, y = _device_f32(x, (ns, F), "x"), _device_f32(y, (nq, F), "y")
    shapes = {"x": (ns, F), "coords": (E, dim)}
    res = {}
    for w in want:
        t = None if out is None else out.get(w)
        if t is None:
            t = torch.empty(shapes[w], dtype=torch.float32, device=dy.device)
        res[w] = _device_f32(t, shapes[w], f"out[{w!r}]")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    _capi.use_torch_stream()
    if "x" in want:
        _capi.call("athena_mp_interp_bwd_x", handle.handle, F, ptr(weights), ptr(dy), ptr(res["x"]))
    if "coords" in want:
        _capi.call("athena_mp_interp_bwd_coords", handle.handle, dim, F, ptr(coords), float(eps), ptr(weights), ptr(x), ptr(y), ptr(dy),
                   ptr(res["coords"]))
    return res


def pool_max(handle, x=None, edges=None, want_arg=True, out=None):
    """The maximum over each row of the handle, and where it was found (athena_mp_pool_max_fwd, athena_mp_pool_max_edges_fwd; the
    definition is in include/athena_mp.h).  Exactly one of x [n_cols, F] (per-vertex values, any handle) and edges [E, F] (per-edge
    values, a handle with one entry per edge column: from_point_sets, from_point_sets_knn) is given: contiguous float32 device
    tensors.  Returns (y, arg): y [n_rows, F] float32, the bits of the first maximum in CSR order (a NaN wins over every number),
    +0 along an empty row; arg [n_rows, F] int32, the 0-based column (source) it came from, -1 along an empty row -- None with
    want_arg=False.  out: a (y, arg) pair of contiguous device tensors to write into (arg: int32, or None)."""
    import torch

    if (x is None) == (edges is None):
        raise ValueError("exactly one of x and edges must be given")
    n = handle.n_rows
    if x is not None:
        v, entry = _device_f32(x, (handle.n_cols, None), "x"), "athena_mp_pool_max_fwd"
    else:
        v, entry = _device_f32(edges, (handle.n_edge_cols, None), "edges"), "athena_mp_pool_max_edges_fwd"
    F = int(v.shape[1])
    y, arg = (None, None) if out is None else out
    if y is None:
        y = torch.empty((n, F), dtype=torch.float32, device=v.device)
    y = _device_f32(y, (n, F), "out[0]")
    if arg is None and want_arg:
        arg = torch.empty((n, F), dtype=torch.int32, device=v.device)
    if arg is not None:
        arg = _device_i32(arg, (n, F), "out[1]")
    _capi.use_torch_stream()
    _capi.call(entry, handle.handle, F, C.c_void_p(v.data_ptr()), C.c_void_p(y.data_ptr()),
               C.c_void_p(arg.data_ptr()) if arg is not None else None)
    return y, arg


def pool_max_grad(handle, arg, dy, to="x", out=None):
    """The reverse of pool_max (athena_mp_pool_max_bwd_x, athena_mp_pool_max_bwd_edges): arg [n_rows, F] int32 as pool_max returned
    it and dy [n_rows, F] float32 on the device.  to="x": dx [n_cols, F], row j = the sum of dy[i] over the rows i that chose j,
    ascending, bit for bit the sequential fp32 sum; a column nobody chose gets 0.  to="edges": dh [E, F], dh[e] = dy[i] where row i
    chose the entry of edge e, else 0.  The whole of dy[i, f] goes to the one entry arg names: a tie is not shared.  out: a contiguous
    float32 device tensor of the result's shape to write into."""
    import torch

    if to not in ("x", "edges"):
        raise ValueError('to must be "x" or "edges"')
    dy = _device_f32(dy, (handle.n_rows, None), "dy")
    F = int(dy.shape[1])
    arg = _device_i32(arg, (handle.n_rows, F), "arg")
    shape = (handle.n_cols if to == "x" else handle.n_edge_cols, F)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dy.device)
    out = _device_f32(out, shape, "out")
    _capi.use_torch_stream()
    _capi.call("athena_mp_pool_max_bwd_x" if to == "x" else "athena_mp_pool_max_bwd_edges", handle.handle, F, C.c_void_p(arg.data_ptr()),
               C.c_void_p(dy.data_ptr()), C.c_void_p(out.data_ptr()))
    return out


def _heads(F, H):
    if H < 1 or F < 1 or F % H != 0:
        raise ValueError(f"F = {F} feature columns do not divide into H = {H} heads")


def attention_weights(handle, scores, out=None):
    """The softmax over each row's entries, per head (athena_mp_attn_softmax_fwd; the definition is in include/athena_mp.h): scores
    [E, H], a contiguous float32 device tensor, one row per edge of a handle with one entry per edge column (from_point_sets,
    from_point_sets_knn).  Returns alpha [E, H]: over the entries of row i in CSR order, alpha = exp(s - max) / sum; each non-empty
    (row, head) adds up to 1 but for rounding, a -inf score gives exactly 0, a NaN or +inf (or only -inf) makes its own (row, head)
    NaN and no other.  out: a contiguous float32 device tensor [E, H] to write into."""
    import torch

    scores = _device_f32(scores, (handle.n_edge_cols, None), "scores")
    E, H = handle.n_edge_cols, int(scores.shape[1])
    _heads(H, H)
    if out is None:
        out = torch.empty((E, H), dtype=torch.float32, device=scores.device)
    out = _device_f32(out, (E, H), "out")
    _capi.use_torch_stream()
    _capi.call("athena_mp_attn_softmax_fwd", handle.handle, H, C.c_void_p(scores.data_ptr()), C.c_void_p(out.data_ptr()))
    return out


def _attend_values(handle, x, edges):
    """(values, "x" or "edges"): exactly one of the two is given"""
    if (x is None) == (edges is None):
        raise ValueError("exactly one of x and edges must be given")
    if x is not None:
        return _device_f32(x, (handle.n_cols, None), "x"), "x"
    return _device_f32(edges, (handle.n_edge_cols, None), "edges"), "edges"


def attend(handle, alpha, x=None, edges=None, out=None):
    """y [n_rows, F] = the sum over each row of the handle of alpha times the values, the weight chosen per head
    (athena_mp_attn_gather_fwd, athena_mp_attn_gather_edges_fwd): alpha [E, H] as attention_weights returned it -- or any weights of
    that shape --, and exactly one of x [n_cols, F] (per-vertex values) and edges [E, F] (per-edge values), F a multiple of H;
    feature column c takes the weight of head c // (F // H).  Bit for bit the sequential fp32 sum in CSR order; an empty row gives
    0.  H = 1 is interpolate; H = F is vector attention.  out: a contiguous float32 device tensor [n_rows, F] to write into."""
    import torch

    v, form = _attend_values(handle, x, edges)
    alpha = _device_f32(alpha, (handle.n_edge_cols, None), "alpha")
    F, H = int(v.shape[1]), int(alpha.shape[1])
    _heads(F, H)
    if out is None:
        out = torch.empty((handle.n_rows, F), dtype=torch.float32, device=v.device)
    out = _device_f32(out, (handle.n_rows, F), "out")
    _capi.use_torch_stream()
    _capi.call("athena_mp_attn_gather_fwd" if form == "x" else "athena_mp_attn_gather_edges_fwd", handle.handle, F, H,
               C.c_void_p(alpha.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(out.data_ptr()))
    return out


def attend_grad(handle, alpha, dy, x=None, edges=None, want=("values", "scores"), out=None):
    """The reverse of attend, and of attention_weights under it: alpha [E, H] as the forward used it, dy [n_rows, F], and the one of
    x and edges that the forward took.  Returns a dict of device tensors for the names in `want`: "values", the gradient with
    respect to the values -- dx [n_cols, F], row j = the sum over the handle's column j, queries ascending, of alpha * dy[i]
    (athena_mp_attn_gather_bwd_x), or dh [E, F] = alpha * dy[i] (athena_mp_attn_gather_bwd_edges), both bit-defined --; "scores"
    [E, H], the gradient with respect to the scores of attention_weights, through athena_mp_attn_gather_bwd_alpha (the sum over
    each head's columns of dy * values) and athena_mp_attn_softmax_bwd.  out: a dict of contiguous float32 device tensors to write
    into, by the same names."""
    import torch

    want = tuple(want)
    if not want or any(w not in ("values", "scores") for w in want):
        raise ValueError('want must name some of ("values", "scores")')
    v, form = _attend_values(handle, x, edges)
    E = handle.n_edge_cols
    alpha = _device_f32(alpha, (E, None), "alpha")
    F, H = int(v.shape[1]), int(alpha.shape[1])
    _heads(F, H)
    dy = _device_f32(dy, (handle.n_rows, F), "dy")
    shapes = {"values": (handle.n_cols if form == "x" else E, F), "scores": (E, H)}
    res = {}
    for w in want:
        t = None if out is None else out.get(w)
        if t is None:
            t = torch.empty(shapes[w], dtype=torch.float32, device=dy.device)
        res[w] = _device_f32(t, shapes[w], f"out[{w!r}]")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    _capi.use_torch_stream()
    if "values" in want:
        _capi.call("athena_mp_attn_gather_bwd_x" if form == "x" else "athena_mp_attn_gather_bwd_edges", handle.handle, F, H, ptr(alpha),
                   ptr(dy), ptr(res["values"]))
    if "scores" in want:
        dalpha = torch.empty((E, H), dtype=torch.float32, device=dy.device)
        _capi.call("athena_mp_attn_gather_bwd_alpha", handle.handle, F, H, ptr(v) if form == "x" else None,
                   ptr(v) if form == "edges" else None, ptr(dy), ptr(dalpha))
        _capi.call("athena_mp_attn_softmax_bwd", handle.handle, H, ptr(alpha), ptr(dalpha), ptr(res["scores"]))
    return res


def _device_rows(t, rows, cols, what):
    """t is a float32 device tensor [rows, cols] (cols None: any) whose rows are contiguous and do not overlap -- a contiguous tensor
    or a view buffer[:, :cols] of one --, or ValueError; returns its row pitch in elements"""
    import torch

    ok = isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and int(t.shape[0]) == rows
    ok = ok and (cols is None or int(t.shape[1]) == cols)
    ok = ok and (t.numel() == 0 or ((t.shape[1] == 1 or t.stride(1) == 1) and (rows == 1 or t.stride(0) >= t.shape[1])))
    if not ok:
        raise ValueError(f"{what} must be a float32 device tensor [{rows}, {'*' if cols is None else cols}] with contiguous rows "
                         "(stride(1) == 1, stride(0) >= the width)")
    return int(t.shape[1]) if t.numel() == 0 or rows == 1 else int(t.stride(0))


def edge_features(handle, x_sources=None, x_queries=None, coords=None, relative=False, pad_to=1, out=None):
    """The edge MLP's input over a two-set handle (athena_mp_edge_gather_fwd; the definition is in include/athena_mp.h): for the
    entry of row i and column j with edge id e, h[e] = (x_sources[j], x_queries[i], coords[e]) -- each block present when its
    tensor is given: x_sources [n_cols, Fs], x_queries [n_rows, Fq], coords [E, dim], contiguous float32 device tensors.
    relative=True (needs Fs == Fq) makes the first block x_sources[j] - x_queries[i].  Copies keep the bits.  Returns h [E, W],
    W = Fs + Fq + dim: a view of an [E, ld] buffer, ld = W rounded up to a multiple of pad_to, so torch.matmul(h, Wt) takes it as
    it is; with ld, Fs and Fq multiples of 4 the rows move 16 bytes at a time (W = 64 + 3: pad_to=4).  The buffer's columns
    beyond W are never written.  out: a float32 device tensor [E, W] with contiguous rows to write into, its stride(0) the pitch
    (pad_to is then not used)."""
    import torch

    E = handle.n_edge_cols
    given = [t for t in (x_sources, x_queries, coords) if t is not None]
    if not given:
        raise ValueError("at least one of x_sources, x_queries and coords must be given")
    xs = None if x_sources is None else _device_f32(x_sources, (handle.n_cols, None), "x_sources")
    xq = None if x_queries is None else _device_f32(x_queries, (handle.n_rows, None), "x_queries")
    co = None if coords is None else _device_f32(coords, (E, None), "coords")
    Fs, Fq, dim = (0 if t is None else int(t.shape[1]) for t in (xs, xq, co))
    W = Fs + Fq + dim
    if out is None:
        if int(pad_to) < 1:
            raise ValueError("pad_to must be at least 1")
        ld = -(-W // int(pad_to)) * int(pad_to)
        out = torch.empty((E, ld), dtype=torch.float32, device=given[0].device)[:, :W]
    else:
        ld = _device_rows(out, E, W, "out")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.shape[1] > 0 else None
    _capi.use_torch_stream()
    _capi.call("athena_mp_edge_gather_fwd", handle.handle, Fs, ptr(xs), Fq, ptr(xq), dim, ptr(co), int(bool(relative)), max(ld, W),
               C.c_void_p(out.data_ptr()))
    return out


def edge_features_grad(handle, dh, widths, relative=False, want=("sources", "queries", "coords"), out=None):
    """The reverse of edge_features (athena_mp_edge_gather_bwd): dh [E, W] float32 on the device, the gradient with respect to h --
    contiguous, or a view with contiguous rows (stride(1) == 1, stride(0) >= W), as edge_features returns one --, and widths =
    (Fs, Fq, dim), W = Fs + Fq + dim.  Returns a dict of device tensors for the names in `want`: "sources" [n_cols, Fs], row j =
    the sum of dh[e, :Fs] over the handle's column j, queries ascending; "queries" [n_rows, Fq], row i = the sum of
    dh[e, Fs:Fs + Fq] over row i in CSR order, with relative each entry's dh[e, :Fs] subtracted after it; "coords" [E, dim], a copy
    of dh's last block, what point_sets_grad takes.  Bit for bit the sequential fp32 sums; no atomics.  out: a dict of contiguous
    float32 device tensors to write into, by the same names."""
    import torch

    Fs, Fq, dim = (int(w) for w in widths)
    E = handle.n_edge_cols
    ld = _device_rows(dh, E, Fs + Fq + dim, "dh")
    want = tuple(want)
    if not want or any(w not in ("sources", "queries", "coords") for w in want):
        raise ValueError('want must name some of ("sources", "queries", "coords")')
    shapes = {"sources": (handle.n_cols, Fs), "queries": (handle.n_rows, Fq), "coords": (E, dim)}
    res = {}
    for w in want:
        t = None if out is None else out.get(w)
        if t is None:
            t = torch.empty(shapes[w], dtype=torch.float32, device=dh.device)
        res[w] = _device_f32(t, shapes[w], f"out[{w!r}]")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.shape[1] > 0 else None
    _capi.use_torch_stream()
    _capi.call("athena_mp_edge_gather_bwd", handle.handle, Fs, Fq, dim, int(bool(relative)), max(ld, Fs + Fq + dim),
               C.c_void_p(dh.data_ptr()), ptr(res.get("sources")), ptr(res.get("queries")), ptr(res.get("coords")))
    return res


def farthest_points(points, offsets=None, n_samples=None, ratio=None, start=None, want_sqdist=False, device=0):
    """Farthest-point samples of a batch of point clouds on the device (athena_mp_farthest_points; the definition, term by term in
    fp32 with ties to the smaller index, is in include/athena_mp.h).  points [n, dim] float32, dim 1..3: a numpy array, or a torch
    tensor already on the device; offsets [B + 1] 0-based on the host (None: one cloud), empty clouds allowed.  Exactly one of
    n_samples (an int for every cloud, or one per cloud) and ratio (m_b = min(n_b, max(1, ceil(ratio * n_b))) for a non-empty
    cloud) is given; start: None, or [B] 1-based global indices of each cloud's first choice (0: its first point).  Returns
    (sample, sample_points, sample_offsets, cover_sqdist) and, with want_sqdist, sample_sqdist last: sample int32 [m] = the chosen
    points as 1-based global indices in selection order (every prefix of a cloud's samples is a sample of it), sample_points
    [m, dim] their rows and cover_sqdist [B] float32 -- device tensors --, sample_offsets numpy int32 [B + 1], what
    from_point_sets(..., query_offsets=...) takes."""
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
    B = off.size - 1
    sizes = np.diff(off.astype(np.int64))
    if (n_samples is None) == (ratio is None):
        raise ValueError("exactly one of n_samples and ratio must be given")
    if ratio is not None:
        if not ratio > 0:
            raise ValueError("ratio must be positive")
        m = np.where(sizes > 0, np.minimum(sizes, np.maximum(1, np.ceil(float(ratio) * sizes))), 0).astype(np.int64)
    else:
        m = np.broadcast_to(np.asarray(n_samples, dtype=np.int64), (B,)) if np.ndim(n_samples) == 0 else np.asarray(n_samples, np.int64)
        if m.shape != (B,) or (m < 0).any():
            raise ValueError("n_samples must be a non-negative int, or one per cloud")
    if m.sum() >= 2 ** 31:
        raise ValueError("more than 2^31 samples")
    soff = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
    st = None
    if start is not None:
        st = np.ascontiguousarray(start, dtype=np.int32)
        if st.shape != (B,):
            raise ValueError("start must hold one index per cloud")
    mt = int(soff[-1])
    sample = torch.empty((mt,), dtype=torch.int32, device=dev)
    sample_points = torch.empty((mt, dim), dtype=torch.float32, device=dev)
    sqdist = torch.empty((mt,), dtype=torch.float32, device=dev) if want_sqdist else None
    cover = torch.empty((B,), dtype=torch.float32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    _capi.use_torch_stream()
    _capi.call("athena_mp_farthest_points", B, n, vp(off), dim, ptr(pts), mt, vp(soff), vp(st), ptr(sample), ptr(sample_points),
               ptr(sqdist), ptr(cover))
    out = (sample, sample_points, soff, cover)
    return out + (sqdist,) if want_sqdist else out


def grid_clusters_grad(cluster, rowptr_or_handle, dcentroid, out=None):
    """The reverse of the centroids of DeviceGraph.from_grid_clusters (athena_mp_grid_clusters_grad): dcentroid [m, dim] float32 on
    the device -> dpoints [n, dim], dpoints[j] = dcentroid[c] / the members of c, c = cluster[j]; every bit is defined.  cluster [n]
    int32 (1-based) as from_grid_clusters returned it; rowptr_or_handle: its handle, or a contiguous int32 device tensor [m + 1]
    whose differences are the clusters' sizes.  out: a contiguous float32 device tensor [n, dim] to write into."""
    import torch

    if isinstance(rowptr_or_handle, torch.Tensor):
        rowptr = rowptr_or_handle
    else:
        rowptr = getattr(rowptr_or_handle, "cluster_rowptr", None)
        if rowptr is None:                       # any handle with these rows: its forward CSR's row pointer, through the host
            rowptr = torch.from_numpy(np.ascontiguousarray(rowptr_or_handle.export("rowptr"), dtype=np.int32)).to(dcentroid.device)
    m = int(rowptr.shape[0]) - 1
    rowptr = _device_i32(rowptr, (m + 1,), "rowptr")
    dcentroid = _device_f32(dcentroid, (m, None), "dcentroid")
    dim = int(dcentroid.shape[1])
    n = int(cluster.shape[0]) if isinstance(cluster, torch.Tensor) and cluster.dim() == 1 else -1
    cluster = _device_i32(cluster, (max(n, 0),), "cluster")
    if out is None:
        out = torch.empty((n, dim), dtype=torch.float32, device=dcentroid.device)
    out = _device_f32(out, (n, dim), "out")
    _capi.use_torch_stream()
    _capi.call("athena_mp_grid_clusters_grad", n, dim, m, C.c_void_p(cluster.data_ptr()), C.c_void_p(rowptr.data_ptr()),
               C.c_void_p(dcentroid.data_ptr()), C.c_void_p(out.data_ptr()))
    return out


def cover_radius(cover_sqdist):
    """The smallest float32 r with fl(r * r) >= max(cover_sqdist): sqrt, then nextafter upwards while short.  With this radius the
    predicate of from_point_sets (s <= fl(r * r)) joins every point of every cloud to at least one of its samples."""
    c = cover_sqdist.detach().cpu().numpy() if hasattr(cover_sqdist, "detach") else np.asarray(cover_sqdist)
    c = np.float32(c.astype(np.float32).max()) if c.size else np.float32(0)
    if not np.isfinite(c):
        raise ValueError("cover_sqdist is not finite: a cloud with points got no sample, or its distances overflow")
    r = np.sqrt(c, dtype=np.float32)
    while np.float32(r * r) < c:
        r = np.nextafter(r, np.float32(np.inf))
    return float(r)


def _host_tables(handle, lat_rows, offsets, edge_offsets, want):
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    eoff = np.ascontiguousarray(edge_offsets, dtype=np.int64)
    if not (off.ndim == 1 and off.size >= 1 and eoff.shape == off.shape and lat_rows == off.size - 1):
        raise ValueError("offsets and edge_offsets must be [B + 1] with lat [B, 3, 3]")
    want = tuple(want)
    if not want or any(w not in WANT for w in want):
        raise ValueError(f"want must name some of {WANT}")
    return off, eoff, want


def structures_grad(handle, lat, offsets, edge_offsets, vec, cutoff_max, dfeature=None, dvec=None, want=WANT, out=None):
    """The reverse of DeviceGraph.from_structures (athena_mp_periodic_grad).  handle, vec [E, 3], offsets (vertex_offsets) and
    edge_offsets as from_structures returned them, lat [B, 3, 3] and cutoff_max as it took them; dfeature [E, fe_cols] (the de of a
    layer whose edge input was `feature` in every column) and / or dvec [E, 3]: float32 device tensors.  Returns a dict of device
    tensors for the names in `want`: "cart" [n, 3] = dE/d(Cartesian position) (forces are its negative), "frac" [n, 3],
    "virial" [B, 3, 3] = sum over a structure's edges of vec (x) gx, "lat" [B, 3, 3] = L^-T virial = dE/dL at fixed fractional
    coordinates.  out: a dict of contiguous float32 device tensors to write into, by the same names."""
    import torch

    dev = vec.device if isinstance(vec, torch.Tensor) else torch.device("cuda", 0)
    f32 = lambda t, what: _f32_device(t, dev, what)
    lat = f32(lat, "lat")
    vec = f32(vec, "vec")
    off, eoff, want = _host_tables(handle, int(lat.shape[0]), offsets, edge_offsets, want)
    B, n, E = off.size - 1, int(off[-1]), int(vec.shape[0])
    if not (tuple(lat.shape[1:]) == (3, 3) and tuple(vec.shape) == (E, 3)):
        raise ValueError("lat must be [B, 3, 3] and vec [E, 3]")
    fe_cols = 0
    if dfeature is not None:
        dfeature = f32(dfeature, "dfeature")
        if dfeature.dim() == 1:
            dfeature = dfeature[:, None]
        if not (dfeature.dim() == 2 and dfeature.shape[0] == E):
            raise ValueError("dfeature must be [E, fe_cols]")
        fe_cols = int(dfeature.shape[1])
    if dvec is not None:
        dvec = f32(dvec, "dvec")
        if tuple(dvec.shape) != (E, 3):
            raise ValueError("dvec must be [E, 3]")
    shapes = {"cart": (n, 3), "frac": (n, 3), "virial": (B, 3, 3), "lat": (B, 3, 3)}
    res = {}
    for w in want:
        t = None if out is None else out.get(w)
        if t is None:
            t = torch.empty(shapes[w], dtype=torch.float32, device=dev)
        elif not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shapes[w] and t.is_contiguous()):
            raise ValueError(f"out[{w!r}] must be a contiguous float32 device tensor {shapes[w]}")
        res[w] = t
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _capi.use_torch_stream()
    _capi.call("athena_mp_periodic_grad", handle.handle, B, n, vp(off), vp(eoff), ptr(lat), float(cutoff_max), ptr(vec), ptr(dfeature),
               fe_cols, ptr(dvec), ptr(res.get("cart")), ptr(res.get("frac")), ptr(res.get("virial")), ptr(res.get("lat")))
    return res


def _f32_device(t, dev, what):
    """a contiguous float32 device tensor as it is (no copy: its address is the caller's), a numpy array uploaded"""
    import torch

    if isinstance(t, torch.Tensor):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous float32 device tensor (or a numpy array)")
        return t
    return torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(dev)


def structures_grad_host(handle, lat, offsets, edge_offsets, vec, cutoff_max, dfeature=None, dvec=None, want=WANT):
    """structures_grad for numpy arrays (athena_mp_periodic_grad_host: every array staged through HBM, what a caller that holds
    Fortran arrays uses); returns a dict of numpy arrays"""
    lat = np.ascontiguousarray(lat, dtype=np.float32).reshape(-1, 3, 3)
    vec = np.ascontiguousarray(vec, dtype=np.float32).reshape(-1, 3)
    off, eoff, want = _host_tables(handle, lat.shape[0], offsets, edge_offsets, want)
    B, n, E = off.size - 1, int(off[-1]), vec.shape[0]
    fe_cols = 0
    if dfeature is not None:
        dfeature = np.ascontiguousarray(dfeature, dtype=np.float32)
        if dfeature.ndim == 1:
            dfeature = dfeature[:, None]
        if not (dfeature.ndim == 2 and dfeature.shape[0] == E):
            raise ValueError("dfeature must be [E, fe_cols]")
        fe_cols = dfeature.shape[1]
    if dvec is not None:
        dvec = np.ascontiguousarray(dvec, dtype=np.float32).reshape(E, 3)
    shapes = {"cart": (n, 3), "frac": (n, 3), "virial": (B, 3, 3), "lat": (B, 3, 3)}
    res = {w: np.empty(shapes[w], np.float32) for w in want}
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    _capi.call("athena_mp_periodic_grad_host", handle.handle, B, n, vp(off), vp(eoff), vp(lat), float(cutoff_max), vp(vec), vp(dfeature),
               fe_cols, vp(dvec), vp(res.get("cart")), vp(res.get("frac")), vp(res.get("virial")), vp(res.get("lat")))
    return res


def entry_vectors(handle, vec, out=None):
    """The vector from every entry's row vertex to its neighbour (athena_mp_entry_vectors_fwd; the definition is in
    include/athena_mp.h): handle is a square handle with edge columns (from_structures, from_points, from_point_clouds[_knn],
    from_edges) and vec [E, dim] what its builder returned (smaller index minus larger), a contiguous float32 device tensor, dim
    1..3.  Returns dir [nnz, dim], one row per CSR entry k of row i and column c: -vec[e] when i <= c, +vec[e] when i > c, +0 for an
    id-less self loop.  DeviceGraph.from_triplets returns the same tensor; the chain is from_structures -> from_triplets ->
    triplet_cos -> ... -> triplet_cos_grad -> entry_vectors_grad -> structures_grad(dvec=...).  out: a contiguous float32 device
    tensor [nnz, dim] to write into."""
    import torch

    vec = _device_f32(vec, (handle.n_edge_cols, None), "vec")
    dim = int(vec.shape[1])
    if out is None:
        out = torch.empty((handle.nnz, dim), dtype=torch.float32, device=vec.device)
    out = _device_f32(out, (handle.nnz, dim), "out")
    _capi.use_torch_stream()
    _capi.call("athena_mp_entry_vectors_fwd", handle.handle, dim, C.c_void_p(vec.data_ptr()), C.c_void_p(out.data_ptr()))
    return out


def entry_vectors_grad(handle, ddir, out=None):
    """The reverse of entry_vectors (athena_mp_entry_vectors_bwd): ddir [nnz, dim] float32 on the device -> dvec [E, dim], row e the
    signed sum of ddir over the entries that carry edge e, in the order of the handle's edge index (- where the entry's row is at
    most its column, + where it is larger); bit for bit the sequential sum.  dvec is what structures_grad takes as dvec=, and
    points_grad as dcoords.  out: a contiguous float32 device tensor [E, dim] to write into."""
    import torch

    ddir = _device_f32(ddir, (handle.nnz, None), "ddir")
    dim = int(ddir.shape[1])
    if out is None:
        out = torch.empty((handle.n_edge_cols, dim), dtype=torch.float32, device=ddir.device)
    out = _device_f32(out, (handle.n_edge_cols, dim), "out")
    _capi.use_torch_stream()
    _capi.call("athena_mp_entry_vectors_bwd", handle.handle, dim, C.c_void_p(ddir.data_ptr()), C.c_void_p(out.data_ptr()))
    return out


def triplet_cos(thandle, dir, out=None):
    """The cosine of the angle of every triplet (athena_mp_triplet_cos_fwd; the definition, term by term in fp32, is in
    include/athena_mp.h): thandle and dir [nnz, dim] as DeviceGraph.from_triplets returned them.  Returns cos [T] float32 on the
    device: for triplet t = (k, k'), dot(dir[k], dir[k']) / (|dir[k]| |dir[k']|), +0 where the denominator is 0 (coincident points);
    no clamp, so |cos| may exceed 1 by rounding.  cos is a per-edge value of thandle: interpolate(thandle, cos, m),
    pool_max(thandle, edges=cos[:, None]), edge_features and attend take it as it is.  out: a contiguous float32 device tensor [T]
    to write into."""
    import torch

    dir = _device_f32(dir, (thandle.n_rows, None), "dir")
    T = thandle.n_edge_cols
    if out is None:
        out = torch.empty((T,), dtype=torch.float32, device=dir.device)
    out = _device_f32(out, (T,), "out")
    _capi.use_torch_stream()
    _capi.call("athena_mp_triplet_cos_fwd", thandle.handle, int(dir.shape[1]), C.c_void_p(dir.data_ptr()), C.c_void_p(out.data_ptr()))
    return out


def triplet_cos_grad(thandle, dir, cos, dcos, out=None):
    """The reverse of triplet_cos (athena_mp_triplet_cos_bwd): dir [nnz, dim] and cos [T] as the forward took and returned them, dcos
    [T] float32 on the device -> ddir [nnz, dim]: row k sums dcos[t] times the gradient of cos[t] with respect to dir[k], first over
    the triplets whose first entry is k (row k of thandle in CSR order), then over those whose second entry is k (its column, rows
    ascending); bit for bit the sequential sum, +0 for an entry in no triplet.  entry_vectors_grad carries ddir on to dvec, and
    structures_grad(dvec=...) to atoms and cell.  out: a contiguous float32 device tensor [nnz, dim] to write into."""
    import torch

    dir = _device_f32(dir, (thandle.n_rows, None), "dir")
    dim, T = int(dir.shape[1]), thandle.n_edge_cols
    cos, dcos = _device_f32(cos, (T,), "cos"), _device_f32(dcos, (T,), "dcos")
    if out is None:
        out = torch.empty((thandle.n_rows, dim), dtype=torch.float32, device=dir.device)
    out = _device_f32(out, (thandle.n_rows, dim), "out")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    _capi.use_torch_stream()
    _capi.call("athena_mp_triplet_cos_bwd", thandle.handle, dim, ptr(dir), ptr(cos), ptr(dcos), ptr(out))
    return out


def triplet_stats():
    """(triplets, participants, the longest run m (m - 1)) of the last triplet build (athena_mp_triplet_stats)"""
    out = np.zeros(3, np.int64)
    _capi.call("athena_mp_triplet_stats", out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out)


def _topk_counts(sizes, k, ratio):
    """k_g [B] int64 from exactly one of k (an int for every graph, or one per graph) and ratio: min(n_g, ceil(float64(ratio) * n_g))"""
    B = sizes.size
    if (k is None) == (ratio is None):
        raise ValueError("exactly one of k and ratio must be given")
    if ratio is not None:
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.integer, np.floating)) or not 0 < float(ratio) <= 1:
            raise ValueError("ratio must be a number in (0, 1]")
        return np.minimum(sizes, np.ceil(np.float64(ratio) * sizes.astype(np.float64)).astype(np.int64))
    kk = np.asarray(k)
    if kk.dtype.kind not in "iu" or kk.ndim > 1 or (kk.ndim == 1 and kk.shape != (B,)):
        raise ValueError("k must be a non-negative int, or one per graph")
    kk = np.broadcast_to(kk.astype(np.int64), (B,))
    if (kk < 0).any():
        raise ValueError("k must be a non-negative int, or one per graph")
    return np.minimum(kk, 2 ** 31 - 1)


def topk_vertices(score, offsets=None, k=None, ratio=None, min_score=None, want_order=False, device=0):
    """The k best-scored vertices of every graph of a batch, on the device (athena_mp_topk_vertices; the definition is in
    include/athena_mp.h): the selection of TopKPooling, SAGPool and ASAPool.  score [n] float32: a numpy array, or a torch tensor
    already on the device; offsets [B + 1] 0-based on the host (None: one graph), empty graphs allowed.  Exactly one of k (an int
    for every graph, or one per graph) and ratio in (0, 1] (k_g = min(n_g, ceil(ratio * n_g)), computed in float64) is given;
    min_score: a kept vertex also has score >= min_score.  Inside a graph the order is value descending, then index ascending; -0
    equals +0, every NaN lies below -inf.  Returns (cluster, selected, sel_offsets) and, with want_order, order last: cluster int32
    [n] = the new 1-based id of a kept vertex, 0 otherwise -- what DeviceGraph.from_contraction(handle, cluster, m) takes for the
    induced subgraph --, selected int32 [m] = the 1-based vertex of each new id (ascending), order int32 [m] = each graph's kept
    vertices in score order -- device tensors --, sel_offsets numpy int32 [B + 1], the vertex_offsets of the pooled batch."""
    import torch

    is_tensor = isinstance(score, torch.Tensor)
    if is_tensor:
        if score.dtype != torch.float32 or score.dim() != 1:
            raise ValueError("score must be float32 [n]")
        n = int(score.shape[0])
    else:
        score = np.asarray(score)
        if score.dtype != np.float32 or score.ndim != 1:
            raise ValueError("score must be float32 [n]")
        n = int(score.shape[0])
    off = np.array([0, n], np.int32) if offsets is None else np.ascontiguousarray(offsets, dtype=np.int32)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("offsets must be [B + 1]")
    B = off.size - 1
    sizes = np.diff(off.astype(np.int64))
    if off[0] != 0 or (sizes < 0).any() or off[-1] != n:
        raise ValueError(f"offsets must ascend from 0 to n = {n}")
    kk = _topk_counts(sizes, k, ratio).astype(np.int32)
    if min_score is not None and (isinstance(min_score, bool) or not isinstance(min_score, (int, float, np.integer, np.floating))):
        raise ValueError("min_score must be a number or None")
    room = int(np.minimum(kk.astype(np.int64), sizes).sum())
    _capi.init(device)
    dev = torch.device("cuda", device)
    sc = score.to(dev).contiguous() if is_tensor else torch.from_numpy(np.ascontiguousarray(score)).to(dev)
    cluster = torch.empty((n,), dtype=torch.int32, device=dev)
    selected = torch.empty((room,), dtype=torch.int32, device=dev)
    order = torch.empty((room,), dtype=torch.int32, device=dev) if want_order else None
    soff = np.zeros(B + 1, np.int32)
    m = C.c_int64()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _capi.use_torch_stream()
    _capi.call("athena_mp_topk_vertices", B, n, vp(off), ptr(sc), 0, vp(kk), int(min_score is not None),
               float(min_score) if min_score is not None else 0.0, ptr(cluster), ptr(selected), ptr(order), vp(soff), C.byref(m))
    out = (cluster, selected[:m.value], soff)
    return out + (order[:m.value],) if want_order else out


def topk_stats():
    """(graphs on the wave route, graphs on the sort route, key bits sorted, radix passes) of the last selection (athena_mp_topk_stats)"""
    out = np.zeros(4, np.int64)
    _capi.call("athena_mp_topk_stats", out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out)


def _ids_1d(t, what):
    """t is a contiguous int32 device tensor [*], or ValueError"""
    import torch

    if not (isinstance(t, torch.Tensor) and t.dim() == 1):
        raise ValueError(f"{what} must be a contiguous int32 device tensor [*]")
    return _device_i32(t, (int(t.shape[0]),), what)


def select_rows(selected, x, gate=None, out=None):
    """The rows of a selection, gated (athena_mp_select_rows_fwd): y[r] = x[selected[r] - 1] * gate[selected[r] - 1].  selected [m]
    int32 (1-based) as topk_vertices returned it, x [n, F] and gate [n] (e.g. ops.activation("tanh", score)) contiguous float32
    device tensors.  Without a gate the rows are copied bit for bit.  out: a contiguous float32 device tensor [m, F] to write into."""
    import torch

    selected = _ids_1d(selected, "selected")
    m = int(selected.shape[0])
    x = _device_f32(x, (None, None), "x")
    n, F = int(x.shape[0]), int(x.shape[1])
    if F < 1:
        raise ValueError("x must have at least one feature column")
    if gate is not None:
        gate = _device_f32(gate, (n,), "gate")
    if out is None:
        out = torch.empty((m, F), dtype=torch.float32, device=x.device)
    out = _device_f32(out, (m, F), "out")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _capi.use_torch_stream()
    _capi.call("athena_mp_select_rows_fwd", n, m, F, ptr(selected), ptr(x), ptr(gate), ptr(out))
    return out


def select_rows_grad(cluster, dy, x=None, gate=None, want=("x", "gate"), out=None):
    """The reverse of select_rows (athena_mp_select_rows_bwd): cluster [n] int32 as topk_vertices returned it and dy [m, F] float32
    on the device -> a dict of device tensors for the names in `want`: "x" [n, F], dx[v] = dy[cluster[v] - 1] * gate[v], +0 for a
    dropped vertex (without a gate: unpool); "gate" [n], dgate[v] = the sum over the columns of dy[cluster[v] - 1] * x[v], +0 for
    a dropped vertex, which needs x [n, F]; ops.activation_bwd carries it on to the scores.  out: a dict of contiguous float32
    device tensors to write into, by the same names."""
    import torch

    want = tuple(want)
    if not want or any(w not in ("x", "gate") for w in want):
        raise ValueError('want must name some of ("x", "gate")')
    cluster = _ids_1d(cluster, "cluster")
    n = int(cluster.shape[0])
    dy = _device_f32(dy, (None, None), "dy")
    m, F = int(dy.shape[0]), int(dy.shape[1])
    if F < 1:
        raise ValueError("dy must have at least one feature column")
    if "gate" in want:
        if x is None:
            raise ValueError('want "gate" needs x')
        x = _device_f32(x, (n, F), "x")
    if gate is not None:
        gate = _device_f32(gate, (n,), "gate")
    shapes = {"x": (n, F), "gate": (n,)}
    res = {}
    for w in want:
        t = None if out is None else out.get(w)
        if t is None:
            t = torch.empty(shapes[w], dtype=torch.float32, device=dy.device)
        res[w] = _device_f32(t, shapes[w], f"out[{w!r}]")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _capi.use_torch_stream()
    _capi.call("athena_mp_select_rows_bwd", n, m, F, ptr(cluster), ptr(dy), ptr(x) if "gate" in want else None, ptr(gate), ptr(res.get("x")),
               ptr(res.get("gate")))
    return res


def unpool(cluster, y, out=None):
    """The way up from a selection (athena_mp_select_rows_bwd without a gate): x[v] = y[cluster[v] - 1] for a kept vertex, +0 for
    a dropped one; cluster [n] int32 and y [m, F] float32 on the device -> [n, F].  unpool(cluster, select_rows(selected, x))
    is x on the kept rows.  out: a contiguous float32 device tensor [n, F] to write into."""
    return select_rows_grad(cluster, y, want=("x",), out=None if out is None else {"x": out})["x"]
