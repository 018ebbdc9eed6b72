"""The yardstick of the geometry gradients (athena_amd/csrc/geometry_grad.hip): the definition of include/athena_mp.h, term by
term in numpy.  dtype = np.float32 is the exact definition (numpy's fp32 add, multiply, divide and sqrt are correctly rounded and
nothing is fused), dtype = np.float64 the same formulas as the twin that error bounds are taken against.

The CSR is the handle's forward CSR as athena_mp_graph_export shows it: rowptr [n + 1], col [nnz], eid [nnz], 0-based, eid = -1 for
an entry without an edge column.  csr_of_graph gives the same three arrays from a host graph_type (graph_create copies them)."""
import numpy as np


def csr_of_graph(g):
    """(rowptr, col, eid) 0-based of a host graph_type (adj_ia / adj_ja 1-based, edge id 0 = none)"""
    ia = np.asarray(g.adj_ia, np.int64) - 1
    ja = np.asarray(g.adj_ja, np.int64)
    return ia, ja[0] - 1, ja[1] - 1


def signed_gather(rowptr, col, eid, terms, dtype):
    """out[i] = the signed sum of terms[e] over row i in CSR order (acc = +0; + when i < c, - when i > c; entries with e < 0 or
    c == i skipped), every addition rounded to dtype -> (out [n, d], mag [n, d] float64 = the sum of |terms| of each element)"""
    rowptr, col, eid = (np.asarray(a, np.int64) for a in (rowptr, col, eid))
    terms = np.asarray(terms, dtype)
    n, d = rowptr.size - 1, terms.shape[1]
    out = np.zeros((n, d), dtype)
    mag = np.zeros((n, d), np.float64)
    lens = np.diff(rowptr)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int(lens.max()) if n else 0):
            rows = np.nonzero(lens > k)[0]
            idx = rowptr[rows] + k
            c, e = col[idx], eid[idx]
            ok = (e >= 0) & (c != rows)
            rows, c, e = rows[ok], c[ok], e[ok]
            t = terms[e]
            out[rows] = np.where((rows < c)[:, None], out[rows] + t, out[rows] - t)
            mag[rows] += np.abs(t.astype(np.float64))
    assert out.dtype == dtype
    return out, mag


def points_grad(rowptr, col, eid, dcoords, dtype=np.float32):
    """points mode -> (dpoints [n, dim], mag)"""
    return signed_gather(rowptr, col, eid, dcoords, dtype)


def edge_terms(vec, cutoff_max, dfeature=None, dvec=None, dtype=np.float32):
    """(x [E, 3], gx [E, 3]) of the definition; cutoff_max is the fp32 value the builder used, in every dtype"""
    assert dfeature is not None or dvec is not None
    x = np.asarray(vec, dtype).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if dfeature is None:
            return x, np.asarray(dvec, dtype).reshape(-1, 3).copy()
        de = np.asarray(dfeature, dtype).reshape(x.shape[0], -1)
        s = ((x[:, 0] * x[:, 0]) + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
        r = np.sqrt(s)
        q = de[:, 0].copy()
        for k in range(1, de.shape[1]):
            q = q + de[:, k]
        q = q / dtype(np.float32(cutoff_max))
        gx = q[:, None] * (x / r[:, None])
        if dvec is not None:
            gx = np.asarray(dvec, dtype).reshape(-1, 3) + gx
    assert gx.dtype == dtype
    return x, gx


def structures_grad(rowptr, col, eid, lat, offsets, edge_offsets, vec, cutoff_max, dfeature=None, dvec=None, dtype=np.float32,
                    cell=True):
    """periodic mode -> dict: cart, frac [n, 3]; virial, lat [B, 3, 3] (cell=False: left out -- the virial's order is free, so a
    caller that compares it with the twin does not need the fp32 one); and the float64 term magnitudes cart_mag, frac_mag
    (sum |L[k][c]| cart_mag[c]), virial_mag (sum |x_c| |gx_d|)"""
    offsets = np.asarray(offsets, np.int64)
    edge_offsets = np.asarray(edge_offsets, np.int64)
    B = offsets.size - 1
    L = np.asarray(lat, dtype).reshape(B, 3, 3)
    x, gx = edge_terms(vec, cutoff_max, dfeature, dvec, dtype)
    cart, cart_mag = signed_gather(rowptr, col, eid, gx, dtype)
    sid = np.repeat(np.arange(B), np.diff(offsets))
    La = L[sid]                                                            # [n, 3, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        frac = ((La[:, :, 0] * cart[:, 0:1]) + La[:, :, 1] * cart[:, 1:2]) + La[:, :, 2] * cart[:, 2:3]
        frac_mag = np.einsum("nkc,nc->nk", np.abs(La.astype(np.float64)), cart_mag)
        assert cart.dtype == dtype and frac.dtype == dtype
        if not cell:
            return {"cart": cart, "frac": frac, "cart_mag": cart_mag, "frac_mag": frac_mag}
        virial = np.zeros((B, 3, 3), dtype)
        virial_mag = np.zeros((B, 3, 3), np.float64)
        for s in range(B):
            e = slice(edge_offsets[s], edge_offsets[s + 1])
            if dtype == np.float64:                                        # the twin: the order is free
                virial[s] = x[e].T @ gx[e]
            else:                                                          # one admissible order: edge by edge
                outer = x[e][:, :, None] * gx[e][:, None, :]
                acc = np.zeros((3, 3), dtype)
                for t in outer:
                    acc = acc + t
                virial[s] = acc
            virial_mag[s] = np.abs(x[e].astype(np.float64)).T @ np.abs(gx[e].astype(np.float64))
    dlat = np.zeros((B, 3, 3), dtype)
    for s in range(B):
        L64 = L[s].astype(np.float64)
        det = np.linalg.det(L64)
        if np.isfinite(det) and det != 0.0:
            dlat[s] = (np.linalg.inv(L64).T @ virial[s].astype(np.float64)).astype(dtype)
        else:
            dlat[s] = np.nan
    assert cart.dtype == dtype and frac.dtype == dtype
    return {"cart": cart, "frac": frac, "virial": virial, "lat": dlat, "cart_mag": cart_mag, "frac_mag": frac_mag,
            "virial_mag": virial_mag}
