"""The pruning rule of the periodic builder's grid route (athena_amd/csrc/periodic_graph.hip), transcribed from the file's header
into numpy: cells per axis from h_a (float64), the cell of an atom (float32, as the kernel computes it), and the candidate pairs
-- atoms in equal or circularly adjacent cells on every axis with at least three cells.  tests/test_periodic_grid.py holds it
against the yardstick of tests/periodic_reference.py: no pair with a kept image may be pruned.  Also the structures both the CPU
and the GPU tests of the route are run on."""
import numpy as np

F32 = np.float32
MARGIN = 2.0 ** -8                   # kGridMargin
CELLS_AXIS = 128                     # kGridCellsAxis
FRAC_MAX = 64.0                      # kGridFracMax, precondition (P1)
LATTICE_SUM = 4096.0                 # kGridLatticeSum, precondition (P2)
GRID_ATOMS = 128                     # kGridAtoms: automatic mode takes the grid above this many atoms, with nc >= 4 somewhere


def axis_cells(lat, cutoff_max, pbc=(1, 1, 1), m=None):
    """-> (nc [3], ok): cells per axis (1, or 3 .. CELLS_AXIS; lowered until there are at most 2 m cells) and whether the lattice
    allows the grid at all (a periodic axis, and (P2))"""
    L = np.asarray(lat, F32).astype(np.float64).reshape(3, 3)
    nc = [1, 1, 1]
    if not any(pbc):
        return nc, False
    cmax = float(F32(cutoff_max))
    det = float(np.dot(L[0], np.cross(L[1], L[2])))
    total = 0.0
    for a in range(3):
        length = float(np.sqrt(np.dot(L[a], L[a])))
        if pbc[a]:
            h = cmax * float(np.linalg.norm(np.cross(L[(a + 1) % 3], L[(a + 2) % 3]))) / abs(det)
            c = np.floor(1.0 / (h * (1.0 + MARGIN)))
            nc[a] = CELLS_AXIS if c >= CELLS_AXIS else int(c) if c >= 3 else 1
            total += (np.floor(h + 0.5) + 2.0) * length                     # searched half-range + 1
        else:
            total += (2.0 * FRAC_MAX + 1.0) * length
    if m is not None:
        while nc[0] * nc[1] * nc[2] > max(1, 2 * m):
            a = int(np.argmax(nc))                                           # the first of the largest
            nc[a] = (nc[a] + 1) // 2
            if nc[a] < 3:
                nc[a] = 1
    return nc, total <= LATTICE_SUM * cmax


def frac_in_range(frac):
    """(P1)"""
    return bool(np.all(np.abs(np.asarray(frac, F32)) <= F32(FRAC_MAX)))


def cell_coords(frac, nc):
    """[m, 3] int: t = frac - floor(frac) and t * nc in float32, truncated, clamped into the last cell"""
    frac = np.ascontiguousarray(frac, F32).reshape(-1, 3)
    out = np.zeros(frac.shape, np.int64)
    for k in range(3):
        if nc[k] > 1:
            t = frac[:, k] - np.floor(frac[:, k])
            assert t.dtype == F32 and np.all(t >= 0) and np.all(t <= 1)
            q = t * F32(nc[k])
            assert q.dtype == F32
            out[:, k] = np.minimum(nc[k] - 1, q.astype(np.int64))
    return out


def candidate_matrix(frac, nc):
    """[m, m] bool, i <= j: the pairs the grid route hands to the predicate"""
    cc = cell_coords(frac, nc)
    m = cc.shape[0]
    ok = np.triu(np.ones((m, m), bool))
    for k in range(3):
        if nc[k] >= 3:
            d = np.abs(cc[:, None, k] - cc[None, :, k])
            ok &= (d <= 1) | (d == nc[k] - 1)
    return ok


def takes_grid_automatically(m, nc, ok, frac):
    return m > GRID_ATOMS and max(nc) >= 4 and ok and frac_in_range(frac)


# ---- the structures of the tests --------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def cubic(edge):
    return (np.eye(3) * edge).astype(F32)


def sheared_cell():
    L = np.diag([20.0, 17.0, 15.0])
    L[1] += 0.6 * L[0]
    L[2] += 0.4 * L[1] - 0.3 * L[0]
    return L.astype(F32)


def boundary_set(edge=18.03, m=500, cutoff_max=3.0, seed=7):
    """atoms on the grid planes k / nc, one float32 step to either side of them, at frac = -1e-9 (t rounds to 1.0) and at
    frac = 1.0, mixed with uniform coordinates"""
    rng = _rng(seed)
    L = cubic(edge)
    nc = axis_cells(L, cutoff_max, (1, 1, 1), m)[0][0]
    assert nc >= 4
    planes = (np.arange(nc + 1, dtype=np.float64) / nc).astype(F32)
    pool = np.concatenate([planes, np.nextafter(planes, F32(2)), np.nextafter(planes, F32(-1)), [F32(-1e-9), F32(1.0)]]).astype(F32)
    frac = rng.random((m, 3)).astype(F32)
    on_plane = rng.random((m, 3)) < 0.5
    frac[on_plane] = rng.choice(pool, int(on_plane.sum()))
    frac[0] = [F32(-1e-9), F32(1.0), planes[1]]
    frac[1] = [F32(1.0), F32(-1e-9), np.nextafter(planes[1], F32(-1))]
    return frac, L


def cpu_sets():
    """name -> (frac, lat, pbc): the seven sets of the rule's CPU check (cutoffs 0.5 / 3.0)"""
    rng = _rng(11)
    sets = {
        "cubic 24, 1000 atoms": (rng.random((1000, 3)).astype(F32), cubic(24.0), (1, 1, 1)),
        "cubic 18, 600 atoms, frac in [-2, 3)": ((rng.random((600, 3)) * 5.0 - 2.0).astype(F32), cubic(18.0), (1, 1, 1)),
        "sheared, 700 atoms": (rng.random((700, 3)).astype(F32), sheared_cell(), (1, 1, 1)),
        "edge exactly 12": (rng.random((300, 3)).astype(F32), cubic(12.0), (1, 1, 1)),
        "diag(15, 15, 4)": (rng.random((200, 3)).astype(F32), np.diag([15.0, 15.0, 4.0]).astype(F32), (1, 1, 1)),
        "slab diag(22, 19, 6), pbc (1, 1, 0)": (rng.random((400, 3)).astype(F32), np.diag([22.0, 19.0, 6.0]).astype(F32), (1, 1, 0)),
    }
    f, L = boundary_set()
    sets["boundary set, edge 18.03"] = (f, L, (1, 1, 1))
    return sets


def cutoff_edge_set(cutoff_max=3.0):
    """cubic 24: 64 atom pairs (2 k, 2 k + 1) exactly cutoff_max apart along one axis (3 / 24 in frac), the second atom then moved
    one float32 step towards the first (kept) or away from it (dropped); across the wrap, across grid planes and inside cells"""
    L = cubic(24.0)
    nc = axis_cells(L, cutoff_max)[0][0]
    starts = [0.9375, 0.96875, 0.0, 0.25, 0.5]                                  # wrap (stored beyond 1 and wrapped), inside cells
    starts += [np.floor(k * 1024.0 / nc) / 1024.0 - 0.0625 for k in (1, 2, 3)]  # a grid plane between the two atoms
    frac = np.zeros((128, 3), F32)
    for k in range(64):
        axis = k % 3
        p = F32(starts[k % len(starts)])
        q = F32(p + F32(0.125))
        assert float(q) - float(p) == 0.125
        if k % 4 >= 2 and q >= 1:
            q = F32(q - F32(1.0))                                                # the wrapped twin
        q = np.nextafter(q, F32(-4) if (k // 8) % 2 == 0 else F32(4))
        other = [F32((k % 8) / 8.0 + 0.01 * k / 64.0), F32((k // 8) / 8.0 + 0.003)]
        a, b = list(other), list(other)
        a.insert(axis, p)
        b.insert(axis, q)
        frac[2 * k], frac[2 * k + 1] = a, b
    return frac, L
