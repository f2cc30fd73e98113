"""The numpy reference of o2v_hip_adjacency_count / _write (include/o2v_hip.h): per pair of labels a < b of
a label grid that touch a row of 5 int64 - face, edge-only and corner-only contacts, and with a values grid the maximum over the
contacts of min(V[u], V[v]) and the minimum of max(V[u], V[v]).  adjacency takes the 13 earlier offsets as shifted views, sorts
the contacts by key and reduces the segments with np.add.reduceat / maximum.reduceat / minimum.reduceat on int64; adjacency_loop
is the definition as a scalar loop over unordered voxel pairs; skeleton_graph is the reference of dense.skeleton_graph."""
import numpy as np

from tests import components_ref as CR

COLUMNS = 5
OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)][:13]   # the earlier neighbours: (dz, dy, dx) < 0


def offset_class(dx, dy, dz):
    return (dx != 0) + (dy != 0) + (dz != 0)


def _views(shape, dx, dy, dz):
    """(slices of u, slices of v = u + (dx, dy, dz)) over the voxels u whose neighbour lies in the box."""
    def cut(n, d):
        return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
    (uz, vz), (uy, vy), (ux, vx) = cut(shape[0], dz), cut(shape[1], dy), cut(shape[2], dx)
    return (uz, uy, ux), (vz, vy, vx)


def adjacency(labels, n, connectivity=6, zero=False, values=None):
    """(pairs int32 [m, 2] sorted by (a, b), table int64 [m, 5], outside) of the grid labels [z, y, x] (any integer or bool dtype)."""
    g = np.asarray(labels).astype(np.int64)
    lo = 0 if zero else 1
    outside = int(((g < 0) | (g > n)).sum())
    top = {6: 1, 18: 2, 26: 3}[connectivity]
    V = None if values is None else np.asarray(values).astype(np.int64)
    keys, classes, his, los = [], [], [], []
    for dx, dy, dz in OFFSETS:
        cls = offset_class(dx, dy, dz)
        if cls > top:
            continue
        u, v = _views(g.shape, dx, dy, dz)
        a, b = g[u], g[v]
        on = (a != b) & (a >= lo) & (a <= n) & (b >= lo) & (b <= n)
        a, b = a[on], b[on]
        keys.append(np.minimum(a, b) << 32 | np.maximum(a, b))
        classes.append(np.full(a.shape, cls - 1, np.int64))
        if V is not None:
            his.append(np.minimum(V[u][on], V[v][on]))
            los.append(np.maximum(V[u][on], V[v][on]))
    key = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    if not key.size:
        return np.zeros((0, 2), np.int32), np.zeros((0, COLUMNS), np.int64), outside
    cls = np.concatenate(classes)
    order = np.argsort(key, kind="stable")
    key, cls = key[order], cls[order]
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    table = np.zeros((len(starts), COLUMNS), np.int64)
    for c in range(3):
        table[:, c] = np.add.reduceat((cls == c).astype(np.int64), starts)
    if V is not None:
        table[:, 3] = np.maximum.reduceat(np.concatenate(his)[order], starts)
        table[:, 4] = np.minimum.reduceat(np.concatenate(los)[order], starts)
    pairs = np.stack([key[starts] >> 32, key[starts] & 0xffffffff], 1).astype(np.int32)
    return pairs, table, outside


def adjacency_loop(labels, n, connectivity=6, zero=False, values=None):
    """The definition, voxel pair by voxel pair."""
    g = np.asarray(labels).astype(np.int64)
    nz, ny, nx = g.shape
    lo = 0 if zero else 1
    top = {6: 1, 18: 2, 26: 3}[connectivity]
    rows = {}
    outside = 0
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                a = int(g[z, y, x])
                if a < 0 or a > n:
                    outside += 1
                for dz in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            X, Y, Z = x + dx, y + dy, z + dz
                            if not (0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz):
                                continue
                            if (Z, Y, X) <= (z, y, x):       # each unordered pair once, u != v
                                continue
                            cls = offset_class(dx, dy, dz)
                            b = int(g[Z, Y, X])
                            if cls > top or a == b or not (lo <= a <= n and lo <= b <= n):
                                continue
                            row = rows.setdefault((min(a, b), max(a, b)), [0, 0, 0, None, None])
                            row[cls - 1] += 1
                            if values is not None:
                                va, vb = int(values[z, y, x]), int(values[Z, Y, X])
                                row[3] = min(va, vb) if row[3] is None else max(row[3], min(va, vb))
                                row[4] = max(va, vb) if row[4] is None else min(row[4], max(va, vb))
    keys = sorted(rows)
    pairs = np.array(keys, np.int32).reshape(-1, 2)
    table = np.array([[v or 0 for v in rows[k]] for k in keys], np.int64).reshape(-1, COLUMNS)
    return pairs, table, outside


def box_pair_row(a, b, c):
    """(faces, edges, corners) between two boxes that share a face of b x c voxels, at connectivity 26."""
    return [b * c, 2 * (b - 1) * c + 2 * (c - 1) * b, 4 * (b - 1) * (c - 1)]


def alternating_row(nx, ny, nz):
    """(faces, edges, corners) of the one pair of a grid whose two labels alternate along x and do not change along y and z."""
    return [(nx - 1) * ny * nz, 2 * (nx - 1) * ((ny - 1) * nz + ny * (nz - 1)), 4 * (nx - 1) * (ny - 1) * (nz - 1)]


def grid_pair_counts(nx, ny, nz):
    """The number of pairs at connectivity (6, 18, 26) of a grid of all-distinct labels: its voxel pairs by class, added up."""
    faces = (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1)
    edges = 2 * ((nx - 1) * (ny - 1) * nz + (nx - 1) * ny * (nz - 1) + nx * (ny - 1) * (nz - 1))
    corners = 4 * (nx - 1) * (ny - 1) * (nz - 1)
    return faces, faces + edges, faces + edges + corners


def skeleton_graph(degree):
    """(labels int32, n_nodes, n_branches, incidence int32 [k, 2], node_contacts int32 [j, 2]) of a degree grid (uint8 [z, y, x]):
    nodes are the 26-components of the skeleton voxels of degree other than 3, numbered first, branches those of degree 3."""
    degree = np.asarray(degree)
    nodes, n_nodes = CR.label((degree != 0) & (degree != 3), 26)
    branches, n_branches = CR.label(degree == 3, 26)
    labels = np.where(branches > 0, branches + n_nodes, nodes).astype(np.int32)
    pairs, _, _ = adjacency(labels, n_nodes + n_branches, 26)
    a, b = pairs[:, 0], pairs[:, 1]
    inc = (a <= n_nodes) & (b > n_nodes)
    both = b <= n_nodes
    incidence = np.stack([a[inc], b[inc] - n_nodes], 1).astype(np.int32)
    return labels, n_nodes, n_branches, incidence, pairs[both]
