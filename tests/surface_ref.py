"""The numpy reference of o2v_hip_surface_count / _write (surface nets), written from the definition in include/o2v_hip.h.

    positions, faces = extract(f, level, origin)

f is a float32 array indexed [z, y, x]; positions float32 [V, 3] (x, y, z), faces int32 [T, 3].  Everything that decides a bit
is float32, op by op; the orders are those of the header: vertices by cell (k, j, i), quads by (z, y, x, axis)."""
import numpy as np

F = np.float32
# the cell's 12 edges: (corner p, corner q) as (a, b, c), p the end with the lower coordinate
EDGES = ([((0, b, c), (1, b, c)) for b, c in ((0, 0), (1, 0), (0, 1), (1, 1))] +
         [((a, 0, c), (a, 1, c)) for a, c in ((0, 0), (1, 0), (0, 1), (1, 1))] +
         [((a, b, 0), (a, b, 1)) for a, b in ((0, 0), (1, 0), (0, 1), (1, 1))])


def inside(f, level):
    with np.errstate(invalid="ignore"):
        return np.asarray(f, F) < F(level)


def _corner(a, nz, ny, nx, abc):
    """The array of corner (a, b, c) of every cell: a view [nz - 1, ny - 1, nx - 1]."""
    x, y, z = abc
    return a[z:z + nz - 1, y:y + ny - 1, x:x + nx - 1]


def active_cells(ins):
    """bool [nz - 1, ny - 1, nx - 1]: the cells whose eight corners are neither all inside nor all outside."""
    nz, ny, nx = ins.shape
    if min(nz, ny, nx) < 2:
        return np.zeros((max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0)), bool)
    corners = [_corner(ins, nz, ny, nx, (a, b, c)) for c in (0, 1) for b in (0, 1) for a in (0, 1)]
    return np.logical_or.reduce(corners) & ~np.logical_and.reduce(corners)


def quad_edges(ins):
    """bool [nz, ny, nx, 3]: sample c and axis ax such that the edge c - c + e_ax exists, crosses and has four cells."""
    nz, ny, nx = ins.shape
    q = np.zeros((nz, ny, nx, 3), bool)
    if min(nz, ny, nx) < 2:
        return q
    q[1:-1, 1:-1, :-1, 0] = ins[1:-1, 1:-1, :-1] != ins[1:-1, 1:-1, 1:]
    q[1:-1, :-1, 1:-1, 1] = ins[1:-1, :-1, 1:-1] != ins[1:-1, 1:, 1:-1]
    q[:-1, 1:-1, 1:-1, 2] = ins[:-1, 1:-1, 1:-1] != ins[1:, 1:-1, 1:-1]
    return q


def vertices(f, level, origin, act, ins):
    """float32 [V, 3]: the positions of the active cells in cell order."""
    f = np.asarray(f, F)
    level = F(level)
    k, j, i = np.nonzero(act)          # (C order: ascending (k, j, i))
    s = [np.zeros(len(i), F) for _ in range(3)]
    n = np.zeros(len(i), np.int32)
    for axis3, (p, q) in enumerate(EDGES):
        axis = axis3 // 4
        fp, fq = (f[k + c, j + b, i + a] for a, b, c in (p, q))
        cross = ins[k + p[2], j + p[1], i + p[0]] != ins[k + q[2], j + q[1], i + q[0]]
        with np.errstate(all="ignore"):
            t = (level - fp) / (fq - fp)
            t = np.where((t >= 0) & (t <= 1), t, F(0.5)).astype(F)
        for comp in range(3):
            add = t if comp == axis else np.full(len(i), p[comp], F)
            s[comp] = np.where(cross, s[comp] + add, s[comp]).astype(F)
        n += cross
    out = np.empty((len(i), 3), F)
    with np.errstate(all="ignore"):
        for comp, idx in enumerate((i, j, k)):
            local = s[comp] / n.astype(F)
            out[:, comp] = ((idx + int(origin[comp])).astype(F) + F(0.5)) + local
    return out


def extract(f, level, origin=(0, 0, 0)):
    f = np.asarray(f, F)
    assert f.ndim == 3 and np.isfinite(F(level))
    nz, ny, nx = f.shape
    ins = inside(f, level)
    act = active_cells(ins)
    number = (np.cumsum(act.reshape(-1), dtype=np.int64) - 1).reshape(act.shape)   # (the vertex of an active cell)
    positions = vertices(f, level, origin, act, ins)
    z, y, x, ax = np.nonzero(quad_edges(ins))   # (C order: ascending ((z ny + y) nx + x) 3 + ax)
    c = np.stack([x, y, z], 1)
    eu, ev = np.eye(3, dtype=np.int64)[(ax + 1) % 3], np.eye(3, dtype=np.int64)[(ax + 2) % 3]

    def num(cell):
        assert act[cell[:, 2], cell[:, 1], cell[:, 0]].all()
        return number[cell[:, 2], cell[:, 1], cell[:, 0]]
    n0, n1, n2, n3 = num(c - eu - ev), num(c - ev), num(c), num(c - eu)
    flip = ~ins[z, y, x]
    q1, q3 = np.where(flip, n3, n1), np.where(flip, n1, n3)
    faces = np.stack([n0, q1, n2, n0, n2, q3], 1).reshape(-1, 3).astype(np.int32)
    assert len(positions) < 2 ** 31
    return positions, faces


def counts_per_layer(ins):
    """(vertices per cell layer k [nz - 1], quads per sample layer z [nz]) of a bool grid, a few layers at a time."""
    nz = ins.shape[0]
    v, q = np.zeros(max(nz - 1, 0), np.int64), np.zeros(nz, np.int64)
    for z in range(0, nz, 8):
        lo, hi = max(z - 1, 0), min(z + 9, nz)
        part = ins[lo:hi]
        a = active_cells(part).sum(axis=(1, 2))
        for k in range(z, min(z + 8, nz - 1)):
            v[k] = a[k - lo]
        # (a layer of the slice has a layer below and above it in the slice exactly when it has them in the grid)
        qe = quad_edges(part).sum(axis=(1, 2, 3))
        for s in range(z, min(z + 8, nz)):
            q[s] = qe[s - lo]
    return v, q


def extract_layers(f, level, origin, z0, z1, v_layers, q_layers):
    """What extract() gives for the cell layers z0 <= k < z1 and the sample layers z0 < z < z1 of a large grid, from the slice
    f[z0:z1 + 1] alone: (first vertex, positions, first triangle, faces).  v_layers, q_layers: counts_per_layer of the grid."""
    assert 0 <= z0 < z1 < f.shape[0]
    part = np.asarray(f[z0:z1 + 1], F)
    positions, faces = extract(part, level, (origin[0], origin[1], origin[2] + z0))
    v0 = int(v_layers[:z0].sum())
    # the slice's sample layer 0 has no quads across x and y, but may have some along z, which the grid files under z0 too:
    # they are left out (the grid's layer z0 may have more)
    qe = quad_edges(inside(part, level))
    skip = int(qe[0].sum())
    t0 = 2 * int(q_layers[:z0 + 1].sum())
    return v0, positions, t0, faces[2 * skip:] + np.int32(v0)


# ---- analytic fields (float64 construction, rounded once) ---------------------------------------------------------------

def _centres(shape):
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz) + 0.5, np.arange(ny) + 0.5, np.arange(nx) + 0.5, indexing="ij")
    return x, y, z


def sphere_field(shape, radius, centre=None):
    """The signed distance to a sphere, sampled at the voxel centres of a box [z, y, x]."""
    shape = (shape,) * 3 if np.isscalar(shape) else tuple(shape)
    cx, cy, cz = centre if centre is not None else (shape[2] / 2 + 0.13, shape[1] / 2 - 0.21, shape[0] / 2 + 0.07)
    x, y, z = _centres(shape)
    return (np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - radius).astype(F)


def torus_field(shape, major, minor):
    shape = (shape,) * 3 if np.isscalar(shape) else tuple(shape)
    x, y, z = _centres(shape)
    x, y, z = x - (shape[2] / 2 + 0.11), y - (shape[1] / 2 + 0.17), z - (shape[0] / 2 - 0.05)
    return (np.sqrt((np.sqrt(x * x + y * y) - major) ** 2 + z * z) - minor).astype(F)


def two_spheres_field(shape, radius, gap):
    """The union of two spheres whose centres are `gap` apart along x."""
    shape = (shape,) * 3 if np.isscalar(shape) else tuple(shape)
    c = (shape[2] / 2 + 0.13, shape[1] / 2 - 0.21, shape[0] / 2 + 0.07)
    a = sphere_field(shape, radius, (c[0] - gap / 2, c[1], c[2]))
    b = sphere_field(shape, radius, (c[0] + gap / 2, c[1], c[2]))
    return np.minimum(a, b)


# ---- properties of an indexed mesh ------------------------------------------------------------------------------------

def edge_uses(faces):
    """(uses of every undirected edge, uses of every directed edge) as arrays of counts."""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, directed = np.unique(d, axis=0, return_counts=True)
    _, undirected = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    return undirected, directed


def euler(positions, faces):
    """V - E + F over the vertices the faces use."""
    f = np.asarray(faces, np.int64)
    und, _ = edge_uses(f)
    return len(np.unique(f)) - len(und) + len(f)


def signed_volume(positions, faces):
    p = np.asarray(positions, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
