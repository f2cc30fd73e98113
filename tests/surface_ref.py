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


def each(fn, items, workers=1):
    """[fn(*item) for item in items], on `workers` threads (numpy leaves the interpreter lock while it works)."""
    if workers <= 1:
        return [fn(*item) for item in items]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(workers) as pool:
        return list(pool.map(lambda item: fn(*item), items))


def counts_per_layer_slabs(ins, slab=64, workers=1):
    """counts_per_layer of a grid of many layers, from slabs of `slab` sample layers with a layer of their neighbours on either
    side, which do not depend on each other."""
    nz = ins.shape[0]

    def one(a, b):
        lo, hi = max(a - 1, 0), min(b + 1, nz)
        v, q = counts_per_layer(ins[lo:hi])
        return v[a - lo:min(b, nz - 1) - lo], q[a - lo:b - lo]
    parts = each(one, [(a, min(a + slab, nz)) for a in range(0, nz, slab)], workers)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def extract_layers(f, level, origin, z0, z1, v_layers, q_layers):
    """What extract() gives for the cell layers z0 <= k < z1 and the sample layers z0 < z < z1 of a large grid (with z0 = 0:
    sample layer 0 too), from the slice f[z0:z1 + 1] alone: (first vertex, positions, first triangle, faces).  v_layers,
    q_layers: counts_per_layer of the grid.  The next range has to begin at z1 - 1 for sample layer z1 to be covered
    (layer_chunks)."""
    assert 0 <= z0 < z1 < f.shape[0]
    part = np.asarray(f[z0:z1 + 1], F)
    positions, faces = extract(part, level, (origin[0], origin[1], origin[2] + z0))
    v0 = int(v_layers[:z0].sum())
    if z0 == 0:
        # the grid's sample layer 0 has quads along z only, and the slice files the same ones under its own layer 0
        return v0, positions, 0, faces
    # the slice's sample layer 0 has no quads across x and y, but may have some along z, which the grid files under z0 too:
    # they are left out (the grid's layer z0 may have more)
    qe = quad_edges(inside(part, level))
    skip = int(qe[0].sum())
    t0 = 2 * int(q_layers[:z0 + 1].sum())
    return v0, positions, t0, faces[2 * skip:] + np.int32(v0)


def layer_chunks(nz, n):
    """Ranges (z0, z1) of at most n cell layers for extract_layers that overlap by one layer, so that laid end to end they give
    every vertex and every triangle of a grid of nz >= 2 layers."""
    assert nz >= 2 and n >= 2
    out, z0 = [], 0
    while True:
        z1 = min(z0 + n, nz - 1)
        out.append((z0, z1))
        if z1 == nz - 1:
            return out
        z0 = z1 - 1


def checkerboard_counts(nx, ny, nz):
    """(V, Q) of f = (-1)^(x + y + z) at level 0: every cell is active, every edge with four cells around it gives a quad."""
    a, b, c = max(nx - 1, 0), max(ny - 1, 0), max(nz - 1, 0)
    a2, b2, c2 = max(nx - 2, 0), max(ny - 2, 0), max(nz - 2, 0)
    return a * b * c, a * b2 * c2 + a2 * b * c2 + a2 * b2 * c


def per_block_counts(ins, block=256):
    """(vertices, quads) per block of `block` words of 64 samples along x, words numbered (z ny + y) W + w as the device
    numbers them, of a bool grid held in memory."""
    nz, ny, nx = ins.shape
    W = (nx + 63) // 64

    def blocks(per_sample):   # [nz, ny, <= nx]
        full = np.zeros((nz, ny, W * 64), np.int64)
        full[:per_sample.shape[0], :per_sample.shape[1], :per_sample.shape[2]] = per_sample
        words = full.reshape(-1, 64).sum(axis=1)
        pad = np.zeros(-(-len(words) // block) * block, np.int64)
        pad[:len(words)] = words
        return pad.reshape(-1, block).sum(axis=1)
    return blocks(active_cells(ins)), blocks(quad_edges(ins).sum(axis=3))


# ---- grids that are strided views of a 1-D array: f(x, y, z) = base[sx x + s1 y + s2 z] ------------------------------------

def row_tables(ins, nx, sx, s1, s2):
    """A row (y, z) of such a grid is decided by its offset o = s1 y + s2 z alone.  Per offset, from ins = (base < level): the
    active cells of the cell row, the crossing edges along x (0 <= x <= nx - 2), along y and along z (1 <= x <= nx - 2), as if the
    rows y + 1 and z + 1 existed (row_counts leaves out what the borders of the grid do not have)."""
    ins = np.asarray(ins, bool)
    n = len(ins) - sx * (nx - 1)
    assert n > 0 and nx >= 2
    pad = np.concatenate([ins, np.zeros(s1 + s2, bool)])

    def rows(o):
        return np.lib.stride_tricks.as_strided(pad[o:], (n, nx), (pad.strides[0], sx * pad.strides[0]), writeable=False)
    r00, r10, r01, r11 = rows(0), rows(s1), rows(s2), rows(s1 + s2)
    corners = [r[:, a:a + nx - 1] for r in (r00, r10, r01, r11) for a in (0, 1)]
    active = (np.logical_or.reduce(corners) & ~np.logical_and.reduce(corners)).sum(axis=1)
    qx = (r00[:, :-1] != r00[:, 1:]).sum(axis=1)
    qy = (r00[:, 1:-1] != r10[:, 1:-1]).sum(axis=1)
    qz = (r00[:, 1:-1] != r01[:, 1:-1]).sum(axis=1)
    return active, qx, qy, qz


def row_counts(tables, ny, nz, s1, s2, k0, k1):
    """(vertices, quads) int64 [k1 - k0, ny] of the rows (y, z), k0 <= z < k1, of such a grid, from its row_tables."""
    active, qx, qy, qz = tables
    j, k = np.arange(ny)[None, :], np.arange(k0, k1)[:, None]
    o = s1 * j + s2 * k
    jc, kc = j + 1 < ny, k + 1 < nz
    ji, ki = jc & (j >= 1), kc & (k >= 1)
    return active[o] * (jc & kc), qx[o] * (ji & ki) + qy[o] * (jc & ki) + qz[o] * (kc & ji)


def grid_counts(tables, ny, nz, s1, s2, block=256, layers=64, workers=1):
    """(vertices per cell layer [nz - 1], quads per sample layer [nz], vertices per block, quads per block) of such a grid with
    nx <= 64 (a word per row: block b holds the rows b block .. b block + block - 1 of (z ny + y)), a few layers at a time."""
    n_blocks = -(-ny * nz // block)
    v_layers, q_layers = np.zeros(nz, np.int64), np.zeros(nz, np.int64)
    v_blocks, q_blocks = np.zeros(n_blocks, np.int64), np.zeros(n_blocks, np.int64)

    def one(k0, k1):
        v, q = row_counts(tables, ny, nz, s1, s2, k0, k1)
        b = np.arange(k0 * ny, k1 * ny) // block
        first = int(b[0])
        # (float64 sums of small integers: exact)
        return v.sum(axis=1), q.sum(axis=1), first, [np.bincount(b - first, weights=rows.reshape(-1)).astype(np.int64) for rows in (v, q)]
    chunks = [(k0, min(k0 + layers, nz)) for k0 in range(0, nz, layers)]
    for (k0, k1), (v, q, first, parts) in zip(chunks, each(one, chunks, workers)):
        v_layers[k0:k1], q_layers[k0:k1] = v, q
        for part, out in zip(parts, (v_blocks, q_blocks)):   # (neighbouring chunks may share a block)
            out[first:first + len(part)] += part
    return v_layers[:nz - 1], q_layers, v_blocks, q_blocks


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
