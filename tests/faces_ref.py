"""The numpy restatement of o2v_hip_faces_count / _write (include/o2v_hip.h): the exposed faces of a
dense grid's solid voxels as coloured quads - one per face, or one per run of faces of one colour -, a scalar triple-loop
restatement of the header to check the vectorised one against, quads back to unit faces, and parsers of the mesh files
dense.save_mesh writes.

Grids are numpy arrays indexed [z, y, x], as the tensors are.  Nothing here imports the code under test."""
import struct

import numpy as np

from tests import gather_ref

F = np.float32
U8, BITS, F32_BELOW = gather_ref.U8, gather_ref.BITS, gather_ref.F32_BELOW
NONE, RUNS = 0, 1                              # O2V_HIP_FACES_MERGE_*
STEP = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))   # direction d -> (dx, dy, dz)

solid = gather_ref.solid


def voxel_colors(grid, fmt, S, argb=0xFFFFFFFF, colors=None, palette=None):
    """uint32 [z, y, x]: the colour of every voxel (looked at where it is solid): argb, colors[z, y, x] or palette[grid[z, y, x]]."""
    assert colors is None or palette is None
    if colors is not None:
        assert np.asarray(colors).shape == S.shape
        return (np.asarray(colors).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    if palette is not None:
        assert fmt == U8 and len(palette) == 256
        return (np.asarray(palette, np.int64) & 0xFFFFFFFF).astype(np.uint32)[np.asarray(grid).astype(np.uint8)]
    return np.full(S.shape, argb & 0xFFFFFFFF, np.uint32)


def shifted(A, d, fill):
    """A at the neighbour in direction d: out[z, y, x] = A[z + dz, y + dy, x + dx], `fill` outside the box."""
    dx, dy, dz = STEP[d]
    out = np.full_like(A, fill)
    nz, ny, nx = A.shape
    src = (slice(max(dz, 0), nz + min(dz, 0)), slice(max(dy, 0), ny + min(dy, 0)), slice(max(dx, 0), nx + min(dx, 0)))
    dst = (slice(max(-dz, 0), nz + min(-dz, 0)), slice(max(-dy, 0), ny + min(-dy, 0)), slice(max(-dx, 0), nx + min(-dx, 0)))
    out[dst] = A[src]
    return out


def exposed(S):
    """The six masks: exposed(S)[d][z, y, x] - voxel (x, y, z) is solid and its neighbour in direction d is not."""
    return [S & ~shifted(S, d, False) for d in range(6)]


def unit_faces(S, C):
    """int64 [n, 5], sorted: (x, y, z, d, argb) of every exposed face with its voxel's colour."""
    rows = []
    for d, E in enumerate(exposed(S)):
        z, y, x = np.nonzero(E)
        rows.append(np.stack([x, y, z, np.full(len(x), d), C[z, y, x].astype(np.int64)], axis=1).astype(np.int64))
    return sort_rows(np.concatenate(rows))


def sort_rows(a):
    a = np.asarray(a, np.int64).reshape(-1, 5)
    return a[np.lexsort(a.T[::-1])]


def runs(S, C, merge):
    """int64 [Q, 6] in the contract's order: (x, y, z, d, length, argb) of every quad's first face."""
    nz, ny, nx = S.shape
    out = []
    for d, E in enumerate(exposed(S)):
        axis, back = (2, 0) if d >= 2 else (1, 2)                # the run axis of the array; the direction that steps back along it
        if merge == RUNS:
            cont = E & shifted(E, back, False) & (C == shifted(C, back, 0))
            cont &= np.arange(S.shape[axis]).reshape([-1 if a == axis else 1 for a in range(3)]) > 0   # (nothing before the first)
        else:
            cont = np.zeros_like(E)
        start = E & ~cont
        # the length of a run: to the next position behind its start that does not continue (or the end of the axis)
        n = S.shape[axis]
        idx = np.arange(n).reshape([-1 if a == axis else 1 for a in range(3)])
        stop = np.where(cont, n, idx) + np.zeros(S.shape, np.int64)
        stop = np.flip(np.minimum.accumulate(np.flip(stop, axis), axis), axis)       # min over j >= i
        after = np.concatenate([np.delete(stop, 0, axis), np.full_like(np.take(stop, [0], axis), n)], axis)   # min over j > i
        z, y, x = np.nonzero(start)
        length = after[z, y, x] - (x if axis == 2 else y)
        out.append(np.stack([x, y, z, np.full(len(x), d), length, C[z, y, x].astype(np.int64)], axis=1).astype(np.int64))
    q = np.concatenate(out)
    key = ((q[:, 2] * ny + q[:, 1]) * 6 + q[:, 3]) * nx + q[:, 0]
    assert len(np.unique(key)) == len(key)
    return q[np.argsort(key, kind="stable")]


def geometry(q, origin=(0, 0, 0)):
    """(positions float32 [4Q, 3], faces int32 [2Q, 3]) of runs q as the header lays them out."""
    Q = len(q)
    lo = q[:, :3] + np.asarray(origin, np.int64)
    hi = lo + 1
    along = np.where(q[:, 3] >= 2, 0, 1)
    hi[np.arange(Q), along] = lo[np.arange(Q), along] + q[:, 4]
    a, s = q[:, 3] >> 1, q[:, 3] & 1
    u, v = (a + 1) % 3, (a + 2) % 3
    r = np.arange(Q)
    pos = np.zeros((Q, 4, 3), np.int64)
    first = np.array([[0, 1, 1, 0], [0, 0, 1, 1]])     # s = 1: (u0,v0) (u1,v0) (u1,v1) (u0,v1): u takes hi at corners 1, 2; v at 2, 3
    for k in range(4):
        ku = np.where(s == 1, first[0][k], first[1][k])
        kv = np.where(s == 1, first[1][k], first[0][k])
        pos[r, k, a] = lo[r, a] + s
        pos[r, k, u] = np.where(ku == 1, hi[r, u], lo[r, u])
        pos[r, k, v] = np.where(kv == 1, hi[r, v], lo[r, v])
    base = 4 * np.arange(Q, dtype=np.int64)[:, None]
    faces = np.concatenate([base + [0, 1, 2], base + [0, 2, 3]], axis=1).reshape(-1, 3)
    return pos.reshape(-1, 3).astype(F), faces.astype(np.int32)


def quads(grid, fmt, level=None, origin=(0, 0, 0), merge=RUNS, argb=0xFFFFFFFF, colors=None, palette=None):
    """(positions float32 [4Q, 3], faces int32 [2Q, 3], quad_argb uint32 [Q]): what o2v_hip_faces_write fills."""
    S = solid(grid, fmt, level)
    C = voxel_colors(grid, fmt, S, argb, colors, palette)
    q = runs(S, C, merge)
    positions, faces = geometry(q, origin)
    return positions, faces, q[:, 5].astype(np.uint32)


def count(grid, fmt, level=None, merge=NONE, argb=0xFFFFFFFF, colors=None, palette=None):
    S = solid(grid, fmt, level)
    return len(runs(S, voxel_colors(grid, fmt, S, argb, colors, palette), merge))


def quads_scalar(grid, fmt, level=None, origin=(0, 0, 0), merge=RUNS, argb=0xFFFFFFFF, colors=None, palette=None):
    """The same by loops that restate the header word for word (the check of `quads`)."""
    g = np.asarray(grid)
    nz, ny = g.shape[:2]
    nx = g.shape[2] * 32 if fmt == BITS else g.shape[2]

    def is_solid(x, y, z):
        if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz):
            return False                                        # everything outside the box is empty
        if fmt == U8:
            return int(g[z, y, x]) != 0
        if fmt == BITS:
            return (int(g[z, y, x // 32]) & 0xFFFFFFFF) >> (x % 32) & 1 == 1
        v = F(g[z, y, x])
        return bool(v < F(level)) if not np.isnan(v) else False

    def color(x, y, z):
        if colors is not None:
            return int(colors[z, y, x]) & 0xFFFFFFFF
        if palette is not None:
            return int(palette[int(g[z, y, x])]) & 0xFFFFFFFF
        return argb & 0xFFFFFFFF

    def is_exposed(x, y, z, d):
        return is_solid(x, y, z) and not is_solid(x + STEP[d][0], y + STEP[d][1], z + STEP[d][2])

    def same_run(x, y, z, d, x2, y2, z2):
        return merge == RUNS and is_exposed(x, y, z, d) and is_exposed(x2, y2, z2, d) and color(x, y, z) == color(x2, y2, z2)

    positions, argbs = [], []
    for z in range(nz):
        for y in range(ny):
            for d in range(6):
                rx, ry = (1, 0) if d >= 2 else (0, 1)           # directions 2 .. 5 run along x, 0 and 1 along y
                for x in range(nx):
                    if not is_exposed(x, y, z, d) or same_run(x - rx, y - ry, z, d, x, y, z):
                        continue
                    n = 1
                    while same_run(x + (n - 1) * rx, y + (n - 1) * ry, z, d, x + n * rx, y + n * ry, z):
                        n += 1
                    lo = [origin[0] + x, origin[1] + y, origin[2] + z]
                    hi = [lo[0] + (n if rx else 1), lo[1] + (n if ry else 1), lo[2] + 1]
                    a, s = d >> 1, d & 1
                    u, v = (a + 1) % 3, (a + 2) % 3
                    corners = ((0, 0), (1, 0), (1, 1), (0, 1)) if s == 1 else ((0, 0), (0, 1), (1, 1), (1, 0))
                    for cu, cv in corners:
                        p = [0, 0, 0]
                        p[a] = lo[a] + s
                        p[u] = hi[u] if cu else lo[u]
                        p[v] = hi[v] if cv else lo[v]
                        positions.append(p)
                    argbs.append(color(x, y, z))
    Q = len(argbs)
    faces = [[4 * q + i for i in tri] for q in range(Q) for tri in ((0, 1, 2), (0, 2, 3))]
    return np.array(positions, F).reshape(-1, 3), np.array(faces, np.int32).reshape(-1, 3), np.array(argbs, np.uint32)


# ---- quads back to what they cover ---------------------------------------------------------------------------------------------------

def quad_boxes(positions):
    """(d int64 [Q], lo int64 [Q, 3], hi int64 [Q, 3], normal float64 [Q, 2, 3]): direction, lattice bounds and the two triangles'
    normals (cross products of their corners) of every quad of positions [4Q, 3]."""
    p = np.asarray(positions, np.float64).reshape(-1, 4, 3)
    n0 = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n1 = np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 0])
    a = np.abs(n0).argmax(axis=1)
    s = (n0[np.arange(len(p)), a] > 0).astype(np.int64)
    return 2 * a + s, p.min(axis=1).astype(np.int64), p.max(axis=1).astype(np.int64), np.stack([n0, n1], axis=1)


def rasterize(positions, quad_argb, origin=(0, 0, 0)):
    """int64 [n, 5], sorted: the (x, y, z, d, argb) unit faces the quads cover, voxel coordinates relative to origin; a face that
    two quads cover appears twice."""
    d, lo, hi, _ = quad_boxes(positions)
    if not len(d):
        return np.zeros((0, 5), np.int64)
    a, s = d >> 1, d & 1
    r = np.arange(len(d))
    assert np.array_equal(lo[r, a], hi[r, a])                                         # flat along its axis
    lo = lo.copy()
    lo[r, a] -= s                                                                       # the voxel the face belongs to
    ext = hi - lo
    ext[r, a] = 1
    n = ext.prod(axis=1)
    which = np.repeat(r, n)
    k = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)                            # the k-th face of its quad
    e = ext[which]
    off = np.stack([k % e[:, 0], k // e[:, 0] % e[:, 1], k // (e[:, 0] * e[:, 1])], axis=1)
    xyz = lo[which] + off - np.asarray(origin, np.int64)
    return sort_rows(np.concatenate([xyz, d[which, None], np.asarray(quad_argb).astype(np.int64)[which, None] & 0xFFFFFFFF], axis=1))


def order_keys(positions, dims, origin=(0, 0, 0)):
    """int64 [Q]: the order key ((z * ny + y) * 6 + d) * nx + x of every quad's first face."""
    d, lo, _, _ = quad_boxes(positions)
    lo = lo - np.asarray(origin, np.int64)
    lo[np.arange(len(d)), d >> 1] -= d & 1
    return ((lo[:, 2] * dims[1] + lo[:, 1]) * 6 + d) * dims[0] + lo[:, 0]


# ---- the mesh files of dense.save_mesh ---------------------------------------------------------------------------------------------

def parse_stl(data):
    """(normals float32 [T, 3], vertices float32 [T, 3, 3]) of a binary STL."""
    n = struct.unpack_from("<I", data, 80)[0]
    assert len(data) == 84 + 50 * n
    rec = np.frombuffer(data, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]), offset=84, count=n)
    return rec["n"].copy(), rec["v"].copy()


def parse_ply(data):
    """(positions float32 [V, 3], rgba uint8 [V, 4] or None, faces int32 [T, 3]) of a binary little-endian PLY of triangles."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode().split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    nv = int([ln for ln in lines if ln.startswith("element vertex ")][0].split()[2])
    nf = int([ln for ln in lines if ln.startswith("element face ")][0].split()[2])
    props = [ln for ln in lines if ln.startswith("property ")]
    colored = "property uchar red" in props
    assert props == (["property float x", "property float y", "property float z"] +
                     (["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"] if colored else []) +
                     ["property list uchar int vertex_indices"])
    vt = np.dtype([("p", "<f4", 3)] + ([("c", "u1", 4)] if colored else []))
    ft = np.dtype([("n", "u1"), ("i", "<i4", 3)])
    assert len(data) == end + nv * vt.itemsize + nf * ft.itemsize
    v = np.frombuffer(data, dtype=vt, offset=end, count=nv)
    f = np.frombuffer(data, dtype=ft, offset=end + nv * vt.itemsize, count=nf)
    assert (f["n"] == 3).all()
    return v["p"].copy(), (v["c"].copy() if colored else None), f["i"].copy()


def parse_obj(obj_text, mtl_text=None):
    """(positions float32 [V, 3], faces int32 [T, 3] 0-based, material name per face, {material: (r, g, b) float32 Kd})."""
    positions, faces, names, current = [], [], [], None
    for ln in obj_text.split("\n"):
        t = ln.split()
        if not t:
            continue
        if t[0] == "v":
            positions.append([F(x) for x in t[1:4]])
        elif t[0] == "usemtl":
            current = t[1]
        elif t[0] == "f":
            assert len(t) == 4
            faces.append([int(x.split("/")[0]) - 1 for x in t[1:]])
            names.append(current)
    kd, name = {}, None
    for ln in (mtl_text or "").split("\n"):
        t = ln.split()
        if t and t[0] == "newmtl":
            name = t[1]
        elif t and t[0] == "Kd":
            kd[name] = tuple(F(x) for x in t[1:4])
    return np.array(positions, F).reshape(-1, 3), np.array(faces, np.int32).reshape(-1, 3), names, kd
