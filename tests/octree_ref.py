"""The numpy reference of the sparse voxel octree (include/o2v_hip.h), for tests/test_host_octree.py and
tests/octree_cases.py.

build() restates the definition with arrays: per level the solid voxels of every touched cell by reshape(...).sum over 2^3 blocks
(non-empty: above 0, full: 8^(D - l)), the stored cells from the parents' stored masks, the node order by a Morton sort.  The arrays
are box-sized - the touched cells of each level, padded to even alignment -, so the depth costs nothing.  build_recursive() is a
second construction: a scalar breadth-first walk that counts the voxels of each child cube in the box and appends the children in
(parent, octant) order.  lookup() is the descent as a scalar loop.  Grids are [z, y, x]; origins and coordinates are (x, y, z)."""
import numpy as np

BIT = 1 << np.arange(8)


def depth_of(origin, dims):
    """the smallest D >= 1 with origin + dims <= 2^D on every axis (dims: (nx, ny, nz))"""
    top = max(o + n for o, n in zip(origin, dims))
    return max(1, int(top - 1).bit_length())


def morton(x, y, z):
    x, y, z = (np.asarray(v, np.uint64) for v in (x, y, z))
    key = np.zeros(x.shape, np.uint64)
    for b in range(17):
        s = np.uint64(b)
        one = np.uint64(1)
        key |= (((x >> s) & one) | (((y >> s) & one) << one) | (((z >> s) & one) << np.uint64(2))) << np.uint64(3 * b)
    return key


def popcount8(m):
    return np.unpackbits(np.asarray(m, np.uint8)[..., None], axis=-1).sum(-1).astype(np.int64)


def pyramid(g, origin, D):
    """Per level l < D the masks of the cells the box touches: a list of dict(valid, full uint8 [kz, ky, kx]; lo: the first cell (z, y,
    x); children: the solid voxels per cell of level l + 1, padded to even alignment; child_voxels; pad)."""
    g = np.asarray(g) != 0
    # bottom up: per level l < D the touched cells' masks, from the counts of level l + 1 padded to even alignment
    cnt, lo = g.astype(np.int64), np.array(origin[::-1], np.int64)   # (z, y, x)
    lv = [None] * D
    for l in range(D - 1, -1, -1):   # noqa: E741
        hi = lo + np.array(cnt.shape)
        pl, ph = lo & 1, hi & 1
        c = np.pad(cnt, list(zip(pl, ph)))
        kz, ky, kx = (s // 2 for s in c.shape)
        blocks = c.reshape(kz, 2, ky, 2, kx, 2).transpose(0, 2, 4, 1, 3, 5).reshape(kz, ky, kx, 8)   # the last index is dx + 2 dy + 4 dz
        child_voxels = 8 ** (D - l - 1)
        lo = (lo - pl) // 2
        lv[l] = dict(valid=((blocks > 0) * BIT).sum(-1).astype(np.uint8), full=((blocks == child_voxels) * BIT).sum(-1).astype(np.uint8), lo=lo,
                     children=c, child_voxels=child_voxels, pad=(pl, ph))
        cnt = blocks.sum(-1)
    assert cnt.shape == (1, 1, 1) and not lo.any(), "the root cube holds the box"
    return lv


def build(g, origin=(0, 0, 0), depth=None, collapse=True):
    """dict(valid, full uint8 [N]; first_child int32 [N]; coords int32 [N, 3]; level_counts list [D]; voxels_listed; depth)"""
    g = np.asarray(g) != 0
    nz, ny, nx = g.shape
    D = depth_of(origin, (nx, ny, nz)) if depth is None else depth
    assert 1 <= D <= 16 and all(o + n <= 2 ** D for o, n in zip(origin, (nx, ny, nz)))
    lv = pyramid(g, origin, D)
    # top down: the stored cells of each level, from the parents' stored masks
    stored = np.ones((1, 1, 1), bool)
    nodes = []
    for l in range(D):   # noqa: E741
        L = lv[l]
        k, j, i = np.nonzero(stored)
        cz, cy, cx = k + L["lo"][0], j + L["lo"][1], i + L["lo"][2]
        order = np.argsort(morton(cx, cy, cz), kind="stable")
        k, j, i, cz, cy, cx = (a[order] for a in (k, j, i, cz, cy, cx))
        side = 2 ** (D - l)
        nodes.append(dict(valid=L["valid"][k, j, i], full=L["full"][k, j, i], coords=np.stack([cx, cy, cz], 1) * side))
        if l + 1 < D:
            c = L["children"]
            child = np.repeat(np.repeat(np.repeat(stored, 2, 0), 2, 1), 2, 2) & (c > 0)
            if collapse:
                child &= c != L["child_voxels"]
            pl, ph = L["pad"]
            stored = child[pl[0]:child.shape[0] - ph[0], pl[1]:child.shape[1] - ph[1], pl[2]:child.shape[2] - ph[2]]
    counts = [len(n["valid"]) for n in nodes]
    offsets = np.concatenate([[0], np.cumsum(counts)])
    first = []
    for l, n in enumerate(nodes):   # noqa: E741
        if l + 1 < D:
            m = n["valid"] & ~n["full"] if collapse else n["valid"]
            ex = np.cumsum(popcount8(m)) - popcount8(m)
            first.append(np.where(m != 0, offsets[l + 1] + ex, -1))
        else:
            pc = popcount8(n["valid"])
            first.append(np.cumsum(pc) - pc)
            listed = int(pc.sum())
    return dict(valid=np.concatenate([n["valid"] for n in nodes]).astype(np.uint8), full=np.concatenate([n["full"] for n in nodes]).astype(np.uint8),
                first_child=np.concatenate(first).astype(np.int32), coords=np.concatenate([n["coords"] for n in nodes]).astype(np.int32),
                level_counts=counts, voxels_listed=listed, depth=D, collapsed=bool(collapse))


def build_recursive(g, origin=(0, 0, 0), depth=None, collapse=True):
    """The same tree by a scalar walk: level by level, each node's children appended in octant order."""
    g = np.asarray(g) != 0
    nz, ny, nx = g.shape
    D = depth_of(origin, (nx, ny, nz)) if depth is None else depth
    ox, oy, oz = origin

    def solid_in(x, y, z, s):   # the solid voxels of the cube [x, x + s) x ... : its part inside the box
        x0, x1, y0, y1, z0, z1 = max(x - ox, 0), min(x + s - ox, nx), max(y - oy, 0), min(y + s - oy, ny), max(z - oz, 0), min(z + s - oz, nz)
        return int(g[z0:z1, y0:y1, x0:x1].sum()) if x0 < x1 and y0 < y1 and z0 < z1 else 0

    level = [(0, 0, 0)]
    valid, full, first, coords, counts = [], [], [], [], []
    n_before, listed = 0, 0
    for l in range(D):   # noqa: E741
        half = 2 ** (D - l - 1)
        nxt = []
        counts.append(len(level))
        n_next_first = n_before + len(level)
        for (x, y, z) in level:
            v = f = 0
            for o in range(8):
                n = solid_in(x + (o & 1) * half, y + ((o >> 1) & 1) * half, z + (o >> 2) * half, half)
                v |= (n > 0) << o
                f |= (n == half ** 3) << o
            valid.append(v), full.append(f), coords.append((x, y, z))
            if l + 1 == D:
                first.append(listed)
                listed += bin(v).count("1")
                continue
            m = v & ~f if collapse else v
            first.append(n_next_first + len(nxt) if m else -1)
            nxt += [(x + (o & 1) * half, y + ((o >> 1) & 1) * half, z + (o >> 2) * half) for o in range(8) if (m >> o) & 1]
        n_before += len(level)
        level = nxt
    return dict(valid=np.array(valid, np.uint8), full=np.array(full, np.uint8), first_child=np.array(first, np.int32),
                coords=np.array(coords, np.int32).reshape(-1, 3), level_counts=counts, voxels_listed=listed, depth=D, collapsed=bool(collapse))


def lookup_one(t, x, y, z):
    """the descent: (solid, level, node, voxel_index)"""
    D, N = t["depth"], len(t["valid"])
    if not (0 <= x < 2 ** D and 0 <= y < 2 ** D and 0 <= z < 2 ** D):
        return (0, -1, -1, -1)
    i = 0
    for l in range(D):   # noqa: E741
        s = D - 1 - l
        o = ((x >> s) & 1) | ((y >> s) & 1) << 1 | ((z >> s) & 1) << 2
        v, f = int(t["valid"][i]), int(t["full"][i])
        if not (v >> o) & 1:
            return (0, l, i, -1)
        if l == D - 1:
            return (1, l, i, int(t["first_child"][i]) + bin(v & ((1 << o) - 1)).count("1"))
        if t["collapsed"] and (f >> o) & 1:
            return (1, l, i, -1)
        m = v & ~f & 255 if t["collapsed"] else v
        fc = int(t["first_child"][i])
        c = fc + bin(m & ((1 << o) - 1)).count("1")
        if fc < 0 or not 0 <= c < N:
            return (0, -2, -1, -1)
        i = c
    raise AssertionError("unreachable")


def lookup(t, points):
    points = np.asarray(points).reshape(-1, 3)
    return np.array([lookup_one(t, int(x), int(y), int(z)) for x, y, z in points], np.int32).reshape(-1, 4)


def to_dense(t, shape, origin=(0, 0, 0)):
    """bool [nz, ny, nx]: the descent's `solid` for every voxel of the box"""
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz) + origin[2], np.arange(ny) + origin[1], np.arange(nx) + origin[0], indexing="ij")
    return lookup(t, np.stack([x, y, z], -1).reshape(-1, 3))[:, 0].reshape(shape).astype(bool)


def same(got, want, what=""):
    """every field of two trees bit for bit"""
    assert got["depth"] == want["depth"] and list(got["level_counts"]) == list(want["level_counts"]), (what, got["depth"], got["level_counts"], want["level_counts"])
    assert got["voxels_listed"] == want["voxels_listed"], (what, "voxels_listed", got["voxels_listed"], want["voxels_listed"])
    for k in ("valid", "full", "first_child", "coords"):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, a.shape, b.dtype, b.shape)
        bad = np.argwhere(a != b)
        assert not len(bad), (what, k, len(bad), "differ, the first at", bad[0].tolist(), a[tuple(bad[0])].tolist(), b[tuple(bad[0])].tolist())


def solid_box_counts(origin, dims, depth=None, collapse=True):
    """(level_counts, voxels_listed) of an all-solid box in Python ints: per level the touched cells, less (collapsed) those wholly
    inside the box; the root is always there."""
    D = depth_of(origin, dims) if depth is None else depth
    counts, full_last = [], 0
    for l in range(D):   # noqa: E741
        s = 2 ** (D - l)
        touched = inside = 1
        for o, n in zip(origin, dims):
            touched *= (o + n - 1) // s - o // s + 1
            inside *= max(0, (o + n) // s - -(-o // s))
        counts.append(1 if l == 0 else touched - inside if collapse else touched)
        full_last = inside
    voxels = dims[0] * dims[1] * dims[2]
    return counts, voxels if D == 1 or not collapse else voxels - 8 * full_last


# ---- generators -------------------------------------------------------------------------------------------------------------------

def blobs(rng, dims, p=0.5, noise=0.02):
    """bool [nz, ny, nx]: coarse random blocks of 4^3 (so that cells are full) with a sprinkle of flipped voxels"""
    nx, ny, nz = dims
    coarse = rng.random((-(-nz // 4), -(-ny // 4), -(-nx // 4))) < p
    g = np.repeat(np.repeat(np.repeat(coarse, 4, 0), 4, 1), 4, 2)[:nz, :ny, :nx]
    return g ^ (rng.random(g.shape) < noise)


def ball(n=64, c=31.5, r2=400):
    z, y, x = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    return (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2 <= r2


def checkerboard(n=16):
    z, y, x = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    return (x + y + z) % 2 == 0


def box(dims):
    return np.ones(dims[::-1], bool)
