"""The numpy reference of o2v_hip_label_stats (include/o2v_hip.h): per value 0 ... n of a label grid a row of
17 int64 - count, inclusive box, coordinate sums, second moments, faces.  label_stats sorts the voxels by label and reduces the
segments with np.add.reduceat / minimum.reduceat on int64 (no float anywhere, no bincount(weights=)); label_stats_loop is the
definition as a scalar loop; box_row gives the closed forms of a one-label box in Python ints."""
import numpy as np

BOX, SUMS, MOMENTS, FACES = 1, 2, 4, 8
ALL = BOX | SUMS | MOMENTS | FACES
COLUMNS = 17
EMPTY_MIN, EMPTY_MAX = 2 ** 31 - 1, -1
MAX_EXTENT, MAX_VOXELS = 65536, 2 ** 31 - 1


def face_counts(g):
    """int64 [z, y, x]: per voxel the number of its six neighbours whose value differs from its own; a neighbour outside the box
    differs."""
    g = np.asarray(g)
    f = np.zeros(g.shape, np.int64)
    for axis in range(3):
        n = g.shape[axis]
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        lo, hi = tuple(lo), tuple(hi)
        d = (g[lo] != g[hi]).astype(np.int64)
        f[lo] += d
        f[hi] += d
        first = [slice(None)] * 3
        last = [slice(None)] * 3
        first[axis], last[axis] = slice(0, 1), slice(n - 1, n)
        f[tuple(first)] += 1
        f[tuple(last)] += 1
    return f


def empty_table(n, which):
    t = np.zeros((n + 1, COLUMNS), np.int64)
    if which & BOX:
        t[:, 1:4], t[:, 4:7] = EMPTY_MIN, EMPTY_MAX
    return t


def label_stats(g, n, origin=(0, 0, 0), which=ALL):
    """(table int64 [n + 1, 17], outside) of the grid g [z, y, x] (any integer or bool dtype), whose voxel (0, 0, 0) is origin
    (x, y, z)."""
    g = np.asarray(g)
    v = g.astype(np.int64).reshape(-1)
    table = empty_table(n, which)
    inside = (v >= 0) & (v <= n)
    outside = int(v.size - inside.sum())
    if not inside.any():
        return table, outside
    nz, ny, nx = g.shape
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.int64) + origin[2], np.arange(ny, dtype=np.int64) + origin[1],
                          np.arange(nx, dtype=np.int64) + origin[0], indexing="ij")
    order = np.argsort(v, kind="stable")
    order = order[inside[order]]
    lab = v[order]
    starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
    rows = lab[starts]
    x, y, z = x.reshape(-1)[order], y.reshape(-1)[order], z.reshape(-1)[order]
    table[rows, 0] = np.add.reduceat(np.ones(lab.size, np.int64), starts)
    if which & BOX:
        for k, c in enumerate((x, y, z)):
            table[rows, 1 + k] = np.minimum.reduceat(c, starts)
            table[rows, 4 + k] = np.maximum.reduceat(c, starts)
    if which & SUMS:
        for k, c in enumerate((x, y, z)):
            table[rows, 7 + k] = np.add.reduceat(c, starts)
    if which & MOMENTS:
        for k, c in enumerate((x * x, y * y, z * z, x * y, x * z, y * z)):
            table[rows, 10 + k] = np.add.reduceat(c, starts)
    if which & FACES:
        table[rows, 16] = np.add.reduceat(face_counts(g).reshape(-1)[order], starts)
    return table, outside


def label_stats_loop(g, n, origin=(0, 0, 0), which=ALL):
    """The definition, voxel by voxel, in Python ints."""
    g = np.asarray(g)
    nz, ny, nx = g.shape
    t = [[0] * COLUMNS for _ in range(n + 1)]
    if which & BOX:
        for r in t:
            r[1:4], r[4:7] = [EMPTY_MIN] * 3, [EMPTY_MAX] * 3
    outside = 0
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                L = int(g[k, j, i])
                if L < 0 or L > n:
                    outside += 1
                    continue
                r = t[L]
                p = (i + origin[0], j + origin[1], k + origin[2])
                r[0] += 1
                if which & BOX:
                    for a in range(3):
                        r[1 + a], r[4 + a] = min(r[1 + a], p[a]), max(r[4 + a], p[a])
                if which & SUMS:
                    for a in range(3):
                        r[7 + a] += p[a]
                if which & MOMENTS:
                    for c, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
                        r[10 + c] += p[a] * p[b]
                if which & FACES:
                    for di, dj, dk in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
                        a, b, c = i + di, j + dj, k + dk
                        if not (0 <= a < nx and 0 <= b < ny and 0 <= c < nz) or int(g[c, b, a]) != L:
                            r[16] += 1
    return np.array(t, dtype=np.int64), outside


def sum_range(o, a):
    """sum of v for v = o ... o + a - 1."""
    return a * o + a * (a - 1) // 2


def sum_squares(o, a):
    """sum of v^2 for v = o ... o + a - 1."""
    return a * o * o + o * a * (a - 1) + (a - 1) * a * (2 * a - 1) // 6


def box_row(dims, origin, which=ALL):
    """The row, as 17 Python ints, of a grid (nx, ny, nz) = dims at origin that holds one value everywhere."""
    (a, b, c), (ox, oy, oz) = dims, origin
    r = [0] * COLUMNS
    r[0] = a * b * c
    if which & BOX:
        r[1:7] = [ox, oy, oz, ox + a - 1, oy + b - 1, oz + c - 1]
    sx, sy, sz = sum_range(ox, a), sum_range(oy, b), sum_range(oz, c)
    if which & SUMS:
        r[7:10] = [b * c * sx, a * c * sy, a * b * sz]
    if which & MOMENTS:
        r[10:16] = [b * c * sum_squares(ox, a), a * c * sum_squares(oy, b), a * b * sum_squares(oz, c), c * sx * sy, b * sx * sz, a * sy * sz]
    if which & FACES:
        r[16] = 2 * (a * b + b * c + a * c)
    return r


def largest_sum():
    """The bound of include/o2v_hip.h: the largest value a column can reach under the limits."""
    return (MAX_EXTENT - 1) ** 2 * MAX_VOXELS


def blobs(rng, dims, n, outside=0.0):
    """int32 [z, y, x]: labels 0 ... n in coherent blobs (the nearest of a few random seeds per label, in a warped metric), as
    labelled parts look; `outside`: the share of voxels overwritten by -1, n + 1, INT32_MIN or INT32_MAX."""
    nx, ny, nz = dims
    k = max(1, min(n + 1, 12))
    seeds = rng.random((k, 3)) * np.array([nz, ny, nx])
    labels = rng.choice(n + 1, size=k, replace=False) if n + 1 >= k else rng.integers(0, n + 1, k)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = np.stack([(z - s[0]) ** 2 + (y - s[1]) ** 2 + 0.3 * (x - s[2]) ** 2 for s in seeds])
    g = labels[np.argmin(d, axis=0)].astype(np.int32)
    speck = rng.random(g.shape) < 0.03   # single voxels of any label: runs of length one
    g[speck] = rng.integers(0, n + 1, int(speck.sum()))
    if outside:
        bad = rng.random(g.shape) < outside
        g[bad] = rng.choice(np.array([-1, n + 1, -2 ** 31, 2 ** 31 - 1], np.int64), int(bad.sum())).astype(np.int32)
    return g
