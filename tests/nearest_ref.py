"""numpy references for o2v_hip_nearest_dense on seed grids [z, y, x] (bool): a brute force over every
seed for small boxes, and the separable feature transform - x by two scans, y and z by the integer lower envelope of
tests/distance_ref.py carrying the vertex -, vectorised over the lines, for everything else.  The index of a seed is
(z * ny + y) * nx + x; among the seeds nearest to a voxel the reference takes the smallest.

ties="high" lets the larger coordinate win in every pass instead.  It is wrong on purpose and exists only so that a test can
show that a grid tells the two rules apart."""
import numpy as np

from tests.distance_ref import INF


def brute_nearest(seed, chunk=2048):
    """(nearest int32, d2 int32) [z, y, x], in int64: per voxel the first seed in (z, y, x) order at the least squared distance;
    -1 and INF without seeds."""
    seed = np.asarray(seed, bool)
    nz, ny, nx = seed.shape
    seeds = np.argwhere(seed).astype(np.int64)             # ascending (z, y, x): argmin takes the first of equal minima
    if len(seeds) == 0:
        return np.full(seed.shape, -1, np.int32), np.full(seed.shape, INF, np.int32)
    index = (seeds[:, 0] * ny + seeds[:, 1]) * nx + seeds[:, 2]
    vox = np.indices(seed.shape).reshape(3, -1).T.astype(np.int64)
    near = np.empty(len(vox), np.int64)
    d2 = np.empty(len(vox), np.int64)
    for i in range(0, len(vox), chunk):
        d = ((vox[i:i + chunk, None, :] - seeds[None, :, :]) ** 2).sum(-1)
        k = d.argmin(1)
        near[i:i + chunk] = index[k]
        d2[i:i + chunk] = d[np.arange(len(k)), k]
    return near.reshape(seed.shape).astype(np.int32), d2.reshape(seed.shape).astype(np.int32)


def tie_share(seed, chunk=2048):
    """The share of the voxels that have more than one nearest seed."""
    seed = np.asarray(seed, bool)
    seeds = np.argwhere(seed).astype(np.int64)
    vox = np.indices(seed.shape).reshape(3, -1).T.astype(np.int64)
    tied = 0
    for i in range(0, len(vox), chunk):
        d = ((vox[i:i + chunk, None, :] - seeds[None, :, :]) ** 2).sum(-1)
        tied += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
    return tied / len(vox)


def d2_of(nearest):
    """int32 [z, y, x]: the squared distance from every voxel to the seed `nearest` names, INF where it is -1."""
    nearest = np.asarray(nearest).astype(np.int64)
    nz, ny, nx = nearest.shape
    z, y, x = np.indices(nearest.shape)
    d = (x - nearest % nx) ** 2 + (y - nearest // nx % ny) ** 2 + (z - nearest // (nx * ny)) ** 2
    return np.where(nearest < 0, INF, d).astype(np.int32)


def _rows(seed, high):
    """The x coordinate of the nearest seed of the row along the last axis (-1 if none); of two equally far the left one,
    the right one with `high`."""
    n = seed.shape[-1]
    idx = np.arange(n, dtype=np.int64)
    big = np.int64(1) << 40
    left = np.maximum.accumulate(np.where(seed, idx, -big), axis=-1)
    right = np.minimum.accumulate(np.where(seed, idx, big)[..., ::-1], axis=-1)[..., ::-1]
    dl, dr = idx - left, right - idx
    fx = np.where((dl < dr) if high else (dl <= dr), left, right)
    return np.where((dl > big // 2) & (dr > big // 2), -1, fx)


def _vertices(f, high):
    """int64 [lines, n]: per position u the vertex v that gives min over v of f[l, v] + (u - v)^2 (-1 on a line without a
    finite f) - the smallest such v, the largest with `high`.  distance_ref.envelope's stacks; `high` pops on equality and
    lets the new parabola take over at ceil(Sep) instead of 1 + floor(Sep)."""
    L, n = f.shape
    rows = np.arange(L)
    s = np.zeros((L, n), np.int64)
    t = np.zeros((L, n), np.int64)
    q = np.full(L, -1, np.int64)
    for u in range(n):
        fu = f[:, u]
        act = fu != INF
        if not act.any():
            continue
        while True:
            qi = np.maximum(q, 0)
            ts, tt = s[rows, qi], t[rows, qi]
            a, b = (tt - ts) ** 2 + f[rows, ts], (tt - u) ** 2 + fu
            pop = act & (q >= 0) & ((a >= b) if high else (a > b))
            if not pop.any():
                break
            q = np.where(pop, q - 1, q)
        empty = act & (q < 0)
        have = act & (q >= 0)
        ts = s[rows, np.maximum(q, 0)]
        den = np.where(have, 2 * (u - ts), 1)
        num = u * u - ts * ts + fu - f[rows, ts]
        w = -((-num) // den) if high else 1 + num // den
        push = have & (w < n)
        q = np.where(push, q + 1, q)
        s[push, q[push]] = u
        t[push, q[push]] = w[push]
        s[empty, 0] = u
        t[empty, 0] = 0
        q[empty] = 0
    v = np.full((L, n), -1, np.int64)
    for u in range(n - 1, -1, -1):
        has = q >= 0
        qi = np.maximum(q, 0)
        v[has, u] = s[rows, qi][has]
        q = q - (has & (t[rows, qi] == u))
    return v


def _pass(f, payloads, high):
    """One envelope pass over lines [lines, n]: (vertex, the new f, the payloads taken from the vertex)."""
    v = _vertices(f, high)
    safe = np.maximum(v, 0)
    pos = np.arange(f.shape[1], dtype=np.int64)
    g = np.where(v >= 0, np.take_along_axis(f, safe, 1) + (pos - v) ** 2, INF)
    return v, g, [np.where(v >= 0, np.take_along_axis(p, safe, 1), -1) for p in payloads]


def separable_nearest(seed, ties="low"):
    """(nearest int32, d2 int32) [z, y, x], equal to brute_nearest with ties="low": x, then y, then z."""
    assert ties in ("low", "high")
    high = ties == "high"
    seed = np.asarray(seed, bool)
    nz, ny, nx = seed.shape
    fx = _rows(seed, high)                                                      # [z, y, x]
    g = np.where(fx >= 0, (np.arange(nx, dtype=np.int64) - fx) ** 2, INF)
    lines_y = lambda a: a.transpose(0, 2, 1).reshape(-1, ny)                    # noqa: E731
    fy, g, (fx,) = _pass(lines_y(g), [lines_y(fx)], high)
    back_y = lambda a: a.reshape(nz, nx, ny).transpose(0, 2, 1)                 # noqa: E731
    lines_z = lambda a: back_y(a).transpose(1, 2, 0).reshape(-1, nz)            # noqa: E731
    fz, g, (fx, fy) = _pass(lines_z(g), [lines_z(fx), lines_z(fy)], high)
    near = np.where(fz >= 0, (fz * ny + fy) * nx + fx, -1)
    back_z = lambda a: np.ascontiguousarray(a.reshape(ny, nx, nz).transpose(2, 0, 1)).astype(np.int32)   # noqa: E731
    return back_z(near), back_z(g)


# ---- seed grids on which many voxels have several nearest seeds (tests/nearest_cases.py on the device, tests/test_host_nearest.py
# for what they prove) ------------------------------------------------------------------------------------------------------

# Of tie_grids, the grids on which no voxel has two nearest seeds, whatever the rule: under a full plane every voxel has the one
# seed below or above it; about the centre of an even box |v - p|^2 - |v - p'|^2 is a sum of three odd numbers, never 0.  They
# are compared like the others, but cannot tell one tie rule from another.
NO_TIES = ("mirrored, even box", "plane")


def tie_grids():
    """name -> bool [z, y, x]."""
    grids = {}
    g = np.zeros((33, 33, 33), bool)
    g[::4, ::4, ::4] = True
    grids["lattice"] = g
    z, y, x = np.indices((9, 10, 11))
    grids["checkerboard"] = (x + y + z) % 2 == 0
    g = np.zeros((9, 9, 9), bool)
    g[1, 2, 3] = g[7, 6, 5] = True
    grids["mirrored, odd box"] = g
    g = np.zeros((8, 8, 8), bool)
    g[1, 2, 3] = g[6, 5, 4] = True
    grids["mirrored, even box"] = g
    g = np.zeros((9, 8, 7), bool)
    g[4] = True
    grids["plane"] = g
    g = g.copy()
    g[4, 3, 3] = False     # the voxels of the column through the hole have four nearest seeds, around it
    grids["plane with a hole"] = g
    return grids
