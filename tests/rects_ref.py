"""The numpy restatement of O2V_HIP_FACES_MERGE_RECTS (include/o2v_hip.h) on top of tests/faces_ref.py:
the runs of the exposed faces stacked into rectangles - a maximal chain of equal runs in consecutive rows is one quad -, and a
scalar restatement with loops that follows the header word for word.

Grids are numpy arrays indexed [z, y, x].  Nothing here imports the code under test."""
import numpy as np

from tests import faces_ref as FR

F = np.float32
NONE, RUNS, RECTS = FR.NONE, FR.RUNS, 3          # O2V_HIP_FACES_MERGE_*


def stack_axis(d):
    """Column of (x, y, z) along which the runs of direction d are stacked: y for the -z / +z faces, z for the others."""
    return np.where(np.asarray(d) >= 4, 1, 2)


def rects(S, C):
    """int64 [Q, 7] in the contract's order: (x, y, z, d, length, height, argb) of every rectangle's first face."""
    nz, ny, nx = S.shape
    q = FR.runs(S, C, RUNS)                                       # (x, y, z, d, length, argb) in key order
    n = len(q)
    if not n:
        return np.zeros((0, 7), np.int64)
    index = np.full((6, nz, ny, nx), -1, np.int64)                # the run that begins at (d, z, y, x)
    index[q[:, 3], q[:, 2], q[:, 1], q[:, 0]] = np.arange(n)
    along = stack_axis(q[:, 3])
    before = q[:, :3].copy()
    before[np.arange(n), along] -= 1                              # the same place in the row before
    inside = before[np.arange(n), along] >= 0
    prev = np.where(inside, index[q[:, 3], before[:, 2] * inside, before[:, 1] * inside, before[:, 0]], -1)
    stacked = (prev >= 0) & (q[prev, 4] == q[:, 4]) & (q[prev, 5] == q[:, 5])   # begins together, same length, same colour
    # heights: a run hands its height to the run it is stacked on, from the last row down
    height = np.ones(n, np.int64)
    level = q[np.arange(n), along]
    for lv in range(int(level.max()), 0, -1):
        sel = np.nonzero(stacked & (level == lv))[0]
        height[prev[sel]] += height[sel]                          # (no two runs are stacked on one)
    keep = ~stacked
    return np.concatenate([q[keep, :5], height[keep, None], q[keep, 5:6]], axis=1)


def geometry(r, origin=(0, 0, 0)):
    """(positions float32 [4Q, 3], faces int32 [2Q, 3]) of rectangles r as the header lays them out."""
    Q = len(r)
    lo = r[:, :3] + np.asarray(origin, np.int64)
    hi = lo + 1
    k = np.arange(Q)
    run = np.where(r[:, 3] >= 2, 0, 1)
    hi[k, run] = lo[k, run] + r[:, 4]
    stack = stack_axis(r[:, 3])
    hi[k, stack] = lo[k, stack] + r[:, 5]
    a, s = r[:, 3] >> 1, r[:, 3] & 1
    u, v = (a + 1) % 3, (a + 2) % 3
    pos = np.zeros((Q, 4, 3), np.int64)
    for c, (cu, cv) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):   # s = 1; s = 0 swaps the roles of u and v
        pos[k, c, a] = lo[k, a] + s
        pos[k, c, u] = np.where(np.where(s == 1, cu, cv) == 1, hi[k, u], lo[k, u])
        pos[k, c, v] = np.where(np.where(s == 1, cv, cu) == 1, hi[k, v], lo[k, v])
    base = 4 * np.arange(Q, dtype=np.int64)[:, None]
    faces = np.concatenate([base + [0, 1, 2], base + [0, 2, 3]], axis=1).reshape(-1, 3)
    return pos.reshape(-1, 3).astype(F), faces.astype(np.int32)


def quads(grid, fmt, level=None, origin=(0, 0, 0), merge=RECTS, argb=0xFFFFFFFF, colors=None, palette=None):
    """(positions float32 [4Q, 3], faces int32 [2Q, 3], quad_argb uint32 [Q]): what o2v_hip_faces_write fills."""
    if merge != RECTS:
        return FR.quads(grid, fmt, level, origin, merge, argb, colors, palette)
    S = FR.solid(grid, fmt, level)
    r = rects(S, FR.voxel_colors(grid, fmt, S, argb, colors, palette))
    positions, faces = geometry(r, origin)
    return positions, faces, r[:, 6].astype(np.uint32)


def count(grid, fmt, level=None, merge=RECTS, argb=0xFFFFFFFF, colors=None, palette=None):
    if merge != RECTS:
        return FR.count(grid, fmt, level, merge, argb, colors, palette)
    S = FR.solid(grid, fmt, level)
    return len(rects(S, FR.voxel_colors(grid, fmt, S, argb, colors, palette)))


def quads_scalar(grid, fmt, level=None, origin=(0, 0, 0), argb=0xFFFFFFFF, colors=None, palette=None):
    """MERGE_RECTS by loops that restate the header word for word (the check of `quads`)."""
    g = np.asarray(grid)
    nz, ny = g.shape[:2]
    nx = g.shape[2] * 32 if fmt == FR.BITS else g.shape[2]
    STEP = FR.STEP

    def is_solid(x, y, z):
        if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz):
            return False
        if fmt == FR.U8:
            return int(g[z, y, x]) != 0
        if fmt == FR.BITS:
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
        return is_exposed(x, y, z, d) and is_exposed(x2, y2, z2, d) and color(x, y, z) == color(x2, y2, z2)

    def run_at(x, y, z, d):
        """The length of the run of direction d that begins at (x, y, z), or 0 if none begins there."""
        rx, ry = (1, 0) if d >= 2 else (0, 1)
        if not is_exposed(x, y, z, d) or same_run(x - rx, y - ry, z, d, x, y, z):
            return 0
        n = 1
        while same_run(x + (n - 1) * rx, y + (n - 1) * ry, z, d, x + n * rx, y + n * ry, z):
            n += 1
        return n

    def equal_runs(x, y, z, d, y2, z2):
        """The run that begins at (x, y, z) and one that begins at (x, y2, z2): the same length and colour."""
        n = run_at(x, y, z, d)
        return n > 0 and run_at(x, y2, z2, d) == n and color(x, y, z) == color(x, y2, z2)

    positions, argbs = [], []
    for z in range(nz):
        for y in range(ny):
            for d in range(6):
                sy, sz = (1, 0) if d >= 4 else (0, 1)              # the stack axis: y for the z faces, z for the others
                for x in range(nx):
                    n = run_at(x, y, z, d)
                    if not n or equal_runs(x, y, z, d, y - sy, z - sz):
                        continue                                    # no run begins here, or it is equal to the run before it
                    h = 1
                    while equal_runs(x, y + (h - 1) * sy, z + (h - 1) * sz, d, y + h * sy, z + h * sz):
                        h += 1
                    lo = [origin[0] + x, origin[1] + y, origin[2] + z]
                    hi = [lo[0] + 1, lo[1] + 1, lo[2] + 1]
                    hi[0 if d >= 2 else 1] += n - 1
                    hi[1 if d >= 4 else 2] += h - 1
                    a, s = d >> 1, d & 1
                    u, v = (a + 1) % 3, (a + 2) % 3
                    for cu, cv in (((0, 0), (1, 0), (1, 1), (0, 1)) if s == 1 else ((0, 0), (0, 1), (1, 1), (1, 0))):
                        p = [0, 0, 0]
                        p[a] = lo[a] + s
                        p[u] = hi[u] if cu else lo[u]
                        p[v] = hi[v] if cv else lo[v]
                        positions.append(p)
                    argbs.append(color(x, y, z))
    Q = len(argbs)
    faces = [[4 * q + i for i in tri] for q in range(Q) for tri in ((0, 1, 2), (0, 2, 3))]
    return np.array(positions, F).reshape(-1, 3), np.array(faces, np.int32).reshape(-1, 3), np.array(argbs, np.uint32)
