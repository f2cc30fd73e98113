"""The definition of o2v_hip_euler_stats (include/o2v_hip.h) restated twice: in numpy (euler_stats: the 2x2x2
window form, every label at once) and as a scalar loop over the cells of the unit lattice (euler_stats_loop: the definition by
cells, word for word); with what follows from a row, closed forms and the grids of the known answers.

A grid is indexed [z, y, x].  Rows 0 ... n take part; a voxel whose value is negative or above n is in no row.  A lattice cell is
closed-in for label L if one of the voxels it touches holds L, inner if every position it touches lies in the box and holds L.
Columns: voxels, closed-in faces, edges, vertices, inner faces, edges, vertices."""
import itertools

import numpy as np

COLUMNS = 7
VOXELS, FACES, EDGES, VERTICES, INNER_FACES, INNER_EDGES, INNER_VERTICES = range(7)
ONE_WINDOW = [1, 3, 3, 1, 3, 3, 1]      # what a window of one label adds
SINGLE_VOXEL = [1, 6, 12, 8, 0, 0, 0]

# The window at lattice vertex v holds the voxels at v + {-1, 0}^3; position b = i + 2 j + 4 k is the voxel at (vx - 1 + i, vy - 1 + j,
# vz - 1 + k).  It owns v, the edges from v towards +x, +y, +z, the faces they span and the cube at v: (closed-in column, the
# positions that the cell touches).
WINDOW_CELLS = ((VERTICES, 0xff), (EDGES, 0xaa), (EDGES, 0xcc), (EDGES, 0xf0), (FACES, 0x88), (FACES, 0xa0), (FACES, 0xc0), (VOXELS, 0x80))
INNER_OF = {VERTICES: INNER_VERTICES, EDGES: INNER_EDGES, FACES: INNER_FACES}


def _rows(g, n):
    """The grid as int64 with -1 where a voxel is in no row, and the number of such voxels."""
    v = np.asarray(g).astype(np.int64)
    out = (v < 0) | (v > n)
    return np.where(out, -1, v), int(out.sum())


def euler_stats(g, n):
    """(table int64 [n + 1, 7], outside) of the grid g [z, y, x]: the window form, all labels at once."""
    v, outside = _rows(g, n)
    nz, ny, nx = v.shape
    pad = np.pad(v, 1, constant_values=-1)
    P = [pad[k:k + nz + 1, j:j + ny + 1, i:i + nx + 1].reshape(-1) for k in (0, 1) for j in (0, 1) for i in (0, 1)]   # P[i + 2 j + 4 k]
    table = np.zeros((n + 1, COLUMNS), np.int64)
    for col, mask in WINDOW_CELLS:
        s = np.sort(np.stack([P[b] for b in range(8) if mask >> b & 1]), axis=0)
        first = np.ones(s.shape, bool)
        first[1:] = s[1:] != s[:-1]
        first &= s >= 0
        table[:, col] += np.bincount(s[first], minlength=n + 1)          # the distinct labels among the positions
        if col in INNER_OF:
            same = (s[0] == s[-1]) & (s[0] >= 0)                          # (a position outside the box is -1)
            table[:, INNER_OF[col]] += np.bincount(s[0][same], minlength=n + 1)
    return table, outside


def euler_stats_loop(g, n):
    """The same by the definition: every cell of the unit lattice - vertices, edges, faces and cubes - with the voxel positions
    it touches, as a scalar loop."""
    g = np.asarray(g)
    nz, ny, nx = g.shape
    table = [[0] * COLUMNS for _ in range(n + 1)]
    outside = 0
    for z, y, x in itertools.product(range(nz), range(ny), range(nx)):
        outside += not 0 <= int(g[z, y, x]) <= n
    # a cell: its lowest corner (x, y, z) and the axes it extends along, e.g. (1, 0, 0) an edge along x, (1, 1, 1) a cube
    for ext in itertools.product((0, 1), repeat=3):
        dim = sum(ext)
        closed_col = (VERTICES, EDGES, FACES, VOXELS)[dim]
        inner_col = (INNER_VERTICES, INNER_EDGES, INNER_FACES, None)[dim]
        for x, y, z in itertools.product(range(nx + 1 - ext[0]), range(ny + 1 - ext[1]), range(nz + 1 - ext[2])):
            # the voxels that contain the cell: along an axis of the cell the voxel at its corner, across it the two beside it
            spans = [(c,) if e else (c - 1, c) for c, e in zip((x, y, z), ext)]
            values = []
            for vx, vy, vz in itertools.product(*spans):
                inside = 0 <= vx < nx and 0 <= vy < ny and 0 <= vz < nz
                value = int(g[vz, vy, vx]) if inside else None
                values.append(value if value is not None and 0 <= value <= n else None)
            for L in set(values) - {None}:
                table[L][closed_col] += 1
                if inner_col is not None and all(v == L for v in values):
                    table[L][inner_col] += 1
    return np.array(table, np.int64).reshape(n + 1, COLUMNS), outside


# ---- what follows from a row ---------------------------------------------------------------------------------------------------

def euler_numbers(table, connectivity=26):
    t = np.asarray(table, np.int64)
    if connectivity == 26:
        return t[..., VERTICES] - t[..., EDGES] + t[..., FACES] - t[..., VOXELS]
    assert connectivity == 6
    return t[..., VOXELS] - t[..., INNER_FACES] + t[..., INNER_EDGES] - t[..., INNER_VERTICES]


def intrinsic_volumes(table):
    t = np.asarray(table, np.int64)
    n3, n2, n1, n0 = t[..., 0], t[..., 1], t[..., 2], t[..., 3]
    return np.stack([n0 - n1 + n2 - n3, n1 - 2 * n2 + 3 * n3, n2 - 3 * n3, n3], axis=-1)


def exposed_faces(table):
    t = np.asarray(table, np.int64)
    return 6 * t[..., VOXELS] - 2 * t[..., INNER_FACES]


def box_row(a, b, c):
    """The row of a solid a x b x c box, in Python ints."""
    return [a * b * c, a * b * (c + 1) + b * c * (a + 1) + a * c * (b + 1), a * (b + 1) * (c + 1) + b * (a + 1) * (c + 1) + c * (a + 1) * (b + 1),
            (a + 1) * (b + 1) * (c + 1), (a - 1) * b * c + a * (b - 1) * c + a * b * (c - 1),
            a * (b - 1) * (c - 1) + (a - 1) * b * (c - 1) + (a - 1) * (b - 1) * c, (a - 1) * (b - 1) * (c - 1)]


def betti_numbers(mask, connectivity=26):
    """(b0, b1, b2) of a 0 / 1 grid with tests/components_ref.py's labels: the numpy twin of dense.betti_numbers."""
    from tests import components_ref as CR
    mask = np.asarray(mask) != 0
    labels, b0 = CR.label(mask, connectivity)
    chi = int(euler_numbers(euler_stats(labels, b0)[0], connectivity)[1:].sum())
    rest, m = CR.label(~mask, 32 - connectivity)
    b2 = 0
    for L in range(1, m + 1):
        idx = np.nonzero(rest == L)
        b2 += not any(i.min() == 0 or i.max() == s - 1 for i, s in zip(idx, rest.shape))
    return b0, b0 + b2 - chi, b2


# ---- grids of the known answers ---------------------------------------------------------------------------------------------------

def hollow_box(n=10):
    g = np.ones((n, n, n), bool)
    g[1:-1, 1:-1, 1:-1] = False
    return g


def square_ring():
    """5 x 5 x 1 with the 3 x 3 middle empty."""
    g = np.ones((1, 5, 5), bool)
    g[0, 1:4, 1:4] = False
    return g


def plate_with_two_holes():
    """The 1 x 3 x 5 plate (x, y, z) with two holes through it along x."""
    g = np.ones((5, 3, 1), bool)
    g[1, 1, 0] = g[3, 1, 0] = False
    return g


def edge_pair():
    g = np.zeros((1, 2, 2), bool)
    g[0, 0, 0] = g[0, 1, 1] = True
    return g


def corner_pair():
    g = np.zeros((2, 2, 2), bool)
    g[0, 0, 0] = g[1, 1, 1] = True
    return g


def checkerboard(n=4):
    z, y, x = np.indices((n, n, n))
    return (x + y + z) % 2 == 0


def ball(n=15, r=5.6):
    z, y, x = np.indices((n, n, n))
    c = (n - 1) / 2
    return (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2 <= r * r


def blobs(rng, dims, n, outside=0.0):
    """tests/label_stats_ref.py's blobs: coherent labels 0 ... n, a share `outside` of the voxels negative or above n."""
    from tests import label_stats_ref as LR
    return LR.blobs(rng, dims, n, outside)
