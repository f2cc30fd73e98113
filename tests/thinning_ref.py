"""A numpy reference of topological thinning as include/o2v_hip.h and DESIGN.md section 25 define it (o2v_hip_thin_dense), with
no compiled code.

S is the set of a set grid.  Voxels outside the box are background.  Objects are 26-connected.  The background is 6-connected.
Neighbourhood mask of a voxel: bit k = 9 (dz + 1) + 3 (dy + 1) + (dx + 1) is set where the neighbour is in S.  k runs 0 ... 26
without 13.
C26(m) is the number of 26-connected components of the set bits of m.
C6(m): take the clear bits of m among the 18 positions that differ from the centre on at most two axes.  Connect them by
6-adjacency within these 18.  Count the components that hold a face neighbour.
Simple: a voxel is simple iff C26 == 1 && C6 == 1.
Border: a voxel of S is a border voxel if one of its six face neighbours is background.
Subfield: the subfield of a voxel is s = (x & 1) | (y & 1) << 1 | (z & 1) << 2, in box coordinates.
One iteration: B := the border voxels of S as it is now.  For s = 0 ... 7 in turn, remove from S at once every voxel v that meets
all of these in the current S: v is in subfield s; v is in B; v is not in `keep`; v is simple; in mode CURVE, v has other than
exactly one 26-neighbour in S.  Iterations repeat until one removes nothing.  That iteration counts.  If max_iterations != 0,
they also stop once max_iterations have run.

Arrays are [z, y, x]."""
import numpy as np

ULTIMATE, CURVE = 0, 1
ALL26 = 0x07FFFFFF & ~(1 << 13)


def offset(k):
    """(dx, dy, dz) of position k."""
    return k % 3 - 1, k // 3 % 3 - 1, k // 9 - 1


def _axes(k):
    return sum(1 for d in offset(k) if d)


N18 = sum(1 << k for k in range(27) if 1 <= _axes(k) <= 2)
FACES = sum(1 << k for k in range(27) if _axes(k) == 1)
# 26-adjacency among the 26 positions; 6-adjacency among the 18
ADJ26 = np.array([sum(1 << j for j in range(27) if j not in (13, k) and k != 13 and max(abs(a - b) for a, b in zip(offset(j), offset(k))) <= 1)
                  for k in range(27)], np.uint32)
ADJ6 = np.array([sum(1 << j for j in range(27) if (N18 >> j) & 1 and (N18 >> k) & 1 and sum(abs(a - b) for a, b in zip(offset(j), offset(k))) == 1)
                 for k in range(27)], np.uint32)


def _flood(seed, within, adj):
    """What the bits of seed reach through the bits of within: a vectorised bit flood, at most 26 rounds."""
    cur = seed.copy()
    for _ in range(26):
        new = cur.copy()
        for k in range(27):
            if adj[k]:
                new |= np.where((cur >> np.uint32(k)) & np.uint32(1), adj[k] & within, np.uint32(0))
        if np.array_equal(new, cur):
            break
        cur = new
    return cur


def _count(start, within, adj):
    """The components of `within` (by adj) that hold a bit of `start`."""
    rest = start.copy()
    n = np.zeros(rest.shape, np.uint32)
    while rest.any():
        seed = rest & (~rest + np.uint32(1))
        n += seed != 0
        rest &= ~_flood(seed, within, adj)
    return n


def c26(m):
    m = np.asarray(m, np.uint32) & np.uint32(ALL26)
    return _count(m, m, ADJ26)


def c6(m):
    clear = ~np.asarray(m, np.uint32) & np.uint32(N18)
    return _count(clear & np.uint32(FACES), clear, ADJ6)


def is_simple(m):
    m = np.atleast_1d(np.asarray(m, np.uint32))
    return (c26(m) == 1) & (c6(m) == 1)


def masks_at(S, z, y, x):
    """The neighbourhood masks of the voxels (x, y, z) [arrays], by shifted views of the padded grid."""
    P = np.pad(np.asarray(S, bool), 1)
    m = np.zeros(len(x), np.uint32)
    for k in range(27):
        if k == 13:
            continue
        dx, dy, dz = offset(k)
        m |= P[z + 1 + dz, y + 1 + dy, x + 1 + dx].astype(np.uint32) << np.uint32(k)
    return m


def border(S):
    """The voxels of S with a face neighbour that is background (outside the box counts)."""
    P = np.pad(np.asarray(S, bool), 1)
    inner = P[1:-1, 1:-1, :-2] & P[1:-1, 1:-1, 2:] & P[1:-1, :-2, 1:-1] & P[1:-1, 2:, 1:-1] & P[:-2, 1:-1, 1:-1] & P[2:, 1:-1, 1:-1]
    return np.asarray(S, bool) & ~inner


def subfields(shape):
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    return (x & 1) | (y & 1) << 1 | (z & 1) << 2


def thin(S, mode=CURVE, keep=None, max_iterations=0):
    """(the skeleton, the iterations, the voxels removed)."""
    S = np.array(S, bool)
    keep = np.zeros(S.shape, bool) if keep is None else np.asarray(keep) != 0
    field = subfields(S.shape)
    iterations = removed = 0
    while True:
        B = border(S) & ~keep
        n = 0
        for s in range(8):
            z, y, x = np.nonzero(B & S & (field == s))
            if not len(x):
                continue
            m = masks_at(S, z, y, x)
            ok = m != 0
            if mode == CURVE:
                ok &= (m & (m - np.uint32(1))) != 0          # other than exactly one 26-neighbour (none: not simple anyway)
            ok[ok] = is_simple(m[ok])
            S[z[ok], y[ok], x[ok]] = False
            n += int(ok.sum())
        iterations += 1
        removed += n
        if n == 0 or (max_iterations and iterations == max_iterations):
            return S, iterations, removed


def degree(K):
    """uint8: 0 outside the skeleton K; inside it 1 + the number of 26-neighbours in K."""
    K = np.asarray(K, bool)
    P = np.pad(K, 1).astype(np.uint8)
    n = np.zeros(K.shape, np.uint8)
    for k in range(27):
        if k != 13:
            dx, dy, dz = offset(k)
            n += P[1 + dz:1 + dz + K.shape[0], 1 + dy:1 + dy + K.shape[1], 1 + dx:1 + dx + K.shape[2]]
    return np.where(K, n + 1, 0).astype(np.uint8)


def nodes(deg):
    """(end points, junctions) of a degree grid: int32 [n, 3] (x, y, z) each, in [z, y, x] order."""
    def coords(mask):
        z, y, x = np.nonzero(mask)
        return np.stack([x, y, z], axis=1).astype(np.int32)
    return coords(deg == 2), coords(deg >= 4)


# ---- shapes -----------------------------------------------------------------------------------------------------------------------

def box(n=9, pad=2):
    S = np.zeros((n + 2 * pad,) * 3, bool)
    S[pad:pad + n, pad:pad + n, pad:pad + n] = True
    return S


def _r2(n=33, c=16):
    z, y, x = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    return x, y, z, (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2


def ball():
    return _r2()[3] <= 144


def shell():
    r2 = _r2()[3]
    return (r2 > 81) & (r2 <= 144)


def torus():
    x, y, z, _ = _r2()
    return (np.sqrt((x - 16.0) ** 2 + (y - 16.0) ** 2) - 10.0) ** 2 + (z - 16.0) ** 2 <= 16.0


def line(axis, n, first=0):
    """A line of voxels first ... n - 1 along the axis ("x", "y", "z") at 1 on the other two, in a box of n x 3 x 3."""
    dims = {"x": (3, 3, n), "y": (3, n, 3), "z": (n, 3, 3)}[axis]
    S = np.zeros(dims, bool)
    S[{"x": (1, 1, slice(first, n)), "y": (1, slice(first, n), 1), "z": (slice(first, n), 1, 1)}[axis]] = True
    return S


def staircase():
    S = np.zeros((20, 20, 130), bool)
    x = np.arange(130)
    yz = np.minimum(x // 7, 19)
    S[yz, yz, x] = True
    return S


def cross():
    """Three bars of 29 x 5 x 5 through the centre of 33^3."""
    S = np.zeros((33, 33, 33), bool)
    S[14:19, 14:19, 2:31] = S[14:19, 2:31, 14:19] = S[2:31, 14:19, 14:19] = True
    return S


def random_grid(rng, dims, density):
    nx, ny, nz = dims
    return rng.random((nz, ny, nx)) < density
