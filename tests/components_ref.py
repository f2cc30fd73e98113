"""numpy reference of connected-component labelling and flood fill as include/o2v_hip.h defines them.
numpy only: the GPU cases run where scipy may be absent.

S is a bool array [z, y, x].  label() builds the list of adjacent pairs from shifted views, hooks the larger index under the
smaller with np.minimum.at and jumps pointers to a fixed point, so every voxel ends at the smallest linear index of its
component; the roots, ranked, give the labels.  The set readers are those of tests/raycast_ref.py."""
import itertools

import numpy as np

from tests.raycast_ref import pack_bits, random_solid, solid_bits, solid_f32, solid_u8  # noqa: F401  (the formats' readers)

CONNECTIVITIES = (6, 18, 26)


def offsets(connectivity):
    """The half of the offsets (dx, dy, dz) of a connectivity that point back in [z, y, x] order."""
    axes = {6: 1, 18: 2, 26: 3}[connectivity]
    out = []
    for dz, dy, dx in itertools.product((-1, 0, 1), repeat=3):
        if (dz, dy, dx) < (0, 0, 0) and abs(dx) + abs(dy) + abs(dz) <= axes:
            out.append((dx, dy, dz))
    return out


def _part(n, d):
    """The part of an axis of length n whose voxels have a neighbour at offset d."""
    return slice(max(0, -d), n - max(0, d))


def pairs(S, connectivity):
    """(a, b) linear indexes of every adjacent pair of S, each once, a > b."""
    nz, ny, nx = S.shape
    A, B = [], []
    for dx, dy, dz in offsets(connectivity):
        both = np.zeros(S.shape, bool)
        me = (_part(nz, dz), _part(ny, dy), _part(nx, dx))
        nb = (_part(nz, -dz), _part(ny, -dy), _part(nx, -dx))
        both[me] = S[me] & S[nb]
        a = np.flatnonzero(both)
        A.append(a)
        B.append(a + ((dz * ny + dy) * nx + dx))
    return np.concatenate(A), np.concatenate(B)


def roots(S, connectivity):
    """int64 [z, y, x]: the smallest linear index of the voxel's component; -1 outside S.  Also returns the rounds taken."""
    S = np.asarray(S, bool)
    parent = np.arange(S.size, dtype=np.int64)
    a, b = pairs(S, connectivity)
    rounds = 0
    while True:
        rounds += 1
        ra, rb = parent[a], parent[b]
        differ = ra != rb
        if not differ.any():
            break
        hi, lo = np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ]
        np.minimum.at(parent, hi, lo)
        while True:   # pointer jumping to a fixed point
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    out = parent.reshape(S.shape)
    out[~S] = -1
    return out, rounds


def label(S, connectivity=6):
    """(labels int32 [z, y, x], n): 0 outside S, 1 + the rank of the component by its smallest linear index inside."""
    S = np.asarray(S, bool)
    r, _ = roots(S, connectivity)
    ids = np.unique(r[S])
    labels = np.zeros(S.shape, np.int32)
    labels[S] = (np.searchsorted(ids, r[S]) + 1).astype(np.int32)
    return labels, len(ids)


def flood(S, connectivity=6, seeds=(), border=False, values=(1, 0, 0), labelled=None):
    """(out uint8 [z, y, x], reached): values[0] in the components of S that hold a seed ((x, y, z) triples; outside the box or
    not in S: ignored; border: and every voxel of S on the box's faces), values[1] in the others, values[2] outside S.
    labelled: label(S, connectivity), if the caller has it."""
    S = np.asarray(S, bool)
    nz, ny, nx = S.shape
    labels, n = label(S, connectivity) if labelled is None else labelled
    seeded = np.zeros(n + 1, bool)
    seeds = np.asarray(seeds, np.int64).reshape(-1, 3)
    ok = ((seeds >= 0) & (seeds < np.array([nx, ny, nz]))).all(axis=1)
    seeds = seeds[ok]
    seeded[labels[seeds[:, 2], seeds[:, 1], seeds[:, 0]]] = True
    if border:
        face = np.zeros(S.shape, bool)
        face[[0, -1], :, :] = face[:, [0, -1], :] = face[:, :, [0, -1]] = True
        seeded[labels[face]] = True
    seeded[0] = False
    hit = seeded[labels]
    out = np.where(S, np.where(hit, np.uint8(values[0]), np.uint8(values[1])), np.uint8(values[2])).astype(np.uint8)
    return out, int(hit.sum())


def solidify(solid, connectivity=6):
    """uint8: 1 solid, 2 empty but enclosed, 0 exterior (dense.solidify)."""
    return flood(~np.asarray(solid, bool), connectivity, border=True, values=(0, 2, 1))[0]


# ---- generators (arrays [z, y, x]; dims are (nx, ny, nz)) -----------------------------------------------------------------------

def random_grid(rng, dims, density):
    return rng.random(dims[::-1]) < density


def serpentine(dims):
    """A path one voxel wide through the whole box: every second row along y, every second layer along z, joined at alternating
    ends - one component whose diameter is about a quarter of the box's voxels."""
    nx, ny, nz = dims
    S = np.zeros((nz, ny, nx), bool)
    row = 0                                   # counts the rows laid, over all layers: the joint's end alternates with it
    for z in range(0, nz, 2):
        ys = list(range(0, ny, 2))
        if (z // 2) % 2:
            ys.reverse()
        for k, y in enumerate(ys):
            S[z, y, :] = True
            end = nx - 1 if row % 2 == 0 else 0
            if k + 1 < len(ys):
                S[z, min(y, ys[k + 1]) + 1, end] = True       # the joint to the next row of the layer
            elif z + 2 < nz:
                S[z + 1, y, end] = True                       # the joint to the next layer
            row += 1
    return S


def checkerboard(dims):
    z, y, x = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    return (x + y + z) % 2 == 0


def touching_pair(dims, corner, kind):
    """Two 3 x 3 x 3 blobs that touch only by an edge (kind "edge": 2 / 1 / 1 components at 6 / 18 / 26) or only by a corner
    ("corner": 2 / 2 / 1); `corner` (x, y, z) is the first voxel of the second blob, so the contact lies on the planes through it."""
    S = np.zeros(dims[::-1], bool)
    x, y, z = corner
    S[z:z + 3, y:y + 3, x:x + 3] = True
    if kind == "edge":
        S[z:z + 3, y - 3:y, x - 3:x] = True       # shares the edge x, y = const along z
    else:
        S[z - 3:z, y - 3:y, x - 3:x] = True
    return S


def comb(dims, pitch=(64, 8, 8)):
    """One tooth per tile column: a one-voxel line along z in the middle of every tile of the (x, y) plane, the teeth of one x
    joined by a line along y in the layer z = 0, those lines by a spine along x - one component that crosses every tile seam."""
    nx, ny, nz = dims
    S = np.zeros((nz, ny, nx), bool)
    S[0, 0, :] = True
    for x in range(pitch[0] // 2, nx, pitch[0]):
        S[0, :, x] = True
        for y in range(pitch[1] // 2, ny, pitch[1]):
            S[:, y, x] = True
    return S


def spiral(dims):
    """A square spiral one voxel wide with gaps of one voxel, walked from a corner inwards, in every second layer; the layers
    are joined at the spiral's two ends in turn: one long 6-connected component that crosses every tile seam many times."""
    nx, ny, nz = dims
    layer = np.zeros((ny, nx), bool)
    x = y = 0
    dx, dy = 1, 0
    layer[0, 0] = True
    while True:
        moved = False
        for _ in range(2):                        # straight on, else one turn
            X, Y, X2, Y2 = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if 0 <= X < nx and 0 <= Y < ny and not layer[Y, X] and not (0 <= X2 < nx and 0 <= Y2 < ny and layer[Y2, X2]):
                x, y, moved = X, Y, True
                layer[y, x] = True
                break
            dx, dy = -dy, dx
        if not moved:
            break
    S = np.zeros((nz, ny, nx), bool)
    S[::2] = layer
    ends = [(0, 0), (y, x)]
    for k, z in enumerate(range(1, nz - 1, 2)):
        S[z][ends[k % 2]] = True
    return S
