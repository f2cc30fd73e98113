"""numpy reference of geodesic distances and shortest paths as include/o2v_hip.h defines them.  numpy
only: the GPU cases run where scipy may be absent.

S is a bool array [z, y, x]; weights = (face, edge, corner) step costs, 0 = no such step; seeds are (x, y, z) triples.
distance() relaxes d = min(d, d[neighbour] + w) over shifted views of a padded int64 array, offset by offset, until a round
changes nothing, then masks to S and max_distance.  dijkstra() is the definition restated voxel by voxel with a heap (and the one
to use on sets one voxel wide, where the relaxation needs a round per voxel); trace() is the walk back as a scalar loop."""
import heapq
import itertools

import numpy as np

INF = 2 ** 31 - 1            # the kernels' "not reached"
MAX_DISTANCE = 2 ** 31 - 2   # the largest and default max_distance
BIG = 1 << 40                # the reference's own "not reached": BIG + 65 535 fits an int64 many times over

WEIGHTS = {("steps", 6): (1, 0, 0), ("steps", 18): (1, 1, 0), ("steps", 26): (1, 1, 1),
           ("chamfer", 6): (3, 0, 0), ("chamfer", 18): (3, 4, 0), ("chamfer", 26): (3, 4, 5)}


def offsets(weights):
    """(dx, dy, dz, w) of every step that exists, in ascending (dz, dy, dx) order."""
    out = []
    for dz, dy, dx in itertools.product((-1, 0, 1), repeat=3):
        axes = abs(dx) + abs(dy) + abs(dz)
        if axes and weights[axes - 1]:
            out.append((dx, dy, dz, int(weights[axes - 1])))
    return out


def seed_mask(S, seeds=(), border=False):
    """bool [z, y, x]: the seeds that count - inside the box and in S; border: and every voxel of S on the box's faces."""
    S = np.asarray(S, bool)
    nz, ny, nx = S.shape
    m = np.zeros(S.shape, bool)
    seeds = np.asarray(seeds, np.int64).reshape(-1, 3)
    ok = ((seeds >= 0) & (seeds < np.array([nx, ny, nz]))).all(axis=1)
    seeds = seeds[ok]
    m[seeds[:, 2], seeds[:, 1], seeds[:, 0]] = True
    if border:
        m[[0, -1], :, :] = m[:, [0, -1], :] = m[:, :, [0, -1]] = True
    return m & S


def cap(dist, max_distance):
    """A distance grid under a smaller max_distance: what lies further is not reached.  (Every weight is positive, so a path
    through a voxel further than the cap only reaches voxels further than the cap: cutting the propagation there changes no
    other voxel - tests/test_host_geodesic.py holds this against dijkstra(), which cuts it.)"""
    out = np.where(dist > max_distance, -1, dist).astype(np.int32)
    return out, int((out >= 0).sum())


def distance(S, weights, seeds=(), border=False, max_distance=MAX_DISTANCE):
    """(dist int32 [z, y, x], reached, rounds): the smallest sum of weights over the paths inside S from a seed; -1 outside S,
    where no path leads, and above max_distance; reached = the voxels with dist >= 0."""
    S = np.asarray(S, bool)
    nz, ny, nx = S.shape
    P = np.full((nz + 2, ny + 2, nx + 2), BIG, np.int64)
    core = P[1:-1, 1:-1, 1:-1]
    core[seed_mask(S, seeds, border)] = 0
    offs = offsets(weights)
    rounds = 0
    tmp = np.empty(S.shape, np.int64)
    floor = np.where(S, 0, BIG)          # a voxel outside S stays at BIG: max(min(BIG, .), BIG)
    while True:
        rounds += 1
        before = core.copy()
        for dx, dy, dz, w in offs:
            np.add(P[1 + dz:nz + 1 + dz, 1 + dy:ny + 1 + dy, 1 + dx:nx + 1 + dx], w, out=tmp)
            np.minimum(core, tmp, out=tmp)
            np.maximum(tmp, floor, out=core)
        if np.array_equal(before, core):
            break
    out = np.where(S & (core <= max_distance), core, -1).astype(np.int32)
    return out, int((out >= 0).sum()), rounds


def dijkstra(S, weights, seeds=(), border=False, max_distance=MAX_DISTANCE):
    """(dist int32 [z, y, x], reached): the header's words, voxel by voxel.  A voxel whose distance would be above max_distance is
    not reached, and nothing is propagated through it."""
    S = np.asarray(S, bool)
    nz, ny, nx = S.shape
    offs = offsets(weights)
    inside = S.tolist()
    dist = {}
    heap = [(0, int(x), int(y), int(z)) for z, y, x in zip(*np.nonzero(seed_mask(S, seeds, border)))]
    best = {(x, y, z): 0 for _, x, y, z in heap}
    heapq.heapify(heap)
    while heap:
        d, x, y, z = heapq.heappop(heap)
        if (x, y, z) in dist:
            continue
        dist[x, y, z] = d
        for dx, dy, dz, w in offs:
            X, Y, Z = x + dx, y + dy, z + dz
            if 0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz and inside[Z][Y][X] and d + w <= max_distance and d + w < best.get((X, Y, Z), BIG):
                best[X, Y, Z] = d + w
                heapq.heappush(heap, (d + w, X, Y, Z))
    out = np.full(S.shape, -1, np.int32)
    for (x, y, z), d in dist.items():
        out[z, y, x] = d
    return out, len(dist)


def trace(dist, weights, target, max_len=None):
    """(path, length) of one target (x, y, z): the walk back as the header words it - from v to the first neighbour u, in
    ascending (dz, dy, dx) order among the steps with a weight, with dist[u] >= 0 and dist[u] + w == dist[v], until dist = 0.
    length: the voxels of the whole path, -1 (outside the box or dist < 0), -2 (no such neighbour); path: its first
    min(length, max_len) voxels (everything walked for -2; max_len None: all)."""
    nz, ny, nx = dist.shape
    x, y, z = (int(v) for v in target)
    if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz) or dist[z, y, x] < 0:
        return [], -1
    offs = offsets(weights)
    path = []
    while True:
        path.append((x, y, z))
        dv = int(dist[z, y, x])
        if dv == 0:
            break
        for dx, dy, dz, w in offs:
            X, Y, Z = x + dx, y + dy, z + dz
            if 0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz and dist[Z, Y, X] >= 0 and int(dist[Z, Y, X]) + w == dv:
                x, y, z = X, Y, Z
                break
        else:
            return path if max_len is None else path[:max_len], -2
    return path if max_len is None else path[:max_len], len(path)


def paths(dist, weights, targets, max_len):
    """(paths int32 [n, max_len, 3] padded with -1, lengths int32 [n]) as dense.shortest_paths returns them."""
    targets = np.asarray(targets, np.int64).reshape(-1, 3)
    out = np.full((len(targets), max_len, 3), -1, np.int32)
    lengths = np.empty(len(targets), np.int32)
    for i, t in enumerate(targets):
        p, lengths[i] = trace(dist, weights, t, max_len)
        if p:
            out[i, :len(p)] = p
    return out, lengths


def default_max_len(dist, weights, targets):
    """The L of dense.shortest_paths without max_len."""
    nz, ny, nx = dist.shape
    t = np.asarray(targets, np.int64).reshape(-1, 3)
    t = t[((t >= 0) & (t < np.array([nx, ny, nz]))).all(axis=1)]
    top = max(int(dist[t[:, 2], t[:, 1], t[:, 0]].max()), 0) if len(t) else 0
    return top // min(w for w in weights if w) + 1


# ---- generators (arrays [z, y, x]; dims are (nx, ny, nz)) -----------------------------------------------------------------------

def door_box(open_door=True):
    """A full 40 x 20 x 20 box with the plane x = 20 removed, except the door (20, 4, 3)."""
    S = np.ones((20, 20, 40), bool)
    S[:, :, 20] = False
    S[3, 4, 20] = open_door
    return S


def u_corridor():
    """A corridor one voxel wide, in the layer z = 3 of a 200 x 24 x 8 box: along x through the first tile at y = 2, on through
    the second and third, back at y = 13 (a row of other tiles), and down the line x = 30 into the first tile again, where it
    ends at y = 5 - beside nothing it passed before.  Returns (S, seed, end): the first tile converges with the first leg, and
    has to be visited again when the way comes back into it."""
    S = np.zeros((8, 24, 200), bool)
    S[3, 2, 0:181] = True
    S[3, 2:14, 180] = True
    S[3, 13, 30:181] = True
    S[3, 5:14, 30] = True
    return S, (0, 2, 3), (30, 5, 3)


def pair_across(kind, at=(64, 8, 8)):
    """Two voxels of a 140 x 24 x 24 box that touch only across the tile boundary at `at`: kind = a set of axes ("x", "y", "z")
    on which they differ - one axis: a face, two: an edge, three: the tile's corner.  Returns (S, a, b)."""
    S = np.zeros((24, 24, 140), bool)
    b = tuple(at)
    a = tuple(c - (1 if ax in kind else 0) for c, ax in zip(at, "xyz"))
    S[a[2], a[1], a[0]] = S[b[2], b[1], b[0]] = True
    return S, a, b
