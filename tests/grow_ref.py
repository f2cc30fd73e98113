"""numpy reference of the seeded watershed as include/o2v_hip.h defines it.  numpy only: the GPU cases run
where scipy may be absent.

H and M are int arrays [z, y, x]; weights = (face, edge, corner) step costs, 0 = no such step.  level(), ticks() and labels() are
the three phases, each a fixed point over shifted views of padded int64 arrays, offset by offset, until a round changes nothing;
grow() runs them in turn.  dijkstra() is the definition restated voxel by voxel - a heap on the joint key (Q, T), then the label
pass in the order the voxels left the heap - and the one to use on sets one voxel wide, where a relaxation needs a round per voxel."""
import heapq

import numpy as np

from tests.geodesic_ref import offsets

CAP = 2 ** 31 - 2       # where the ticks saturate
BIG = 1 << 40           # the reference's own "not yet": BIG + 65 535 fits an int64 many times over


def _shift(P, dims, dx, dy, dz):
    nz, ny, nx = dims
    return P[1 + dz:nz + 1 + dz, 1 + dy:ny + 1 + dy, 1 + dx:nx + 1 + dx]


def _padded(shape, fill):
    P = np.full((shape[0] + 2, shape[1] + 2, shape[2] + 2), fill, np.int64)
    return P, P[1:-1, 1:-1, 1:-1]


def seeds_of(H, M):
    return (np.asarray(H) > 0) & (np.asarray(M) > 0)


def level(H, M, weights):
    """int64 [z, y, x]: Q, the max-min height over all paths from a seed; 0 outside S and where no seed reaches."""
    H = np.maximum(np.asarray(H, np.int64), 0)
    P, Q = _padded(H.shape, 0)
    Q[...] = np.where(seeds_of(H, M), H, 0)
    offs = offsets(weights)
    tmp = np.empty(H.shape, np.int64)
    while True:
        before = Q.copy()
        for dx, dy, dz, _ in offs:
            np.minimum(_shift(P, H.shape, dx, dy, dz), H, out=tmp)
            np.maximum(Q, tmp, out=Q)
        if np.array_equal(before, Q):
            return Q.copy()


def ticks(H, M, weights, Q, cap=CAP):
    """int64 [z, y, x]: T of the reached voxels, BIG elsewhere."""
    H = np.asarray(H, np.int64)
    PQ, q = _padded(H.shape, 0)
    q[...] = Q
    reached = Q > 0
    offs = offsets(weights)
    source = seeds_of(H, M)
    for dx, dy, dz, _ in offs:
        source = source | (reached & (_shift(PQ, H.shape, dx, dy, dz) > H))
    free = reached & ~source
    same = [free & (_shift(PQ, H.shape, dx, dy, dz) == Q) for dx, dy, dz, _ in offs]     # the neighbours of equal level, once
    P, T = _padded(H.shape, BIG)
    T[source] = 0
    tmp = np.empty(H.shape, np.int64)
    while True:
        before = T.copy()
        for (dx, dy, dz, w), on in zip(offs, same):
            np.add(_shift(P, H.shape, dx, dy, dz), w, out=tmp)
            np.minimum(tmp, cap, out=tmp)
            np.minimum(T, np.where(on, tmp, BIG), out=T)
        if np.array_equal(before, T):
            return T.copy()


def labels(H, M, weights, Q, T, cap=CAP):
    """int64 [z, y, x]: L of the reached voxels, BIG elsewhere."""
    H, M = np.asarray(H, np.int64), np.asarray(M, np.int64)
    PQ, q = _padded(H.shape, 0)
    q[...] = Q
    PT, t = _padded(H.shape, BIG)
    t[...] = T
    seed = seeds_of(H, M)
    free = (Q > 0) & ~seed
    offs = offsets(weights)
    tight = []
    for dx, dy, dz, w in offs:
        qu, tu = _shift(PQ, H.shape, dx, dy, dz), _shift(PT, H.shape, dx, dy, dz)
        tight.append(free & ((qu > H) | ((qu == Q) & (np.minimum(tu + w, cap) == T))))
    P, L = _padded(H.shape, BIG)
    L[seed] = M[seed]
    while True:
        before = L.copy()
        for (dx, dy, dz, _), on in zip(offs, tight):
            np.minimum(L, np.where(on, _shift(P, H.shape, dx, dy, dz), BIG), out=L)
        if np.array_equal(before, L):
            return L.copy()


def finish(Q, T, L):
    """(labels, level, ticks int32 [z, y, x], reached) as the call writes them: 0 / 0 / -1 outside S and where not reached."""
    hit = Q > 0
    assert (L[hit] < BIG).all() and (T[hit] <= CAP).all()
    return (np.where(hit, L, 0).astype(np.int32), Q.astype(np.int32), np.where(hit, T, -1).astype(np.int32), int(hit.sum()))


def grow(H, M, weights, cap=CAP):
    """(labels, level, ticks, reached) by the three phases."""
    Q = level(H, M, weights)
    T = ticks(H, M, weights, Q, cap)
    return finish(Q, T, labels(H, M, weights, Q, T, cap))


def grow_frontier(H, M, weights, cap=CAP, chunk=1 << 17):
    """(labels, level, ticks, reached), the same three fixed points with a frontier: a round pulls, for the voxels with a neighbour
    that moved in the round before, the best value over all their neighbours (from the values of the round before), so a round
    costs its frontier, not the box.  For the grids on which the shifted views take many rounds; tests/test_host_grow.py holds it
    equal to grow()."""
    H, M = np.asarray(H, np.int64), np.asarray(M, np.int64)
    nz, ny, nx = H.shape
    offs = offsets(weights)
    flat = np.array([(dz * (ny + 2) + dy) * (nx + 2) + dx for dx, dy, dz, _ in offs], np.int64)
    w = np.array([o[3] for o in offs], np.int64)
    pad = lambda a, fill: np.pad(a, 1, constant_values=fill).reshape(-1)   # noqa: E731
    h, seed = pad(np.maximum(H, 0), 0), pad(seeds_of(H, M), False)

    def fixed_point(V, free, active, pull):
        while len(active):
            moved = []
            for i in range(0, len(active), chunk):
                idx = active[i:i + chunk]
                new = pull(idx, idx[:, None] + flat[None, :])
                ch = new != V[idx]
                moved.append((idx[ch], new[ch]))
            at = np.concatenate([m[0] for m in moved])
            V[at] = np.concatenate([m[1] for m in moved])            # (after every pull of the round: a Jacobi step)
            mark = np.zeros(len(V), bool)
            mark[(at[:, None] + flat[None, :]).reshape(-1)] = True
            active = np.flatnonzero(mark & free)

    Q = np.where(seed, h, 0)
    fixed_point(Q, h > 0, np.flatnonzero(h > 0), lambda idx, nb: np.maximum(Q[idx], np.minimum(Q[nb].max(axis=1), h[idx])))
    reached = Q > 0
    source = seed.copy()
    at = np.flatnonzero(reached)
    for i in range(0, len(at), chunk):
        idx = at[i:i + chunk]
        source[idx] |= (Q[idx[:, None] + flat[None, :]] > h[idx, None]).any(axis=1)
    T = np.where(source, 0, BIG)
    free = reached & ~source
    fixed_point(T, free, np.flatnonzero(free),
                lambda idx, nb: np.minimum(T[idx], np.where(Q[nb] == Q[idx, None], np.minimum(T[nb] + w[None, :], cap), BIG).min(axis=1)))
    L = np.where(seed, pad(M, 0), BIG)
    free = reached & ~seed

    def pull_label(idx, nb):
        tight = (Q[nb] > h[idx, None]) | ((Q[nb] == Q[idx, None]) & (np.minimum(T[nb] + w[None, :], cap) == T[idx, None]))
        return np.minimum(L[idx], np.where(tight, L[nb], BIG).min(axis=1))
    fixed_point(L, free, np.flatnonzero(free), pull_label)
    core = lambda a: a.reshape(nz + 2, ny + 2, nx + 2)[1:-1, 1:-1, 1:-1]   # noqa: E731
    return finish(core(Q), core(T), core(L))


def dijkstra(H, M, weights, cap=CAP):
    """(labels, level, ticks, reached): the joint key with a heap - the best key first: the highest Q, then the lowest T -, then
    the label pass over the voxels in the order they left the heap, repeated until it changes nothing (a tight neighbour left the
    heap earlier, except among the saturated)."""
    H, M = np.asarray(H, np.int64), np.asarray(M, np.int64)
    nz, ny, nx = H.shape
    offs = offsets(weights)
    h = H.tolist()
    key, order = {}, []
    best = {(int(x), int(y), int(z)): (-h[z][y][x], 0) for z, y, x in zip(*np.nonzero(seeds_of(H, M)))}
    heap = [(k[0], k[1], v) for v, k in best.items()]
    heapq.heapify(heap)
    while heap:
        nq, t, v = heapq.heappop(heap)
        if v in key:
            continue
        key[v] = (nq, t)
        order.append(v)
        x, y, z = v
        for dx, dy, dz, w in offs:
            X, Y, Z = x + dx, y + dy, z + dz
            if not (0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz) or h[Z][Y][X] <= 0:
                continue
            k = (-h[Z][Y][X], 0) if h[Z][Y][X] < -nq else (nq, min(t + w, cap))
            if k < best.get((X, Y, Z), (1, 0)):
                best[X, Y, Z] = k
                heapq.heappush(heap, (k[0], k[1], (X, Y, Z)))
    m = M.tolist()
    lab = {v: (m[v[2]][v[1]][v[0]] if m[v[2]][v[1]][v[0]] > 0 else BIG) for v in order}
    changed = True
    while changed:
        changed = False
        for v in order:
            x, y, z = v
            if m[z][y][x] > 0:
                continue
            nq, t = key[v]
            for dx, dy, dz, w in offs:
                u = (x + dx, y + dy, z + dz)
                if u not in key:
                    continue
                uq, ut = key[u]
                step = (-h[z][y][x], 0) if h[z][y][x] < -uq else (uq, min(ut + w, cap))
                if step == (nq, t) and lab[u] < lab[v]:
                    lab[v] = lab[u]
                    changed = True
    Q, T, L = np.zeros(H.shape, np.int64), np.full(H.shape, BIG, np.int64), np.full(H.shape, BIG, np.int64)
    for (x, y, z), (nq, t) in key.items():
        Q[z, y, x], T[z, y, x], L[z, y, x] = -nq, t, lab[x, y, z]
    return finish(Q, T, L)


# ---- generators (arrays [z, y, x]; dims are (nx, ny, nz)) -----------------------------------------------------------------------

def random_case(rng, dims, top, n_markers, density=0.7):
    """(H, M): a relief with values 0 .. top (0 with probability 1 - density) and n_markers markers of labels 1 .. n_markers at
    random voxels of the box, inside S or not."""
    shape = dims[::-1]
    H = np.where(rng.random(shape) < density, rng.integers(1, top + 1, shape), 0).astype(np.int32)
    M = np.zeros(shape, np.int32)
    for label in range(n_markers, 0, -1):
        z, y, x = (int(rng.integers(0, n)) for n in shape)
        M[z, y, x] = label
    return H, M


def pair_across(kind, descent, at=(64, 8, 8)):
    """(H, M, a, b): two voxels of a 70 x 12 x 12 box that touch only across the tile boundary at `at`: kind = the axes ("x", "y",
    "z") on which they differ - one axis: a face, two: an edge, three: the tile's corner.  The marker 5 is on a; descent: H is 2
    at a and 1 at b, else 1 at both."""
    H, M = np.zeros((12, 12, 70), np.int32), np.zeros((12, 12, 70), np.int32)
    b = tuple(at)
    a = tuple(c - (1 if ax in kind else 0) for c, ax in zip(at, "xyz"))
    H[a[2], a[1], a[0]] = 2 if descent else 1
    H[b[2], b[1], b[0]] = 1
    M[a[2], a[1], a[0]] = 5
    return H, M, a, b


def two_hills(dims=(140, 24, 24), at=64):
    """(H, M): two pyramids along x whose tops, marked 2 and 1, lie 12 voxels on either side of the tile boundary x = at; the
    valley is on the boundary."""
    nx, ny, nz = dims
    x = np.arange(nx)
    row = np.maximum(1, 20 - np.minimum(np.abs(x - (at - 12)), np.abs(x - (at + 12))))
    H = np.broadcast_to(row.astype(np.int32), (nz, ny, nx)).copy()
    M = np.zeros(H.shape, np.int32)
    M[nz // 2, ny // 2, at - 12], M[nz // 2, ny // 2, at + 12] = 2, 1
    return H, M
