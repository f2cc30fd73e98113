"""The numpy reference of K23, the watershed basins of a relief merged by persistence (include/o2v_hip.h, o2v_hip_watershed_dense;
DESIGN.md section 26), in the words of the definition:

  Relief.  H is an int32 grid, indexed [z, y, x].
  The set.  S = { v : H[v] > 0 }.  Voxels outside the box are not in S.
  Index.  i(v) = (z * ny + y) * nx + x.
  Key.  K(v) = (H[v], i(v)), compared lexicographically: a strict total order.  Packed: H << 31 | i.
  Ascent.  For v in S, take the neighbour u of v in S with the greatest key (6, 18 or 26 neighbours).  If K(u) > K(v) then
  parent(v) = u, otherwise v is a peak.  basin(v) is the peak that v reaches.  Ascent by value, not by slope.
  Saddle.  Two basins A != B are adjacent if some u in A and v in B are neighbours; saddle(A, B) is the maximum over such pairs of
  min(H[u], H[v]).
  Persistence (elder rule).  The adjacent pairs sorted by (saddle descending, smaller peak index ascending, larger peak index
  ascending) are walked with a union-find over the peaks, each class represented by its peak of greatest key.  A pair that joins
  two classes kills the class whose representative p has the smaller key: pers(p) = H[p] - saddle, partner(p) = the other class's
  representative at that moment.  A class that is never killed has infinite persistence.
  Result for min_depth = h >= 0.  final(p) = p if pers(p) >= h, else final(partner(p)).  The label of v in S is 1 +
  rank(final(basin(v))), rank among the surviving peaks in ascending index; 0 outside S; count = the survivors.

numpy only: the ascent by shifted padded views of the packed key, the basins by pointer doubling, the pairs by the 13 forward
offsets and a lexsort, the elder-rule walk pair by pair."""
import numpy as np

INF = 1 << 62   # the persistence of a class that is never killed


def offsets(connectivity):
    """The offsets (dz, dy, dx) of the connectivity in ascending (dz, dy, dx) order - K20's order, k = 9 (dz + 1) + 3 (dy + 1) + dx + 1."""
    assert connectivity in (6, 18, 26)
    axes = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) != (0, 0, 0) and (dz != 0) + (dy != 0) + (dx != 0) <= axes]


def packed_keys(H):
    """int64 [z, y, x]: H << 31 | i in S, -1 outside."""
    H = np.asarray(H)
    i = np.arange(H.size, dtype=np.int64).reshape(H.shape)
    return np.where(H > 0, (H.astype(np.int64) << 31) | i, -1)


def ascent(H, connectivity):
    """The parents, flat int64: parent(v) in S, v itself for a peak, -1 outside S."""
    H = np.asarray(H)
    nz, ny, nx = H.shape
    K = packed_keys(H)
    pad = np.pad(K, 1, constant_values=-1)
    best = K.copy()
    for dz, dy, dx in offsets(connectivity):
        np.maximum(best, pad[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx], out=best)
    return np.where(K >= 0, best & 0x7fffffff, -1).ravel()


def basins(parent):
    """basin(v), flat int64, by pointer doubling; -1 outside S."""
    P = parent.copy()
    inside = np.flatnonzero(P >= 0)
    while True:
        Q = P[P[inside]]
        if np.array_equal(Q, P[inside]):
            return P
        P[inside] = Q


def adjacent_pairs(H, basin, connectivity):
    """(a, b, saddle, seen): the distinct adjacent basin pairs a < b (peak indices) in ascending (a, b) order with their saddles,
    and the number of neighbour pairs whose basins differ - each unordered pair looked at once, through its forward offset."""
    H = np.asarray(H)
    nz, ny, nx = H.shape
    B = basin.reshape(H.shape)
    lo, hi, val = [], [], []
    for dz, dy, dx in offsets(connectivity):
        if (dz, dy, dx) < (0, 0, 0):
            continue
        u = (slice(0, nz - dz), slice(max(0, -dy), ny - max(0, dy)), slice(max(0, -dx), nx - max(0, dx)))
        v = (slice(dz, nz), slice(max(0, dy), ny + min(0, dy)), slice(max(0, dx), nx + min(0, dx)))
        bu, bv = B[u], B[v]
        m = (bu >= 0) & (bv >= 0) & (bu != bv)
        lo.append(np.minimum(bu[m], bv[m]))
        hi.append(np.maximum(bu[m], bv[m]))
        val.append(np.minimum(H[u][m], H[v][m]).astype(np.int64))
    lo, hi, val = np.concatenate(lo), np.concatenate(hi), np.concatenate(val)
    seen = len(lo)
    if not seen:
        return lo, hi, val, 0
    order = np.lexsort((hi, lo))
    lo, hi, val = lo[order], hi[order], val[order]
    first = np.flatnonzero(np.r_[True, (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])])
    return lo[first], hi[first], np.maximum.reduceat(val, first), seen


class Watershed:
    """Everything the definition says of one relief and connectivity, computed once; labels(min_depth) for any depth."""

    def __init__(self, H, connectivity=26):
        self.H = np.asarray(H)
        assert self.H.ndim == 3 and self.H.size < 2 ** 31
        self.connectivity = connectivity
        self.parent = ascent(self.H, connectivity)
        self.basin = basins(self.parent)
        flat = self.H.ravel()
        self.peaks = np.flatnonzero(self.basin == np.arange(flat.size))          # ascending index: a peak's rank is its place
        self.heights = flat[self.peaks].astype(np.int64)
        self.a, self.b, self.saddle, self.seen = adjacent_pairs(self.H, self.basin, connectivity)
        self.pers, self.partner = self._elder()

    def _elder(self):
        n = len(self.peaks)
        ra, rb = np.searchsorted(self.peaks, self.a), np.searchsorted(self.peaks, self.b)
        order = np.lexsort((rb, ra, -self.saddle))
        rep = list(range(n))
        pers, partner = [INF] * n, [-1] * n
        h = self.heights.tolist()

        def find(p):
            while rep[p] != p:
                rep[p] = rep[rep[p]]
                p = rep[p]
            return p
        for e in order.tolist():
            p, q = find(int(ra[e])), find(int(rb[e]))
            if p == q:
                continue
            if (h[p], p) > (h[q], q):        # (ranks order as indices do)
                p, q = q, p
            pers[p], partner[p], rep[p] = h[p] - int(self.saddle[e]), q, q
        return pers, partner

    def final(self, min_depth):
        """final(p) per peak rank."""
        n = len(self.peaks)
        fin = [-1] * n
        for p in range(n):
            chain, f = [], p
            while fin[f] < 0 and self.pers[f] < min_depth:
                chain.append(f)
                f = self.partner[f]
            f = f if fin[f] < 0 else fin[f]
            fin[f] = f
            for c in chain:
                fin[c] = f
        return np.array(fin, np.int64).reshape(n)

    def labels(self, min_depth=0):
        """(labels int32 [z, y, x], count)."""
        fin = self.final(min_depth)
        alive = fin == np.arange(len(fin))
        number = np.cumsum(alive)                              # 1 + the rank among the survivors, at a survivor
        out = np.zeros(self.H.size, np.int32)
        inside = self.basin >= 0
        if len(fin):
            out[inside] = number[fin[np.searchsorted(self.peaks, self.basin[inside])]]
        return out.reshape(self.H.shape), int(alive.sum())


def watershed(H, min_depth=0, connectivity=26):
    """(labels, count) of the definition."""
    return Watershed(H, connectivity).labels(min_depth)


def part_peaks(labels, H, n):
    """Per label 1 .. n the voxel of greatest key: (int32 [n, 3] (x, y, z), int32 [n] heights)."""
    labels, H = np.asarray(labels), np.asarray(H)
    K = packed_keys(H).ravel()
    L = labels.ravel()
    order = np.lexsort((K, L))
    last = np.flatnonzero(np.r_[L[order][1:] != L[order][:-1], True])
    at = order[last][L[order][last] > 0]
    assert len(at) == n
    nz, ny, nx = H.shape
    return np.stack([at % nx, at // nx % ny, at // (nx * ny)], 1).astype(np.int32), H.ravel()[at].astype(np.int32)


# ---- the shapes of the pinned results ------------------------------------------------------------------------------------------------

def squared_edt(S):
    """The exact squared Euclidean distance of every voxel of S to the nearest voxel outside it (the outside of the box included),
    by brute force over the separable minima: int32."""
    S = np.asarray(S, bool)
    big = 1 << 30
    d = np.where(np.pad(S, 1), big, 0).astype(np.int64)
    for axis in range(3):
        n = d.shape[axis]
        idx = np.arange(n)
        cost = (idx[:, None] - idx[None, :]) ** 2                       # [to, from]
        d = np.moveaxis(d, axis, -1)
        d = (d[..., None, :] + cost).min(-1)
        d = np.moveaxis(d, -1, axis)
    return d[1:-1, 1:-1, 1:-1].astype(np.int32)


def dumbbell():
    """Two balls of radius 10 at x = 14 and x = 28 in 28 x 28 x 48 [z, y, x]: bool."""
    z, y, x = np.mgrid[0:28, 0:28, 0:48]
    return ((x - 14) ** 2 + (y - 14) ** 2 + (z - 14) ** 2 <= 100) | ((x - 28) ** 2 + (y - 14) ** 2 + (z - 14) ** 2 <= 100)


def flat_u():
    """H = 1 on rows y = 0 and y = 4 and column x = 0 of 1 x 5 x 9."""
    H = np.zeros((1, 5, 9), np.int32)
    H[0, 0, :] = H[0, 4, :] = H[0, :, 0] = 1
    return H


def random_relief(seed=1, shape=(17, 19, 70), high=6):
    return np.random.default_rng(seed).integers(0, high, shape).astype(np.int32)
