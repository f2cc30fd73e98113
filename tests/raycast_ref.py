"""The definition of o2v_hip_raycast (include/o2v_hip.h) in numpy float64: the fine walk, cell by cell.
Nothing here skips a cell; the device must return these bits for every ray.

cast_lockstep walks all rays together, one fine step per iteration, finished rays dropped.  A ray that starts far from the box
(more than FAR cells) would keep that loop running for millions of iterations with a handful of rays in it, so cast() hands such
rays to walk_events: the same walk for one ray, vectorised along its steps instead of across rays - the planes of a chunk per
axis, merged in order of (T, axis) (per axis T rises, which the function asserts, so the merge is step 1 of the walk), every
cell after every event tested.  tests/test_host_raycast.py pins the two equal.

Grids are [z, y, x] arrays; `solid` is the bool array of the solid predicate, `origin` = (ox, oy, oz)."""
import numpy as np

F = np.float32
D = np.float64
LIMIT = 2.0 ** 22     # |o_a| above this: an invalid ray
FAR = 1024            # cast(): rays that start farther than this from the box go through walk_events


def solid_u8(grid):
    return np.asarray(grid) != 0


def solid_bits(words, nx=None):
    """words int32 / uint32 [nz, ny, W]: bit x % 32 of word x / 32; nx (default 32 W) voxels along x."""
    w = np.ascontiguousarray(words).view(np.uint32)
    bits = (w[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    out = bits.reshape(w.shape[0], w.shape[1], -1).astype(bool)
    return out if nx is None else out[:, :, :nx]


def solid_f32(field, level):
    with np.errstate(invalid="ignore"):
        return np.asarray(field, F) < F(level)


def pack_bits(solid):
    """The int32 words [nz, ny, ceil(nx / 32)] of a bool grid, as o2v_hip_write_dense BITS lays them out."""
    nz, ny, nx = solid.shape
    W = (nx + 31) // 32
    padded = np.zeros((nz, ny, W * 32), np.uint32)
    padded[:, :, :nx] = solid
    return (padded.reshape(nz, ny, W, 32) << np.arange(32, dtype=np.uint32)).sum(axis=3, dtype=np.uint32).view(np.int32)


def is_solid(solid, origin, c):
    """c int64 [m, 3] global cells (x, y, z): in the box and solid."""
    nz, ny, nx = solid.shape
    l = c - np.asarray(origin, np.int64)
    inb = (l >= 0).all(axis=1) & (l[:, 0] < nx) & (l[:, 1] < ny) & (l[:, 2] < nz)
    out = np.zeros(len(c), bool)
    out[inb] = solid[l[inb, 2], l[inb, 1], l[inb, 0]]
    return out


def gone(solid, origin, c, s):
    """c [m, 3], s [m, 3] (or [3]): the ray has left the box on an axis for good."""
    nz, ny, nx = solid.shape
    lo = np.asarray(origin, np.int64)
    hi = lo + np.array([nx, ny, nz], np.int64)
    below, above = c < lo, c >= hi
    return (((s > 0) & above) | ((s < 0) & below) | ((s == 0) & (below | above))).any(axis=1)


def setup(o32, d32):
    """(valid, o, d, s, inv, c, nxt) of float32 rays [n, 3]; the arrays after `valid` hold the valid rays only."""
    o32, d32 = np.asarray(o32, F).reshape(-1, 3), np.asarray(d32, F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(o32).all(axis=1) & np.isfinite(d32).all(axis=1) & (np.abs(o32) <= F(LIMIT)).all(axis=1)
    o, d = o32[valid].astype(D), d32[valid].astype(D)
    s = (d > 0).astype(np.int64) - (d < 0).astype(np.int64)
    inv = np.zeros_like(d)
    inv[s != 0] = 1.0 / d[s != 0]
    c = np.floor(o).astype(np.int64)
    nxt = c + (s > 0)
    return valid, o, d, s, inv, c, nxt


def plane_T(i, o, inv):
    """T_a(i) = ((double) i - o_a) * inv_a, op by op."""
    return (np.asarray(i).astype(D) - o) * inv


def cast_lockstep(solid, origin, o32, d32, t_max=np.inf):
    """(hit int32 [n, 4], t float32 [n], fine steps taken) by the walk of the header, all rays in lockstep."""
    valid, o, d, s, inv, c, nxt = setup(o32, d32)
    n = len(valid)
    hit, t = np.full((n, 4), -1, np.int32), np.full(n, np.inf, F)
    hit[~valid, 3] = -2
    t[~valid] = np.nan
    tmax = D(F(t_max))
    idx = np.nonzero(valid)[0]
    start = is_solid(solid, origin, c)
    hit[idx[start], :3], t[idx[start]] = c[start], 0
    keep = ~start
    idx, o, s, inv, c, nxt = idx[keep], o[keep], s[keep], inv[keep], c[keep], nxt[keep]
    steps = 0
    while len(idx):
        T = np.where(s != 0, plane_T(nxt, o, inv), np.inf)
        a = np.argmin(T, axis=1)                      # (the first of equal ones: the lowest axis)
        ar = np.arange(len(idx))
        Ta = T[ar, a]
        go = (s != 0).any(axis=1) & ~(Ta > tmax)
        idx, o, s, inv, c, nxt, a, Ta = idx[go], o[go], s[go], inv[go], c[go], nxt[go], a[go], Ta[go]
        ar = np.arange(len(idx))
        sa = s[ar, a]
        c[ar, a] += sa
        nxt[ar, a] += sa
        steps += len(idx)
        sol = is_solid(solid, origin, c)
        hit[idx[sol], :3], hit[idx[sol], 3] = c[sol], 2 * a[sol] + (sa[sol] < 0)
        with np.errstate(over="ignore"):
            t[idx[sol]] = Ta[sol].astype(F)
        keep = ~sol & ~gone(solid, origin, c, s)
        idx, o, s, inv, c, nxt = idx[keep], o[keep], s[keep], inv[keep], c[keep], nxt[keep]
    return hit, t, steps


def walk_events(solid, origin, o32, d32, t_max=np.inf, first_chunk=4096, max_chunk=1 << 18):
    """(hit int32 [4], t float32, fine steps) of one ray: the same walk, a chunk of events at a time.  Per axis the next K_a
    planes are laid out; the merge is complete up to the earliest of the axes' last events, and that far every cell is tested.
    K_a follows what the axis used, so an axis that hardly moves does not cost what the fast one costs."""
    valid, o, d, s, inv, c, nxt = setup(o32, d32)
    if not valid[0]:
        return np.array([-1, -1, -1, -2], np.int32), F(np.nan), 0
    o, s, inv, c, nxt = o[0], s[0], inv[0], c[0], nxt[0]
    miss = np.array([-1, -1, -1, -1], np.int32), F(np.inf)
    tmax = D(F(t_max))
    if is_solid(solid, origin, c[None])[0]:
        return np.array([c[0], c[1], c[2], -1], np.int32), F(0), 0
    K, steps = [first_chunk] * 3, 0
    while True:
        Ts, As, end = [], [], None
        for a in range(3):
            if s[a] != 0:
                Ta = plane_T(nxt[a] + s[a] * np.arange(K[a], dtype=np.int64), o[a], inv[a])
                assert (np.diff(Ta) >= 0).all(), "T_a does not rise along the stepping direction"
                Ts.append(Ta)
                As.append(np.full(K[a], a, np.int64))
                end = (Ta[-1], a) if end is None else min(end, (Ta[-1], a))
        if not Ts:
            return miss + (steps,)
        T, A = np.concatenate(Ts), np.concatenate(As)
        order = np.argsort(T, kind="stable")         # by T, equal ones in axis order (the axes' runs lie end to end)
        T, A = T[order], A[order]
        n = int(np.count_nonzero((T < end[0]) | ((T == end[0]) & (A <= end[1]))))   # the events up to `end`: a prefix
        T, A = T[:n], A[:n]
        cells = np.empty((n, 3), np.int64)
        count = np.zeros(3, np.int64)
        for a in range(3):
            n_a = np.cumsum(A == a)
            cells[:, a] = c[a] + s[a] * n_a
            count[a] = n_a[-1]
        past = T > tmax
        sol = is_solid(solid, origin, cells)
        stop = past | sol | gone(solid, origin, cells, s[None, :])
        if stop.any():
            k = int(np.argmax(stop))
            if past[k]:
                return miss + (steps + k,)
            if sol[k]:
                with np.errstate(over="ignore"):
                    return np.array([*cells[k], 2 * A[k] + (s[A[k]] < 0)], np.int32), T[k].astype(F), steps + k + 1
            return miss + (steps + k + 1,)
        c, nxt, steps = cells[-1].copy(), nxt + s * count, steps + n
        K = [min(2 * K[a], max_chunk) if a == end[1] else int(min(max_chunk, 2 * count[a] + 16)) for a in range(3)]


def distance_to_box(solid, origin, o32):
    """Chebyshev distance (cells) of the rays' start cells from the box; 0 inside."""
    nz, ny, nx = solid.shape
    lo = np.asarray(origin, D)
    hi = lo + np.array([nx, ny, nz], D)
    with np.errstate(invalid="ignore"):
        o = np.nan_to_num(np.asarray(o32, F).reshape(-1, 3).astype(D), nan=0.0, posinf=0.0, neginf=0.0)
    return np.maximum(np.maximum(lo - o, o - hi), 0).max(axis=1)


def cast(solid, origin, o32, d32, t_max=np.inf):
    """(hit, t, fine steps): cast_lockstep for the rays near the box, walk_events for each of the others."""
    o32, d32 = np.asarray(o32, F).reshape(-1, 3), np.asarray(d32, F).reshape(-1, 3)
    far = distance_to_box(solid, origin, o32) > FAR
    hit, t, steps = cast_lockstep(solid, origin, o32[~far], d32[~far], t_max)
    out_hit, out_t = np.empty((len(o32), 4), np.int32), np.empty(len(o32), F)
    out_hit[~far], out_t[~far] = hit, t
    for i in np.nonzero(far)[0]:
        out_hit[i], out_t[i], k = walk_events(solid, origin, o32[i:i + 1], d32[i:i + 1], t_max)
        steps += k
    return out_hit, out_t, steps


def same(a, b):
    """hit and t of two results equal as integers, bit for bit (t as its uint32 bits: NaN and inf count)."""
    return (np.array_equal(np.asarray(a[0], np.int32), np.asarray(b[0], np.int32)) and
            np.array_equal(np.asarray(a[1], F).view(np.uint32), np.asarray(b[1], F).view(np.uint32)))


# ---- grids and ray sets of the tests ---------------------------------------------------------------------------------------

def random_solid(rng, dims, density):
    """A bool grid [nz, ny, nx] of dims = (nx, ny, nz): sparse noise and one filled box, so that most 64^3, 16^3 and 4^3 blocks
    of a large grid are empty, some are crowded, and at least one voxel is solid."""
    nx, ny, nz = dims
    solid = rng.random((nz, ny, nx)) < density
    lo = [int(rng.integers(0, n)) for n in (nz, ny, nx)]
    hi = [min(n, a + 1 + int(rng.integers(0, max(1, n // 3)))) for a, n in zip(lo, (nz, ny, nx))]
    solid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    return solid


def ray_set(rng, solid, origin, n=20000, far=200, limit=8):
    """(origins, directions) float32 [m, 3], m >= n: a mix of
      rays from around the box at the centres (and faces' edges) of solid cells: they hit;
      rays from outside that point away from the box, or anywhere: they miss, or graze;
      random origins and targets in and around the box;
      lattice rays (integer and half-integer origins, small integer directions: ties on every step) and axis-parallel rays;
      invalid rays (NaN, inf, an origin past 2^22);
      `far` rays from up to 2 10^5 cells away and `limit` from 2^22 away along one axis, aimed at the box."""
    nz, ny, nx = solid.shape
    dims = np.array([nx, ny, nz], D)
    lo = np.asarray(origin, D)
    hi, mid, size = lo + dims, lo + dims / 2, float(dims.max())
    cells = np.argwhere(solid)[:, ::-1].astype(D) + lo            # (x, y, z) of the solid cells
    O, Dd = [], []

    def around(m, reach=1.5):
        """m points around the box, most of them outside"""
        return mid + (rng.random((m, 3)) - 0.5) * (dims + 2 * reach * size * rng.random((m, 1)))

    def outside(m):
        p = around(m)
        axis = rng.integers(0, 3, m)
        side = rng.integers(0, 2, m)
        ar = np.arange(m)
        p[ar, axis] = np.where(side == 1, hi[axis] + 0.5 + rng.random(m) * size, lo[axis] - 0.5 - rng.random(m) * size)
        return p

    # aimed at solid cells
    m = int(n * 0.36)
    if len(cells):
        target = cells[rng.integers(0, len(cells), m)] + 0.5
        edge = rng.random(m) < 0.25          # the middle of an edge of the cell: two coordinates on planes
        off = rng.integers(0, 2, (m, 3)).astype(D) - 0.5
        off[np.arange(m), rng.integers(0, 3, m)] = 0.0
        target = np.where(edge[:, None], target + off, target)
        o = np.where(rng.random((m, 1)) < 0.8, outside(m), around(m, 0.2))
        O.append(o)
        Dd.append((target - o) * (0.25 + rng.random((m, 1)) * 4))
    # from outside, pointing away from the box or anywhere
    m = int(n * 0.26)
    o = outside(m)
    away = (o - mid) * (0.1 + rng.random((m, 1))) + (rng.random((m, 3)) - 0.5) * 0.2 * size
    d = np.where(rng.random((m, 1)) < 0.7, away, rng.normal(size=(m, 3)))
    O.append(o)
    Dd.append(d)
    # random origins and targets
    m = int(n * 0.2)
    o = around(m, 0.6)
    O.append(o)
    Dd.append(around(m, 0.1) - o)
    # lattice rays
    m = int(n * 0.1)
    o = np.floor(around(m, 0.3)) + rng.integers(0, 2, (m, 3)) * 0.5
    O.append(o)
    Dd.append(rng.integers(-3, 4, (m, 3)).astype(D))
    # axis-parallel rays, some along cell faces and edges
    m = int(n * 0.07)
    o = around(m, 0.3)
    o = np.where(rng.random((m, 3)) < 0.3, np.floor(o), o)
    d = np.zeros((m, 3))
    d[np.arange(m), rng.integers(0, 3, m)] = rng.choice([-1.0, 1.0, 0.37, -2.5], m)
    d[rng.random(m) < 0.1] = 0.0             # d = 0: only the start cell
    d[rng.random((m, 3)) < 0.05] = -0.0
    O.append(o)
    Dd.append(d)
    # invalid rays
    m = max(6, n - sum(len(x) for x in O))
    o, d = around(m), rng.normal(size=(m, 3))
    bad = rng.choice([np.nan, np.inf, -np.inf, 2.0 ** 22 + 1, -2.0 ** 23], m)
    which = rng.integers(0, 6, m)
    both = np.concatenate([o, d], axis=1)
    both[np.arange(m), which] = np.where((which >= 3) & (np.abs(bad) < 1e9), np.nan, bad)
    O.append(both[:, :3])
    Dd.append(both[:, 3:])
    # far rays, aimed at the box: a long way to its entry
    if far:
        # (most within 2 10^4 cells, one in sixteen up to 2 10^5: the reference walks every cell of the way)
        dist = np.exp(rng.uniform(np.log(2.0 * FAR), np.where(np.arange(far) % 16 == 0, np.log(2e5), np.log(2e4))))
        u = rng.normal(size=(far, 3))
        u /= np.abs(u).max(axis=1, keepdims=True)
        o = np.clip(mid + u * (dist[:, None] + size), -LIMIT, LIMIT)
        target = lo + rng.random((far, 3)) * dims
        O.append(o)
        Dd.append((target - o) * rng.choice([1.0, 1e-3, 7.0], (far, 1)))
    if limit:
        axis = np.arange(limit) % 3
        sign = np.where(np.arange(limit) % 2 == 0, 1.0, -1.0)
        o = lo + rng.random((limit, 3)) * dims
        o[np.arange(limit), axis] = sign * LIMIT
        target = lo + rng.random((limit, 3)) * dims
        if len(cells):
            target[: limit // 2] = cells[rng.integers(0, len(cells), limit // 2)] + 0.5
        O.append(o)
        Dd.append(target - o)
    o, d = np.concatenate(O).astype(F), np.concatenate(Dd).astype(F)
    order = rng.permutation(len(o))          # (the families mixed over the wavefronts)
    return o[order], d[order]


def shares(hit):
    """(share of rays that hit, share that miss)"""
    hit = np.asarray(hit)
    return float((hit[:, 0] >= 0).mean()), float((hit[:, 3] == -1).mean() - ((hit[:, 3] == -1) & (hit[:, 0] >= 0)).mean())


def extreme_rays(rng, solid, origin, m=4000):
    """Rays whose direction components are denormal (1e-42), huge (3e38), -0.0 or small integers, from origins exactly on
    planes, edges and corners of cells in and around the box."""
    nz, ny, nx = solid.shape
    dims = np.array([nx, ny, nz], D)
    lo = np.asarray(origin, D)
    o = lo + np.floor((rng.random((m, 3)) * 1.6 - 0.3) * dims)
    o += np.where(rng.random((m, 3)) < 0.6, 0.0, rng.choice([0.5, 0.25, 1e-30, 0.99999994], (m, 3)))
    d = rng.choice(np.array([1e-42, -1e-42, 3e38, -3e38, -0.0, 0.0, 1.0, -1.0, 0.5, -2.0, 3.0], D), (m, 3))
    return o.astype(F), d.astype(F)
