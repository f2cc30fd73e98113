"""numpy references for o2v_hip_thickness_dense and obj2voxel_amd.dense.local_thickness, inner_distance, erode, dilate, opening,
closing and thin_regions, on bool sets S [z, y, x].  numpy only.

    depth2       tests/distance_ref.py's separable transform from the voxels that are not in S, plus the border's min
    thickness    T as the literal scatter of the definition: every centre of S, unpruned, its ball clipped to the box, a maximum in
                 place - a numpy slice per centre, or (the same balls, for small caps) a shifted view per ball offset
    brute        the definition over all pairs of voxels in int64, for small boxes, several caps at once
    by_levels    T as a sweep over the distinct radii, one dilation each
    cover_table  L_k[R] by enumeration
    kept_centres the centres that the cover table does not prune, and their count: what the device's counters must show
    tile, tiled  a tile with an empty outer layer, and what its repetition gives: the reference of the boxes past 2^28 voxels
    line_reduction, line_visited   sets constant over a long box's cross-section, reduced to a line
    full_box_thickness             T of a full box with the border on, by levels in closed form
tests/test_host_thickness.py holds them against each other."""
import numpy as np

from tests import distance_ref as DR

INF = DR.INF
OFFSETS = ((1, 0, 0), (1, 1, 0), (1, 1, 1))   # the neighbour offsets v of k = |v|^2 = 1, 2, 3


def cap_of(radius):
    """floor(radius^2) + 1: the ball {|q|^2 < cap} is {|q| <= radius}."""
    return int(np.floor(float(radius) * float(radius))) + 1


def depth2(S, border):
    """int32 [z, y, x]: for p in S the smallest |p - e|^2 over the voxels e of the box not in S (border: and outside the box), INF
    where there is none; 0 outside S."""
    S = np.asarray(S, bool)
    d = DR.separable_d2((~S).astype(np.uint8)).astype(np.int64)
    if border:
        nz, ny, nx = S.shape
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        m = np.minimum(np.minimum(np.minimum(x + 1, nx - x), np.minimum(y + 1, ny - y)), np.minimum(z + 1, nz - z)).astype(np.int64)
        d = np.minimum(d, m * m)
    return np.where(S, d, 0).astype(np.int32)


def ball(R):
    """(mask [2 r + 1]^3 of {|q|^2 < R}, r) with r = the largest |q_i| in it."""
    r = int(np.floor(np.sqrt(R - 1)))
    while r * r > R - 1:
        r -= 1
    while (r + 1) * (r + 1) <= R - 1:
        r += 1
    a = np.arange(-r, r + 1, dtype=np.int64)
    return (a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2) < R, r


def scatter(Rc, centres=None):
    """int32 T from the radii Rc [z, y, x] (0: no centre): T(p) = max { Rc(c) : |p - c|^2 < Rc(c) }, balls clipped to the box.
    centres: a bool mask of the centres to scatter (all with Rc > 0 when None)."""
    Rc = np.asarray(Rc, np.int64)
    nz, ny, nx = Rc.shape
    T = np.zeros(Rc.shape, np.int64)
    use = Rc > 0 if centres is None else (np.asarray(centres, bool) & (Rc > 0))
    radii, counts = np.unique(Rc[use], return_counts=True)
    for R, n in zip(radii.tolist(), counts.tolist()):
        mask, r = ball(R)
        at = use & (Rc == R)
        if int(mask.sum()) * Rc.size < 4000 * n:
            # many centres of a small ball: per ball offset q, every centre of this radius at once (the same balls, the same maximum)
            for dz, dy, dx in (np.argwhere(mask) - r).tolist():
                if abs(dz) >= nz or abs(dy) >= ny or abs(dx) >= nx:
                    continue   # (past the box from every centre)
                src = at[max(0, -dz):nz - max(0, dz), max(0, -dy):ny - max(0, dy), max(0, -dx):nx - max(0, dx)]
                dst = T[max(0, dz):nz - max(0, -dz), max(0, dy):ny - max(0, -dy), max(0, dx):nx - max(0, -dx)]
                np.maximum(dst, np.where(src, R, 0), out=dst)
            continue
        part_of = np.where(mask, R, 0)
        for z, y, x in np.argwhere(at).tolist():
            z0, z1, y0, y1, x0, x1 = max(0, z - r), min(nz, z + r + 1), max(0, y - r), min(ny, y + r + 1), max(0, x - r), min(nx, x + r + 1)
            dst = T[z0:z1, y0:y1, x0:x1]
            np.maximum(dst, part_of[z0 - z + r:z1 - z + r, y0 - y + r:y1 - y + r, x0 - x + r:x1 - x + r], out=dst)
    return T.astype(np.int32)


def thickness(S, cap, border, d2=None):
    """int32 T [z, y, x] of the set S: the literal scatter over every centre of S with R = min(depth2, cap)."""
    d2 = depth2(S, border) if d2 is None else d2
    return scatter(np.minimum(d2.astype(np.int64), cap))


def open_only(S, cap, border, d2=None):
    """int32: what O2V_HIP_THICK_OPEN_ONLY gives - cap inside the opening by {|q|^2 < cap}, R(p) elsewhere in S, 0 outside S.  The
    opening is the dilation of the core {depth2 >= cap}: the voxels within |.|^2 < cap of it."""
    S = np.asarray(S, bool)
    d2 = depth2(S, border) if d2 is None else d2
    to_core = DR.separable_d2((d2 >= cap).astype(np.uint8))
    return np.where(S, np.where(to_core < cap, cap, np.minimum(d2, cap)), 0).astype(np.int32)


def as_float(T):
    """float32: 2 sqrt(T) - 1 in float64, rounded once; 0 where T is 0."""
    T = np.asarray(T)
    return np.where(T == 0, 0.0, 2.0 * np.sqrt(T.astype(np.float64)) - 1.0).astype(np.float32)


def brute(S, caps, border):
    """({cap: T}, depth2) by the definition over all pairs of voxels, int64: for boxes of a few thousand voxels."""
    S = np.asarray(S, bool)
    nz, ny, nx = S.shape
    p = np.indices(S.shape).reshape(3, -1).T.astype(np.int64)   # (z, y, x)
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    s = S.reshape(-1)
    big = np.int64(INF)
    dep = np.where(s[None, :], big, d).min(1) if (~s).any() else np.full(len(p), big)
    if border:
        m = np.minimum(np.minimum(np.minimum(p[:, 2] + 1, nx - p[:, 2]), np.minimum(p[:, 1] + 1, ny - p[:, 1])), np.minimum(p[:, 0] + 1, nz - p[:, 0]))
        dep = np.minimum(dep, m * m)
    dep = np.where(s, dep, 0)
    out = {}
    for cap in caps:
        R = np.minimum(dep, cap)
        T = np.where((d < R[None, :]) & s[None, :], R[None, :], 0).max(1)
        out[cap] = np.where(s, T, 0).reshape(S.shape).astype(np.int32)
    return out, dep.reshape(S.shape).astype(np.int32)


def by_levels(S, cap, border):
    """int32 T by a sweep over the distinct radii R of S's voxels, rising: T = R wherever a voxel lies within |.|^2 < R of the
    level set {min(depth2, cap) >= R} - its opening by the ball of R."""
    S = np.asarray(S, bool)
    Rc = np.minimum(depth2(S, border).astype(np.int64), cap)
    T = np.zeros(S.shape, np.int64)
    for R in np.unique(Rc[Rc > 0]).tolist():
        near = DR.separable_d2((Rc >= R).astype(np.uint8)) < R
        T[near] = R
    return T.astype(np.int32)


def cover_table(cap):
    """uint32 [3, cap + 1]: L_k[R] = 1 + max { |q - v|^2 : |q|^2 < R } for v = OFFSETS[k - 1], by enumeration; column 0 is 0."""
    out = np.zeros((3, cap + 1), np.uint32)
    r = int(np.sqrt(cap)) + 1
    a = np.arange(-r, r + 1, dtype=np.int64)
    z, y, x = np.meshgrid(a, a, a, indexing="ij")
    q2 = x * x + y * y + z * z
    for k, (vx, vy, vz) in enumerate(OFFSETS):
        f = (x - vx) ** 2 + (y - vy) ** 2 + (z - vz) ** 2
        for R in range(1, cap + 1):
            out[k, R] = 1 + f[q2 < R].max()
    return out


def cover_entry(R):
    """(L_1[R], L_2[R], L_3[R]) by enumeration over the ball of R alone."""
    r = int(np.sqrt(R)) + 1
    a = np.arange(-r, r + 1, dtype=np.int64)
    z, y, x = np.meshgrid(a, a, a, indexing="ij")
    inside = x * x + y * y + z * z < R
    return tuple(int(1 + ((x - vx) ** 2 + (y - vy) ** 2 + (z - vz) ** 2)[inside].max()) for vx, vy, vz in OFFSETS)


def kept_centres(S, cap, border, table=None, d2=None):
    """(candidates, kept): bool masks of the ball centres - the voxels of S with depth2 < cap - and of those among them that no
    26-neighbour covers: R(c + v) >= L_|v|^2[R(c)] for no v.  table: cover_table(cap) or the library's."""
    S = np.asarray(S, bool)
    d2 = depth2(S, border) if d2 is None else d2
    table = cover_table(cap) if table is None else np.asarray(table)
    Rc = np.minimum(d2.astype(np.int64), cap)
    cand = S & (d2 < cap)
    nz, ny, nx = S.shape
    pad = np.zeros((nz + 2, ny + 2, nx + 2), np.int64)
    pad[1:-1, 1:-1, 1:-1] = Rc
    covered = np.zeros(S.shape, bool)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = dx * dx + dy * dy + dz * dz
                if k:
                    covered |= pad[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx] >= table[k - 1].astype(np.int64)[Rc]
    return cand, cand & ~covered


def pruned(S, cap, border, table=None):
    """int32 T the way the device builds it: the opening first, then the balls of the kept centres only."""
    d2 = depth2(S, border)
    _, kept = kept_centres(S, cap, border, table, d2)
    return np.maximum(open_only(S, cap, border, d2), scatter(np.minimum(d2.astype(np.int64), cap), kept))


def visited(S, cap, border, table=None):
    """The ball voxels the kept centres' balls hold inside the box, over all of them: the device's third counter."""
    S = np.asarray(S, bool)
    d2 = depth2(S, border)
    _, kept = kept_centres(S, cap, border, table, d2)
    nz, ny, nx = S.shape
    n = 0
    for z, y, x in np.argwhere(kept).tolist():
        mask, r = ball(int(d2[z, y, x]))
        n += int(mask[max(0, r - z):r + nz - z, max(0, r - y):r + ny - y, max(0, r - x):r + nx - x].sum())
    return n


def visited_small(d2, kept):
    """visited() from depth2 and the kept centres, per ball offset and all centres of a radius at once: for many centres of small
    balls (the long boxes, where the border keeps every radius^2 at most 4)."""
    d2, kept = np.asarray(d2), np.asarray(kept, bool)
    nz, ny, nx = d2.shape
    n = 0
    for R in np.unique(d2[kept]).tolist():
        mask, r = ball(R)
        at = kept & (d2 == R)
        for dz, dy, dx in (np.argwhere(mask) - r).tolist():
            if abs(dz) < nz and abs(dy) < ny and abs(dx) < nx:
                n += int(at[max(0, -dz):nz - max(0, dz), max(0, -dy):ny - max(0, dy), max(0, -dx):nx - max(0, dx)].sum())
    return n


# ---- the derived grids of obj2voxel_amd.dense -----------------------------------------------------------------------------------

def erode(S, radius, border=True):
    return depth2(S, border) > cap_of(radius) - 1


def opening(S, radius, border=True):
    cap = cap_of(radius)
    return open_only(S, cap, border) == cap


def dilate(S, radius):
    return ~erode(~np.asarray(S, bool), radius, False)


def closing(S, radius):
    return ~opening(~np.asarray(S, bool), radius, False)


def thin_regions(S, min_thickness, border=True):
    return np.asarray(S, bool) & ~opening(S, (float(min_thickness) - 1.0) / 2.0, border)


# ---- sets -------------------------------------------------------------------------------------------------------------------------

def digital_ball(dims, centre, radius):
    """bool [z, y, x] of dims (nx, ny, nz): (x - cx)^2 + (y - cy)^2 + (z - cz)^2 < radius^2."""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 < radius * radius


def plate(dims, axis, first, width):
    """bool [z, y, x] of dims (nx, ny, nz): the layers first .. first + width - 1 along axis (0: x, 1: y, 2: z)."""
    S = np.zeros(dims[::-1], bool)
    sl = [slice(None)] * 3
    sl[2 - axis] = slice(first, first + width)
    S[tuple(sl)] = True
    return S


# ---- tiles that do not see each other -------------------------------------------------------------------------------------------
#
# A tile P whose outermost voxel layer is empty on all six sides, repeated: G = np.tile(P, reps).  The clamp of a voxel outside a tile
# to the tile's box is an empty voxel of that tile and at least as near, coordinate by coordinate, so depth2 of a voxel of S is
# decided inside its own tile, every ball stays inside its tile's content, and the neighbours across a tile boundary have depth 0
# and cover nothing: T, depth2 and OPEN_ONLY of G are the tile's repeated, the candidates, kept centres and ball voxels prod(reps)
# times the tile's, with the border on or off (the tile's values are those of border=False).  tests/test_host_thickness.py holds
# this against the literal reference; the GPU cases past 2^28 voxels rest on it.

def outer_layer_empty(P):
    P = np.asarray(P, bool)
    return not (P[0].any() or P[-1].any() or P[:, 0].any() or P[:, -1].any() or P[:, :, 0].any() or P[:, :, -1].any())


def tile(dims, cap, seed, balls, noise=0.004, holes=0.002, table=None):
    """bool [z, y, x] of dims (nx, ny, nz): the digital balls ((cx, cy, cz), radius), a one-voxel plate, a rod along x in the last
    row of content (y = ny - 2, z = nz - 2), some noise and a few holes, the outer layer cleared.  Asserts what the large cases rely
    on at `cap`: a core (depth2 >= cap somewhere), voxels of S outside the opening, 0 < kept centres < candidates, a kept centre in
    the last row of content (so the largest listed index of a repetition lies in its last row of content).  table: the cover table
    of cap (by enumeration when None)."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    S = rng.random(dims[::-1]) < noise
    for c, rad in balls:
        S |= digital_ball(dims, c, rad)
    S[nz // 3, 2:ny // 2, nx // 2:] = True
    S &= ~(rng.random(dims[::-1]) < holes)
    S[nz - 2, ny - 2, :] = True
    S[0] = S[-1] = S[:, 0] = S[:, -1] = S[:, :, 0] = S[:, :, -1] = False
    assert outer_layer_empty(S)
    d2 = depth2(S, False)
    assert np.array_equal(d2, depth2(S, True))
    low = open_only(S, cap, False, d2)
    cand, kept = kept_centres(S, cap, False, table, d2)
    assert (d2 >= cap).any() and (low == cap).any() and (S & (low != cap)).any(), "the tile needs a core and voxels outside its opening"
    assert 0 < kept.sum() < cand.sum() and kept[nz - 2, ny - 2].any(), (int(kept.sum()), int(cand.sum()))
    return S


def tiled(P, reps, cap, table=None):
    """What the repetition np.tile(P, reps) (reps along z, y, x) must give at `cap`, from the tile alone: dict of T, depth2, open
    (int32 [z, y, x] of the tile, to be repeated), candidates, kept, visited (counts of the whole repetition), and last: the
    largest linear index of a kept centre in the repetition."""
    P = np.asarray(P, bool)
    assert outer_layer_empty(P)
    d2 = depth2(P, False)
    cand, kept = kept_centres(P, cap, False, table, d2)
    n = int(np.prod(reps))
    nz, ny, nx = P.shape
    z, y, x = np.argwhere(kept)[-1].tolist()   # (row-major: the last kept centre of the tile, so of the last tile)
    Z, Y, X = z + (reps[0] - 1) * nz, y + (reps[1] - 1) * ny, x + (reps[2] - 1) * nx
    return dict(T=thickness(P, cap, False, d2), depth2=d2, open=open_only(P, cap, False, d2), candidates=n * int(cand.sum()), kept=n * int(kept.sum()),
                visited=n * visited(P, cap, False, table), last=(Z * reps[1] * ny + Y) * reps[2] * nx + X)


# ---- sets that are constant over the cross-section of a long box ------------------------------------------------------------------
#
# S = {voxels whose coordinate u along one axis lies in a set of runs}, border off.  Everything reduces to the line along u:
# depth(u) is the distance to the nearest gap position (the ends of the box do not count), R = min(depth^2, cap),
# T(u) = max { R(u') : (u - u')^2 < R(u') } (the centre with the same cross-section offset is the best one), the opening is what
# lies within (u - u')^2 < cap of a u' with R(u') = cap, and a centre is kept exactly when neither axis neighbour reaches
# L_1[R(u)] (the off-axis neighbours have the axis neighbours' radii and need L_2, L_3 >= L_1; a neighbour at the same u has
# R(u) < L_k[R(u)]).  tests/test_host_thickness.py holds this against the literal reference on a short box.

LONG = 46341   # the longest axis accepted: (LONG - 1)^2 + 20 <= 2^31 - 2
LONG_SHAPES = [(3, 5, LONG), (3, LONG, 5), (LONG, 3, 4)]   # [z, y, x]: x, y, z long
SHORT_SHAPES = [(3, 5, 640), (3, 640, 5), (640, 3, 4)]


def runs_line(n, seed, longest=300):
    """bool [n]: runs of 1 .. longest positions separated by gaps of 1 .. 3; the first starts at 0, the last goes through the end."""
    rng = np.random.default_rng(seed)
    line = np.zeros(n, bool)
    u = 0
    while u < n:
        run = int(rng.integers(1, longest + 1))
        if n - (u + run) < 4:      # (no gap left behind it: the run goes through the far end, at least 4 long)
            run = n - u
        line[u:u + run] = True
        u += run + int(rng.integers(1, 4))
    assert line[0] and line[-1] and not line.all()
    return line


def _shifted(a, k, fill=0):
    """b[u] = a[u + k], fill past the ends."""
    out = np.full_like(a, fill)
    if k >= 0:
        out[:len(a) - k] = a[k:]
    else:
        out[-k:] = a[:len(a) + k]
    return out


def line_reduction(line, cap, table):
    """Per position u of the line (bool [n], at least one gap), border off: dict of int32 T, depth2, open, and bool candidates,
    kept.  table: the cover table of cap ([3, cap + 1])."""
    line = np.asarray(line, bool)
    n = len(line)
    assert not line.all()
    idx = np.arange(n, dtype=np.int64)
    big = np.int64(1) << 40
    left = np.maximum.accumulate(np.where(~line, idx, -big))
    right = np.minimum.accumulate(np.where(~line, idx, big)[::-1])[::-1]
    d = np.minimum(idx - left, right - idx)
    d2 = np.where(line, d * d, 0)
    R = np.minimum(d2, cap)
    w = int(np.floor(np.sqrt(cap - 1)))
    while w * w > cap - 1:
        w -= 1
    T = np.zeros(n, np.int64)
    near = np.zeros(n, bool)
    for k in range(-min(w, n - 1), min(w, n - 1) + 1):
        Rk = _shifted(R, k)
        T = np.maximum(T, np.where(k * k < Rk, Rk, 0))
        if k * k < cap:
            near |= Rk == cap
    cand = line & (d2 < cap)
    need = np.asarray(table)[0].astype(np.int64)[R]
    kept = cand & (np.maximum(_shifted(R, -1), _shifted(R, 1)) < need)
    return dict(T=np.where(line, T, 0).astype(np.int32), depth2=d2.astype(np.int32), open=np.where(line, np.where(near, cap, R), 0).astype(np.int32),
                candidates=cand, kept=kept)


def line_visited(red, cross):
    """The ball voxels inside a box of cross-section `cross` (a, b) of the kept centres of a line_reduction: for the centre at
    (u, c) and the cross-section position c', the positions u' with (u - u')^2 < R(u) - |c - c'|^2, clipped to the line."""
    n = len(red["kept"])
    u = np.nonzero(red["kept"])[0].astype(np.int64)
    R = red["depth2"].astype(np.int64)[u]
    total = 0
    a, b = cross
    for da in range(-(a - 1), a):
        for db in range(-(b - 1), b):
            pairs = (a - abs(da)) * (b - abs(db))      # ordered pairs (c, c') of the cross-section with this offset
            rem = R - (da * da + db * db)
            ok = rem > 0
            h = np.floor(np.sqrt(np.maximum(rem - 1, 0).astype(np.float64))).astype(np.int64)
            h = np.where(h * h > rem - 1, h - 1, h)
            h = np.where((h + 1) * (h + 1) <= rem - 1, h + 1, h)
            cnt = np.minimum(u + h, n - 1) - np.maximum(u - h, 0) + 1
            total += pairs * int(cnt[ok].sum())
    return total


def full_box_thickness(dims, cap):
    """int32 T [z, y, x] of the full box of dims (nx, ny, nz) with the border on, by levels in closed form: depth2' is m^2, the level
    set {m >= k} is the box shrunk by k - 1 voxels on every side, and the squared distance to a box is the sum of the squared
    overshoots per axis: T = max { min(k^2, cap) : dist2(p, {m >= k}) < min(k^2, cap) }.  (Past k^2 >= cap the level sets only
    shrink and R stays the cap, so they add nothing.)  For boxes whose literal scatter is out of reach."""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij", sparse=True)
    T = np.zeros((nz, ny, nx), np.int64)
    for k in range(1, (min(dims) + 1) // 2 + 1):
        R = min(k * k, cap)
        over = [np.maximum(np.maximum(k - 1 - c, c - (n - k)), 0) for c, n in ((x, nx), (y, ny), (z, nz))]
        T = np.where(over[0] ** 2 + over[1] ** 2 + over[2] ** 2 < R, R, T)
    return T.astype(np.int32)


def along(v, shape, axis):
    """The values v [n] of a line along `axis` of [z, y, x] (0: z) spread over a box of `shape`, a copy."""
    sl = [None, None, None]
    sl[axis] = slice(None)
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v)[tuple(sl)], shape))


def border_term(shape):
    """int64 [z, y, x]: m^2 with m = the distance to the nearest voxel outside the box along the axes."""
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij", sparse=True)
    m = np.minimum(np.minimum(np.minimum(x + 1, nx - x), np.minimum(y + 1, ny - y)), np.minimum(z + 1, nz - z)).astype(np.int64)
    return m * m
