"""numpy references for o2v_hip_thickness_dense and obj2voxel_amd.dense.local_thickness, inner_distance, erode, dilate, opening,
closing and thin_regions, on bool sets S [z, y, x].  numpy only.

    depth2       tests/distance_ref.py's separable transform from the voxels that are not in S, plus the border's min
    thickness    T as the literal scatter of the definition: every centre of S, unpruned, its ball clipped to the box, a maximum in
                 place - a numpy slice per centre, or (the same balls, for small caps) a shifted view per ball offset
    brute        the definition over all pairs of voxels in int64, for small boxes, several caps at once
    by_levels    T as a sweep over the distinct radii, one dilation each
    cover_table  L_k[R] by enumeration
    kept_centres the centres that the cover table does not prune, and their count: what the device's counters must show
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
