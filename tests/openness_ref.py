"""The numpy reference of o2v_hip_openness (include/o2v_hip.h): in how many of D integer directions a ray
from a voxel's centre leaves the grid, or passes the cut-off, before it meets the open interior of a solid voxel.

openness() is the definition and nothing else: the fine walk, vectorised over the targets, a direction at a time, in int64.
scalar_open() is the same walk for one ray in Python ints, skip_open() the walk with the block skip of the kernel (DESIGN.md
section 31) restated in Python ints on boolean block pyramids; tests/test_host_openness.py holds the three against each other.
Grids are numpy bool arrays [z, y, x]; directions, cells and counters are (x, y, z)."""
import numpy as np

NOT_A_TARGET = 255
SIZES = {6: 1, 26: 1, 98: 2, 290: 3}


def _gcd3(a, b, c):
    return int(np.gcd(np.gcd(abs(a), abs(b)), abs(c)))


def direction_set(n):
    """int32 [n, 3] (dx, dy, dz): the primitive integer vectors with components up to 1, 1, 2, 3 in magnitude for n = 6 (the axes
    alone), 26, 98, 290, in ascending order of (dz, dy, dx)."""
    r = SIZES[n]
    out = []
    for dz in range(-r, r + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if (dx, dy, dz) == (0, 0, 0) or _gcd3(dx, dy, dz) != 1:
                    continue
                if n == 6 and abs(dx) + abs(dy) + abs(dz) != 1:
                    continue
                out.append((dx, dy, dz))
    assert len(out) == n
    return np.array(out, np.int32)


def targets(g, mode="surface"):
    """bool [z, y, x]: the target voxels of a mode ("surface", "solid", "empty") or a grid of nonzero = target."""
    g = np.asarray(g, bool)
    if not isinstance(mode, str):
        t = np.asarray(mode) != 0
        assert t.shape == g.shape
        return t
    if mode == "solid":
        return g.copy()
    if mode == "empty":
        return ~g
    assert mode == "surface"
    p = np.pad(g, 1)
    inner = p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:]
    return g & ~inner


def max_distance2(r):
    """floor(r * r) of a cut-off radius; None: 0, unlimited."""
    return 0 if r is None else int(np.floor(float(r) * float(r)))


def open_rays(g, directions, tg, md2=0):
    """bool [T, D]: ray (target, direction) is open, the targets being the True voxels of tg in order of (z, y, x).  Any D."""
    g = np.asarray(g, bool)
    nz, ny, nx = g.shape
    dirs = direction_set(directions) if isinstance(directions, int) else np.asarray(directions, np.int64).reshape(-1, 3)
    assert len(dirs) >= 1 and (np.abs(dirs).max(1) > 0).all() and np.abs(dirs).max() <= 127
    cz, cy, cx = np.nonzero(tg)
    c0 = np.stack([cx, cy, cz], 1).astype(np.int64)
    dims = np.array([nx, ny, nz], np.int64)
    result = np.zeros((len(c0), len(dirs)), bool)
    for i, d in enumerate(dirs):
        d = np.asarray(d, np.int64)
        s, m = np.sign(d), np.abs(d)
        moving = [a for a in range(3) if m[a]]
        k = np.zeros((len(c0), 3), np.int64)
        live = np.arange(len(c0))
        is_open = np.zeros(len(c0), bool)
        while len(live):
            kk = k[live]
            n = 2 * kk + 1
            # the least event (2 k_a + 1) / (2 m_a) by cross-multiplication, then every axis whose event equals it
            bn, bm = n[:, moving[0]], np.full(len(live), m[moving[0]])
            for b in moving[1:]:
                less = n[:, b] * bm < bn * m[b]
                bn, bm = np.where(less, n[:, b], bn), np.where(less, m[b], bm)
            for b in moving:
                kk[:, b] += n[:, b] * bm == bn * m[b]
            k[live] = kk
            c = c0[live] + s * kk
            out = ((c < 0) | (c >= dims)).any(1)
            far = (kk * kk).sum(1) > md2 if md2 else np.zeros(len(live), bool)
            done_open = out | far
            cc = np.where(done_open[:, None], 0, c)
            blocked = ~done_open & g[cc[:, 2], cc[:, 1], cc[:, 0]]
            is_open[live[done_open]] = True
            live = live[~done_open & ~blocked]
        result[:, i] = is_open
    return result


def open_counts(g, directions=26, mode="surface", md2=0):
    """int64 [z, y, x]: the open directions of every target, -1 elsewhere.  Any D (the 290 set does not fit a call's byte)."""
    g = np.asarray(g, bool)
    tg = targets(g, mode)
    out = np.full(g.shape, -1, np.int64)
    out[tg] = open_rays(g, directions, tg, md2).sum(1)
    return out


def openness(g, directions=26, mode="surface", md2=0, mask=False):
    """(count uint8 [z, y, x], mask int64 [z, y, x] or None): what o2v_hip_openness writes - the open directions of every target,
    255 and 0 elsewhere; 1 <= D <= 254, with a mask D <= 64."""
    g = np.asarray(g, bool)
    tg = targets(g, mode)
    rays = open_rays(g, directions, tg, md2)
    D = rays.shape[1]
    assert D <= 254 and (not mask or D <= 64)
    dst = np.full(g.shape, NOT_A_TARGET, np.uint8)
    dst[tg] = rays.sum(1).astype(np.uint8)
    if not mask:
        return dst, None
    mk = np.zeros(g.shape, np.int64)
    mk[tg] = (rays.astype(np.uint64) << np.arange(D, dtype=np.uint64)).sum(1, dtype=np.uint64).view(np.int64)
    return dst, mk


def open_along_x(g, tg, sign, md2=0):
    """bool [T]: the ray along (sign * m, 0, 0), any m, from each target is open - a closed form for rays too long to walk here: it
    is blocked iff the row holds a solid voxel ahead, the nearest at distance j, and the cut-off does not come first (j * j <= md2)."""
    g = np.asarray(g, bool)
    out = []
    for z, y, x in np.argwhere(tg):
        ahead = np.nonzero(g[z, y, x + 1:] if sign > 0 else g[z, y, :x][::-1])[0]
        j = int(ahead[0]) + 1 if len(ahead) else 0
        out.append(not (j and (md2 == 0 or j * j <= md2)))
    return np.array(out, bool)


# ---- one ray in Python ints: the fine walk, and the walk with the skip -------------------------------------------------------------

def _step(k, m):
    """One step of the fine walk: every axis whose event is the least one crosses."""
    moving = [a for a in range(3) if m[a]]
    a = moving[0]
    for b in moving[1:]:
        if (2 * k[b] + 1) * m[a] < (2 * k[a] + 1) * m[b]:
            a = b
    na = 2 * k[a] + 1
    return [k[b] + (1 if m[b] and (2 * k[b] + 1) * m[a] == na * m[b] else 0) for b in range(3)]


def _after(g, c0, s, k, md2):
    """"open", "blocked" or None for the cell the ray is in after a step."""
    nz, ny, nx = g.shape
    c = [c0[a] + s[a] * k[a] for a in range(3)]
    if not (0 <= c[0] < nx and 0 <= c[1] < ny and 0 <= c[2] < nz):
        return "open"
    if md2 and k[0] * k[0] + k[1] * k[1] + k[2] * k[2] > md2:
        return "open"
    return "blocked" if g[c[2], c[1], c[0]] else None


def scalar_open(g, c0, d, md2=0):
    """True: the ray from cell c0 (x, y, z) along d is open.  The fine walk."""
    s = [(v > 0) - (v < 0) for v in d]
    m = [abs(int(v)) for v in d]
    k = [0, 0, 0]
    while True:
        k = _step(k, m)
        r = _after(g, c0, s, k, md2)
        if r:
            return r == "open"


def pyramid(g, levels=(2, 4, 6)):
    """{L: bool array over the aligned blocks of side 2^L, True where the block holds a solid voxel}"""
    out = {}
    for L in levels:
        b = 1 << L
        nz, ny, nx = (-(-n // b) for n in g.shape)
        p = np.zeros((nz * b, ny * b, nx * b), bool)
        p[:g.shape[0], :g.shape[1], :g.shape[2]] = g
        out[L] = p.reshape(nz, b, ny, b, nx, b).any(axis=(1, 3, 5))
    return out


def skip(c0, s, m, k, L):
    """The counters after the skip out of the aligned block of side 2^L around the cell c0 + s k."""
    K = [0, 0, 0]
    for a in range(3):
        if m[a]:
            c = c0[a] + s[a] * k[a]
            lo = (c >> L) << L
            K[a] = k[a] + (lo + (1 << L) - c if s[a] > 0 else c - lo + 1)
    moving = [a for a in range(3) if m[a]]
    e = moving[0]
    for b in moving[1:]:
        if (2 * K[b] - 1) * m[e] < (2 * K[e] - 1) * m[b]:
            e = b
    N, M = 2 * K[e] - 1, m[e]
    return [K[b] if b == e else ((N * m[b]) // M + 1) // 2 if m[b] else 0 for b in range(3)]


def skip_open(g, pyr, c0, d, md2=0):
    """True: the ray is open.  The walk that leaves every empty aligned block of pyr's levels in one skip."""
    s = [(v > 0) - (v < 0) for v in d]
    m = [abs(int(v)) for v in d]
    k = [0, 0, 0]
    levels = sorted(pyr, reverse=True)
    while True:
        c = [c0[a] + s[a] * k[a] for a in range(3)]
        for L in levels:
            if not pyr[L][c[2] >> L, c[1] >> L, c[0] >> L]:
                k = skip(c0, s, m, k, L)
                break
        else:
            k = _step(k, m)
        r = _after(g, c0, s, k, md2)
        if r:
            return r == "open"


def count_scalar(g, c0, dirs, md2=0, walk=scalar_open, **kw):
    return sum(bool(walk(g, c0=c0, d=d, md2=md2, **kw)) for d in np.asarray(dirs).tolist())


# ---- grids ---------------------------------------------------------------------------------------------------------------------------

def box_in(n, lo, hi, hollow=False):
    """A solid box [lo, hi)^3 in an n^3 grid; hollow: walls one voxel thick."""
    g = np.zeros((n, n, n), bool)
    g[lo:hi, lo:hi, lo:hi] = True
    if hollow:
        g[lo + 1:hi - 1, lo + 1:hi - 1, lo + 1:hi - 1] = False
    return g


def shaft(depth, n=9, thick=4):
    """A slab of `thick` layers at the bottom of an n x n x (thick + 3) grid with a 1 x 1 shaft of `depth` from its top at the
    middle; returns (grid, the shaft's floor cell (x, y, z))."""
    g = np.zeros((thick + 3, n, n), bool)
    g[:thick] = True
    g[thick - depth:thick, n // 2, n // 2] = False
    return g, (n // 2, n // 2, thick - depth)


def ball(n=33, c=16, r=14):
    z, y, x = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    return (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2 <= r * r


def blobs(rng, dims, density):
    """A random grid (nx, ny, nz) -> [z, y, x] of the given density: single voxels and a few boxes."""
    nx, ny, nz = dims
    g = rng.random((nz, ny, nx)) < density
    for _ in range(2):
        lo = [int(rng.integers(0, n)) for n in (nz, ny, nx)]
        hi = [min(n, l + 1 + int(rng.integers(0, max(1, n // 3)))) for n, l in zip((nz, ny, nx), lo)]
        if density >= 0.05:
            g[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    return g
