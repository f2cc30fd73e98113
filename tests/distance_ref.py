"""numpy references for o2v_hip_distance_dense on label grids [z, y, x] (0 empty, 1 surface,
2 interior): a brute force over every surface voxel for small boxes, and the exact separable transform (x by two scans, y and z
by the integer lower envelope of Meijster et al. 2000, vectorised over the lines): seconds for boxes up to about 256^3, and
for the long thin boxes of the limit cases (tests/test_host_distance.py checks it there against a sampled brute force)."""
import numpy as np

INF = 0x7FFFFFFF


def brute_d2(labels, chunk=4096):
    """int32 [z, y, x]: min over surface voxels s of |v - s|^2, INF if there are none."""
    labels = np.asarray(labels)
    seeds = np.argwhere(labels == 1).astype(np.int64)
    if len(seeds) == 0:
        return np.full(labels.shape, INF, np.int32)
    vox = np.indices(labels.shape).reshape(3, -1).T.astype(np.int64)
    out = np.empty(len(vox), np.int64)
    for i in range(0, len(vox), chunk):
        v = vox[i:i + chunk]
        out[i:i + chunk] = (((v[:, None, :] - seeds[None, :, :]) ** 2).sum(-1)).min(1)
    return out.reshape(labels.shape).astype(np.int32)


def _rows(seed):
    """Squared distance along the last axis to the nearest True of the row (INF if none): an inclusive max-scan of the last
    seed index from the left and a min-scan of the next one from the right."""
    n = seed.shape[-1]
    idx = np.arange(n, dtype=np.int64)
    big = np.int64(1) << 40
    left = np.maximum.accumulate(np.where(seed, idx, -big), axis=-1)
    right = np.minimum.accumulate(np.where(seed, idx, big)[..., ::-1], axis=-1)[..., ::-1]
    d = np.minimum(idx - left, right - idx)
    return np.where(d < big // 2, d * d, INF)


def _forward(f):
    """The forward sweep of `envelope`: the stacks (s, t, q) and, per line, the largest number of entries its stack held and
    the largest number of entries popped at one position."""
    L, n = f.shape
    rows = np.arange(L)
    s = np.zeros((L, n), np.int64)
    t = np.zeros((L, n), np.int64)
    q = np.full(L, -1, np.int64)
    depth = np.zeros(L, np.int64)
    pops = np.zeros(L, np.int64)
    for u in range(n):
        fu = f[:, u]
        act = fu != INF
        q0 = q
        while True:
            qi = np.maximum(q, 0)
            ts, tt = s[rows, qi], t[rows, qi]
            tf = f[rows, ts]
            pop = act & (q >= 0) & ((tt - ts) ** 2 + tf > (tt - u) ** 2 + fu)
            if not pop.any():
                break
            q = np.where(pop, q - 1, q)
        pops = np.maximum(pops, q0 - q)
        empty = act & (q < 0)
        have = act & (q >= 0)
        qi = np.maximum(q, 0)
        ts = s[rows, qi]
        tf = f[rows, ts]
        den = np.where(have, 2 * (u - ts), 1)
        w = 1 + (u * u - ts * ts + fu - tf) // den
        push = have & (w < n)
        q = np.where(push, q + 1, q)
        s[push, q[push]] = u
        t[push, q[push]] = w[push]
        s[empty, 0] = u
        t[empty, 0] = 0
        q[empty] = 0
        depth = np.maximum(depth, q + 1)
    return s, t, q, depth, pops


def final_stack(s, t, q, line):
    """The (s, t) of the entries left on a line's stack at the end of the forward sweep, bottom first."""
    return list(zip(s[line, :q[line] + 1].tolist(), t[line, :q[line] + 1].tolist()))


def envelope(f, record=None):
    """d[l, u] = min over v of f[l, v] + (u - v)^2 for int64 f [lines, n] with INF entries (never seeds): Meijster's lower
    envelope of parabolas with a stack per line, integer Sep by floor division.  record: a list that takes what
    envelope_stats gives for f."""
    L, n = f.shape
    rows = np.arange(L)
    s, t, q, depth, pops = _forward(f)
    if record is not None:
        record.append((depth, pops, (s, t, q)))
    d = np.full((L, n), INF, np.int64)
    for u in range(n - 1, -1, -1):
        has = q >= 0
        qi = np.maximum(q, 0)
        ts = s[rows, qi]
        d[has, u] = (u - ts[has]) ** 2 + f[rows[has], ts[has]]
        q = q - (has & (t[rows, qi] == u))
    return d


def envelope_stats(f):
    """(depth, pops, stacks) of `envelope`'s forward sweep over f [lines, n]: per line the largest number of entries its stack
    held and the largest number popped at one position, and the stacks as the sweep left them (s, t, q: final_stack reads a
    line's).  What a test asserts about the paths its grid drives the device's stack through."""
    s, t, q, depth, pops = _forward(f)
    return depth, pops, (s, t, q)


def pass_inputs(labels):
    """The int64 inputs [lines, n] of the y and the z envelope pass of separable_d2 (lines in the device's order: x fastest)."""
    labels = np.asarray(labels)
    nz, ny, nx = labels.shape
    g = _rows(labels == 1)
    fy = g.transpose(0, 2, 1).reshape(-1, ny)
    g = envelope(fy).reshape(nz, nx, ny).transpose(0, 2, 1)
    return fy, g.transpose(1, 2, 0).reshape(-1, nz)


def sampled_brute_d2(labels, pts, chunk=64):
    """int64 [n]: the squared distance from each voxel pts [n, 3] (z, y, x) to the nearest surface voxel, over every one of
    them (INF if there are none)."""
    seeds = np.argwhere(np.asarray(labels) == 1).astype(np.int64)
    pts = np.asarray(pts, np.int64)
    if len(seeds) == 0:
        return np.full(len(pts), INF, np.int64)
    out = np.empty(len(pts), np.int64)
    for i in range(0, len(pts), chunk):
        out[i:i + chunk] = ((pts[i:i + chunk, None, :] - seeds[None, :, :]) ** 2).sum(-1).min(1)
    return out


def separable_d2(labels, record=None):
    """int32 [z, y, x], equal to brute_d2: x, then y, then z.  record: a list that takes envelope_stats of the y pass' lines,
    then of the z pass' (lines in the device's order, x fastest)."""
    labels = np.asarray(labels)
    nz, ny, nx = labels.shape
    g = _rows(labels == 1)                                                     # [z, y, x]
    g = envelope(g.transpose(0, 2, 1).reshape(-1, ny), record).reshape(nz, nx, ny).transpose(0, 2, 1)
    g = envelope(g.transpose(1, 2, 0).reshape(-1, nz), record).reshape(ny, nx, nz).transpose(2, 0, 1)
    return np.ascontiguousarray(g).astype(np.int32)


def sdf(labels, d2):
    """float32: -sqrt(d2) where labels == 2, +sqrt(d2) elsewhere, +-inf where d2 is INF (no surface voxel)."""
    r = np.sqrt(np.asarray(d2).astype(np.float64)).astype(np.float32)
    r[np.asarray(d2) == INF] = np.inf
    return np.where(np.asarray(labels) == 2, -r, r)


def scan_rows():
    """Seeds, bool [3, 2, 193]: the smallest box whose rows put the row scan's left carry, a look-ahead across more than one
    empty chunk and a last chunk one lane wide (four chunks of 64) into one row.  Its six rows: no seed; only x = 0; only
    x = 192; only x = 63 and 64, either side of a chunk's edge; every voxel; x = 5 and 133, equally far from x = 69."""
    seed = np.zeros((6, 193), bool)
    seed[1, 0] = seed[2, 192] = seed[3, 63] = seed[3, 64] = seed[5, 5] = seed[5, 133] = True
    seed[4] = True
    return seed.reshape(3, 2, 193)


def random_labels(rng, shape, density, interior=0.3):
    """Labels with surface voxels at `density` and interior (2) labels at random elsewhere."""
    u = rng.random(shape)
    return np.where(u < density, 1, np.where(rng.random(shape) < interior, 2, 0)).astype(np.uint8)


# ---- label grids at the limits the call documents (tests/distance_cases.py on the device, tests/test_host_distance.py for
# the reference itself) --------------------------------------------------------------------------------------------------

LANE_CAP = 1 << 17                  # lanes of one envelope pass (kDistMaxSlots)
LANE_CAP_SHAPES = [(5, 7, 26500), (6, 7, 21851)]   # [z, y, x]: both passes above the cap; the second a multiple of neither
LONG = 46341                        # the longest accepted axis: (LONG - 1)^2 <= 2^31 - 2
LONG_SHAPES = [(LONG, 2, 3), (2, LONG, 3), (1, 48, LONG)]
D2_LIMIT = 0x7FFFFFFE


def pass_lines(shape):
    """(lines of the y pass, lines of the z pass) of a grid [z, y, x]."""
    nz, ny, nx = shape
    return nx * nz, nx * ny


def lane_cap_labels(shape, density, seed, empty_plane=None):
    """Random labels; `empty_plane`: a z plane without seeds, whose lines along y then hold no finite value."""
    lab = random_labels(np.random.default_rng(seed), shape, density)
    if empty_plane is not None:
        lab[empty_plane][lab[empty_plane] == 1] = 0
    return lab


LONG_RUN = (33000, 35000, 37000, 39500, 41000, 43000, 45000)   # seeds of one line past position 2^15


def long_line_labels(shape, seed):
    """Seeds along the longest axis of `shape` on the line through the origin: its first and last voxel, LONG_RUN past
    position 2^15 (equal values 2 000 apart: each stays on the envelope), 40 seeds anywhere and a crowd either side of 2^15;
    interior labels at random elsewhere."""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, np.uint8)
    v = np.moveaxis(lab, int(np.argmax(shape)), 0)      # a view [long, p, q]
    n, p, q = v.shape
    v[rng.random(v.shape) < 0.3] = 2
    v[[0, n - 1] + list(LONG_RUN), 0, 0] = 1
    v[rng.integers(0, n, 40), rng.integers(0, p, 40), rng.integers(0, q, 40)] = 1
    crowd = np.arange((1 << 15) - 150, (1 << 15) + 150)
    crowd = crowd[rng.random(len(crowd)) < 0.3]
    v[crowd, rng.integers(0, p, len(crowd)), rng.integers(0, q, len(crowd))] = 1
    return lab


def deep_stack_labels(along_z=False, interior=None):
    """[z, y, x] = (1, 1024, 2100) with the last column and the last row seeds: column x of the y pass holds the constant
    (2099 - x)^2 down 1023 rows, each pushed (equal values one apart all stay on the envelope), then 0 in the last row, which
    pops every entry it lies below.  along_z: the same as (1024, 1, 2100), for the z pass.  interior: a seed for labels 2 at
    random on the other voxels."""
    lab = np.zeros((1, 1024, 2100), np.uint8)
    if interior is not None:
        lab[np.random.default_rng(interior).random(lab.shape) < 0.4] = 2
    lab[0, :, 2099] = 1
    lab[0, 1023, :] = 1
    return np.ascontiguousarray(lab.transpose(1, 0, 2)) if along_z else lab
