"""numpy references for o2v_hip_distance_dense on label grids [z, y, x] (0 empty, 1 surface,
2 interior): a brute force over every surface voxel for small boxes, and the exact separable transform (x by two scans, y and z
by the integer lower envelope of Meijster et al. 2000, vectorised over the lines) for boxes up to about 256^3."""
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


def envelope(f):
    """d[l, u] = min over v of f[l, v] + (u - v)^2 for int64 f [lines, n] with INF entries (never seeds): Meijster's lower
    envelope of parabolas with a stack per line, integer Sep by floor division."""
    L, n = f.shape
    rows = np.arange(L)
    s = np.zeros((L, n), np.int64)
    t = np.zeros((L, n), np.int64)
    q = np.full(L, -1, np.int64)
    for u in range(n):
        fu = f[:, u]
        act = fu != INF
        while True:
            qi = np.maximum(q, 0)
            ts, tt = s[rows, qi], t[rows, qi]
            tf = f[rows, ts]
            pop = act & (q >= 0) & ((tt - ts) ** 2 + tf > (tt - u) ** 2 + fu)
            if not pop.any():
                break
            q = np.where(pop, q - 1, q)
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
    d = np.full((L, n), INF, np.int64)
    for u in range(n - 1, -1, -1):
        has = q >= 0
        qi = np.maximum(q, 0)
        ts = s[rows, qi]
        d[has, u] = (u - ts[has]) ** 2 + f[rows[has], ts[has]]
        q = q - (has & (t[rows, qi] == u))
    return d


def separable_d2(labels):
    """int32 [z, y, x], equal to brute_d2: x, then y, then z."""
    labels = np.asarray(labels)
    nz, ny, nx = labels.shape
    g = _rows(labels == 1)                                                     # [z, y, x]
    g = envelope(g.transpose(0, 2, 1).reshape(-1, ny)).reshape(nz, nx, ny).transpose(0, 2, 1)
    g = envelope(g.transpose(1, 2, 0).reshape(-1, nz)).reshape(ny, nx, nz).transpose(2, 0, 1)
    return np.ascontiguousarray(g).astype(np.int32)


def sdf(labels, d2):
    """float32: -sqrt(d2) where labels == 2, +sqrt(d2) elsewhere, +-inf where d2 is INF (no surface voxel)."""
    r = np.sqrt(np.asarray(d2).astype(np.float64)).astype(np.float32)
    r[np.asarray(d2) == INF] = np.inf
    return np.where(np.asarray(labels) == 2, -r, r)


def random_labels(rng, shape, density, interior=0.3):
    """Labels with surface voxels at `density` and interior (2) labels at random elsewhere."""
    u = rng.random(shape)
    return np.where(u < density, 1, np.where(rng.random(shape) < interior, 2, 0)).astype(np.uint8)
