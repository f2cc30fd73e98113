"""Restatement of the narrow-band distance to the triangles (o2v_hip_mesh_distance_dense, include/o2v_hip.h) in numpy.

d2 is evaluated in float64 op by op, left to right, as the header writes it; numpy does not contract multiply-adds, so every
value is the device's bit for bit.  Sample-space vertices come from fill_ref.sample_vertices, the sign from fill_ref.parity_keys.
A (centre, triangle) pair is evaluated only when the centre lies in the triangle's AABB dilated by band ss + ss, as on the
device; `cull=False` evaluates every pair (the host tests show both agree)."""
import numpy as np

from tests import fill_ref


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _side(n, u, v, p):
    """n . cross(V - U, P - U), arrays [..., 3]"""
    ex, ey, ez = v[..., 0] - u[..., 0], v[..., 1] - u[..., 1], v[..., 2] - u[..., 2]
    wx, wy, wz = p[..., 0] - u[..., 0], p[..., 1] - u[..., 1], p[..., 2] - u[..., 2]
    return _dot(n[..., 0], n[..., 1], n[..., 2], ey * wz - ez * wy, ez * wx - ex * wz, ex * wy - ey * wx)


def _seg(u, v, p):
    ex, ey, ez = v[..., 0] - u[..., 0], v[..., 1] - u[..., 1], v[..., 2] - u[..., 2]
    wx, wy, wz = p[..., 0] - u[..., 0], p[..., 1] - u[..., 1], p[..., 2] - u[..., 2]
    ee = _dot(ex, ey, ez, ex, ey, ez)
    with np.errstate(all="ignore"):
        t = _dot(wx, wy, wz, ex, ey, ez) / ee
    t = np.where(ee == 0, 0.0, t)
    t = np.where(t < 0, 0.0, np.where(t > 1, 1.0, t))
    qx, qy, qz = wx - t * ex, wy - t * ey, wz - t * ez
    return _dot(qx, qy, qz, qx, qy, qz)


def d2(p, a, b, c):
    """Squared distance of points p to triangles (a, b, c): float64 arrays [..., 3] that broadcast (a, b, c hold float32
    values)."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    abx, aby, abz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
    acx, acy, acz = c[..., 0] - a[..., 0], c[..., 1] - a[..., 1], c[..., 2] - a[..., 2]
    n = np.stack([aby * acz - abz * acy, abz * acx - abx * acz, abx * acy - aby * acx], -1)
    nn = _dot(n[..., 0], n[..., 1], n[..., 2], n[..., 0], n[..., 1], n[..., 2])
    face = (nn > 0) & (_side(n, a, b, p) >= 0) & (_side(n, b, c, p) >= 0) & (_side(n, c, a, p) >= 0)
    h = _dot(n[..., 0], n[..., 1], n[..., 2], p[..., 0] - a[..., 0], p[..., 1] - a[..., 1], p[..., 2] - a[..., 2])
    with np.errstate(all="ignore"):
        plane = (h * h) / nn
    segs = np.minimum(np.minimum(_seg(a, b, p), _seg(b, c, p)), _seg(c, a, p))
    return np.where(face, plane, segs)


def f32_band(band):
    """The band as the call takes it: a float.  Every use below widens that float32 to double, as the header writes
    (double) band; a Python double that is no float32 (2.6, say) would put other voxels in the band."""
    return np.float64(np.float32(band))


def _finite(sv):
    sv = np.asarray(sv, np.float32).reshape(-1, 3, 3)
    return sv, np.all(np.isfinite(sv), axis=(1, 2))


def dilated_aabb(sv, band, ss):
    """[T, 3] lower and upper corners (float64) of every triangle's AABB dilated by band ss + ss."""
    sv = np.asarray(sv, np.float32).reshape(-1, 3, 3)
    m = f32_band(band) * ss + ss
    return sv.min(axis=1).astype(np.float64) - m, sv.max(axis=1).astype(np.float64) + m


def centres(idx, ss):
    return idx.astype(np.float64) * ss + 0.5 * ss


def finish(best, best_id, band, ss, negative=None):
    """(values float32, closest int32) from the best d2 and index per voxel; Bs2 = (double) band * band * ss * ss of the
    float32 band."""
    bs2 = f32_band(band) * f32_band(band) * ss * ss
    inside = best < bs2
    with np.errstate(invalid="ignore"):
        u = np.where(inside, (np.sqrt(best) / ss).astype(np.float32), np.float32(band)).astype(np.float32)
    if negative is not None:
        u = np.where(negative, -u, u)
    return u, np.where(inside, best_id, -1).astype(np.int32)


def best_d2(sv, G, ss, band, origin=(0, 0, 0), dims=None, cull=True):
    """(D float64 [nz, ny, nx], index int64) of the box: per voxel the smallest d2 over the triangles whose AABB, dilated by
    the band's margin, holds its centre (inf and -1 where there is none), before the band is applied."""
    sv, ok = _finite(sv)
    dims = (G, G, G) if dims is None else tuple(dims)
    nx, ny, nz = dims
    ox, oy, oz = origin
    best = np.full((nz, ny, nx), np.inf)
    best_id = np.full((nz, ny, nx), -1, np.int64)
    lo, hi = dilated_aabb(sv, band, ss)
    cx, cy, cz = centres(np.arange(ox, ox + nx), ss), centres(np.arange(oy, oy + ny), ss), centres(np.arange(oz, oz + nz), ss)
    for t in np.nonzero(ok)[0]:
        if cull:
            rx = np.nonzero((cx >= lo[t, 0]) & (cx <= hi[t, 0]))[0]
            ry = np.nonzero((cy >= lo[t, 1]) & (cy <= hi[t, 1]))[0]
            rz = np.nonzero((cz >= lo[t, 2]) & (cz <= hi[t, 2]))[0]
            if not (len(rx) and len(ry) and len(rz)):
                continue
        else:
            rx, ry, rz = np.arange(nx), np.arange(ny), np.arange(nz)
        z, y, x = np.meshgrid(rz, ry, rx, indexing="ij")
        p = np.stack([cx[x], cy[y], cz[z]], -1)
        v = sv[t].astype(np.float64)
        d = d2(p, v[0], v[1], v[2])
        sub = best[z, y, x]
        take = d < sub     # (triangles in ascending order: a tie keeps the smaller index)
        best[z[take], y[take], x[take]] = d[take]
        best_id[z[take], y[take], x[take]] = t
    return best, best_id


def mesh_distance(sv, G, ss, band, signed, origin=(0, 0, 0), dims=None, cull=True):
    """(values float32 [nz, ny, nx], closest int32 [nz, ny, nx]) of the box origin + [0, dims) (x, y, z) of a G^3 grid for
    sample-space triangles sv [T, 3, 3]."""
    best, best_id = best_d2(sv, G, ss, band, origin, dims, cull)
    negative = None
    if signed:
        nx, ny, nz = (G, G, G) if dims is None else tuple(dims)
        ox, oy, oz = origin
        keys = fill_ref.parity_keys(_finite(sv)[0], G, ss)
        z, y, x = np.meshgrid(np.arange(oz, oz + nz), np.arange(oy, oy + ny), np.arange(ox, ox + nx), indexing="ij")
        negative = np.isin((x.astype(np.int64) * G + y) * G + z, keys)
    return finish(best, best_id, band, ss, negative)


def threshold_band(D):
    """(f, narrow) for a d2 value D: f, the smallest float32 band that still holds it, (double) f * f > D, and whether the
    float32 product f * f, widened, is <= D: a Bs2 squared in float32 would then leave the voxel out of band f."""
    f = np.float32(np.sqrt(D))
    while np.float64(f) * np.float64(f) > D:
        f = np.nextafter(f, np.float32(0))
    while not np.float64(f) * np.float64(f) > D:
        f = np.nextafter(f, np.float32(np.inf))
    return f, bool(np.float64(f * f) <= D)


def point_distance(pts, sv, ss, band, chunk=256):
    """(unsigned values float32 [n], closest int32 [n]) at voxel centres pts [n, 3] (x, y, z), each over the triangles whose
    dilated AABB holds its centre (numpy's argmin takes the first, i.e. smallest, index of a tie)."""
    sv, ok = _finite(sv)
    idx = np.nonzero(ok)[0]
    lo, hi = dilated_aabb(sv[idx], band, ss)
    v = sv[idx].astype(np.float64)
    best = np.full(len(pts), np.inf)
    best_id = np.full(len(pts), -1, np.int64)
    for i, q in enumerate(np.asarray(pts)):
        p = centres(np.asarray(q, np.int64), ss)
        cand = np.nonzero(np.all((p >= lo) & (p <= hi), axis=1))[0]
        if not len(cand):
            continue
        d = d2(p[None, :], v[cand, 0], v[cand, 1], v[cand, 2])
        k = int(np.argmin(d))
        best[i], best_id[i] = d[k], idx[cand[k]]
    return finish(best, best_id, band, ss)
