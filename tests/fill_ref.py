"""Restatement of the solid fill's parity set (O2V_HIP_FLAG_FILL_INTERIOR, include/o2v_hip.h) in numpy, for small meshes.

Signs of the 2-D edge function are exact: a float64 evaluation with Shewchuk's orient2d error bound decides where it can, the
rest is evaluated with Python fractions on the float32 values (EXACT counts those column tests).  The crossing height is float64,
op by op, as specified; numpy does not contract multiply-adds.  The set ends at the mesh's top layer floor(zmax / ss), zmax the
largest sample-space z of a triangle with finite coordinates: above it an open mesh's parity does not reach.  Voxels are
returned as int64 keys (x * G + y) * G + z."""
from fractions import Fraction

import numpy as np

_BOUND = (3.0 + 16.0 * 2.0 ** -53) * 2.0 ** -53   # ccwerrboundA

# edge signs the float64 filter left to the exact evaluation since the last reset: all of them, and those that were not zero
EXACT = {"calls": 0, "nonzero": 0}


def sample_vertices(verts, xform):
    """[T, 9] model-space vertices -> [T, 3, 3] float32 sample space, with affine_apply's order (o2v_math.h): per row a
    sequential dot product from zero, then the translation."""
    v = np.asarray(verts, np.float32).reshape(-1, 3, 3)
    m = np.asarray(xform, np.float32)[:9].reshape(3, 3)
    t = np.asarray(xform, np.float32)[9:12]
    out = np.empty_like(v)
    with np.errstate(all="ignore"):
        for r in range(3):
            acc = np.float32(0) + m[r, 0] * v[..., 0]
            acc = acc + m[r, 1] * v[..., 1]
            acc = acc + m[r, 2] * v[..., 2]
            out[..., r] = acc + t[r]
    return out


def odd_edges(sv):
    """Edges (unordered pairs of bit-identical sample-space vertices) used by an odd number of triangles; [] = closed."""
    bits = np.ascontiguousarray(sv, np.float32).view(np.uint32).reshape(-1, 3, 3)
    count = {}
    for tri in bits:
        vs = [tuple(int(c) for c in tri[k]) for k in range(3)]
        for a, b in ((0, 1), (1, 2), (2, 0)):
            key = (min(vs[a], vs[b]), max(vs[a], vs[b]))
            count[key] = count.get(key, 0) + 1
    return [k for k, n in count.items() if n % 2]


def weld(verts):
    """Vertices that lie within 1e-6 of each other replaced by one of them (model space): closes uv_sphere's seam and poles,
    whose copies are rounded separately."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).copy()
    q = np.round(v.astype(np.float64) * 1e6).astype(np.int64)
    _, first, inverse = np.unique(q, axis=0, return_index=True, return_inverse=True)
    return v[first[inverse.ravel()]].reshape(-1, 9)


def _exact_sign(ux, uy, vx, vy, px, py):
    F = Fraction
    d = (F(vx) - F(ux)) * (F(py) - F(uy)) - (F(vy) - F(uy)) * (F(px) - F(ux))
    return (d > 0) - (d < 0)


def _signs(u, v, px, py, exact=True):
    """Column-test signs of edges u -> v ([n, 2] float32 each) at the columns (px, py), perturbation included.  exact=False:
    the plain float64 sign instead (not the definition; for tests that show the exact path matters)."""
    ux, uy = u[:, 0].astype(np.float64), u[:, 1].astype(np.float64)
    vx, vy = v[:, 0].astype(np.float64), v[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        left = (vx - ux) * (py - uy)
        right = (vy - uy) * (px - ux)
        det = left - right
        bound = _BOUND * (np.abs(left) + np.abs(right)) if exact else 0.0
    s = np.where(det > bound, 1, np.where(-det > bound, -1, 2)).astype(np.int64)
    if not exact:
        s[s == 2] = 0
    for n in np.nonzero(s == 2)[0]:
        s[n] = _exact_sign(float(ux[n]), float(uy[n]), float(vx[n]), float(vy[n]), float(px[n]), float(py[n]))
        EXACT["calls"] += 1
        EXACT["nonzero"] += int(s[n] != 0)
    tie = np.where(vy != uy, np.where(vy > uy, -1, 1), np.where(vx > ux, 1, -1))
    s = np.where(s == 0, tie, s)
    return np.where((ux == vx) & (uy == vy), 0, s)


def _e(u, v, px, py):
    return (v[:, 0].astype(np.float64) - u[:, 0]) * (py - u[:, 1]) - (v[:, 1].astype(np.float64) - u[:, 1]) * (px - u[:, 0])


def _first_centre(x, ss, n, strict):
    """first index i in [0, n] with centre i ss + ss/2 >= x (> x if strict)"""
    h = 0.5 * ss
    i = np.clip(np.floor((x.astype(np.float64) - h) / ss), 0, n).astype(np.int64)
    after = (lambda j: j * float(ss) + h > x) if strict else (lambda j: j * float(ss) + h >= x)
    for _ in range(3):
        i = np.where((i > 0) & after(i - 1), i - 1, i)
        i = np.where((i < n) & ~after(np.minimum(i, n)), i + 1, i)
    return i


def top_layer(sv, ss):
    """The mesh's top layer floor(zmax / ss) (zmax over the triangles with finite coordinates); -1 if there is none."""
    sv = np.asarray(sv, np.float32).reshape(-1, 3, 3)
    sv = sv[np.all(np.isfinite(sv), axis=(1, 2))]
    if not len(sv):
        return -1
    return max(int(np.floor(float(sv[:, :, 2].max()) / ss)), -1)


def crossings(sv, G, ss, exact=True):
    """(column x, column y, k0) of every crossing of the parity definition, k0 clamped to G (= above the grid)."""
    sv = np.asarray(sv, np.float32).reshape(-1, 3, 3)
    sv = sv[np.all(np.isfinite(sv), axis=(1, 2))]
    h = 0.5 * ss
    lo, hi = sv.min(axis=1), sv.max(axis=1)
    i0, i1 = _first_centre(lo[:, 0], ss, G, False), _first_centre(hi[:, 0], ss, G, True)
    j0, j1 = _first_centre(lo[:, 1], ss, G, False), _first_centre(hi[:, 1], ss, G, True)
    wi, wj = np.maximum(i1 - i0, 0), np.maximum(j1 - j0, 0)
    cnt = wi * wj
    tri = np.repeat(np.arange(len(sv)), cnt)
    local = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ci = i0[tri] + local % np.maximum(wi[tri], 1)
    cj = j0[tri] + local // np.maximum(wi[tri], 1)
    px, py = ci * float(ss) + h, cj * float(ss) + h
    V0, V1, V2 = sv[tri, 0], sv[tri, 1], sv[tri, 2]
    s0, s1, s2 = _signs(V0, V1, px, py, exact), _signs(V1, V2, px, py, exact), _signs(V2, V0, px, py, exact)
    cov = (s0 != 0) & (s0 == s1) & (s1 == s2)
    V0, V1, V2, px, py, ci, cj = V0[cov], V1[cov], V2[cov], px[cov], py[cov], ci[cov], cj[cov]
    with np.errstate(all="ignore"):
        w0, w1, w2 = _e(V1, V2, px, py), _e(V2, V0, px, py), _e(V0, V1, px, py)
        den = (w0 + w1) + w2
        z = ((w0 * V0[:, 2].astype(np.float64) + w1 * V1[:, 2].astype(np.float64)) + w2 * V2[:, 2].astype(np.float64)) / den
    zmin = np.minimum(np.minimum(V0[:, 2], V1[:, 2]), V2[:, 2]).astype(np.float64)
    z = np.where((den == 0) | ~np.isfinite(z), zmin, z)
    k = np.clip(np.floor((z - h) / ss) + 1, 0, G).astype(np.int64)
    for _ in range(3):
        k = np.where((k > 0) & ((k - 1) * float(ss) + h > z), k - 1, k)
        k = np.where((k < G) & (k * float(ss) + h <= z), k + 1, k)
    return ci, cj, k


def parity_keys(sv, G, ss, exact=True):
    """Sorted int64 keys of the parity set of the whole G^3 grid for sample-space triangles sv (layers up to the mesh's top)."""
    ci, cj, k = crossings(sv, G, ss, exact)
    top = min(top_layer(sv, ss) + 1, G)   # (layers [0, top) can hold a voxel of the set)
    keep = k < top
    toggles = (ci[keep] * G + cj[keep]) * G + k[keep]   # (column, layer) as one key
    # equal toggles cancel in pairs; per column the remaining ones, in order, bound the runs [k_a, k_b) of odd parity
    vals, n = np.unique(toggles, return_counts=True)
    vals = vals[n % 2 == 1]
    cols, counts = np.unique(vals // G, return_counts=True)
    vals = np.sort(np.concatenate([vals, cols[counts % 2 == 1] * G + top]))   # (an odd column runs up to the mesh's top)
    starts, ends = vals[0::2], vals[1::2]
    n = ends - starts
    if not n.sum():
        return np.zeros(0, np.int64)
    return np.repeat(starts - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(n.sum())


def keys(vox, G):
    v = np.asarray(vox).astype(np.int64).reshape(-1, 4)
    return np.sort((v[:, 0] * G + v[:, 1]) * G + v[:, 2])
