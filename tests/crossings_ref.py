"""Restatement of the signed crossing numbers (o2v_hip_crossings_dense, include/o2v_hip.h) in numpy, for
small meshes, built on tests/fill_ref.py: the same exact signs (a float64 filter, then fractions), the same float64 crossing
height.  Twice: crossing_numbers is vectorised; crossing_numbers_scalar walks voxels, rays and triangles and evaluates each of
the six rays literally, with fractions for every sign.  Grids are int32 [z, y, x] of the whole G^3 grid; a box is a slice."""
from fractions import Fraction

import numpy as np

from obj2voxel_amd import meshes
from tests import fill_ref

AXES = "xyz"
# (u, v, w) of ray axis a as indices into (x, y, z): a = z reads (x, y, z), a = x (y, z, x), a = y (z, x, y)
PERM = {"x": (1, 2, 0), "y": (2, 0, 1), "z": (0, 1, 2)}
# the grid [w, v, u] of axis a as [z, y, x]
_TO_ZYX = {"x": (1, 2, 0), "y": (2, 0, 1), "z": (0, 1, 2)}


def axes_mask(axes):
    return sum(1 << AXES.index(a) for a in axes)


def _finite(sv):
    sv = np.asarray(sv, np.float32).reshape(-1, 3, 3)
    return sv[np.all(np.isfinite(sv), axis=(1, 2))]


def line_crossings(sv, G, ss, axis):
    """(line u, line v, k0, sigma) of every crossing of the rays along `axis` with the lines of the G^2 grid, k0 clamped to
    [0, G] (G: above every voxel of the grid)."""
    sv = _finite(sv)[:, :, list(PERM[axis])]
    h = 0.5 * ss
    lo, hi = sv.min(axis=1), sv.max(axis=1)
    i0, i1 = fill_ref._first_centre(lo[:, 0], ss, G, False), fill_ref._first_centre(hi[:, 0], ss, G, True)
    j0, j1 = fill_ref._first_centre(lo[:, 1], ss, G, False), fill_ref._first_centre(hi[:, 1], ss, G, True)
    wi, wj = np.maximum(i1 - i0, 0), np.maximum(j1 - j0, 0)
    cnt = wi * wj
    tri = np.repeat(np.arange(len(sv)), cnt)
    local = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ci = i0[tri] + local % np.maximum(wi[tri], 1)
    cj = j0[tri] + local // np.maximum(wi[tri], 1)
    px, py = ci * float(ss) + h, cj * float(ss) + h
    V0, V1, V2 = sv[tri, 0], sv[tri, 1], sv[tri, 2]
    s0, s1, s2 = fill_ref._signs(V0, V1, px, py), fill_ref._signs(V1, V2, px, py), fill_ref._signs(V2, V0, px, py)
    cov = (s0 != 0) & (s0 == s1) & (s1 == s2)
    V0, V1, V2, px, py, ci, cj, sigma = V0[cov], V1[cov], V2[cov], px[cov], py[cov], ci[cov], cj[cov], s0[cov]
    with np.errstate(all="ignore"):
        w0, w1, w2 = fill_ref._e(V1, V2, px, py), fill_ref._e(V2, V0, px, py), fill_ref._e(V0, V1, px, py)
        den = (w0 + w1) + w2
        z = ((w0 * V0[:, 2].astype(np.float64) + w1 * V1[:, 2].astype(np.float64)) + w2 * V2[:, 2].astype(np.float64)) / den
    zmin = np.minimum(np.minimum(V0[:, 2], V1[:, 2]), V2[:, 2]).astype(np.float64)
    z = np.where((den == 0) | ~np.isfinite(z), zmin, z)
    k = np.clip(np.floor((z - h) / ss) + 1, 0, G).astype(np.int64)
    for _ in range(3):
        k = np.where((k > 0) & ((k - 1) * float(ss) + h > z), k - 1, k)
        k = np.where((k < G) & (k * float(ss) + h <= z), k + 1, k)
    return ci, cj, k, sigma


def ray_sums(sv, G, ss, axis):
    """(D, U) of the rays along `axis`: int32 [z, y, x] each."""
    ci, cj, k, sigma = line_crossings(sv, G, ss, axis)
    delta = np.zeros((G + 1, G, G), np.int64)   # [w, v, u]
    np.add.at(delta, (k, cj, ci), -sigma)
    run = np.cumsum(delta, axis=0)
    D, T = run[:G], run[G]
    U = D - T[None]
    t = _TO_ZYX[axis]
    return D.transpose(t).astype(np.int32), U.transpose(t).astype(np.int32)


def crossing_numbers(sv, G, ss=1, axes="xyz"):
    """The sum over `axes` of D + U: int32 [z, y, x] of the whole grid, for sample-space triangles sv."""
    S = np.zeros((G, G, G), np.int32)
    for a in axes:
        D, U = ray_sums(sv, G, ss, a)
        S += D + U
    return S


def _sign_scalar(u, v, px, py):
    """the column test's sign of the edge u -> v at (px, py): the exact value, ties by the perturbation, 0 for a degenerate edge"""
    F = Fraction
    ux, uy, vx, vy = float(u[0]), float(u[1]), float(v[0]), float(v[1])
    if ux == vx and uy == vy:
        return 0
    d = (F(vx) - F(ux)) * (F(py) - F(uy)) - (F(vy) - F(uy)) * (F(px) - F(ux))
    if d:
        return 1 if d > 0 else -1
    return (-1 if vy > uy else 1) if vy != uy else (1 if vx > ux else -1)


def _height_scalar(t, px, py):
    """the crossing height, float64 op by op"""
    def e(u, v):
        return (np.float64(v[0]) - np.float64(u[0])) * (np.float64(py) - np.float64(u[1])) - \
               (np.float64(v[1]) - np.float64(u[1])) * (np.float64(px) - np.float64(u[0]))
    with np.errstate(all="ignore"):
        w0, w1, w2 = e(t[1], t[2]), e(t[2], t[0]), e(t[0], t[1])
        den = (w0 + w1) + w2
        z = ((w0 * np.float64(t[0][2]) + w1 * np.float64(t[1][2])) + w2 * np.float64(t[2][2])) / den
    if den == 0 or not np.isfinite(z):
        z = np.float64(min(t[0][2], t[1][2], t[2][2]))
    return float(z)


def crossing_numbers_scalar(sv, G, ss=1, axes="xyz", rays=False):
    """The definition as loops: per axis and line the list of crossings (height, sigma); per voxel the crossings split at its
    centre into those below (the centre lies above the height) and those above.  rays=True: the six sums apart,
    {axis: (D, U)}."""
    sv = _finite(sv)
    h = 0.5 * ss
    out = {a: (np.zeros((G, G, G), np.int32), np.zeros((G, G, G), np.int32)) for a in axes}
    for a in axes:
        p = PERM[a]
        D, U = out[a]
        for j in range(G):
            for i in range(G):
                px, py = i * ss + h, j * ss + h
                hits = []
                for tri in sv:
                    t = [tuple(float(tri[n][c]) for c in p) for n in range(3)]
                    s = [_sign_scalar(t[0], t[1], px, py), _sign_scalar(t[1], t[2], px, py), _sign_scalar(t[2], t[0], px, py)]
                    if s[0] != 0 and s[0] == s[1] == s[2]:
                        hits.append((_height_scalar(t, px, py), s[0]))
                for k in range(G):
                    centre = k * ss + h
                    idx = [0, 0, 0]
                    idx[p[0]], idx[p[1]], idx[p[2]] = i, j, k
                    x, y, z = idx
                    D[z, y, x] = -sum(s for hgt, s in hits if centre > hgt)
                    U[z, y, x] = sum(s for hgt, s in hits if not centre > hgt)
    if rays:
        return out
    S = np.zeros((G, G, G), np.int32)
    for a in axes:
        S += out[a][0] + out[a][1]
    return S


def inside(S, n_axes, rule="nonzero", min_sum=None):
    """dense.winding_fill's vote on a grid of crossing numbers"""
    m = n_axes + 1 if min_sum is None else min_sum
    return (np.abs(S) >= m) if rule == "nonzero" else (S >= m)


def labels(S, surface, n_axes, rule="nonzero", min_sum=None):
    """dense.winding_fill's labels: 1 on the surface voxels (a bool grid), 2 on the other voxels that the vote calls inside"""
    return np.where(surface, 1, np.where(inside(S, n_axes, rule, min_sum), 2, 0)).astype(np.uint8)


# ---- what the host tests and the device cases share ---------------------------------------------------------------------------------

R_HOLE = 134   # the triangle taken out of weld(uv_sphere(8)): near the lowest z and facing it, so that the z rays alone see the hole

# unit transforms of the soups: the identity, a cyclic permutation, a permutation with a flip, the point reflection, a quarter turn
PERMS = [[1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 1, 0, 0, 0, 1, 1, 0, 0], [0, 0, -1, 0, 1, 0, 1, 0, 0],
         [-1, 0, 0, 0, -1, 0, 0, 0, -1], [0, -1, 0, 1, 0, 0, 0, 0, 1]]


def _tetra(p):
    a, b, c, d = p
    return np.array([np.concatenate(t) for t in ((a, b, c), (a, d, b), (a, c, d), (b, d, c))])


def pieces(rng):
    """A soup of closed and open pieces about the unit cube (model space, float64 [T, 9]): tetrahedra, boxes, welded spheres,
    open sheets (tilted or level), open fans (a cap without its base), faces parallel to an axis, a closed piece with a sheet
    through it, and now and then duplicated triangles."""
    out = []
    for _ in range(int(rng.integers(2, 6))):
        k = int(rng.integers(0, 7))
        c = rng.random(3) * 0.8 + 0.1
        s = rng.uniform(0.05, 0.45)
        if k == 0:
            out.append(_tetra(c + s * (rng.random((4, 3)) - 0.5)))
        elif k == 1:
            lo, hi = c - s / 2 * rng.random(3), c + s / 2 * rng.random(3) + 1e-3
            out.append((lo + meshes.unit_cube().reshape(-1, 3).astype(np.float64) * (hi - lo)).reshape(-1, 9))
        elif k == 2:
            out.append(fill_ref.weld(meshes.uv_sphere(int(rng.integers(6, 13)))).astype(np.float64) * (s / 2) + np.tile(c, 3))
        elif k == 3:
            p = c + s * (rng.random((4, 3)) - 0.5)
            if rng.random() < 0.4:
                p[:, int(rng.integers(0, 3))] = c[0]
            out.append(np.array([np.concatenate([p[0], p[1], p[2]]), np.concatenate([p[0], p[2], p[3]])])[: int(rng.integers(1, 3))])
        elif k == 4:
            n = int(rng.integers(3, 9))
            ang = 2 * np.pi * np.arange(n + 1) / n
            ring = c + np.roll(np.stack([s * np.cos(ang), s * np.sin(ang), np.zeros(n + 1)], axis=1), int(rng.integers(0, 3)), axis=1)
            hub = c + s * rng.uniform(-1, 1, 3)
            out.append(np.array([np.concatenate([hub, ring[i], ring[i + 1]]) for i in range(n)]))
        elif k == 5:
            p = c + s * (rng.random((3, 3)) - 0.5)
            p[:, int(rng.integers(0, 3))] = c[0]
            out.append(p.reshape(1, 9))
        else:
            out.append(_tetra(c + s * (rng.random((4, 3)) - 0.5)))
            out.append((c + s * (rng.random((3, 3)) - 0.5)).reshape(1, 9))
    v = np.concatenate(out)
    if rng.random() < 0.3:
        v = np.concatenate([v, v[rng.integers(0, len(v), size=max(1, len(v) // 4))]])
    return v


def lattice(v, S, ss):
    """unit-cube pieces scaled to a sample space of S with every coordinate on a line or layer centre (k ss + ss/2) or on a
    boundary, some beyond the grid; a rule of the value alone, so bit-identical vertices stay identical and closed pieces closed"""
    sv = np.asarray(v, np.float64).reshape(-1, 3) * (S + 2 * ss) - ss
    sv = np.where(np.floor(sv * 7) % 3 != 0, np.floor(sv / ss) * ss + 0.5 * ss, np.round(sv))
    return sv.reshape(-1, 9)
