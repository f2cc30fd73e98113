"""What the solid-fill tests share: the record-for-record check of a fill call against the flag-off call and the numpy
restatement (tests/fill_ref.py), materials, user bounds with a power-of-two mesh transform, and the seeded construction of
triangles whose column test only the exact sign decides."""
from fractions import Fraction
from math import gcd

import numpy as np
import pytest

from obj2voxel_amd import meshes
from tests import fill_ref

ARGB = 0xFF12AB34


def materials(kind, v):
    from obj2voxel_amd import hip
    T = len(v)
    if kind == "none":
        return {}, []
    if kind == "coloured":
        return dict(types=np.full(T, hip.TRI_UNTEXTURED, np.uint32), colors=meshes.triangle_colors(T)), []
    uv = np.tile(np.array([[0, 0, 1, 0, 0.5, 1]], np.float32), (T, 1))
    return dict(uvs=uv, types=np.full(T, hip.TRI_TEXTURED, np.uint32), texids=np.zeros(T, np.int32)), [(meshes.checker_texture(64, 8), 1)]


def in_region(keys, G, zslab=(0, 0), xtile=(0, 0), ytile=(0, 0)):
    """the keys (x * G + y) * G + z inside a call's z-slab and x / y tile ((0, 0): the whole axis)"""
    x, y, z = keys // (G * G), keys // G % G, keys % G
    ok = np.ones(len(keys), bool)
    for c, (a, b) in ((x, xtile), (y, ytile), (z, zslab)):
        if (a, b) != (0, 0):
            ok &= (c >= a) & (c < b)
    return keys[ok]


def check_fill(dv, v, res, ss=1, bounds=None, **kw):
    """flag off, then on: surface part, interior against the restatement (within the call's slab and tile), stats.
    Returns (surface, filled)."""
    region = {k: kw[k] for k in ("zslab", "xtile", "ytile") if k in kw}
    if region:
        # (a call whose slab or tile misses the mesh's box returns before it computes the transform; the whole grid's call,
        # with the same resolution, bounds and unit transform, sets the one the restatement needs)
        dv.voxelize(res, supersampling=ss, bounds=bounds, **{k: a for k, a in kw.items() if k not in region})
    surf = dv.voxelize(res, supersampling=ss, bounds=bounds, **kw)
    filled = dv.voxelize(res, supersampling=ss, bounds=bounds, fill=True, fill_argb=ARGB, **kw)
    st = dv.stats()
    n = len(surf)
    assert len(filled) >= n
    assert np.array_equal(meshes.sorted_voxels(filled[:n]), meshes.sorted_voxels(surf)), "the surface part differs"
    tail = filled[n:]
    assert np.all(tail[:, 3] == ARGB)
    assert st["interior_voxels"] == len(tail) and st["voxels"] == len(filled)
    sv = fill_ref.sample_vertices(v, dv.transform())
    want = np.setdiff1d(in_region(fill_ref.parity_keys(sv, res, ss), res, **region), fill_ref.keys(surf, res))
    got = fill_ref.keys(tail, res)
    assert len(np.unique(got)) == len(got)
    assert np.array_equal(got, want), (len(got), len(want))
    return surf, filled


def power_of_two_bounds(dv, G, ss):
    """User bounds [0, B]^3 under which the mesh transform is x -> 2^k x + 0.25 exactly (found by trying B = (S - 1/2) / 2^k),
    so that model coordinates land exactly on any half-integer sample coordinate."""
    S = G * ss
    for k in range(12):
        bounds = [0, 0, 0] + [float(np.float32((S - 0.5) / 2.0 ** k))] * 3
        dv.voxelize(G, supersampling=ss, bounds=bounds)
        xf = dv.transform()
        m = float(xf[0])
        if m > 0 and np.log2(m) == int(np.log2(m)) and xf[9] == 0.25 and xf[0] == xf[4] == xf[8] and xf[9] == xf[10] == xf[11]:
            return bounds, m
    pytest.fail("no user bounds with a power-of-two mesh transform")


def to_model(sv, m):
    """sample-space coordinates -> model coordinates under x -> m x + 0.25 (m a power of two); asserts that they are exact"""
    s = np.asarray(sv, np.float32)
    v = ((s.astype(np.float64) - 0.25) / m).astype(np.float32)
    assert np.array_equal((v.astype(np.float64) * m + 0.25).astype(np.float32), s) and np.array_equal(v.astype(np.float64) * m + 0.25, s)
    return v.reshape(-1, 9)


def _naive_sign(ux, uy, vx, vy, px, py):
    """the column-test sign with the plain float64 value of the edge function (ties by the perturbation)"""
    det = (vx - ux) * (py - uy) - (vy - uy) * (px - ux)
    if det:
        return 1 if det > 0 else -1
    return (-1 if vy > uy else 1) if vy != uy else (1 if vx > ux else -1)


def exact_sign_set(seed, G, ss, n=6):
    """n sample-space triangles, each covering one column P only by a sign that Shewchuk's float64 filter cannot decide and
    the plain float64 value gets wrong.  Found by a seeded search: the edge U -> V runs from U in [1/4, 1/2)^2 (float32 steps of
    2^-25) to V about 4 * 10^4 away, through P up to a few 2^-33.  The edge function is affine in U,
    e = C + A U.x + B U.y (A = V.y - P.y, B = P.x - V.x), so for each U.x of a window the U.y nearest the line follows by integer
    division; the candidates with a small non-zero residual are kept if the filter leaves them open and the naive sign differs.
    The third vertex W lies 20 samples off the edge on P's side, high up, so that P is well inside the other two edges and
    toggles from layer 2 to the mesh's top.  Returns ([n, 3, 3] float32, [(i, j)] the columns)."""
    F = Fraction
    rng = np.random.default_rng(seed)
    h, S, q = 0.5 * ss, G * ss, F(1, 2 ** 25)
    zl, zh = 2 * ss + 0.125, S - 3.75
    tris, cols = [], []
    while len(tris) < n:
        i, j = (int(c) for c in rng.integers(G // 4, 3 * G // 4, size=2))
        if (i, j) in cols:
            continue
        px, py = i * ss + h, j * ss + h
        d = np.array([px, py]) - 0.375
        v = (0.375 + d * (1.0 + rng.uniform(2e4, 4.5e4) / np.linalg.norm(d))).astype(np.float32)
        vx, vy = F(float(v[0])), F(float(v[1]))
        A, B = vy - F(py), F(px) - vx
        D = vx * F(py) - vy * F(px) + (A + B) / 4   # e at U = (1/4, 1/4)
        den = 1
        for x in (D, A * q, B * q):
            den = den * x.denominator // gcd(den, x.denominator)
        Di, Ai, Bi = int(D * den), int(A * q * den), int(B * q * den)   # e den = Di + Ai a + Bi b for U = 1/4 + (a, b) 2^-25
        a0 = int(rng.integers(0, 2 ** 23 - 2 ** 21))
        a = np.arange(a0, a0 + 2 ** 21, dtype=np.int64)
        num = -(Di + Ai * a)
        b = (2 * num + Bi) // (2 * Bi)   # (the integer nearest to num / Bi, for either sign of Bi)
        t = Di + Ai * a + Bi * b
        ok = (b >= 0) & (b < 2 ** 23) & (t != 0) & (np.abs(t) < 64)
        for k in np.nonzero(ok)[0]:
            ux, uy = np.float32(0.25 + int(a[k]) * 2.0 ** -25), np.float32(0.25 + int(b[k]) * 2.0 ** -25)
            args = (float(ux), float(uy), float(v[0]), float(v[1]), px, py)
            exact = fill_ref._exact_sign(*args)
            assert exact == (1 if t[k] > 0 else -1)
            l, r = (args[2] - args[0]) * (py - args[1]), (args[3] - args[1]) * (px - args[0])
            if abs(l - r) > fill_ref._BOUND * (abs(l) + abs(r)) or _naive_sign(*args) == exact:
                continue
            e = np.array([-(float(v[1]) - float(uy)), float(v[0]) - float(ux)])
            w = np.array([px, py]) + np.round(20 * ss * exact * e / np.linalg.norm(e))
            tri = np.array([[ux, uy, zl], [v[0], v[1], zl], [w[0], w[1], zh]], np.float32)
            # P well inside the other two edges, on the side of the exact sign
            if fill_ref._e(tri[1:2], tri[2:3], px, py)[0] * exact < 1 or fill_ref._e(tri[2:3], tri[0:1], px, py)[0] * exact < 1:
                continue
            tris.append(tri)
            cols.append((i, j))
            break
    return np.array(tris, np.float32), cols
