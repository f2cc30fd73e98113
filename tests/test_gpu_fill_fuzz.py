"""Solid fill (O2V_HIP_FLAG_FILL_INTERIOR) on meshes that are open, cropped, mirrored, far from the origin or degenerate, record
for record against the numpy restatement (tests/fill_ref.py) through tests.fill_cases.check_fill: seeded soups, the exact-sign
fallback, far coordinates, the bitmap's and the emission's edges, empty calls, and invariance under the A/B switches."""
import numpy as np
import pytest

from obj2voxel_amd import meshes
from tests import fill_ref
from tests.fill_cases import ARGB, check_fill, exact_sign_set, materials, power_of_two_bounds, to_model

pytestmark = pytest.mark.gpu

PERMS = [[1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 1, 0, 0, 0, 1, 1, 0, 0], [0, 0, -1, 0, 1, 0, 1, 0, 0],
         [-1, 0, 0, 0, -1, 0, 0, 0, -1], [0, -1, 0, 1, 0, 0, 0, 0, 1]]


@pytest.fixture(scope="module")
def dv():
    from obj2voxel_amd import hip
    d = hip.DeviceVoxelizer(0)
    yield d
    d.close()


def _box(lo, hi):
    v = meshes.unit_cube().reshape(-1, 3).astype(np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return (lo + v * (hi - lo)).reshape(-1, 9)


def _tetra(p):
    a, b, c, d = p
    return np.array([np.concatenate(t) for t in ((a, b, c), (a, d, b), (a, c, d), (b, d, c))])


def _sphere(n, r, c):
    return fill_ref.weld(meshes.uv_sphere(n)).astype(np.float64) * r + np.tile(c, 3)


def _fan(hub, ring):
    return np.array([np.concatenate([hub, ring[k], ring[k + 1]]) for k in range(len(ring) - 1)])


def _soup(rng, T):
    """the kinds of tests/test_gpu_fuzz.py::_case: small, large, axis-aligned, degenerate, sliver"""
    kind = rng.integers(0, 5, size=T)
    c = rng.random((T, 1, 3))
    v = np.empty((T, 3, 3))
    for i in range(T):
        if kind[i] == 0:
            v[i] = c[i] + 0.08 * (rng.random((3, 3)) - 0.5)
        elif kind[i] == 1:
            v[i] = rng.random((3, 3))
        elif kind[i] == 2:
            v[i] = rng.random((3, 3))
            v[i][:, rng.integers(0, 3)] = np.round(rng.random() * 8) / 8
        elif kind[i] == 3:
            a, b = rng.random(3), rng.random(3)
            v[i] = [a, b, a if rng.random() < 0.5 else (a + b) / 2]
        else:
            v[i] = c[i] + 1e-3 * (rng.random((3, 3)) - 0.5)
    return v.reshape(T, 9)


def _pieces(rng):
    """closed and open pieces about the unit cube (model space; _lattice_mesh snaps them to column and layer centres)"""
    out = []
    for _ in range(int(rng.integers(1, 6))):
        k = int(rng.integers(0, 8))
        c = rng.random(3) * 0.8 + 0.1
        s = rng.uniform(0.05, 0.45)
        if k == 0:
            out.append(_tetra(c + s * (rng.random((4, 3)) - 0.5)))
        elif k == 1:
            out.append(_box(c - s / 2 * rng.random(3), c + s / 2 * rng.random(3) + 1e-3))
        elif k == 2:
            out.append(_sphere(int(rng.integers(6, 13)), s / 2, c))
        elif k == 3:   # open sheet: one triangle or a quad, tilted or horizontal
            p = c + s * (rng.random((4, 3)) - 0.5)
            if rng.random() < 0.4:
                p[:, 2] = c[2]
            out.append(np.array([np.concatenate([p[0], p[1], p[2]]), np.concatenate([p[0], p[2], p[3]])])[: int(rng.integers(1, 3))])
        elif k == 4:   # open fan (a cap without its base), hub above or below the ring
            n = int(rng.integers(3, 9))
            ang = 2 * np.pi * np.arange(n + 1) / n
            ring = c + np.stack([s * np.cos(ang), s * np.sin(ang), np.zeros(n + 1)], axis=1)
            out.append(_fan(c + [0, 0, s * rng.uniform(-1, 1)], ring))
        elif k == 5:   # vertical faces
            p = c + s * (rng.random((3, 3)) - 0.5)
            p[:, 0] = c[0]
            q = c + s * (rng.random((3, 3)) - 0.5)
            q[:, 1] = q[0, 1] + (q[:, 0] - q[0, 0]) * 0.5
            out.append(np.stack([p.reshape(9), q.reshape(9)]))
        elif k == 6:   # a closed piece with an open sheet through it
            out.append(_tetra(c + s * (rng.random((4, 3)) - 0.5)))
            p = c + s * (rng.random((3, 3)) - 0.5)
            out.append(p.reshape(1, 9))
        else:
            out.append(_soup(rng, int(rng.integers(1, 40))))
    v = np.concatenate(out)
    if rng.random() < 0.3:
        v = np.concatenate([v, v[rng.integers(0, len(v), size=max(1, len(v) // 4))]])   # duplicates: toggle twice
    return v


def _fill_case(seed):
    rng = np.random.default_rng(31000 + seed)
    lattice = seed % 5 == 4
    res = int(rng.choice([16, 33, 48, 64, 65, 90, 128, 200] if seed % 10 else [200]))
    ss = int(rng.choice([1, 1, 2]))
    kw = dict(strategy=int(rng.integers(0, 2)))
    v = _pieces(rng)
    if not lattice:
        if rng.random() < 0.4:
            kw["unit_transform"] = PERMS[int(rng.integers(0, len(PERMS)))]
        r = rng.random()
        if r < 0.35:   # user bounds that cut the mesh on every side (crossings below layer 0, columns outside the grid)
            kw["bounds"] = list(rng.uniform(0.1, 0.3, 3)) + list(rng.uniform(0.7, 0.9, 3))
        elif r < 0.5:
            kw["bounds"] = [-0.1, -0.2, -0.05, 1.3, 1.1, 1.2]
    if rng.random() < 0.3:
        z0 = int(rng.integers(0, res - 1))
        kw["zslab"] = (z0, int(rng.integers(z0 + 1, res + 1)))
    if rng.random() < 0.25:
        x0 = int(rng.integers(0, res // 4)) * 4 if res >= 8 else 0
        kw["xtile"] = (x0, int(rng.integers(x0 + 1, res + 1)))
        y0 = int(rng.integers(0, res // 4)) * 4 if res >= 8 else 0
        kw["ytile"] = (y0, int(rng.integers(y0 + 1, res + 1)))
    mat = ["none", "coloured", "textured"][seed % 3]
    return v, res, ss, kw, mat, lattice


def _lattice_mesh(v, S, ss):
    """unit-cube pieces scaled to sample space with every coordinate on a column or layer centre (k ss + ss/2) or a
    boundary, some beyond the grid"""
    sv = np.asarray(v, np.float64).reshape(-1, 3) * (S + 2 * ss) - ss
    h = 0.5 * ss
    # (a rule of the value alone: bit-identical vertices stay identical and closed pieces closed)
    sv = np.where(np.floor(sv * 7) % 3 != 0, np.floor(sv / ss) * ss + h, np.round(sv))
    return sv.reshape(-1, 9)


@pytest.mark.parametrize("seed", range(100))
def test_fill_fuzz_case(dv, seed):
    v, res, ss, kw, mat, lattice = _fill_case(seed)
    kw = dict(kw)
    if lattice:
        dv.set_triangles(meshes.unit_cube())
        kw["bounds"], m = power_of_two_bounds(dv, res, ss)
        want_s = _lattice_mesh(v, res * ss, ss)
        v = to_model(want_s, m)
    else:
        v = v.astype(np.float32)
    kwm, tex = materials(mat, v)
    dv.set_textures(tex)
    dv.set_triangles(v, **kwm)
    check_fill(dv, v, res, ss, **kw)
    if lattice:
        assert np.array_equal(fill_ref.sample_vertices(v, dv.transform()).reshape(-1, 9), want_s.astype(np.float32))


@pytest.mark.parametrize("G,ss", [(96, 1), (64, 2)])
def test_exact_sign_fallback_on_device(dv, G, ss):
    """Edges that pass a few 2^-33 from a column centre, from a vertex near 1/4 to one near 4 * 10^4: only the exact sign
    decides their columns, and the plain float64 sign gets them wrong (tests/test_host_fill.py checks that on the host)."""
    sv, cols = exact_sign_set(23 + ss, G, ss)
    dv.set_triangles(meshes.unit_cube())
    bounds, m = power_of_two_bounds(dv, G, ss)
    v = to_model(sv, m)
    for strategy, mat in ((0, "none"), (1, "coloured")):
        kwm, _ = materials(mat, v)
        dv.set_textures([])
        dv.set_triangles(v, **kwm)
        surf, filled = check_fill(dv, v, G, ss, bounds=bounds, strategy=strategy)
        assert np.array_equal(fill_ref.sample_vertices(v, dv.transform()), sv)
        # the columns the naive sign gets wrong hold interior records: a kernel without the exact path would differ
        naive = np.setdiff1d(fill_ref.parity_keys(sv, G, ss, exact=False), fill_ref.keys(surf, G))
        assert not np.array_equal(naive, fill_ref.keys(filled[len(surf):], G))


def _far_case(seed, G, ss, base):
    """small closed boxes and tetrahedra and open sheets at x, y ~ base (output voxels) in the top 8 layers of a G^3 grid,
    vertices on sample planes or a few float32 ulps beside them (mesh transform x -> x + 0.5 up to rounding)"""
    rng = np.random.default_rng(41000 + seed)
    S = G * ss
    ulp = 2.0 ** (np.floor(np.log2(base * ss)) - 23)
    out = []
    for n in range(12):
        c = np.array([base * ss + rng.integers(0, 24 * ss), base * ss + rng.integers(0, 24 * ss), S - rng.integers(4, 7 * ss)], np.float64)
        s = rng.integers(2, 5 * ss, size=3).astype(np.float64) if n else np.full(3, 4.0 * ss)
        k = int(rng.integers(0, 3)) if n else 0
        if k == 0:
            out.append(_box(c - s, c + s))
        elif k == 1:
            out.append(_tetra(c + rng.integers(-4, 5, size=(4, 3)) * ss))
        else:
            p = c + rng.integers(-4, 5, size=(3, 3)) * ss
            p[:, 2] = np.clip(p[:, 2], S - 7 * ss, S - 1)
            out.append(p.reshape(1, 9))
    k = np.concatenate(out).reshape(-1, 3)
    k[:, 2] = np.clip(k[:, 2], S - 8 * ss, S - 1)
    noise = np.array([0.0, 0.0, ulp, -ulp, 0.25, 0.5])[(k.astype(np.int64) * 7919) % 6]   # (by value: closed pieces stay closed)
    return (k - 0.5 + noise).astype(np.float32).reshape(-1, 9), [-0.25] * 3 + [S - 0.75] * 3


@pytest.mark.parametrize("seed,G,ss,base", [(0, 60000, 1, 59960), (1, 60000, 1, 59960), (2, 33000, 2, 32760)])
def test_far_coordinates(seed, G, ss, base):
    from obj2voxel_amd import hip
    v, bounds = _far_case(seed, G, ss, base)
    hip._bind().o2v_release_cached_device_memory()
    d = hip.DeviceVoxelizer(0)   # own context
    try:
        for mat in ("none", "coloured"):
            kwm, _ = materials(mat, v)
            d.set_triangles(v, **kwm)
            _, filled = check_fill(d, v, G, ss, bounds=bounds, strategy=1, zslab=(G - 9, G))
            assert np.sum(filled[:, 3] == ARGB) > 50
    finally:
        d.close()
        hip._bind().o2v_release_cached_device_memory()


def _slab_box(G, ss, hi):
    """a closed box from beyond the grid's low faces to just above output voxel hi = (x, y, z): every cell of the tile / slab
    below hi is inside (user bounds [0, 1]^3)"""
    S = G * ss
    top = [min((h * ss + 1.3) / S, 1.05) for h in hi]
    return _box([-0.05] * 3, top).astype(np.float32)


EDGES = [  # G, zslab, xtile, ytile: pass boxes 1 .. 65 layers tall; 2047, 2048 and 2049 bitmap words
    *[(96, (7, 7 + h), (0, 0), (0, 0)) for h in (1, 31, 32, 33, 63, 64, 65)],
    (96, (0, 20), (0, 23), (0, 89)),     # 1 x 23 x 89 = 2047 words, one chunk
    (96, (0, 32), (0, 32), (0, 64)),     # 2048: one chunk exactly, every word full
    (704, (0, 80), (0, 683), (0, 1)),    # 3 x 683 = 2049: a second chunk with one word
]


@pytest.mark.parametrize("G,zslab,xtile,ytile", EDGES)
def test_bitmap_and_emission_edges(dv, G, zslab, xtile, ytile):
    for ss in (1, 2):
        v = _slab_box(G, ss, (xtile[1] or G, ytile[1] or G, zslab[1]))
        dv.set_textures([])
        dv.set_triangles(v)
        _, filled = check_fill(dv, v, G, ss, bounds=[0, 0, 0, 1, 1, 1], zslab=zslab, xtile=xtile, ytile=ytile)
        nx, ny = (xtile[1] or G) - xtile[0], (ytile[1] or G) - ytile[0]
        # the box's faces lie outside the pass box but for its top: nearly every cell is an interior record
        assert dv.stats()["interior_voxels"] >= nx * ny * (zslab[1] - zslab[0] - 1)


def test_interior_beyond_the_output_of_an_earlier_call():
    from obj2voxel_amd import hip
    d = hip.DeviceVoxelizer(0)
    try:
        small = _tetra(np.array([[0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [0.1, 0.3, 0.1], [0.1, 0.1, 0.3]])).astype(np.float32)
        d.set_triangles(small)
        check_fill(d, small, 16, 1, bounds=[0, 0, 0, 1, 1, 1])
        big = _slab_box(160, 1, (160, 160, 150))
        d.set_triangles(big)
        filled = d.voxelize(160, bounds=[0, 0, 0, 1, 1, 1], fill=True, fill_argb=ARGB)   # (d_out as the small call left it)
        n_int = d.stats()["interior_voxels"]
        assert n_int > 160 * 160 * 140 and len(filled) == d.stats()["voxels"]
        surf = d.voxelize(160, bounds=[0, 0, 0, 1, 1, 1])
        assert np.array_equal(meshes.sorted_voxels(filled[:len(surf)]), meshes.sorted_voxels(surf))
        want = np.setdiff1d(fill_ref.parity_keys(fill_ref.sample_vertices(big, d.transform()), 160, 1), fill_ref.keys(surf, 160))
        assert np.all(filled[len(surf):, 3] == ARGB) and np.array_equal(fill_ref.keys(filled[len(surf):], 160), want)
    finally:
        d.close()


def _degenerate(kind):
    rng = np.random.default_rng(51000)
    if kind == "vertical":
        p = rng.random((40, 3, 3)) * 0.8 + 0.1
        p[:20, :, 0] = p[:20, :1, 0]
        p[20:, :, 1] = p[20:, :1, 1]
        return p.reshape(-1, 9)
    if kind == "degenerate":
        a, b = rng.random((30, 3)), rng.random((30, 3))
        return np.concatenate([np.concatenate([a, a, b], 1), np.concatenate([a, b, (a + b) / 2], 1), np.concatenate([a, a, a], 1)])
    if kind == "non-finite":
        p = rng.random((40, 9))
        p[np.arange(40), rng.integers(0, 9, size=40)] = rng.choice([np.nan, np.inf, -np.inf], size=40)
        return p
    return np.array([[0.2, 0.2, 0.3, 0.8, 0.3, 0.3, 0.4, 0.9, 0.3]])   # one horizontal triangle


@pytest.mark.parametrize("kind", ["vertical", "degenerate", "non-finite", "single", "slab above", "slab below", "tile beside"])
def test_calls_without_interior(dv, kind):
    """meshes that cover no column, and calls whose slab or tile misses the mesh: the flag-off records, no interior"""
    kw = dict(bounds=[0, 0, 0, 1, 1, 1])
    if kind in ("slab above", "slab below", "tile beside"):
        v = _box([0.3, 0.3, 0.3], [0.6, 0.55, 0.5])
        kw.update({"slab above": dict(zslab=(60, 64)), "slab below": dict(zslab=(0, 12)), "tile beside": dict(xtile=(48, 64))}[kind])
    else:
        v = _degenerate(kind)
    v = v.astype(np.float32)
    for ss, mat in ((1, "none"), (2, "coloured")):
        kwm, _ = materials(mat, v)
        dv.set_textures([])
        dv.set_triangles(v, **kwm)
        check_fill(dv, v, 64, ss, **kw)
        assert dv.stats()["interior_voxels"] == 0


def _open_mesh():
    """a bowl (the lower half of a welded sphere) and a tilted sheet, lower than wide: the mesh's top lies inside the grid"""
    s = fill_ref.weld(meshes.uv_sphere(16)).reshape(-1, 3, 3)
    bowl = s[s[:, :, 2].max(axis=1) <= 0].reshape(-1, 9) * np.array([0.5, 0.5, 0.3] * 3, np.float32) + np.array([-0.4, 0, 0.1] * 3, np.float32)
    sheet = np.array([[0.2, -0.5, -0.2, 0.9, -0.5, 0.25, 0.2, 0.5, -0.1], [0.9, -0.5, 0.25, 0.9, 0.5, 0.3, 0.2, 0.5, -0.1]], np.float32)
    return np.concatenate([bowl, sheet]).astype(np.float32)


def _switch_meshes():
    rng = np.random.default_rng(61000)
    soup = np.concatenate([_pieces(rng) for _ in range(3)]).astype(np.float32)
    sphere = fill_ref.weld(meshes.uv_sphere(20))
    return [("open", _open_mesh(), None), ("cropped closed", sphere, [-0.7, -0.8, -0.6, 0.75, 0.65, 0.9]), ("mixed soup", soup, None)]


SWITCHES = ["O2V_NO_CROP", "O2V_NO_DIRECT_MAX", "O2V_NO_OCCUPANCY_ONLY", "O2V_EXACT_CLIP", "O2V_ALL_LAUNCHES"]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_switch_invariance(dv, monkeypatch, which):
    """The fill depends on the mesh alone: the A/B switches, a non-finite triangle more (which turns the crop off) and the
    mesh's own bounds given as user bounds leave it bit for bit as it is; slabs and tiles split it exactly."""
    name, v, bounds = _switch_meshes()[which]
    G = 80
    for ss, mat in ((1, "none"), (2, "coloured")):
        kwm, _ = materials(mat, v)
        dv.set_textures([])
        dv.set_triangles(v, **kwm)
        _, base = check_fill(dv, v, G, ss, bounds=bounds)
        base = meshes.sorted_voxels(base)
        n_int = dv.stats()["interior_voxels"]
        assert n_int > 0, name
        for sw in SWITCHES:
            monkeypatch.setenv(sw, "1")
            got = dv.voxelize(G, supersampling=ss, bounds=bounds, fill=True, fill_argb=ARGB)
            assert dv.stats()["interior_voxels"] == n_int, (name, sw)
            assert np.array_equal(meshes.sorted_voxels(got), base), (name, sw)
            check_fill(dv, v, G, ss, bounds=bounds)
            monkeypatch.delenv(sw)
        # the mesh's bounds as user bounds, then a NaN and an inf triangle more (the bounds hint is no longer finite)
        b = bounds or [float(x) for x in np.concatenate([v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)])]
        got = dv.voxelize(G, supersampling=ss, bounds=b, fill=True, fill_argb=ARGB)
        assert np.array_equal(meshes.sorted_voxels(got), base), name
        bad = np.array([[np.nan, 0, 0, 0.1, 0.1, 0.1, 0.2, 0, 0.1], [0.1, 0.2, 0.3, 0.4, np.inf, 0.1, 0.3, 0.3, 0.3]], np.float32)
        vb = np.concatenate([v, bad])
        kwm, _ = materials(mat, vb)
        dv.set_triangles(vb, **kwm)
        check_fill(dv, vb, G, ss, bounds=b)
        # slabs and tiles of the same call split the set exactly
        dv.set_triangles(v, **materials(mat, v)[0])
        want = fill_ref.keys(base, G)
        cuts = [0, 5, 30, 31, 64, G]
        parts = [dv.voxelize(G, supersampling=ss, bounds=bounds, zslab=(a, c), fill=True, fill_argb=ARGB) for a, c in zip(cuts, cuts[1:])]
        assert np.array_equal(np.sort(np.concatenate([fill_ref.keys(p, G) for p in parts])), want), name
        xs = [0, 12, 40, G]
        parts = [dv.voxelize(G, supersampling=ss, bounds=bounds, xtile=(x0, x1), ytile=(y0, y1), fill=True, fill_argb=ARGB)
                 for x0, x1 in zip(xs, xs[1:]) for y0, y1 in zip(xs, xs[1:])]
        assert np.array_equal(np.sort(np.concatenate([fill_ref.keys(p, G) for p in parts])), want), name
