"""The bands that k_voxelize's work-removal margins decide (obj2voxel_amd/csrc/o2v_dev_k2_voxelize.hpp): kSatMargin, the floor F
of the row test's inflation, and kCertainMargin, the floor D of the certain-hit test's margins.  A (triangle, voxel) pair whose
distance is inside F becomes a voxel job that the clip rejects; one outside it is never looked at.  A hit that enters its voxel
by more than D is marked without a clip.  Both only remove work - by argument (the error budgets beside the constants); here
geometry is placed on both sides of F, D and of the floors they replaced (0.02, 0.03), and every case must give the same records
three ways: fast mode, exact mode (O2V_HIP_FLAG_EXACT_CLIP: every margin off) and the CPU oracle - without materials (the
certain test, the job filter), coloured MAX, and coloured BLEND (where a lost sliver of weight would change a colour).

With bounds [-0.25, S - 0.75] the mesh transform is x -> x + 0.5 up to rounding (tests/test_gpu_fuzz.py::_planar_case), so
model coordinate k - 0.5 + o lies o beside the voxel plane k."""
import numpy as np
import pytest

from obj2voxel_amd import meshes

pytestmark = pytest.mark.gpu

F = 0.01     # kSatMargin (O2V_SAT_FLOOR)
D = 0.0075   # kCertainMargin (O2V_CERTAIN_FLOOR)
_MAG = [2.0 ** -16, 2.0 ** -12, 1e-3, F / 2, F, 1.5 * F, 2 * F, D, 2 * D, 0.02, 0.03]
NOISE = np.array([0.0] + _MAG + [-x for x in _MAG])


def _bounds(S):
    return [-0.25] * 3 + [S - 0.75] * 3


def _lattice(rng, T, S, slab):
    """Integer voxel planes for T triangles' first vertices, a few voxels inside the grid (the triangles are at most four voxels
    across); with a slab, z inside its eight layers and half of the triangles at the far end of x and y."""
    if slab is None:
        return rng.integers(5, S - 5, size=(T, 1, 3)).astype(np.float64)
    k = rng.integers(5, S - 5, size=(T, 1, 3))
    far = rng.random(T) < 0.5
    k[far, :, 0:2] = rng.integers(S - 40, S - 5, size=(int(far.sum()), 1, 2))
    k[:, :, 2] = rng.integers(slab[0] + 2, slab[1] - 2, size=(T, 1))
    return k.astype(np.float64)


def _signed_perm(rng, T):
    """A random signed axis permutation per triangle, as (T, 3, 3) matrices."""
    m = np.zeros((T, 3, 3))
    for i in range(T):
        m[i, np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], size=3)
    return m


def _plane_case(normal, S, seed):
    """Triangles one to four voxels across whose plane lies a NOISE offset beside the voxel plane (axis-aligned normal), the voxel
    edge (a normal at 45 degrees about one axis) or the lattice point (the normal (3, 2, 6) / 7) through k."""
    rng = np.random.default_rng(11_000 + 100 * seed + {"axis": 0, "diag": 1, "generic": 2}[normal] + (7 if S > 16 else 0))
    T = 600
    slab = None if S == 16 else (S - 10, S - 2)
    k = _lattice(rng, T, S, slab)
    off = rng.choice(NOISE, size=(T, 1, 1))
    if normal == "axis":
        n, u, w = np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
        s = rng.integers(-2, 3, size=(T, 3, 1)) + rng.choice(NOISE, size=(T, 3, 1))
        t = rng.integers(-2, 3, size=(T, 3, 1)) + rng.choice(NOISE, size=(T, 3, 1))
    elif normal == "diag":
        r = np.sqrt(0.5)
        n, u, w = np.array([r, r, 0.0]), np.array([r, -r, 0.0]), np.array([0.0, 0.0, 1.0])
        # along u in half diagonals (edge to centre line to edge), along w in voxels
        s = (rng.integers(-2, 3, size=(T, 3, 1)) + rng.choice(NOISE, size=(T, 3, 1))) * np.sqrt(2.0) / 2
        t = rng.integers(-2, 3, size=(T, 3, 1)) + rng.choice(NOISE, size=(T, 3, 1))
    else:
        n = np.array([3.0, 2.0, 6.0]) / 7.0
        u = np.array([2.0, -3.0, 0.0]) / np.sqrt(13.0)
        w = np.cross(n, u)
        s = rng.random((T, 3, 1)) * 4 - 2
        t = rng.random((T, 3, 1)) * 4 - 2
    rel = off * n + s * u + t * w                       # (T, 3 vertices, 3 axes) around the lattice point
    rel = np.einsum("tij,tvj->tvi", _signed_perm(rng, T), rel)
    v = (k - 0.5 + rel).astype(np.float32).reshape(T, 9)
    kw = dict(bounds=_bounds(S))
    if slab is not None:
        kw["zslab"] = slab
    return v, S, kw, None


def _edge_case(S, seed):
    """Vertices a NOISE offset beside voxel corners (every coordinate its own offset: edges run beside voxel edges), a fifth
    of the triangles in a voxel plane's band, and slivers of altitude below 0.05 along such edges."""
    rng = np.random.default_rng(12_000 + seed + (7 if S > 16 else 0))
    T, T_sliver = 500, 300
    slab = None if S == 16 else (S - 10, S - 2)
    k = np.repeat(_lattice(rng, T + T_sliver, S, slab), 3, axis=1)
    k[:, 1:, :] += rng.integers(-3, 4, size=(T + T_sliver, 2, 3))
    rel = rng.choice(NOISE, size=(T + T_sliver, 3, 3))
    for i in range(0, T, 5):
        a = int(rng.integers(0, 3))
        k[i, :, a] = k[i, 0, a]
        rel[i, :, a] = rel[i, 0, a]
    # slivers: the third vertex on the edge of the first two, moved off it by a NOISE magnitude (all below 0.05)
    a, b = k[T:, 0] + rel[T:, 0], k[T:, 1] + rel[T:, 1]
    same = np.all(k[T:, 0] == k[T:, 1], axis=1)
    b[same, 0] += 2.0
    e = b - a
    perp = np.cross(e, np.eye(3)[rng.integers(0, 3, size=T_sliver)])
    flat = np.linalg.norm(perp, axis=1) < 1e-6
    perp[flat] = np.cross(e[flat], np.array([1.0, 1.0, 0.0]))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    c = a + (0.2 + 0.6 * rng.random((T_sliver, 1))) * e + np.abs(rng.choice(NOISE, size=(T_sliver, 1))) * perp
    pts = k + rel
    pts[T:, 2] = c
    v = (pts - 0.5).astype(np.float32).reshape(T + T_sliver, 9)
    kw = dict(bounds=_bounds(S))
    if slab is not None:
        kw["zslab"] = slab
    return v, S, kw, None


def _handover_case(base_xy, seed, S=8000):
    """tests/test_gpu_fuzz.py::_far_corner_case's recipe where the floors hand over to the proportional terms 2.5e-6 m and
    3.75e-6 m (m: a leaf's largest |coordinate|): small triangles around x = y = base_xy in a thin slab - at the bottom of the
    grid, so that m is base_xy and not S - with offsets on both sides of both terms.  An x / y tile keeps the grids small."""
    rng = np.random.default_rng(13_000 + seed + int(base_xy))
    T = 500
    k = np.empty((T, 3, 3))
    k[:, :, 0:2] = base_xy + rng.integers(0, 8, size=(T, 3, 2))
    k[:, :, 2] = rng.integers(2, 14, size=(T, 3))
    k[:, 1:, :] = k[:, :1, :] + rng.integers(-3, 4, size=(T, 2, 3))
    k[:, :, 2] = np.clip(k[:, :, 2], 2, 14)
    k[:, :, 0:2] = np.minimum(k[:, :, 0:2], S - 2)     # (every vertex inside the bounds, see _planar_case)
    m = min(base_xy + 8.0, S - 2.0)
    prop = [f * c * m for c in (2.5e-6, 3.75e-6) for f in (0.5, 0.9, 1.1, 2.0)]
    noise = np.concatenate([NOISE, prop, [-x for x in prop], [np.spacing(np.float32(m)), -np.spacing(np.float32(m))]])
    v = (k - 0.5 + rng.choice(noise, size=(T, 3, 3))).astype(np.float32).reshape(T, 9)
    b = (int(base_xy) - 8) // 4 * 4
    tile = (b, min(int(base_xy) + 20, S))
    kw = dict(bounds=_bounds(S), zslab=(0, 16))
    return v, S, kw, tile


def _routes(v, seed, which):
    rng = np.random.default_rng(14_000 + seed)
    col = dict(types=np.full(len(v), 2, np.uint32), colors=rng.random((len(v), 3)).astype(np.float32))
    all_routes = {"none": ({}, 0), "max": (col, 0), "blend": (col, 1)}
    return [(r, *all_routes[r]) for r in which]


def _inside(vox, tile):
    if tile is None:
        return vox
    m = np.ones(len(vox), bool)
    for axis in (0, 1):
        m &= (vox[:, axis] >= tile[0]) & (vox[:, axis] < tile[1])
    return vox[m]


@pytest.fixture(scope="module")
def dv():
    from obj2voxel_amd import hip
    d = hip.DeviceVoxelizer(0)
    yield d
    d.close()


def _check(dv, oracle, case, seed, which=("none", "max", "blend")):
    v, S, kw, tile = case
    assert len(v) <= 2000
    tiles = {} if tile is None else dict(xtile=tile, ytile=tile)
    for route, mat, strategy in _routes(v, seed, which):
        want = meshes.sorted_voxels(_inside(oracle.voxelize(v, S, strategy=strategy, **mat, **kw), tile))
        assert len(want) > 200, (route, len(want))      # (a condition on the inputs)
        dv.set_triangles(v, **mat)
        fast = meshes.sorted_voxels(dv.voxelize(S, strategy=strategy, **kw, **tiles))
        st = dv.stats()
        exact = meshes.sorted_voxels(dv.voxelize(S, strategy=strategy, exact_clip=True, **kw, **tiles))
        st_exact = dv.stats()
        print(route, "voxels", len(want), "fast", {x: st[x] for x in ("jobs", "skipped_jobs", "hits", "certain_hits")}, "exact jobs", st_exact["jobs"])
        # the case is inside the bands: hits that need no clip, survivors of the row test that the clip rejects, and a row test
        # that removes candidates at all
        if route == "none":
            assert st["certain_hits"] > 0, st
        assert st["jobs"] + st["certain_hits"] > st["hits"] + st["skipped_jobs"], st
        assert st_exact["jobs"] > st["jobs"], (st, st_exact)
        assert fast.shape == want.shape and np.array_equal(fast, want), (route, "fast", fast.shape, want.shape)
        assert exact.shape == want.shape and np.array_equal(exact, want), (route, "exact", exact.shape, want.shape)
        assert np.array_equal(fast, exact), route


@pytest.mark.parametrize("S", [16, 1024])
@pytest.mark.parametrize("normal", ["axis", "diag", "generic"])
def test_planes_beside_voxel_faces(dv, oracle, normal, S):
    _check(dv, oracle, _plane_case(normal, S, 0), 0)


@pytest.mark.parametrize("S", [16, 1024])
def test_edges_beside_voxel_edges_and_corners(dv, oracle, S):
    _check(dv, oracle, _edge_case(S, 0), 1)


@pytest.mark.parametrize("base_xy,seed", [(b, s) for b in (2000.0, 4090.0, 7990.0) for s in (0, 1)])
def test_floor_hands_over_to_the_proportional_term(dv, oracle, base_xy, seed):
    # (odd seeds without materials only, as in test_far_corner_case; even ones on all three routes, so that both seeds put the
    # certain test's floor at its hand-over)
    _check(dv, oracle, _handover_case(base_xy, seed), seed, which=("none",) if seed % 2 == 1 else ("none", "max", "blend"))
