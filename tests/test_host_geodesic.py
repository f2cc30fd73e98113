"""Geodesic distances and shortest paths without a GPU: the numpy reference (tests/geodesic_ref.py) against
a heap Dijkstra that restates the header's words and against scipy.sparse.csgraph where scipy is present; closed forms; the kernel's
own relaxation, "which tiles see this voxel" mask and trace step compiled for the host and run tile by tile in a shuffled order and
as whole-grid sweeps, with one deliberate change that must be caught; the torch layer against a stub; the scratch formula; the K20
kernels in the gfx950 code object."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import bits_host
from tests import components_ref as CR
from tests import geodesic_ref as GR

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_components import words64  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401

K20 = os.path.join(SRC, "o2v_dev_k20_geodesic.hpp")
ALL_WEIGHTS = [(1, 0, 0), (1, 1, 0), (1, 1, 1), (3, 4, 5), (3, 4, 0), (2, 3, 0), (7, 1, 1)]
SMALL_DIMS = [(1, 1, 1), (1, 1, 9), (7, 1, 1), (1, 6, 1), (2, 2, 2), (5, 4, 3), (3, 7, 2)]


def seeds_for(rng, S, n=3):
    """Seeds in S (where it has voxels), one not in S or anywhere, and some outside the box."""
    nz, ny, nx = S.shape
    z, y, x = np.nonzero(S)
    pick = rng.integers(0, len(x), min(n, len(x))) if len(x) else []
    inside = [(int(x[i]), int(y[i]), int(z[i])) for i in pick]
    return inside + [tuple(int(v) for v in rng.integers(0, (nx, ny, nz)))] + [(-1, 0, 0), (nx, 0, 0), (0, ny + 3, 0), (2 ** 31 - 1, 0, 0)]


# ---- the reference against the definition --------------------------------------------------------------------------------------

@pytest.mark.parametrize("weights", ALL_WEIGHTS)
def test_reference_equals_dijkstra(weights):
    rng = np.random.default_rng(sum(weights))
    n = 0
    for dims in SMALL_DIMS:
        for density in (0.3, 0.6, 1.0):
            S = CR.random_grid(rng, dims, density)
            seeds = seeds_for(rng, S)
            for border in (False, True):
                for max_distance in (GR.MAX_DISTANCE, 6):
                    got = GR.distance(S, weights, seeds, border, max_distance)
                    want = GR.dijkstra(S, weights, seeds, border, max_distance)
                    assert got[0].dtype == np.int32 and got[1] == want[1] and np.array_equal(got[0], want[0]), (dims, density, border, max_distance)
                    n += 1
            uncapped = GR.distance(S, weights, seeds)
            assert np.array_equal(GR.cap(uncapped[0], 6)[0], GR.dijkstra(S, weights, seeds, False, 6)[0])   # the cap cuts nothing it should not
    assert n == 84


def test_reference_on_larger_grids_and_no_seeds():
    rng = np.random.default_rng(5)
    for dims, density, weights in (((30, 20, 10), 0.35, (3, 4, 5)), ((17, 33, 9), 0.5, (1, 0, 0)), ((40, 9, 9), 0.25, (1, 1, 0))):
        S = CR.random_grid(rng, dims, density)
        seeds = seeds_for(rng, S, 2)
        for cap in (GR.MAX_DISTANCE, 6, 0):
            got, want = GR.distance(S, weights, seeds, False, cap), GR.dijkstra(S, weights, seeds, False, cap)
            assert got[1] == want[1] and np.array_equal(got[0], want[0]), (dims, weights, cap)
        none = GR.distance(S, weights)
        assert none[1] == 0 and (none[0] == -1).all()
        assert GR.distance(S, weights, [(-5, 0, 0)])[1] == 0


@pytest.mark.parametrize("weights", [(1, 0, 0), (1, 1, 1), (3, 4, 5), (2, 3, 0)])
def test_reference_equals_scipy(weights):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(11)
    for dims, density in (((20, 15, 10), 0.35), ((12, 12, 12), 0.7), ((33, 1, 17), 0.6)):
        S = CR.random_grid(rng, dims, density)
        nz, ny, nx = S.shape
        idx = np.arange(S.size).reshape(S.shape)
        rows, cols, vals = [], [], []
        for dx, dy, dz, w in GR.offsets(weights):
            me = (CR._part(nz, dz), CR._part(ny, dy), CR._part(nx, dx))
            nb = (CR._part(nz, -dz), CR._part(ny, -dy), CR._part(nx, -dx))
            both = S[me] & S[nb]
            rows.append(idx[me][both]), cols.append(idx[nb][both]), vals.append(np.full(int(both.sum()), w))
        graph = sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(S.size, S.size))
        seeds = [s for s in seeds_for(rng, S) if 0 <= s[0] < nx and 0 <= s[1] < ny and 0 <= s[2] < nz and S[s[2], s[1], s[0]]]
        if not seeds:
            continue
        d = csgraph.dijkstra(graph, indices=[idx[z, y, x] for x, y, z in seeds], min_only=True)
        want = np.where(np.isfinite(d), d, -1).astype(np.int32).reshape(S.shape)
        assert np.array_equal(GR.distance(S, weights, seeds)[0], want)


# ---- closed forms --------------------------------------------------------------------------------------------------------------

def test_closed_forms_on_a_full_box():
    S = np.ones((9, 11, 13), bool)
    z, y, x = np.meshgrid(np.arange(9), np.arange(11), np.arange(13), indexing="ij")
    r, q, p = np.sort(np.stack([x, y, z]), axis=0)
    for weights, want in (((1, 0, 0), x + y + z), ((1, 1, 1), p), ((1, 1, 0), np.maximum(p, -(-(x + y + z) // 2))), ((3, 4, 5), 3 * p + q + r)):
        got, reached, _ = GR.distance(S, weights, [(0, 0, 0)])
        assert reached == S.size and np.array_equal(got, want), weights


def test_the_door_box():
    d, reached, _ = GR.distance(GR.door_box(), (3, 4, 5), [(0, 0, 0)])
    assert (int(d[3, 4, 20]), int(d[19, 19, 39]), int(d[0, 0, 21])) == (67, 155, 83) and reached == 15601
    d, reached, _ = GR.distance(GR.door_box(False), (3, 4, 5), [(0, 0, 0)])
    assert reached == 8000 and (d[:, :, 21:] == -1).all() and int(GR.door_box(False).sum()) == 15600
    assert (d[:, :, :20] >= 0).all()


@pytest.mark.parametrize("dims", [(20, 11, 7), (64, 16, 4), (9, 3, 3)])
def test_along_a_path_one_voxel_wide_the_hops_count_its_voxels(dims):
    S = CR.serpentine(dims)
    d, reached = GR.dijkstra(S, (1, 0, 0), [(0, 0, 0)])
    assert reached == S.sum() and d.max() == S.sum() - 1 and (np.sort(d[S]) == np.arange(S.sum())).all()
    S, seed, end = GR.u_corridor()
    d, reached = GR.dijkstra(S, (1, 0, 0), [seed])
    assert reached == S.sum() and d[end[2], end[1], end[0]] == S.sum() - 1
    assert np.array_equal(GR.dijkstra(S, (1, 1, 1), [seed])[0] >= 0, S)   # (nothing of it touches diagonally: the same way at 26)
    assert GR.dijkstra(S, (1, 1, 1), [seed])[0].max() < S.sum() - 1       # ... but its corners are cut


def test_pairs_across_a_tile_boundary():
    for kind, steps in (("x", 1), ("y", 1), ("z", 1), ("xy", 2), ("xz", 2), ("yz", 2), ("xyz", 3)):
        S, a, b = GR.pair_across(kind)
        assert S.sum() == 2
        for weights in ((1, 0, 0), (1, 1, 0), (1, 1, 1), (0, 4, 0), (0, 0, 5)):
            d = GR.distance(S, weights, [a])[0]
            assert int(d[b[2], b[1], b[0]]) == (weights[steps - 1] if weights[steps - 1] else -1), (kind, weights)


# ---- the kernel's own logic on the host ------------------------------------------------------------------------------------------

HOST_GEO = r"""
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>
#define O2V_GEO_HOST
#define O2V_GEO_FN static inline
constexpr uint32_t kGeoInf = 0x7fffffffu, kGeoRowStride = 66u, kGeoLayerStride = 660u, kGeoHalo = 6600u;
%s
// The passes in the kernels' order, a "lane" at a time.  D ends as the kernels leave it before k_geo_write.  Tiles: the tiles of a
// round in an order shuffled by `shuffle`, each reading what the tiles before it have stored.  out4: rounds, tile visits,
// in-tile sweeps, the most visits of one tile.  Returns 0, or 1 if a tile was listed twice in a round.
extern "C" int geo_host(const uint64_t *bits, uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t *w, uint32_t max_distance, const uint8_t *seed,
                        int no_tiles, uint32_t shuffle, uint32_t *D, uint64_t *out4)
{
    GeoGrid g;
    g.nx = nx, g.ny = ny, g.nz = nz, g.W = (nx + 63u) / 64u, g.tiles_y = (ny + 7u) / 8u, g.tiles_z = (nz + 7u) / 8u;
    g.w[0] = w[0], g.w[1] = w[1], g.w[2] = w[2], g.max_distance = max_distance, g.words = (uint64_t) g.W * ny * nz;
    const uint32_t tiles = g.W * g.tiles_y * g.tiles_z;
    std::vector<uint32_t> list, next, visits(tiles, 0u);
    std::vector<uint8_t> flag(tiles, 0), flag_next(tiles, 0);
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    for (uint32_t z = 0; z < nz; ++z)
        for (uint32_t y = 0; y < ny; ++y)
            for (uint32_t x = 0; x < nx; ++x) {
                const uint32_t i = (z * ny + y) * nx + x;
                D[i] = seed[i] ? 0u : kGeoInf;
                if (!seed[i]) continue;
                const uint32_t see = geo_see_mask(x & 63u, y & 7u, z & 7u, g.w) | 1u << 13;   // its own tile and those that see it
                for (int k = 0; k < 27; ++k) {
                    const uint32_t X = (x >> 6) + (uint32_t) geo_dx(k), Y = (y >> 3) + (uint32_t) geo_dy(k), Z = (z >> 3) + (uint32_t) geo_dz(k);
                    if (!((see >> k) & 1u) || X >= g.W || Y >= g.tiles_y || Z >= g.tiles_z) continue;
                    const uint32_t t = (Z * g.tiles_y + Y) * g.W + X;
                    if (!flag[t]) flag[t] = 1, list.push_back(t);
                }
            }
    if (no_tiles) {
        for (bool any = true; any;) {
            any = false;
            ++out4[0];
            for (uint32_t z = 0; z < nz; ++z)
                for (uint32_t y = 0; y < ny; ++y)
                    for (uint32_t x = 0; x < nx; ++x) {
                        if (!((bits[((uint64_t) z * ny + y) * g.W + (x >> 6)] >> (x & 63u)) & 1ull)) continue;
                        const uint32_t i = (z * ny + y) * nx + x, d = geo_relax_grid(g, D, x, y, z);
                        if (d < D[i]) D[i] = d, any = true;
                    }
        }
        return 0;
    }
    std::mt19937 rng(shuffle);
    static uint32_t s_d[kGeoHalo];
    static uint64_t s_w[64];
    static uint8_t changed[4096];
    while (!list.empty()) {
        ++out4[0];
        std::shuffle(list.begin(), list.end(), rng);
        next.clear();
        for (const uint32_t tile : list) {
            const uint32_t trow = tile / g.W, tx = tile - trow * g.W, tz = trow / g.tiles_y, ty = trow - tz * g.tiles_y;
            const uint32_t x0 = tx * 64u, y0 = ty * 8u, z0 = tz * 8u;
            flag[tile] = 0;
            ++out4[1];
            out4[3] = std::max<uint64_t>(out4[3], ++visits[tile]);
            for (uint32_t row = 0; row < 64u; ++row) {
                const uint32_t y = y0 + (row & 7u), z = z0 + (row >> 3);
                s_w[row] = y < ny && z < nz ? bits[((uint64_t) z * ny + y) * g.W + tx] : 0ull;
            }
            for (uint32_t row = 0; row < 100u; ++row)
                for (uint32_t c = 0; c < 66u; ++c) {
                    const uint32_t X = x0 + c - 1u, Y = y0 + row %% 10u - 1u, Z = z0 + row / 10u - 1u;
                    s_d[row * kGeoRowStride + c] = X < nx && Y < ny && Z < nz ? D[(Z * ny + Y) * nx + X] : kGeoInf;
                }
            std::memset(changed, 0, sizeof changed);
            for (bool any = true; any;) {
                any = false;
                ++out4[2];
                for (uint32_t row = 0; row < 64u; ++row)
                    for (uint32_t x = 0; x < 64u; ++x) {
                        if (!((s_w[row] >> x) & 1ull)) continue;
                        uint32_t *const p = s_d + ((row >> 3) + 1u) * kGeoLayerStride + ((row & 7u) + 1u) * kGeoRowStride + 1u + x;
                        const uint32_t d = geo_relax(p, (int) kGeoRowStride, (int) kGeoLayerStride, g.w, g.max_distance);
                        if (d < *p) *p = d, changed[row * 64u + x] = 1, any = true;
                    }
            }
            uint32_t see = 0;
            for (uint32_t row = 0; row < 64u; ++row)
                for (uint32_t x = 0; x < 64u; ++x) {
                    if (!changed[row * 64u + x]) continue;
                    const uint32_t y = row & 7u, z = row >> 3;
                    D[((z0 + z) * ny + (y0 + y)) * nx + (x0 + x)] = s_d[(z + 1u) * kGeoLayerStride + (y + 1u) * kGeoRowStride + 1u + x];
                    see |= geo_see_mask(x, y, z, g.w);
                }
            for (int k = 0; k < 27; ++k) {
                if (!((see >> k) & 1u)) continue;
                const uint32_t X = tx + (uint32_t) geo_dx(k), Y = ty + (uint32_t) geo_dy(k), Z = tz + (uint32_t) geo_dz(k);
                if (X >= g.W || Y >= g.tiles_y || Z >= g.tiles_z) continue;
                const uint32_t t = (Z * g.tiles_y + Y) * g.W + X;
                if (!flag_next[t]) flag_next[t] = 1, next.push_back(t);
            }
        }
        for (const uint32_t t : next)
            if (flag[t]) return 1;
        list.swap(next);
        flag.swap(flag_next);
    }
    return 0;
}

extern "C" void geo_host_trace(const int32_t *dist, const uint64_t *strides, const uint32_t *dims, const uint32_t *w, const int32_t *targets, uint64_t n,
                               uint32_t max_len, int32_t *paths, int32_t *lengths)
{
    for (uint64_t i = 0; i < n; ++i)
        lengths[i] = geo_trace(dist, strides[0], strides[1], strides[2], dims, w, targets[3u * i], targets[3u * i + 1u], targets[3u * i + 2u], max_len,
                               paths + i * 3u * max_len);
}
"""


@pytest.fixture(scope="module")
def host_geo(tmp_path_factory):
    """build(defines) -> a library with geo_host and geo_host_trace: the part of o2v_dev_k20_geodesic.hpp between "the relaxation"
    and "kernels", compiled for the host behind the plain part of o2v_dev_bits.hpp."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    text = open(K20).read()
    part = text[text.index("// ---- the relaxation, the tiles that see a voxel, the trace step"):text.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_geo")
    built = {}

    def build(defines=()):
        if defines not in built:
            name = "geo_%d" % len(built)
            (tmp / (name + ".cpp")).write_text(HOST_GEO % (bits_host.plain_part() + part))
            subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                           [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
            built[defines] = hip.C.CDLL(str(tmp / (name + ".so")))
        return built[defines]
    return build


def host_distance(L, S, weights, seeds=(), border=False, max_distance=GR.MAX_DISTANCE, no_tiles=False, shuffle=0):
    """(dist, reached, (rounds, visits, sweeps, most visits of a tile)) of the host build."""
    C = hip.C
    S = np.asarray(S, bool)
    nz, ny, nx = S.shape
    bits = words64(S)
    seed = np.ascontiguousarray(GR.seed_mask(S, seeds, border).astype(np.uint8))
    D = np.full(S.size, 0xFFFFFFFF, np.uint32)
    w = np.asarray(weights, np.uint32)
    out4 = np.zeros(4, np.uint64)
    rc = L.geo_host(C.c_void_p(bits.ctypes.data), nx, ny, nz, C.c_void_p(w.ctypes.data), C.c_uint32(max_distance), C.c_void_p(seed.ctypes.data),
                    int(no_tiles), shuffle, C.c_void_p(D.ctypes.data), C.c_void_p(out4.ctypes.data))
    assert rc == 0, "a tile was in a round's list twice"
    D = D.reshape(S.shape)
    assert (D[~S] == GR.INF).all()                                # nothing outside S is ever reached
    assert ((D == GR.INF) | (D <= max_distance)).all()            # nothing above the cap is ever stored
    dist = np.where(D == GR.INF, -1, D.astype(np.int64)).astype(np.int32)
    return dist, int((dist >= 0).sum()), tuple(int(v) for v in out4)


def host_cases():
    rng = np.random.default_rng(20)
    for dims in ((70, 50, 40), (64, 8, 8), (65, 9, 9), (1, 30, 30), (130, 1, 17), (200, 3, 1), (63, 17, 25)):
        for density in ((0.3, 0.95) if dims == (70, 50, 40) else (0.3, 0.6, 0.95)):
            S = CR.random_grid(rng, dims, density)
            yield f"random {dims} {density}", S, seeds_for(rng, S), False
    yield "door", GR.door_box(), [(0, 0, 0)], False
    yield "closed door", GR.door_box(False), [(0, 0, 0)], False
    yield "serpentine", CR.serpentine((70, 21, 19)), [(0, 0, 0)], False
    yield "u corridor", GR.u_corridor()[0], [GR.u_corridor()[1]], False
    yield "border", ~CR.random_grid(rng, (90, 30, 20), 0.5), [], True
    yield "full", np.ones((9, 17, 129), bool), [(128, 16, 8), (0, 0, 0)], True
    yield "empty", np.zeros((9, 17, 129), bool), [(3, 3, 3)], True
    for kind in ("x", "y", "z", "xy", "xz", "yz", "xyz"):
        S, a, _ = GR.pair_across(kind)
        yield "pair " + kind, S, [a], False


@pytest.mark.parametrize("no_tiles", [False, True])
def test_the_kernels_passes_on_the_host_equal_the_reference(host_geo, no_tiles):
    L = host_geo()
    n = 0
    for name, S, seeds, border in host_cases():
        for weights in ((1, 0, 0), (1, 1, 1), (3, 4, 5), (3, 4, 0), (7, 1, 1)):
            if no_tiles and weights in ((3, 4, 0), (7, 1, 1)) and "random" in name:
                continue
            thin = name in ("serpentine", "u corridor")
            want = (GR.dijkstra if thin else GR.distance)(S, weights, seeds, border)
            for shuffle in ((0,) if no_tiles else (1, 2)):
                got = host_distance(L, S, weights, seeds, border, no_tiles=no_tiles, shuffle=shuffle)
                assert got[1] == want[1] and np.array_equal(got[0], want[0]), (name, weights, no_tiles, shuffle)
            for cap in ((0, 6, 100) if weights in ((1, 0, 0), (3, 4, 5)) else ()):
                got = host_distance(L, S, weights, seeds, border, cap, no_tiles, 3)
                capped = GR.cap(want[0], cap)
                assert got[1] == capped[1] and np.array_equal(got[0], capped[0]), (name, weights, no_tiles, cap)
            n += 1
    assert n > 100


def test_a_tile_that_has_converged_is_visited_again(host_geo):
    L = host_geo()
    S, seed, end = GR.u_corridor()
    for shuffle in (1, 2, 3):
        dist, reached, (rounds, visits, sweeps, most) = host_distance(L, S, (1, 0, 0), [seed], shuffle=shuffle)
        assert reached == S.sum() and dist[end[2], end[1], end[0]] == S.sum() - 1
        assert most >= 2 and visits > rounds >= 6 and sweeps >= visits     # the way passes 3 tiles out, 3 back, and re-enters the first


def test_the_see_mask(host_geo):
    """The mask against its definition, through the tile pass: a voxel that decreases on a rim wakes exactly the neighbour tiles
    that hold it in their halo and have a step to reach it by - fewer and the pairs across a boundary would fail above; here: not
    more tiles than the weights allow.  A seed wakes them from the start: it never decreases."""
    L = host_geo()
    S = np.zeros((24, 24, 192), bool)
    S[8, 8, 64] = True                                    # the first voxel of the middle tile: on its -x, -y and -z sides
    for weights, woken in (((1, 0, 0), 3), ((1, 1, 0), 6), ((1, 1, 1), 7), ((0, 0, 5), 7), ((0, 4, 0), 6)):
        _, reached, (rounds, visits, _, _) = host_distance(L, S, weights, [(64, 8, 8)])
        assert reached == 1 and rounds == 1 and visits == 1 + woken, (weights, visits)   # the seed's tile and those that see the seed
        S2 = S.copy()
        S2[8, 8, 65] = True                                          # (65, 8, 8) decreases in round 1: on the -y and -z sides only
        _, reached, (rounds, visits, _, _) = host_distance(L, S2, weights, [(64, 8, 8)])
        if weights[0]:
            assert reached == 2 and rounds == 2 and visits == 1 + woken + {3: 2, 6: 3, 7: 3}[woken], (weights, visits)
        else:
            assert reached == 1 and rounds == 1 and visits == 1 + woken


@pytest.mark.parametrize("no_tiles", [False, True])
def test_a_changed_rule_is_caught(host_geo, no_tiles):
    """DESIGN.md section 23, mutation: the offset (+1, +1, -1) left out - wrong only where corner steps have a weight."""
    L = host_geo(("O2V_GEO_MUTATE_DROP_CORNER",))
    rng = np.random.default_rng(8)
    S = CR.random_grid(rng, (70, 50, 40), 0.3)
    seeds = seeds_for(rng, S)
    for weights, same in (((3, 4, 5), False), ((3, 4, 0), True), ((1, 1, 1), False), ((1, 0, 0), True)):
        got = host_distance(L, S, weights, seeds, no_tiles=no_tiles)[0]
        assert np.array_equal(got, GR.distance(S, weights, seeds)[0]) == same, (weights, no_tiles)


def host_paths(L, dist, weights, targets, max_len, fill=-1):
    C = hip.C
    targets = np.ascontiguousarray(np.asarray(targets, np.int64).reshape(-1, 3).clip(-1, 2 ** 31 - 1).astype(np.int32))
    strides = np.array([dist.strides[2] // 4, dist.strides[1] // 4, dist.strides[0] // 4], np.uint64)
    dims, w = np.array(dist.shape[::-1], np.uint32), np.asarray(weights, np.uint32)
    paths = np.full((len(targets), max_len, 3), fill, np.int32)
    lengths = np.full(len(targets), -9, np.int32)
    L.geo_host_trace(C.c_void_p(dist.ctypes.data), C.c_void_p(strides.ctypes.data), C.c_void_p(dims.ctypes.data), C.c_void_p(w.ctypes.data),
                     C.c_void_p(targets.ctypes.data), len(targets), max_len, C.c_void_p(paths.ctypes.data), C.c_void_p(lengths.ctypes.data))
    return paths, lengths


def check_paths(dist, weights, targets, paths, lengths):
    """What a path is: from its target to a voxel of distance 0, each step one that has a weight, the weights summing to the
    target's distance."""
    for t, p, n in zip(targets, paths, lengths):
        if n < 0:
            continue
        p = p[:n]
        assert tuple(p[0]) == tuple(t) and dist[p[-1][2], p[-1][1], p[-1][0]] == 0
        steps = np.abs(np.diff(p.astype(np.int64), axis=0))
        assert (steps.max(axis=1) == 1).all() if n > 1 else True
        kinds = steps.sum(axis=1)
        assert all(weights[k - 1] for k in kinds) and sum(weights[k - 1] for k in kinds) == dist[t[2], t[1], t[0]]


def test_the_trace_body_equals_the_scalar_trace(host_geo):
    L = host_geo()
    rng = np.random.default_rng(4)
    for S, seeds, weights in ((GR.door_box(), [(0, 0, 0)], (3, 4, 5)), (CR.serpentine((20, 11, 7)), [(0, 0, 0)], (1, 0, 0)),
                              (CR.random_grid(rng, (30, 20, 12), 0.4), None, (3, 4, 5)), (CR.random_grid(rng, (30, 20, 12), 0.5), None, (2, 3, 0))):
        seeds = seeds_for(rng, S) if seeds is None else seeds
        dist = GR.distance(S, weights, seeds)[0]
        nz, ny, nx = S.shape
        targets = np.concatenate([rng.integers(0, (nx, ny, nz), (60, 3)), [[-1, 0, 0], [nx, 0, 0], [0, 0, nz], [2 ** 31 - 1, 1, 1]]])
        L_all = GR.default_max_len(dist, weights, targets)
        want = GR.paths(dist, weights, targets, L_all)
        got = host_paths(L, dist, weights, targets, L_all)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]) and (want[1] > 1).any() and (want[1] == -1).any()
        assert want[1].max() <= L_all
        check_paths(dist, weights, targets, got[0], got[1])
        short = host_paths(L, dist, weights, targets, 3, fill=-7)            # the true length, the row's tail left alone
        assert np.array_equal(short[1], want[1]) and np.array_equal(short[0], np.where(np.arange(3)[None, :, None] < want[1][:, None, None], want[0][:, :3], -7))
        none = host_paths(L, dist, weights, targets, 0)
        assert np.array_equal(none[1], want[1])
        # a strided grid: the same walk
        wide = np.full((nz, ny, 2 * nx), -1, np.int32)
        wide[:, :, ::2] = dist
        assert all(np.array_equal(a, b) for a, b in zip(host_paths(L, wide[:, :, ::2], weights, targets, L_all), want))
    # the wrong weights: -2 (and the scalar trace says the same)
    dist = GR.distance(GR.door_box(), (3, 4, 5), [(0, 0, 0)])[0]
    targets = [(39, 19, 19), (0, 0, 0), (20, 0, 0)]
    got, want = host_paths(L, dist, (1, 1, 1), targets, 8), GR.paths(dist, (1, 1, 1), targets, 8)
    assert got[1].tolist() == [-2, 1, -1] and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


# ---- the torch layer against a stub ----------------------------------------------------------------------------------------------

class GeoStub(StubVoxelizer):
    """Computes with the reference, on the tensors' own memory (CPU)."""

    def geodesic_dense(self, grid_ptr, fmt, strides, dims, level, weights, flags, seeds_ptr, n_seeds, max_distance, dist_ptr, dist_strides):
        self.calls.append(("geodesic", grid_ptr, fmt, tuple(strides), tuple(dims), level, tuple(weights), flags, seeds_ptr, n_seeds, max_distance, dist_ptr,
                           tuple(dist_strides)))
        C = hip.C
        assert fmt == hip.GRID_U8
        nx, ny, nz = dims
        span = sum((d - 1) * s for d, s in zip(dims, strides)) + 1
        raw = np.ctypeslib.as_array(C.cast(grid_ptr, C.POINTER(C.c_uint8)), (span,))
        S = np.lib.stride_tricks.as_strided(raw, (nz, ny, nx), (strides[2], strides[1], strides[0])) != 0
        if flags & hip.CC_INVERT:
            S = ~S
        seeds = np.ctypeslib.as_array(C.cast(seeds_ptr, C.POINTER(C.c_int32)), (n_seeds, 3)) if n_seeds else ()
        d, reached, _ = GR.distance(S, weights, seeds, bool(flags & hip.CC_SEED_BORDER), max_distance)
        span = sum((d_ - 1) * s for d_, s in zip(dims, dist_strides)) + 1
        out = np.ctypeslib.as_array(C.cast(dist_ptr, C.POINTER(C.c_int32)), (span,))
        np.lib.stride_tricks.as_strided(out, (nz, ny, nx), tuple(4 * s for s in (dist_strides[2], dist_strides[1], dist_strides[0])))[...] = d
        return reached

    def geodesic_paths(self, dist_ptr, dist_strides, dims, weights, targets_ptr, n_targets, max_len, paths_ptr, lengths_ptr):
        self.calls.append(("paths", dist_ptr, tuple(dist_strides), tuple(dims), tuple(weights), targets_ptr, n_targets, max_len, paths_ptr, lengths_ptr))
        C = hip.C
        nx, ny, nz = dims
        span = sum((d - 1) * s for d, s in zip(dims, dist_strides)) + 1
        raw = np.ctypeslib.as_array(C.cast(dist_ptr, C.POINTER(C.c_int32)), (span,))
        dist = np.lib.stride_tricks.as_strided(raw, (nz, ny, nx), tuple(4 * s for s in (dist_strides[2], dist_strides[1], dist_strides[0])))
        targets = np.ctypeslib.as_array(C.cast(targets_ptr, C.POINTER(C.c_int32)), (n_targets, 3))
        lengths = np.ctypeslib.as_array(C.cast(lengths_ptr, C.POINTER(C.c_int32)), (n_targets,))
        for i, t in enumerate(targets):
            p, lengths[i] = GR.trace(dist, weights, t, max_len)
            if p:
                np.ctypeslib.as_array(C.cast(paths_ptr, C.POINTER(C.c_int32)), (n_targets, max_len, 3))[i, :len(p)] = p


@pytest.mark.parametrize("metric, connectivity, weights", [(m, c, w) for (m, c), w in GR.WEIGHTS.items()])
def test_the_weights_of_each_metric_and_connectivity(metric, connectivity, weights):
    assert dense.CHAMFER_UNIT == 3 and weights == {"steps": (1, 1, 1), "chamfer": (3, 4, 5)}[metric][:{6: 1, 18: 2, 26: 3}[connectivity]] + \
        (0,) * {6: 2, 18: 1, 26: 0}[connectivity]
    dv = GeoStub()
    grid = torch.from_numpy(GR.door_box())
    dist = dense.geodesic_distance(dv, grid, [(0, 0, 0)], metric=metric, connectivity=connectivity)
    assert dv.calls[-1][6] == weights and dist.dtype == torch.int32 and dist.is_contiguous()
    assert np.array_equal(dist.numpy(), GR.distance(GR.door_box(), weights, [(0, 0, 0)])[0])
    paths, lengths = dense.shortest_paths(dv, dist, [(39, 19, 19), (20, 0, 0)], metric=metric, connectivity=connectivity)
    assert dv.calls[-1][0] == "paths" and dv.calls[-1][4] == weights
    L = GR.default_max_len(dist.numpy(), weights, [(39, 19, 19), (20, 0, 0)])
    want = GR.paths(dist.numpy(), weights, [(39, 19, 19), (20, 0, 0)], L)
    assert tuple(paths.shape) == (2, L, 3) and paths.dtype == lengths.dtype == torch.int32
    assert np.array_equal(paths.numpy(), want[0]) and np.array_equal(lengths.numpy(), want[1]) and lengths[1] == -1 and lengths[0] > 20


def test_geodesic_distance_arguments():
    dv = GeoStub()
    S = GR.door_box()
    grid = torch.from_numpy(S.astype(np.uint8))
    dist = dense.geodesic_distance(dv, grid, torch.tensor([[0, 0, 0], [2 ** 40, 0, 0]]), weights=(2, 3, 0), max_distance=50)
    c = dv.calls[-1]
    assert c[2:8] == (hip.GRID_U8, (1, 40, 800), (40, 20, 20), 0.0, (2, 3, 0), 0) and c[9:] == (2, 50, dist.data_ptr(), (1, 40, 800))
    assert np.array_equal(dist.numpy(), GR.distance(S, (2, 3, 0), [(0, 0, 0)], False, 50)[0]) and (dist.numpy() == -1).any()
    # the defaults: chamfer at 26, no cap; background and border; no seeds at all: the pointer is not passed
    drain = dense.geodesic_distance(dv, grid, background=True, border=True)
    c = dv.calls[-1]
    assert c[6:11] == ((3, 4, 5), hip.CC_INVERT | hip.CC_SEED_BORDER, None, 0, hip.GEO_MAX_DISTANCE) and hip.GEO_MAX_DISTANCE == 2 ** 31 - 2
    assert np.array_equal(drain.numpy(), GR.distance(~S, (3, 4, 5), (), True)[0])
    dense.geodesic_distance(dv, grid, torch.zeros((0, 3), dtype=torch.int32))
    assert dv.calls[-1][8] is None and dv.calls[-1][9] == 0
    dense.geodesic_distance(dv, grid, [(1, 1, 1)], max_distance=0)
    assert dv.calls[-1][10] == 0
    dense.geodesic_distance(dv, grid, [(1, 1, 1)], max_distance=2 ** 31 - 2, weights=np.array([65535, 0, 0]))
    assert dv.calls[-1][6] == (65535, 0, 0)
    # out= is written as it is
    wide = torch.full((20, 20, 80), -7, dtype=torch.int32)
    got = dense.geodesic_distance(dv, grid, [(0, 0, 0)], out=wide[:, :, ::2])
    assert got.data_ptr() == wide.data_ptr() and dv.calls[-1][12] == (2, 80, 1600) and bool((wide[:, :, 1::2] == -7).all())
    assert np.array_equal(wide[:, :, ::2].numpy(), GR.distance(S, (3, 4, 5), [(0, 0, 0)])[0])
    # a float grid with a level
    field = torch.where(torch.from_numpy(S), -1.0, 1.0)

    class Any(GeoStub):
        def geodesic_dense(self, *args):
            self.calls.append(("geodesic",) + args)
            return 0
    dv2 = Any()
    dense.geodesic_distance(dv2, field, level=0.0, metric="steps", connectivity=6)
    assert dv2.calls[-1][2] == hip.GRID_F32_BELOW and dv2.calls[-1][6] == (1, 0, 0)
    for text in ("CHAMFER_UNIT", "section 23", "not reached"):
        assert text in " ".join(dense.geodesic_distance.__doc__.split())
    assert "section 23" in dense.shortest_paths.__doc__


def test_shortest_paths_arguments():
    dv = GeoStub()
    S = GR.door_box()
    dist = dense.geodesic_distance(dv, torch.from_numpy(S), [(0, 0, 0)])
    targets = torch.tensor([[39, 19, 19], [-1, 0, 0], [2 ** 40, 0, 0], [20, 0, 0], [0, 0, 0]], dtype=torch.int64)
    paths, lengths = dense.shortest_paths(dv, dist, targets)
    assert dv.calls[-1][7] == 155 // 3 + 1 and tuple(paths.shape) == (5, 52, 3) and lengths.tolist()[1:] == [-1, -1, -1, 1]
    assert paths[4, 0].tolist() == [0, 0, 0] and bool((paths[4, 1:] == -1).all()) and bool((paths[1:4] == -1).all())
    paths, lengths = dense.shortest_paths(dv, dist, targets, max_len=4)
    assert tuple(paths.shape) == (5, 4, 3) and lengths[0] > 4 and dv.calls[-1][7] == 4 and bool((paths[0] >= 0).all())
    paths, lengths = dense.shortest_paths(dv, dist, [(39, 19, 19)], metric="steps")
    assert lengths.tolist() == [-2]
    n_calls = len(dv.calls)
    paths, lengths = dense.shortest_paths(dv, dist, torch.zeros((0, 3), dtype=torch.int32))
    assert tuple(paths.shape) == (0, 1, 3) and tuple(lengths.shape) == (0,) and len(dv.calls) == n_calls      # nothing to walk
    paths, lengths = dense.shortest_paths(dv, dist, [(1, 1, 1)], max_len=0)
    assert tuple(paths.shape) == (1, 0, 3) and lengths.tolist() == [2] and dv.calls[-1][8] is None
    view = torch.full((20, 20, 80), -1, dtype=torch.int32)
    view[:, :, ::2] = dist
    got = dense.shortest_paths(dv, view[:, :, ::2], targets)
    assert dv.calls[-1][2] == (2, 80, 1600) and torch.equal(got[0], dense.shortest_paths(dv, dist, targets)[0])


U8 = torch.zeros((4, 4, 4), dtype=torch.uint8)
I32 = torch.zeros((4, 4, 4), dtype=torch.int32)


@pytest.mark.parametrize("kw, exc", [
    (dict(grid=torch.zeros((4, 4, 4), dtype=torch.float64)), TypeError), (dict(grid=torch.zeros((4, 4))), ValueError), (dict(grid=np.zeros((4, 4, 4), np.uint8)), ValueError),
    (dict(grid=torch.zeros((4, 4, 4))), ValueError), (dict(grid=torch.zeros((4, 4, 4)), level=float("nan")), ValueError), (dict(level=0.0), ValueError),
    (dict(grid=torch.zeros((4, 4, 8), dtype=torch.int32)[:, :, ::2]), ValueError), (dict(grid=torch.zeros((4, 0, 4), dtype=torch.uint8)), ValueError),
    (dict(grid=torch.zeros((4, 4, 4), dtype=torch.uint8, device="meta")), ValueError),
    (dict(grid=torch.zeros((1, 1, 1), dtype=torch.uint8).expand(1, 1, 65537)), ValueError),
    (dict(grid=torch.zeros((1, 1, 1), dtype=torch.uint8).expand(2048, 1024, 1024)), ValueError),
    (dict(connectivity=8), ValueError), (dict(connectivity=True), ValueError), (dict(connectivity="6"), ValueError),
    (dict(metric="euclidean"), ValueError), (dict(metric=None), ValueError),
    (dict(weights=(1, 0)), ValueError), (dict(weights=(0, 0, 0)), ValueError), (dict(weights=(65536, 0, 0)), ValueError), (dict(weights=(-1, 1, 1)), ValueError),
    (dict(weights=(1.0, 0, 0)), ValueError), (dict(weights=(True, 0, 0)), ValueError), (dict(weights=3), ValueError), (dict(weights="345"), ValueError),
    (dict(max_distance=-1), ValueError), (dict(max_distance=2 ** 31 - 1), ValueError), (dict(max_distance=6.0), ValueError), (dict(max_distance=True), ValueError),
    (dict(seeds=torch.zeros((2, 3))), TypeError), (dict(seeds=torch.zeros((2, 4), dtype=torch.int32)), ValueError),
    (dict(seeds=torch.zeros((2, 3), dtype=torch.int32, device="meta")), ValueError),
    (dict(out=torch.zeros((4, 4, 4), dtype=torch.int64)), TypeError), (dict(out=torch.zeros((4, 4, 5), dtype=torch.int32)), ValueError),
    (dict(out=torch.zeros((4, 4, 4), dtype=torch.int32, device="meta")), ValueError), (dict(out=np.zeros((4, 4, 4), np.int32)), ValueError),
])
def test_geodesic_distance_rejects(kw, exc):
    dv = GeoStub()
    args = dict(grid=U8)
    args.update(kw)
    with pytest.raises(exc):
        dense.geodesic_distance(dv, args.pop("grid"), **args)
    assert not dv.calls


@pytest.mark.parametrize("kw, exc", [
    (dict(dist=torch.zeros((4, 4, 4), dtype=torch.int64)), TypeError), (dict(dist=torch.zeros((4, 4, 4))), TypeError), (dict(dist=torch.zeros((4, 4), dtype=torch.int32)), ValueError),
    (dict(dist=np.zeros((4, 4, 4), np.int32)), ValueError), (dict(dist=torch.zeros((4, 4, 4), dtype=torch.int32, device="meta")), ValueError),
    (dict(dist=torch.zeros((4, 0, 4), dtype=torch.int32)), ValueError), (dict(dist=torch.zeros((1, 1, 1), dtype=torch.int32).expand(1, 1, 65537)), ValueError),
    (dict(targets=None), ValueError), (dict(targets=torch.zeros((2, 3))), TypeError), (dict(targets=torch.zeros((2, 2), dtype=torch.int32)), ValueError),
    (dict(targets=torch.zeros((2, 3), dtype=torch.int32, device="meta")), ValueError),
    (dict(connectivity=7), ValueError), (dict(metric="hops"), ValueError), (dict(weights=(0, 0, 0)), ValueError), (dict(weights=(1, 2, 3, 4)), ValueError),
    (dict(max_len=-1), ValueError), (dict(max_len=2 ** 31), ValueError), (dict(max_len=1.5), ValueError), (dict(max_len=True), ValueError),
])
def test_shortest_paths_rejects(kw, exc):
    dv = GeoStub()
    args = dict(dist=I32, targets=[(0, 0, 0)])
    args.update(kw)
    with pytest.raises(exc):
        dense.shortest_paths(dv, args.pop("dist"), args.pop("targets"), **args)
    assert not dv.calls


def test_refused_when_the_library_came_first(monkeypatch):
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: False)
    with pytest.raises(RuntimeError, match="before torch"):
        dense.geodesic_distance(GeoStub(), U8)
    with pytest.raises(RuntimeError, match="before torch"):
        dense.shortest_paths(GeoStub(), I32, [(0, 0, 0)])


def test_a_wait_comes_before_the_library(monkeypatch):
    """As tests/test_host_dense.py holds it for the other functions: the first library call that takes a tensor comes behind a
    wait on the voxelizer's own device."""
    for call, name in ((lambda dv: dense.geodesic_distance(dv, U8 + 1, [(0, 0, 0)]), "geodesic"), (lambda dv: dense.shortest_paths(dv, I32, [(1, 1, 1)]), "paths")):
        dv = GeoStub()
        own = torch.device("cpu")
        monkeypatch.setattr(dense, "_device", lambda v: own)
        monkeypatch.setattr(dense, "_sync", lambda device: dv.calls.append(("sync", device)))
        call(dv)
        names = [c[0] for c in dv.calls]
        assert name in names and "sync" in names[:names.index(name)] and all(c[1] is own for c in dv.calls if c[0] == "sync")


# ---- the scratch formula and the code object -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(1, 1, 1), (64, 8, 8), (65, 9, 9), (1024, 1024, 1024), (65536, 1, 7), (1000, 999, 17)])
def test_scratch_bytes_formula(dims):
    words, voxels = -(-dims[0] // 64) * dims[1] * dims[2], math.prod(dims)
    tiles = -(-dims[0] // 64) * -(-dims[1] // 8) * -(-dims[2] // 8)
    want = 8 * words + 16 * tiles + 64
    assert hip.geodesic_scratch_bytes(dims) == hip.geodesic_scratch_bytes(dims, hip.GEO_SCRATCH_CONTIGUOUS) == want
    assert hip.geodesic_scratch_bytes(dims, hip.GEO_SCRATCH_STRIDED) == want + 4 * voxels
    assert hip.geodesic_scratch_bytes((4, 0, 4)) == 0 and hip.geodesic_scratch_bytes(dims, 2) == 0
    assert hip.DeviceVoxelizer.geodesic_scratch_bytes(None, dims) == want


K20_KERNELS = ["k_geo_seed_listE", "k_geo_seed_borderE", "k_geo_tilesILb0EE", "k_geo_tilesILb1EE", "k_geo_sweepE", "k_geo_writeE", "k_geo_traceE"]
# the distances with their halo, the row words, the mask of tiles to wake (and its padding), and the 256 bytes that the
# workgroup reduction of __syncthreads_or takes: DESIGN.md section 23
TILE_LDS = 66 * 10 * 10 * 4 + 64 * 8 + 8 + 256


@pytest.mark.parametrize("kernel", K20_KERNELS)
def test_k20_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    name, body = m.group(1), m.group(2)
    scratch = re.findall(r"; ScratchSize: (\d+)", device_asm[m.end():m.end() + 4000])
    assert scratch and scratch[0] == "0", scratch[:1]
    assert "scratch_" not in body
    entry = [e for e in device_asm[device_asm.index("amdhsa.kernels:"):].split("\n  - ") if re.search(r"\.name: +" + re.escape(name) + r"\n", e)]
    assert len(entry) == 1
    lds = int(re.search(r"\.group_segment_fixed_size: +(\d+)", entry[0]).group(1))
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
    atomics = set(re.findall(r"^\s*(\S*atomic\S*)", body, re.M))
    if "k_geo_tiles" in kernel:
        assert lds == TILE_LDS and 6 * lds <= 160 * 1024 < 7 * lds        # six workgroups in a CU's LDS
        assert int(re.search(r"\.vgpr_count: +(\d+)", entry[0]).group(1)) <= 80   # ... and six waves a SIMD: registers come in eights, 88 - 96 give five
        assert "ds_read" in body and "global_atomic_swap" in atomics       # the relaxation reads LDS; the flag is an exchange
        assert not any("min" in a for a in atomics), atomics               # no atomic min: a voxel has one writer
    elif kernel == "k_geo_sweepE":
        assert any(re.fullmatch(r"global_atomic_\w*min\w*", a) for a in atomics), atomics
    elif kernel in ("k_geo_traceE",):
        assert not atomics and lds == 0


def test_the_new_source_has_no_waiting_loop():
    """No kernel of K20 waits for another workgroup, lane or flag: nothing in the source polls or sleeps."""
    text = open(K20).read()
    kernels = text[text.index("// ---- kernels"):]
    assert "s_sleep" not in kernels and "while (" not in kernels and "__builtin_amdgcn_s_sleep" not in kernels
