"""Seeded watershed without a GPU: the numpy reference (tests/grow_ref.py) against a heap Dijkstra on the
joint key that restates the header's words; closed forms; the statements the header makes about level, ticks and labels; the
kernels' own lane bodies compiled for the host and run tile by tile in a shuffled order and as whole-grid sweeps, with two
deliberate changes that must be caught; the torch layer against a stub; the scratch formula; the K28 kernels in the gfx950 code
object."""
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
from tests import grow_ref as WR

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401

K20 = os.path.join(SRC, "o2v_dev_k20_geodesic.hpp")
K28 = os.path.join(SRC, "o2v_dev_k28_grow.hpp")
ALL_WEIGHTS = [(1, 0, 0), (1, 1, 0), (1, 1, 1), (3, 4, 5), (3, 4, 0), (7, 1, 1), (65535, 0, 0)]
INF, NO_LABEL = 2 ** 31 - 1, 2 ** 32 - 1


def same(a, b):
    return a[3] == b[3] and all(x.dtype == np.int32 and np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


def row(h, markers, weights=(1, 0, 0)):
    """The reference on a 1 x 1 x n row: (labels, level, ticks) as lists."""
    H = np.array(h, np.int32).reshape(1, 1, -1)
    M = np.zeros_like(H)
    for x, label in markers:
        M[0, 0, x] = label
    return [a.ravel().tolist() for a in WR.grow(H, M, weights)[:3]], H, M


# ---- the reference against the definition --------------------------------------------------------------------------------------

def lowered_cap(H, M, weights, cap):
    """The three phases with the ticks saturating at `cap` (finish() holds the real cap only)."""
    Q = WR.level(H, M, weights)
    T = WR.ticks(H, M, weights, Q, cap)
    L = WR.labels(H, M, weights, Q, T, cap)
    return np.where(Q > 0, L, 0), Q, np.where(Q > 0, T, -1)


@pytest.mark.parametrize("weights", ALL_WEIGHTS)
def test_reference_equals_dijkstra(weights):
    rng = np.random.default_rng(sum(weights))
    n = saturated = 0
    for i in range(36):
        dims = (1, 1, 1) if i == 0 else tuple(int(v) for v in rng.integers(1, 7, 3))
        H, M = WR.random_case(rng, dims, (1, 3, 8)[i % 3], int(rng.integers(0, 5)), (0.5, 0.8, 1.0)[i // 3 % 3])
        if i % 9 == 4:
            M[...] = 0                                          # no marker
        if i % 9 == 5:
            M = np.where(H > 0, 0, 3).astype(np.int32)          # every marker outside S
        if i % 9 == 6:
            M = (1 + np.arange(H.size, dtype=np.int32)[::-1]).reshape(H.shape)      # every voxel a marker
        got, want = WR.grow(H, M, weights), WR.dijkstra(H, M, weights)
        assert same(got, want), (dims, weights, i)
        assert same(WR.grow_frontier(H, M, weights), want), (dims, weights, i)
        if i % 9 in (4, 5):
            assert got[3] == 0 and not got[0].any() and (got[2] == -1).all()
        if i % 9 == 6:
            assert np.array_equal(got[0], np.where(H > 0, M, 0)) and np.array_equal(got[1], np.maximum(H, 0)) and (got[2][H > 0] == 0).all()
        # the cap lowered to 9, so that saturation is exercised: the phases against the Dijkstra with that cap
        low, heap = lowered_cap(H, M, weights, 9), WR.dijkstra(H, M, weights, 9)
        assert all(np.array_equal(a, b) for a, b in zip(low, heap[:3])), (dims, weights, i, "cap 9")
        saturated += int((low[2] == 9).sum())
        n += 1
    assert n == 36 and (saturated > 0 or weights in ((1, 0, 0), (1, 1, 0), (1, 1, 1)))      # 7 x 36 = 252 grids in all


def test_closed_forms():
    """The three rows of the header."""
    got, _, _ = row([3] * 9, [(0, 2), (8, 1)])
    assert got == [[2, 2, 2, 2, 1, 1, 1, 1, 1], [3] * 9, [0, 1, 2, 3, 4, 3, 2, 1, 0]]
    h = [5, 4, 3, 2, 1, 2, 3, 4, 5, 4, 3]
    got, _, _ = row(h, [(0, 1), (8, 2)])
    assert got == [[1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2], h, [0] * 11]     # the valley is reached by both at (1, 0): the smaller label takes it
    got, _, _ = row(h, [(0, 1)])
    assert got == [[1] * 11, [5, 4, 3, 2, 1, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6]]


@pytest.mark.parametrize("weights", [(1, 0, 0), (1, 1, 1), (3, 4, 5), (3, 4, 0)])
def test_on_a_flat_relief_ticks_are_the_geodesic_distance(weights):
    rng = np.random.default_rng(3)
    for dims, density in (((20, 15, 10), 0.5), ((33, 1, 17), 0.7), ((12, 12, 12), 1.0)):
        S = CR.random_grid(rng, dims, density)
        z, y, x = np.nonzero(S)
        pick = rng.integers(0, len(x), 5)
        seeds = [(int(x[i]), int(y[i]), int(z[i])) for i in pick]
        M = np.zeros(S.shape, np.int32)
        for k, (sx, sy, sz) in enumerate(seeds):
            M[sz, sy, sx] = 5 - k if M[sz, sy, sx] == 0 else M[sz, sy, sx]
        labels, level, ticks, reached = WR.grow(S.astype(np.int32) * 4, M, weights)
        dist, n, _ = GR.distance(S, weights, seeds)
        assert np.array_equal(ticks, dist) and reached == n and np.array_equal(level, np.where(dist >= 0, 4, 0))
        # labels: the nearest marker, the smallest label on a tie
        per = {}
        for sx, sy, sz in seeds:
            per[int(M[sz, sy, sx])] = GR.distance(S, weights, [(sx, sy, sz)])[0].astype(np.int64)
        order = sorted(per)
        stack = np.stack([np.where(per[k] < 0, WR.BIG, per[k]) for k in order])
        nearest = np.array(order)[np.argmin(stack, axis=0)]              # (argmin: the first, so the smallest label, on a tie)
        assert np.array_equal(labels, np.where(dist >= 0, nearest, 0))


@pytest.mark.parametrize("connectivity, weights", [(6, (1, 0, 0)), (18, (2, 3, 0)), (26, (3, 4, 5))])
def test_the_level_is_a_statement_about_thresholds(connectivity, weights):
    """Q(v) >= t exactly if the component of {H >= t} that holds v holds a seed s with H[s] >= t."""
    rng = np.random.default_rng(connectivity)
    for dims in ((12, 9, 7), (20, 1, 11)):
        H, M = WR.random_case(rng, dims, 6, 4, 0.8)
        Q = WR.grow(H, M, weights)[1]
        for t in range(1, 8):
            comp, n = CR.label(H >= t, connectivity)
            seeded = np.zeros(n + 1, bool)
            seeded[comp[(M > 0) & (H >= t)]] = True
            seeded[0] = False
            assert np.array_equal(Q >= t, seeded[comp]), (dims, t)


@pytest.mark.parametrize("connectivity, weights", [(6, (1, 0, 0)), (18, (3, 4, 0)), (26, (3, 4, 5)), (26, (7, 1, 1))])
def test_regions_are_connected_and_reach_is_the_seeded_components(connectivity, weights):
    rng = np.random.default_rng(connectivity + sum(weights))
    for dims, density in (((14, 10, 8), 0.6), ((25, 6, 5), 0.85)):
        H, M = WR.random_case(rng, dims, 8, 5, density)
        labels, level, ticks, reached = WR.grow(H, M, weights)
        seeds = WR.seeds_of(H, M)
        # reached: exactly the components of S that hold a seed
        comp, n = CR.label(H > 0, connectivity)
        seeded = np.zeros(n + 1, bool)
        seeded[comp[seeds]] = True
        seeded[0] = False
        assert np.array_equal(labels > 0, seeded[comp]) and reached == int(seeded[comp].sum())
        # every label's region is connected and holds a marker of its label
        for label in np.unique(labels[labels > 0]):
            region = labels == label
            assert CR.label(region, connectivity)[1] == 1 and (seeds & (M == label) & region).any(), (dims, label)
        assert set(np.unique(labels[labels > 0])) <= set(np.unique(M[seeds]))


def test_saturation_on_a_serpentine():
    """A flat corridor one voxel wide with a step of 65 535: ticks are 65 535 i until they stay at 2^31 - 2.  The reference here is
    the Dijkstra: the shifted views would take a pass per voxel."""
    S = CR.serpentine((128, 64, 16))
    M = np.zeros(S.shape, np.int32)
    M[0, 0, 0] = 1
    labels, level, ticks, reached = WR.dijkstra(S.astype(np.int32), M, (65535, 0, 0))
    n = int(S.sum())
    assert reached == n and (labels[S] == 1).all() and (level[S] == 1).all() and not labels[~S].any()
    want = np.minimum(np.arange(n, dtype=np.int64) * 65535, 2 ** 31 - 2)
    assert np.array_equal(np.sort(ticks[S]), want) and (ticks[S] == 2 ** 31 - 2).sum() == n - 32769 > 100
    hops = WR.dijkstra(S.astype(np.int32), M, (1, 0, 0))[2]
    assert np.array_equal(ticks[S], np.minimum(hops[S].astype(np.int64) * 65535, 2 ** 31 - 2))     # ... in the corridor's own order


# ---- the kernels' lane bodies on the host ------------------------------------------------------------------------------------------

HOST_GROW = r"""
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>
#define O2V_GEO_HOST
#define O2V_GEO_FN static inline
#define O2V_GROW_HOST
#define O2V_GROW_FN static inline
constexpr uint32_t kGeoInf = 0x7fffffffu, kGeoRowStride = 66u, kGeoLayerStride = 660u, kGeoHalo = 6600u;
constexpr uint32_t kGrowCap = 0x7ffffffeu, kGrowNoLabel = 0xffffffffu;
static inline uint32_t grow_load(const uint32_t *p) { return *p; }
static inline void grow_store(uint32_t *p, uint32_t v) { *p = v; }
%s
struct Host {
    GeoGrid g;
    const int32_t *H, *M;
    uint32_t *mask;
    uint32_t tiles;
    std::mt19937 rng;
    uint64_t *out9;
    int no_tiles;
};

static uint32_t own_of(const Host &h, int P, uint32_t x, uint32_t y, uint32_t z)
{
    const uint32_t i = (z * h.g.ny + y) * h.g.nx + x;
    return P == 0 ? (h.H[i] > 0 ? (uint32_t) h.H[i] : 0u) : h.mask[i];
}

static void wake(const Host &h, uint32_t tx, uint32_t ty, uint32_t tz, uint32_t see, std::vector<uint8_t> &flag, std::vector<uint32_t> &list)
{
    for (int k = 0; k < 27; ++k) {
        const uint32_t X = tx + (uint32_t) geo_dx(k), Y = ty + (uint32_t) geo_dy(k), Z = tz + (uint32_t) geo_dz(k);
        if (!((see >> k) & 1u) || X >= h.g.W || Y >= h.g.tiles_y || Z >= h.g.tiles_z) continue;
        const uint32_t t = (Z * h.g.tiles_y + Y) * h.g.W + X;
        if (!flag[t]) flag[t] = 1, list.push_back(t);
    }
}

// The rounds of phase P on V, a "lane" at a time, as k_grow_tiles / k_grow_sweep run them.  list: round 0.  Tiles: the tiles of a
// round in a shuffled order, each reading what the tiles before it have stored.  Returns 1 if a tile was listed twice in a round.
template <int P>
static int rounds(Host &h, uint32_t *V, std::vector<uint32_t> list, std::vector<uint8_t> flag)
{
    const GeoGrid &g = h.g;
    uint64_t *out = h.out9 + 3 * P;
    if (h.no_tiles) {
        for (bool any = true; any;) {
            any = false;
            ++out[0];
            for (uint32_t z = 0; z < g.nz; ++z)
                for (uint32_t y = 0; y < g.ny; ++y)
                    for (uint32_t x = 0; x < g.nx; ++x) {
                        const uint32_t own = own_of(h, P, x, y, z), i = (z * g.ny + y) * g.nx + x;
                        if (!own) continue;
                        const uint32_t v = grow_relax<P>(V + i, (int64_t) g.nx, (int64_t) g.nx * g.ny, g.w, own, P == 0 ? grow_box_mask(g, x, y, z) : 0u);
                        if (v != V[i]) V[i] = v, any = true;
                    }
        }
        return 0;
    }
    std::vector<uint32_t> next;
    std::vector<uint8_t> flag_next(h.tiles, 0);
    static uint32_t s_v[kGeoHalo], own[4096];
    static uint8_t changed[4096];
    while (!list.empty()) {
        ++out[0];
        std::shuffle(list.begin(), list.end(), h.rng);
        next.clear();
        for (const uint32_t tile : list) {
            const uint32_t trow = tile / g.W, tx = tile - trow * g.W, tz = trow / g.tiles_y, ty = trow - tz * g.tiles_y;
            const uint32_t x0 = tx * 64u, y0 = ty * 8u, z0 = tz * 8u;
            flag[tile] = 0;
            ++out[1];
            for (uint32_t row = 0; row < 100u; ++row)
                for (uint32_t c = 0; c < 66u; ++c) {
                    const uint32_t X = x0 + c - 1u, Y = y0 + row %% 10u - 1u, Z = z0 + row / 10u - 1u;
                    s_v[row * kGeoRowStride + c] = X < g.nx && Y < g.ny && Z < g.nz ? V[(Z * g.ny + Y) * g.nx + X] : grow_outside<P>();
                }
            for (uint32_t row = 0; row < 64u; ++row)
                for (uint32_t x = 0; x < 64u; ++x) {
                    const uint32_t X = x0 + x, Y = y0 + (row & 7u), Z = z0 + (row >> 3);
                    own[row * 64u + x] = X < g.nx && Y < g.ny && Z < g.nz ? own_of(h, P, X, Y, Z) : 0u;
                }
            std::memset(changed, 0, sizeof changed);
            for (bool any = true; any;) {
                any = false;
                ++out[2];
                for (uint32_t row = 0; row < 64u; ++row)
                    for (uint32_t x = 0; x < 64u; ++x) {
                        if (!own[row * 64u + x]) continue;
                        uint32_t *const p = s_v + ((row >> 3) + 1u) * kGeoLayerStride + ((row & 7u) + 1u) * kGeoRowStride + 1u + x;
                        const uint32_t v = grow_relax<P>(p, (int64_t) kGeoRowStride, (int64_t) kGeoLayerStride, g.w, own[row * 64u + x], 0x7ffffffu);
                        if (v != *p) *p = v, changed[row * 64u + x] = 1, any = true;
                    }
            }
            uint32_t see = 0;
            for (uint32_t row = 0; row < 64u; ++row)
                for (uint32_t x = 0; x < 64u; ++x) {
                    if (!changed[row * 64u + x]) continue;
                    const uint32_t y = row & 7u, z = row >> 3;
                    V[((z0 + z) * g.ny + (y0 + y)) * g.nx + (x0 + x)] = s_v[(z + 1u) * kGeoLayerStride + (y + 1u) * kGeoRowStride + 1u + x];
                    see |= geo_see_mask(x, y, z, g.w);
                }
            wake(h, tx, ty, tz, see, flag_next, next);
        }
        for (const uint32_t t : next)
            if (flag[t]) return 1;
        list.swap(next);
        flag.swap(flag_next);
    }
    return 0;
}

// The whole call in the kernels' order; Q, T, L and mask end as the kernels leave them before k_grow_write.  out9: per phase the
// rounds, tile visits and in-tile sweeps.
extern "C" int grow_host(const int32_t *H, const int32_t *M, uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t *w, int no_tiles, uint32_t shuffle,
                         uint32_t *Q, uint32_t *T, uint32_t *L, uint32_t *mask, uint64_t *out9)
{
    Host h;
    GeoGrid &g = h.g;
    g.nx = nx, g.ny = ny, g.nz = nz, g.W = (nx + 63u) / 64u, g.tiles_y = (ny + 7u) / 8u, g.tiles_z = (nz + 7u) / 8u;
    g.w[0] = w[0], g.w[1] = w[1], g.w[2] = w[2], g.max_distance = kGrowCap, g.words = (uint64_t) g.W * ny * nz;
    h.H = H, h.M = M, h.mask = mask, h.tiles = g.W * g.tiles_y * g.tiles_z, h.rng.seed(shuffle), h.out9 = out9, h.no_tiles = no_tiles;
    std::fill(out9, out9 + 9, 0);
    const int64_t sy = nx, sz = (int64_t) nx * ny;
    std::vector<uint32_t> list;
    std::vector<uint8_t> flag(h.tiles, 0);
    // k_grow_init
    for (uint32_t z = 0; z < nz; ++z)
        for (uint32_t y = 0; y < ny; ++y)
            for (uint32_t x = 0; x < nx; ++x) {
                const uint32_t i = (z * ny + y) * nx + x;
                const bool seed = H[i] > 0 && M[i] > 0;
                Q[i] = seed ? (uint32_t) H[i] : 0u;
                if (seed) wake(h, x >> 6, y >> 3, z >> 3, geo_see_mask(x & 63u, y & 7u, z & 7u, g.w) | 1u << 13, flag, list);
            }
    if (rounds<0>(h, Q, list, flag)) return 1;
    // k_grow_between<false>, k_grow_between<true>: every tile with a reached voxel is listed
    for (int tight = 0; tight < 2; ++tight) {
        list.clear();
        std::fill(flag.begin(), flag.end(), 0);
        for (uint32_t z = 0; z < nz; ++z)
            for (uint32_t y = 0; y < ny; ++y)
                for (uint32_t x = 0; x < nx; ++x) {
                    const uint32_t i = (z * ny + y) * nx + x, box = grow_box_mask(g, x, y, z);
                    uint32_t m = 0, t = kGeoInf, l = kGrowNoLabel;
                    if (Q[i]) {
                        if (tight) {
                            m = grow_tight_mask(Q + i, T + i, sy, sz, g.w, (uint32_t) H[i], M[i] > 0, box);
                            if (M[i] > 0) l = (uint32_t) M[i];
                        } else {
                            t = grow_sources(Q + i, sy, sz, g.w, (uint32_t) H[i], M[i] > 0, box, &m);
                        }
                        wake(h, x >> 6, y >> 3, z >> 3, 1u << 13, flag, list);
                    }
                    mask[i] = m;
                    if (tight) L[i] = l;
                    else T[i] = t;
                }
        if (tight ? rounds<2>(h, L, list, flag) : rounds<1>(h, T, list, flag)) return 1;
    }
    return 0;
}

#ifdef O2V_GROW_MUTATE_LABEL_IN_KEY
// The mutation's run: the level as above (whole-grid sweeps), then one relaxation of the packed pairs (T, L) instead of the ticks
// and the labels - tile by tile, the tiles of a round in a shuffled order, a tile's voxels swept in place until nothing moves, each
// tile reading what the tiles before it have stored - until a round moves nothing.
extern "C" int grow_host_joint(const int32_t *H, const int32_t *M, uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t *w, uint32_t shuffle, uint32_t *Q,
                               uint32_t *T, uint32_t *L)
{
    Host h;
    GeoGrid &g = h.g;
    g.nx = nx, g.ny = ny, g.nz = nz, g.W = (nx + 63u) / 64u, g.tiles_y = (ny + 7u) / 8u, g.tiles_z = (nz + 7u) / 8u;
    g.w[0] = w[0], g.w[1] = w[1], g.w[2] = w[2], g.max_distance = kGrowCap, g.words = (uint64_t) g.W * ny * nz;
    uint64_t out9[9] = {};
    std::vector<uint32_t> same((size_t) nx * ny * nz), higher(same.size());
    h.H = H, h.M = M, h.mask = same.data(), h.tiles = g.W * g.tiles_y * g.tiles_z, h.rng.seed(shuffle), h.out9 = out9, h.no_tiles = 1;
    const int64_t sy = nx, sz = (int64_t) nx * ny;
    for (size_t i = 0; i < same.size(); ++i) Q[i] = H[i] > 0 && M[i] > 0 ? (uint32_t) H[i] : 0u;
    rounds<0>(h, Q, {}, {});
    std::vector<uint64_t> V(same.size());
    for (uint32_t z = 0; z < nz; ++z)
        for (uint32_t y = 0; y < ny; ++y)
            for (uint32_t x = 0; x < nx; ++x) {
                const uint32_t i = (z * ny + y) * nx + x, box = grow_box_mask(g, x, y, z);
                const bool seed = H[i] > 0 && M[i] > 0;
                same[i] = higher[i] = 0;
                V[i] = seed ? (uint64_t) (uint32_t) M[i] : (uint64_t) kGeoInf << 32 | kGrowNoLabel;
                if (!Q[i] || seed) continue;
                (void) grow_sources(Q + i, sy, sz, g.w, (uint32_t) H[i], false, box, &same[i]);
                higher[i] = grow_higher_mask(Q + i, sy, sz, g.w, (uint32_t) H[i], box);
            }
    std::vector<uint32_t> order(h.tiles);
    for (uint32_t t = 0; t < h.tiles; ++t) order[t] = t;
    for (bool moved = true; moved;) {
        moved = false;
        std::shuffle(order.begin(), order.end(), h.rng);
        for (const uint32_t tile : order) {
            const uint32_t trow = tile / g.W, x0 = (tile - trow * g.W) * 64u, z0 = trow / g.tiles_y * 8u, y0 = (trow - trow / g.tiles_y * g.tiles_y) * 8u;
            for (bool any = true; any;) {
                any = false;
                for (uint32_t z = z0; z < std::min(z0 + 8u, nz); ++z)
                    for (uint32_t y = y0; y < std::min(y0 + 8u, ny); ++y)
                        for (uint32_t x = x0; x < std::min(x0 + 64u, nx); ++x) {
                            const uint32_t i = (z * ny + y) * nx + x;
                            if (!(same[i] | higher[i])) continue;
                            const uint64_t v = grow_joint_relax(V.data() + i, sy, sz, g.w, same[i], higher[i]);
                            if (v != V[i]) V[i] = v, any = moved = true;
                        }
            }
        }
    }
    for (size_t i = 0; i < V.size(); ++i) T[i] = (uint32_t) (V[i] >> 32), L[i] = (uint32_t) V[i];
    return 0;
}
#endif
"""


@pytest.fixture(scope="module")
def host_grow(tmp_path_factory):
    """build(defines) -> a library with grow_host: the plain parts of o2v_dev_bits.hpp, o2v_dev_k20_geodesic.hpp (the offsets and
    the see mask) and o2v_dev_k28_grow.hpp (the lane bodies), compiled for the host."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    text = open(K20).read()
    geo = text[text.index("// ---- the relaxation, the tiles that see a voxel, the trace step"):text.index("// ---- kernels")]
    text = open(K28).read()
    grow = text[text.index("// ---- the lane bodies"):text.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_grow")
    built = {}

    def build(defines=()):
        if defines not in built:
            name = "grow_%d" % len(built)
            (tmp / (name + ".cpp")).write_text(HOST_GROW % (bits_host.plain_part() + geo + grow))
            subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                           [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
            built[defines] = hip.C.CDLL(str(tmp / (name + ".so")))
        return built[defines]
    return build


def host_run(L, H, M, weights, no_tiles=False, shuffle=0):
    """((labels, level, ticks, reached), counters) of the host build, as k_grow_write would write them."""
    C = hip.C
    H, M = np.ascontiguousarray(H, np.int32), np.ascontiguousarray(M, np.int32)
    nz, ny, nx = H.shape
    Q, T, Lb, mask = (np.full(H.size, 0xABABABAB, np.uint32) for _ in range(4))
    w = np.asarray(weights, np.uint32)
    out9 = np.zeros(9, np.uint64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    rc = L.grow_host(ptr(H), ptr(M), nx, ny, nz, ptr(w), int(no_tiles), shuffle, ptr(Q), ptr(T), ptr(Lb), ptr(mask), ptr(out9))
    assert rc == 0, "a tile was in a round's list twice"
    Q, T, Lb, mask = (a.reshape(H.shape) for a in (Q, T, Lb, mask))
    out = H <= 0
    assert (Q[out] == 0).all() and (T[out] == INF).all() and (Lb[out] == NO_LABEL).all() and (mask[out] == 0).all()    # nothing outside S is ever reached
    hit = Q > 0
    assert (T[~hit] == INF).all() and (Lb[~hit] == NO_LABEL).all() and (T[hit] <= WR.CAP).all()
    got = (np.where(hit, Lb, 0).astype(np.int32), Q.astype(np.int32), np.where(hit, T.astype(np.int64), -1).astype(np.int32), int(hit.sum()))
    return got, tuple(int(v) for v in out9)


@pytest.mark.parametrize("no_tiles", [False, True])
def test_the_lane_bodies_on_the_host_equal_the_reference(host_grow, no_tiles):
    L = host_grow()
    rng = np.random.default_rng(28)
    for i in range(20):                                       # 70 x 20 x 12 crosses a tile in x, y and z
        H, M = WR.random_case(rng, (70, 20, 12), (1, 3, 8)[i % 3], 1 + i % 7, (0.5, 0.75, 1.0)[i // 3 % 3])
        weights = ALL_WEIGHTS[i % 7]
        want = WR.grow_frontier(H, M, weights)
        for shuffle in ((0,) if no_tiles else (1, 2, 3)):
            got, counters = host_run(L, H, M, weights, no_tiles, shuffle)
            assert same(got, want), (i, weights, no_tiles, shuffle)
            assert no_tiles or all(counters[3 * p + 2] >= counters[3 * p + 1] >= counters[3 * p] for p in range(3))
    H, M = WR.random_case(rng, (70, 20, 12), 8, 4, 0.8)
    assert same(WR.grow(H, M, (3, 4, 5)), WR.grow_frontier(H, M, (3, 4, 5)))      # (the frontier form is the shifted views' equal here too)


@pytest.mark.parametrize("no_tiles", [False, True])
def test_pairs_across_a_tile_boundary(host_grow, no_tiles):
    """The seven kinds of voxel pairs that touch only across a tile's face, edge or corner, seeded on either side, flat and with a
    descent (H 2 -> 1) across the boundary: reached exactly when that kind of step has a weight."""
    L = host_grow()
    for kind, steps in (("x", 1), ("y", 1), ("z", 1), ("xy", 2), ("xz", 2), ("yz", 2), ("xyz", 3)):
        for descent in (False, True):
            H, M, a, b = WR.pair_across(kind, descent)
            back = np.zeros_like(M)
            back[b[2], b[1], b[0]] = 5
            for weights in ((1, 0, 0), (1, 1, 0), (1, 1, 1), (3, 4, 5), (0, 4, 0), (0, 0, 5)):
                w = weights[steps - 1]
                for markers, far, near_h in ((M, b, H[a[2], a[1], a[0]]), (back, a, 1)):
                    want = WR.grow(H, markers, weights)
                    assert want[3] == (2 if w else 1) and want[0][far[2], far[1], far[0]] == (5 if w else 0)
                    down = markers is M and descent
                    assert want[2][far[2], far[1], far[0]] == ((0 if down else w) if w else -1) and want[1][far[2], far[1], far[0]] == (1 if w else 0)
                    got, _ = host_run(L, H, markers, weights, no_tiles, 5)
                    assert same(got, want), (kind, descent, weights, no_tiles)


def test_a_corridor_and_two_hills_on_the_host(host_grow):
    L = host_grow()
    S = CR.serpentine((70, 21, 19))
    M = np.zeros(S.shape, np.int32)
    M[0, 0, 0] = 3
    for weights in ((1, 0, 0), (65535, 0, 0)):
        want = WR.dijkstra(S.astype(np.int32), M, weights)
        for no_tiles in (False, True):
            got, counters = host_run(L, S.astype(np.int32), M, weights, no_tiles, 7)
            assert same(got, want) and (no_tiles or counters[3] > 10)          # the ticks walk the corridor tile by tile
    H, M = WR.two_hills((70, 12, 12), 64 - 30)
    want = WR.grow(H, M, (3, 4, 5))
    assert same(host_run(L, H, M, (3, 4, 5))[0], want)
    H, M = WR.two_hills((140, 10, 9))
    want = WR.grow_frontier(H, M, (1, 0, 0))
    assert (want[0][:, :, :64] == 2).all() and (want[0][:, :, 64:] == 1).all()     # the valley lies on the tile boundary: the smaller label takes it
    assert same(host_run(L, H, M, (1, 0, 0), shuffle=2)[0], want)


def test_a_clock_that_keeps_running_on_a_descent_is_caught(host_grow):
    """DESIGN.md section 32, mutation: with -DO2V_GROW_MUTATE_NO_RESET a descent is no source of the ticks.  The second and the
    third closed form fail, the flat one passes."""
    L = host_grow(("O2V_GROW_MUTATE_NO_RESET",))
    h = [5, 4, 3, 2, 1, 2, 3, 4, 5, 4, 3]
    for heights, markers, holds in (([3] * 9, [(0, 2), (8, 1)], True), (h, [(0, 1), (8, 2)], False), (h, [(0, 1)], False)):
        want, H, M = row(heights, markers)
        for no_tiles in (False, True):
            try:
                got = [a.ravel().tolist() for a in host_run(L, H, M, (1, 0, 0), no_tiles)[0][:3]]
            except AssertionError:          # (a reached voxel whose ticks stayed at "not yet")
                got = None
            assert (got == want) == holds, (heights, markers, no_tiles)
            assert [a.ravel().tolist() for a in host_run(host_grow(), H, M, (1, 0, 0), no_tiles)[0][:3]] == want


def test_a_label_inside_the_key_of_the_ticks_is_caught(host_grow):
    """DESIGN.md section 32, mutation: with -DO2V_GROW_MUTATE_LABEL_IN_KEY the smallest label is taken inside the comparison of the
    ticks (one relaxation of the pairs (T, L)) instead of in a phase of its own.  A pair that falls from (3, 1) to (2, 7) has
    handed its 1 on, so the result depends on the order of the visits: over the 20 random grids of the lane-body test in the
    shuffled orders 1, 2, 3 at least one differs from the reference - grid MUTANT_GRID in order MUTANT_SHUFFLE is one -, while the
    level, which the mutation leaves alone, never does."""
    L = host_grow(("O2V_GROW_MUTATE_LABEL_IN_KEY",))
    C = hip.C
    rng = np.random.default_rng(28)
    differ = []
    for i in range(20):
        H, M = WR.random_case(rng, (70, 20, 12), (1, 3, 8)[i % 3], 1 + i % 7, (0.5, 0.75, 1.0)[i // 3 % 3])
        weights = ALL_WEIGHTS[i % 7]
        want = WR.grow_frontier(H, M, weights)
        for shuffle in (1, 2, 3):
            Q, T, Lb = (np.zeros(H.size, np.uint32) for _ in range(3))
            w = np.asarray(weights, np.uint32)
            ptr = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
            assert L.grow_host_joint(ptr(np.ascontiguousarray(H)), ptr(np.ascontiguousarray(M)), 70, 20, 12, ptr(w), shuffle, ptr(Q), ptr(T), ptr(Lb)) == 0
            hit = Q.reshape(H.shape) > 0
            assert np.array_equal(Q.reshape(H.shape).astype(np.int32), want[1])
            labels = np.where(hit, Lb.reshape(H.shape), 0).astype(np.int32)
            ticks = np.where(hit, T.reshape(H.shape).astype(np.int64), -1).astype(np.int32)
            if not (np.array_equal(labels, want[0]) and np.array_equal(ticks, want[2])):
                differ.append((i, shuffle))
    print("the label-in-key mutation differs on (grid, shuffle):", differ)
    assert differ and (MUTANT_GRID, MUTANT_SHUFFLE) in differ
    assert not hasattr(host_grow(), "grow_host_joint")          # (the mutation is in no other build)


MUTANT_GRID, MUTANT_SHUFFLE = 4, 1      # one (grid, shuffled order) of the test above on which the mutation is seen


# ---- the torch layer against a stub ----------------------------------------------------------------------------------------------

class GrowStub(StubVoxelizer):
    """Computes with the reference, on the tensors' own memory (CPU)."""

    @staticmethod
    def view(ptr, strides, dims):
        C = hip.C
        nx, ny, nz = dims
        span = sum((d - 1) * s for d, s in zip(dims, strides)) + 1
        raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), (span,))
        return np.lib.stride_tricks.as_strided(raw, (nz, ny, nx), tuple(4 * s for s in (strides[2], strides[1], strides[0])))

    def grow_dense(self, relief_ptr, relief_strides, markers_ptr, marker_strides, dims, weights, flags, labels_ptr, labels_strides, level_ptr=None,
                   level_strides=None, ticks_ptr=None, ticks_strides=None):
        self.calls.append(("grow", relief_ptr, tuple(relief_strides), markers_ptr, tuple(marker_strides), tuple(dims), tuple(weights), flags, labels_ptr,
                           tuple(labels_strides), level_ptr, level_strides and tuple(level_strides), ticks_ptr, ticks_strides and tuple(ticks_strides)))
        want = WR.grow(self.view(relief_ptr, relief_strides, dims), self.view(markers_ptr, marker_strides, dims), weights)
        for ptr, strides, a in ((labels_ptr, labels_strides, want[0]), (level_ptr, level_strides, want[1]), (ticks_ptr, ticks_strides, want[2])):
            if ptr is not None:
                self.view(ptr, strides, dims)[...] = a
        return want[3]

    def geodesic_dense(self, *args):
        raise AssertionError("grow_labels does not call geodesic_dense")


def test_seeded_watershed_against_the_stub():
    dv = GrowStub()
    rng = np.random.default_rng(1)
    Hn, Mn = WR.random_case(rng, (9, 7, 5), 6, 4, 0.8)
    H, M = torch.from_numpy(Hn), torch.from_numpy(Mn)
    want = WR.grow(Hn, Mn, (3, 4, 5))
    labels = dense.seeded_watershed(dv, H, M)
    c = dv.calls[-1]
    assert c[0] == "grow" and c[5:8] == ((9, 7, 5), (3, 4, 5), 0) and c[10] is None and c[12] is None and c[2] == c[4] == c[9] == (1, 9, 63)
    assert labels.dtype == torch.int32 and labels.is_contiguous() and np.array_equal(labels.numpy(), want[0])
    labels, level, ticks = dense.seeded_watershed(dv, H, M, level=True, distance=True)
    assert all(np.array_equal(t.numpy(), w) for t, w in zip((labels, level, ticks), want[:3])) and dv.calls[-1][10] is not None
    labels, level, ticks = dense.seeded_watershed(dv, H, M, distance=True, metric="steps", connectivity=6)
    assert level is None and dv.calls[-1][6] == (1, 0, 0) and dv.calls[-1][10] is None and np.array_equal(ticks.numpy(), WR.grow(Hn, Mn, (1, 0, 0))[2])
    labels, level, ticks = dense.seeded_watershed(dv, H, M, level=True, weights=(2, 3, 0))
    assert ticks is None and dv.calls[-1][6] == (2, 3, 0) and np.array_equal(level.numpy(), WR.grow(Hn, Mn, (2, 3, 0))[1])
    # strided inputs are passed as they are; out= is written as it is
    wide = torch.zeros((5, 7, 18), dtype=torch.int32)
    wide[:, :, ::2] = H
    out = torch.full((5, 7, 18), -7, dtype=torch.int32)
    got = dense.seeded_watershed(dv, wide[:, :, ::2], M.permute(2, 1, 0).contiguous().permute(2, 1, 0), out=out[:, :, 1::2])
    assert dv.calls[-1][2] == (2, 18, 126) and dv.calls[-1][4] == (35, 5, 1) and dv.calls[-1][9] == (2, 18, 126)
    assert got.data_ptr() == out[:, :, 1::2].data_ptr() and np.array_equal(out[:, :, 1::2].numpy(), want[0]) and bool((out[:, :, ::2] == -7).all())
    for text in ("section 32", "Meyer", "label_adjacency"):
        assert text in " ".join(dense.seeded_watershed.__doc__.split())


def test_grow_labels_against_the_stub():
    dv = GrowStub()
    S = GR.door_box()
    grid = torch.from_numpy(S)
    seeds = [(0, 0, 0), (39, 19, 19), (0, 0, 0), (-1, 0, 0), (40, 0, 0), (5, 5, 5)]
    markers = dense.markers_from_seeds(seeds, grid.shape, device="cpu")
    assert markers.dtype == torch.int32 and tuple(markers.shape) == (20, 20, 40) and int((markers > 0).sum()) == 3
    assert int(markers[0, 0, 0]) == 1 and int(markers[19, 19, 39]) == 2 and int(markers[5, 5, 5]) == 6          # a duplicate: the smallest label
    labels, dist = dense.grow_labels(dv, grid, markers)
    assert dv.calls[-1][6] == (3, 4, 5) and dv.calls[-1][10] is None and dv.calls[-1][12] is not None
    want = GR.distance(S, (3, 4, 5), [(0, 0, 0), (39, 19, 19), (5, 5, 5)])[0]
    assert np.array_equal(dist.numpy(), want) and np.array_equal(labels.numpy() > 0, want >= 0) and set(np.unique(labels.numpy())) == {0, 1, 2, 6}
    # max_distance is a mask on the result
    near, d6 = dense.grow_labels(dv, grid, markers, max_distance=6)
    assert np.array_equal(d6.numpy(), np.where(want > 6, -1, want)) and np.array_equal(near.numpy(), np.where(want > 6, 0, labels.numpy()))
    zero, d0 = dense.grow_labels(dv, grid, markers, max_distance=0)
    assert np.array_equal(zero.numpy(), np.where(S, markers.numpy(), 0)) and int((d0 == 0).sum()) == 3
    # uint8, float32 with a level, the background
    same_labels = dense.grow_labels(dv, torch.from_numpy(S.astype(np.uint8) * 7), markers)[0]
    assert torch.equal(same_labels, labels)
    assert torch.equal(dense.grow_labels(dv, torch.where(grid, -1.0, 1.0), markers, level=0.0)[0], labels)
    assert torch.equal(dense.grow_labels(dv, ~grid, markers, background=True, metric="steps", connectivity=6)[1],
                       torch.from_numpy(GR.distance(S, (1, 0, 0), [(0, 0, 0), (39, 19, 19), (5, 5, 5)])[0]))
    assert "section 32" in dense.grow_labels.__doc__ and "expand_labels" in dense.grow_labels.__doc__


def test_markers_from_seeds():
    m = dense.markers_from_seeds(torch.tensor([[1, 2, 3], [0, 0, 0], [1, 2, 3], [4, 0, 0], [0, 5, 0], [0, 0, 6], [-1, 2, 3]], dtype=torch.int32), (6, 5, 4), device="cpu")
    want = np.zeros((6, 5, 4), np.int32)
    want[3, 2, 1], want[0, 0, 0] = 1, 2
    assert np.array_equal(m.numpy(), want)
    assert not dense.markers_from_seeds(torch.zeros((0, 3), dtype=torch.int32), (2, 2, 2), device="cpu").any()
    for bad, exc in ((dict(seeds=torch.zeros((2, 3))), TypeError), (dict(seeds=torch.zeros((2, 3), dtype=torch.int64)), TypeError),
                     (dict(seeds=torch.zeros((2, 2), dtype=torch.int32)), ValueError), (dict(seeds=torch.zeros((2, 3), dtype=torch.int32, device="meta")), ValueError),
                     (dict(shape=(2, 2)), ValueError), (dict(shape=(2, 0, 2)), ValueError), (dict(shape=(2, 2.0, 2)), ValueError), (dict(shape=(2048, 1024, 1024)), ValueError)):
        args = dict(seeds=torch.zeros((2, 3), dtype=torch.int32), shape=(2, 2, 2))
        args.update(bad)
        with pytest.raises(exc):
            dense.markers_from_seeds(args["seeds"], args["shape"], device="cpu")


I32 = torch.ones((4, 4, 4), dtype=torch.int32)
U8 = torch.ones((4, 4, 4), dtype=torch.uint8)


@pytest.mark.parametrize("kw, exc", [
    (dict(relief=torch.zeros((4, 4, 4), dtype=torch.int64)), TypeError), (dict(relief=torch.zeros((4, 4, 4))), TypeError), (dict(relief=torch.zeros((4, 4), dtype=torch.int32)), ValueError),
    (dict(relief=np.zeros((4, 4, 4), np.int32)), ValueError), (dict(relief=torch.zeros((4, 4, 4), dtype=torch.int32, device="meta")), ValueError),
    (dict(relief=torch.zeros((4, 0, 4), dtype=torch.int32), markers=torch.zeros((4, 0, 4), dtype=torch.int32)), ValueError),
    (dict(relief=torch.zeros((1, 1, 1), dtype=torch.int32).expand(1, 1, 65537), markers=torch.zeros((1, 1, 1), dtype=torch.int32).expand(1, 1, 65537)), ValueError),
    (dict(markers=torch.zeros((4, 4, 4), dtype=torch.int64)), TypeError), (dict(markers=torch.zeros((4, 4, 4), dtype=torch.uint8)), TypeError),
    (dict(markers=torch.zeros((4, 4, 5), dtype=torch.int32)), ValueError), (dict(markers=None), ValueError),
    (dict(markers=torch.zeros((4, 4, 4), dtype=torch.int32, device="meta")), ValueError),
    (dict(connectivity=8), ValueError), (dict(connectivity=True), ValueError), (dict(metric="euclidean"), ValueError),
    (dict(weights=(1, 0)), ValueError), (dict(weights=(0, 0, 0)), ValueError), (dict(weights=(65536, 0, 0)), ValueError), (dict(weights=(1.0, 0, 0)), ValueError),
    (dict(level=1), TypeError), (dict(distance="yes"), TypeError), (dict(level=None), TypeError),
    (dict(out=torch.zeros((4, 4, 4), dtype=torch.int64)), TypeError), (dict(out=torch.zeros((4, 4, 5), dtype=torch.int32)), ValueError),
    (dict(out=torch.zeros((4, 4, 4), dtype=torch.int32, device="meta")), ValueError), (dict(out=np.zeros((4, 4, 4), np.int32)), ValueError),
    (dict(out=I32), ValueError),
])
def test_seeded_watershed_rejects(kw, exc):
    dv = GrowStub()
    args = dict(relief=I32, markers=torch.ones((4, 4, 4), dtype=torch.int32))
    args.update(kw)
    with pytest.raises(exc):
        dense.seeded_watershed(dv, args.pop("relief"), args.pop("markers"), **args)
    assert not dv.calls


@pytest.mark.parametrize("kw, exc", [
    (dict(grid=torch.zeros((4, 4, 4), dtype=torch.int32)), ValueError), (dict(grid=torch.zeros((4, 4, 4), dtype=torch.float64)), TypeError),
    (dict(grid=torch.zeros((4, 4))), ValueError), (dict(grid=np.zeros((4, 4, 4), np.uint8)), ValueError), (dict(grid=torch.zeros((4, 4, 4))), ValueError),
    (dict(grid=torch.zeros((4, 4, 4)), level=float("nan")), ValueError), (dict(level=0.0), ValueError),
    (dict(grid=torch.zeros((4, 0, 4), dtype=torch.uint8)), ValueError), (dict(grid=torch.zeros((4, 4, 4), dtype=torch.uint8, device="meta")), ValueError),
    (dict(grid=torch.zeros((1, 1, 1), dtype=torch.uint8).expand(2048, 1024, 1024)), ValueError),
    (dict(markers=torch.zeros((4, 4, 4), dtype=torch.int64)), TypeError), (dict(markers=torch.zeros((4, 4, 5), dtype=torch.int32)), ValueError),
    (dict(markers=[(0, 0, 0)]), ValueError), (dict(background=1), TypeError),
    (dict(connectivity=7), ValueError), (dict(metric="hops"), ValueError), (dict(weights=(0, 0, 0)), ValueError), (dict(weights="345"), ValueError),
    (dict(max_distance=-1), ValueError), (dict(max_distance=2 ** 31 - 1), ValueError), (dict(max_distance=6.0), ValueError), (dict(max_distance=True), ValueError),
])
def test_grow_labels_rejects(kw, exc):
    dv = GrowStub()
    args = dict(grid=U8, markers=torch.ones((4, 4, 4), dtype=torch.int32))
    args.update(kw)
    with pytest.raises(exc):
        dense.grow_labels(dv, args.pop("grid"), args.pop("markers"), **args)
    assert not dv.calls


def test_refused_when_the_library_came_first(monkeypatch):
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: False)
    with pytest.raises(RuntimeError, match="before torch"):
        dense.seeded_watershed(GrowStub(), I32, I32.clone())
    with pytest.raises(RuntimeError, match="before torch"):
        dense.grow_labels(GrowStub(), U8, I32)


def test_a_wait_comes_before_the_library(monkeypatch):
    """As tests/test_host_dense.py holds it for the other functions: the library call comes behind a wait on the voxelizer's own
    device."""
    for call in (lambda dv: dense.seeded_watershed(dv, I32, I32.clone(), level=True), lambda dv: dense.grow_labels(dv, U8, I32, max_distance=3)):
        dv = GrowStub()
        own = torch.device("cpu")
        monkeypatch.setattr(dense, "_device", lambda v: own)
        monkeypatch.setattr(dense, "_sync", lambda device: dv.calls.append(("sync", device)))
        call(dv)
        names = [c[0] for c in dv.calls]
        assert names == ["sync", "grow"] and dv.calls[0][1] is own


# ---- the scratch formula and the code object -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(1, 1, 1), (64, 8, 8), (65, 9, 9), (1024, 1024, 1024), (65536, 1, 7), (1000, 999, 17)])
def test_scratch_bytes_formula(dims):
    voxels = math.prod(dims)
    tiles = -(-dims[0] // 64) * -(-dims[1] // 8) * -(-dims[2] // 8)
    base = 4 * voxels + 16 * tiles + 128
    assert hip.grow_scratch_bytes(dims) == hip.grow_scratch_bytes(dims, 0) == base                      # labels, level and ticks given and contiguous
    for which in range(8):
        assert hip.grow_scratch_bytes(dims, which) == base + 4 * voxels * bin(which).count("1")
    assert hip.grow_scratch_bytes(dims, hip.GROW_SCRATCH_LABELS | hip.GROW_SCRATCH_LEVEL | hip.GROW_SCRATCH_TICKS) == base + 12 * voxels
    assert hip.grow_scratch_bytes((4, 0, 4)) == 0 and hip.grow_scratch_bytes(dims, 8) == 0
    assert hip.DeviceVoxelizer.grow_scratch_bytes(None, dims) == base and hip.GROW_MAX_TICKS == WR.CAP


K28_KERNELS = ["k_grow_initE", "k_grow_tilesILi0ELb0EE", "k_grow_tilesILi0ELb1EE", "k_grow_tilesILi1ELb0EE", "k_grow_tilesILi1ELb1EE", "k_grow_tilesILi2ELb0EE",
               "k_grow_tilesILi2ELb1EE", "k_grow_sweepILi0EE", "k_grow_sweepILi1EE", "k_grow_sweepILi2EE", "k_grow_betweenILb0EE", "k_grow_betweenILb1EE", "k_grow_writeE"]
# the phase's values with their halo, the mask of tiles to wake (and its padding), and the 256 bytes that the workgroup reduction
# of __syncthreads_or takes: DESIGN.md section 32
TILE_LDS = 66 * 10 * 10 * 4 + 8 + 256


@pytest.mark.parametrize("kernel", K28_KERNELS)
def test_k28_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
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
    if "k_grow_tiles" in kernel:
        # The LDS would hold six workgroups a CU; that is not the attained occupancy: the registers hold it to four (at most 128
        # VGPRs, four waves a SIMD - DESIGN.md section 32, deviation (4)).  One register more than 128 and it is three.
        assert lds == TILE_LDS and 6 * lds <= 160 * 1024 < 7 * lds
        assert 96 < int(re.search(r"\.vgpr_count: +(\d+)", entry[0]).group(1)) <= 128
        assert "ds_read" in body and "global_atomic_swap" in atomics       # the relaxation reads LDS; the flag is an exchange
        assert not any("min" in a or "max" in a for a in atomics), atomics   # no atomic min or max: a voxel has one writer
    elif "k_grow_sweep" in kernel:
        assert lds == 0 and not any("min" in a or "max" in a for a in atomics), atomics      # a lane writes its own voxel only
    elif kernel == "k_grow_writeE":
        assert lds <= 64


def test_the_new_source_has_no_waiting_loop():
    """No kernel of K28 waits for another workgroup, lane or flag: nothing in the source polls or sleeps."""
    text = open(K28).read()
    kernels = text[text.index("// ---- kernels"):]
    assert "s_sleep" not in kernels and "while (" not in kernels and "__builtin_amdgcn_s_sleep" not in kernels
