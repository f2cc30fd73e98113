// o2v_dev_k20_geodesic.hpp -- K20: geodesic distances and shortest paths through a dense grid (o2v_hip_geodesic_dense /
// o2v_hip_geodesic_paths).  Included from o2v_device.hip inside its anonymous namespace, after K12 (whose classification it uses)
// and o2v_dev_bits.hpp (the bit grid, its words, tiles and walk).
//
// The set S is the bit grid of o2v_dev_bits.hpp, classified by K12's k_cc_classify.  D[i] is the
// distance of voxel i = (z * ny + y) * nx + x so far, a uint32: kGeoInf (0x7fffffff) where nothing has reached it - so for every
// voxel outside S, for good: a neighbour's D says by itself whether that neighbour is in S, and no pass but the owner's reads
// the bits.  d(v) is the least fixed point of D[v] = min(D[v], D[u] + w(u, v)) over the neighbours u of v, with the seeds at 0:
// unique, so the same bits under every schedule.  A value above max_distance is never stored: nothing goes through such a voxel.
//
//   hipMemsetD32Async      D = kGeoInf everywhere.
//   k_geo_seed_list / k_geo_seed_border   D = 0 at the seeds of S (listed; on the six faces of the box); their tiles, and the
//                   neighbour tiles that see a seed on their rim, flagged and listed for round 0.
//   k_geo_tiles     a workgroup per listed tile of 64 x 8 x 8 voxels: the tile's D with a halo of one voxel (66 x 10 x 10 uint32,
//                   kGeoInf outside the box) and its 64 row words in LDS; sweeps over the tile's voxels of S (a wavefront per
//                   row, a lane per voxel; rows of 66 dwords: the lanes of a row read consecutive banks) until a sweep changes
//                   nothing (__syncthreads_or); then only the voxels that decreased are stored, and where one of them lies on a
//                   face, edge or corner of the tile, the neighbour tiles that see it are flagged (one atomicExch per tile) and,
//                   if newly flagged, appended to the next round's list (one atomicAdd).
//   the host        reads the length of the next list (4 bytes) and launches the next round, until a list is empty.
//   k_geo_sweep     O2V_GEO_NO_TILES=1: a lane per voxel over the whole grid, atomicMin into D, a changed word per sweep; the
//                   host repeats it until a sweep changes nothing.  Same results: the cross-check and the baseline.
//   k_geo_write     dist(x, y, z) = D, or -1 for kGeoInf (and anything above max_distance); `reached` from one atomic per workgroup.
//   k_geo_trace     o2v_hip_geodesic_paths: a lane per target walks down the distances.
//
// Invariants.  D[i] is written only by the workgroup of the tile that owns i (k_geo_tiles), or by i's own lane (k_geo_sweep).
// A tile is in a round's list at most once: the flag words of two rounds alternate, a tile clears its own word of the round that
// runs, its neighbours set its word of the round that follows.  Values only decrease, so a halo read that races with the
// neighbour's store - or comes from a stale cache line - reads a valid upper bound, and the neighbour's flag brings the tile back
// in a later launch, which reads what the earlier one stored.  No kernel waits for another workgroup, lane or flag: every launch
// ends on its own, every loop ends because a distance strictly decreased or a sweep changed nothing; there is no round cap.

constexpr uint32_t kGeoInf = 0x7fffffffu;           // not reached (yet); never a distance
constexpr uint32_t kGeoMaxDistance = 0x7ffffffeu;   // the largest max_distance
constexpr uint32_t kGeoMaxWeight = 65535u;
constexpr uint32_t kGeoRowStride = 66u, kGeoLayerStride = 660u, kGeoHalo = 6600u;   // the tile with its halo: 66 (x) x 10 (y) x 10 (z)
// every d + w of a relaxation fits a uint32: d <= kGeoInf and w <= kGeoMaxWeight
static_assert((uint64_t) kGeoInf + kGeoMaxWeight <= 0xffffffffull && kGeoMaxDistance < kGeoInf, "d + w must not wrap");

#ifndef O2V_GEO_HOST
#define O2V_GEO_FN __device__ __forceinline__
#endif

// ---- the relaxation, the tiles that see a voxel, the trace step ------------------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_geodesic.py compiles this part for the host, with an O2V_GEO_FN of its
// own, runs it tile by tile in a shuffled order and as whole-grid sweeps against the reference, and checks that one change is caught.)

struct GeoGrid : BitGrid {
    uint32_t tiles_y, tiles_z;   // ceil(ny / 8), ceil(nz / 8); tiles along x: W
    uint32_t w[3];               // the cost of a step that differs on 1, 2, 3 axes; 0: no such step
    uint32_t max_distance;
};

// The 26 offsets in ascending (dz, dy, dx) order: k = 0 .. 26 without 13.
O2V_GEO_FN int geo_dx(int k) { return k % 3 - 1; }
O2V_GEO_FN int geo_dy(int k) { return k / 3 % 3 - 1; }
O2V_GEO_FN int geo_dz(int k) { return k / 9 - 1; }
O2V_GEO_FN int geo_axes(int k) { return (geo_dx(k) != 0) + (geo_dy(k) != 0) + (geo_dz(k) != 0); }

// (test only: the offset (+1, +1, -1) left out)
O2V_GEO_FN bool geo_dropped(int k)
{
#ifdef O2V_GEO_MUTATE_DROP_CORNER
    return geo_dx(k) == 1 && geo_dy(k) == 1 && geo_dz(k) == -1;
#else
    (void) k;
    return false;
#endif
}

// The new distance of the voxel at d[0], from an array in which every neighbour has an element - x, y, z strides 1, sy, sz -
// that holds kGeoInf where the neighbour is not in S or not in the box (the tile with its halo).  d + w <= 0x7fffffff + 65535
// fits a uint32 (the static_assert above); a value above max_distance is not taken.
O2V_GEO_FN uint32_t geo_relax(const uint32_t *d, int sy, int sz, const uint32_t w[3], uint32_t max_distance)
{
    const uint32_t old = d[0];
    uint32_t best = old;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        if (k == 13 || geo_dropped(k)) continue;
        const uint32_t wk = w[geo_axes(k) - 1];
        if (!wk) continue;
        const uint32_t c = d[geo_dz(k) * sz + geo_dy(k) * sy + geo_dx(k)] + wk;
        best = c < best ? c : best;
    }
    return best <= max_distance ? best : old;
}

// The same for voxel (x, y, z) of the whole grid D (O2V_GEO_NO_TILES): the neighbours outside the box are left out.
O2V_GEO_FN uint32_t geo_relax_grid(const GeoGrid &g, const uint32_t *D, uint32_t x, uint32_t y, uint32_t z)
{
    const uint32_t i = (z * g.ny + y) * g.nx + x, old = D[i];
    uint32_t best = old;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        if (k == 13 || geo_dropped(k)) continue;
        const uint32_t wk = g.w[geo_axes(k) - 1];
        if (!wk) continue;
        const uint32_t X = x + (uint32_t) geo_dx(k), Y = y + (uint32_t) geo_dy(k), Z = z + (uint32_t) geo_dz(k);   // (-1 wraps to above any dim)
        if (X >= g.nx || Y >= g.ny || Z >= g.nz) continue;
        const uint32_t c = D[(Z * g.ny + Y) * g.nx + X] + wk;
        best = c < best ? c : best;
    }
    return best <= g.max_distance ? best : old;
}

// Which neighbour tiles see voxel (x, y, z) of a tile (0 .. 63, 0 .. 7, 0 .. 7): bit k for the tile at offset (geo_dx(k),
// geo_dy(k), geo_dz(k)).  That tile holds the voxel in its halo if the voxel lies on the tile's side towards it on every axis
// of the offset, and it can be reached from the voxel if a step that differs on at least those axes has a weight.  (Tiles
// outside the grid are the caller's to leave out.)
O2V_GEO_FN uint32_t geo_see_mask(uint32_t x, uint32_t y, uint32_t z, const uint32_t w[3])
{
    const uint32_t on_x = (x == 0u ? 1u : 0u) | 2u | (x == 63u ? 4u : 0u);   // bit d + 1: on the side towards offset d
    const uint32_t on_y = (y == 0u ? 1u : 0u) | 2u | (y == 7u ? 4u : 0u);
    const uint32_t on_z = (z == 0u ? 1u : 0u) | 2u | (z == 7u ? 4u : 0u);
    const bool step[3] = {(w[0] | w[1] | w[2]) != 0u, (w[1] | w[2]) != 0u, w[2] != 0u};   // a step over at least 1, 2, 3 axes
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        if (k == 13 || !step[geo_axes(k) - 1]) continue;
        if (((on_x >> (geo_dx(k) + 1)) & (on_y >> (geo_dy(k) + 1)) & (on_z >> (geo_dz(k) + 1)) & 1u) != 0u) m |= 1u << k;
    }
    return m;
}

// One step of the walk back from voxel (x, y, z) with dist = dv > 0: the first offset k in ascending (dz, dy, dx) order, among
// the step kinds with a weight, whose voxel u is in the box with dist[u] >= 0 and dist[u] + w == dv; -1 if there is none.
O2V_GEO_FN int geo_trace_step(const int32_t *dist, uint64_t s0, uint64_t s1, uint64_t s2, const uint32_t dims[3], const uint32_t w[3], uint32_t x,
                              uint32_t y, uint32_t z, int32_t dv)
{
    for (int k = 0; k < 27; ++k) {
        if (k == 13) continue;
        const uint32_t wk = w[geo_axes(k) - 1];
        if (!wk) continue;
        const uint32_t X = x + (uint32_t) geo_dx(k), Y = y + (uint32_t) geo_dy(k), Z = z + (uint32_t) geo_dz(k);
        if (X >= dims[0] || Y >= dims[1] || Z >= dims[2]) continue;
        const int32_t du = dist[X * s0 + Y * s1 + Z * s2];
        if (du >= 0 && (uint32_t) du + wk == (uint32_t) dv) return k;
    }
    return -1;
}

// The walk of one target (include/o2v_hip.h): the length of its path, -1 or -2; the first min(length, max_len) voxels to path.
O2V_GEO_FN int32_t geo_trace(const int32_t *dist, uint64_t s0, uint64_t s1, uint64_t s2, const uint32_t dims[3], const uint32_t w[3], int32_t tx,
                             int32_t ty, int32_t tz, uint32_t max_len, int32_t *path)
{
    uint32_t x = (uint32_t) tx, y = (uint32_t) ty, z = (uint32_t) tz;
    if (x >= dims[0] || y >= dims[1] || z >= dims[2]) return -1;
    int32_t dv = dist[x * s0 + y * s1 + z * s2];
    if (dv < 0) return -1;
    for (uint32_t n = 0;; ++n) {   // (ends: dv strictly decreases, every weight tried is above 0)
        if (n < max_len) path[3u * n] = (int32_t) x, path[3u * n + 1u] = (int32_t) y, path[3u * n + 2u] = (int32_t) z;
        if (dv == 0) return (int32_t) (n + 1u);
        const int k = geo_trace_step(dist, s0, s1, s2, dims, w, x, y, z, dv);
        if (k < 0) return -2;
        x += (uint32_t) geo_dx(k), y += (uint32_t) geo_dy(k), z += (uint32_t) geo_dz(k);
        dv -= (int32_t) w[geo_axes(k) - 1];
    }
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_GEO_HOST

// the tile's word of round 0; a tile flagged for the first time goes to the list
__device__ __forceinline__ void geo_flag_tile(uint32_t tile, uint32_t *flags, uint32_t *list, uint32_t *count)
{
    if (cc_load(flags + tile) == 0u && atomicExch(flags + tile, 1u) == 0u) list[atomicAdd(count, 1u)] = tile;
}

// A seed wakes its own tile and the neighbour tiles that see it (bit k of see, geo_see_mask): a seed is at 0 from the start
// and never decreases, so no round would tell them.
__device__ __forceinline__ void geo_flag_seed(const GeoGrid &g, uint32_t tx, uint32_t ty, uint32_t tz, uint32_t see, uint32_t *flags, uint32_t *list,
                                              uint32_t *count)
{
    see |= 1u << 13;
    for (int k = 0; k < 27; ++k) {
        if (!((see >> k) & 1u)) continue;
        const uint32_t X = tx + (uint32_t) geo_dx(k), Y = ty + (uint32_t) geo_dy(k), Z = tz + (uint32_t) geo_dz(k);   // (-1 wraps to above any count)
        if (X < g.W && Y < g.tiles_y && Z < g.tiles_z) geo_flag_tile((Z * g.tiles_y + Y) * g.W + X, flags, list, count);
    }
}

// the listed seeds: D = 0 where the seed is in the box and in S (flags null: no tiles to wake)
__global__ __launch_bounds__(kBlock) void k_geo_seed_list(GeoGrid g, const unsigned long long *__restrict__ bits, const int32_t *__restrict__ seeds,
                                                          uint64_t n, uint32_t *D, uint32_t *flags, uint32_t *list, uint32_t *count)
{
    for (uint64_t s = (uint64_t) blockIdx.x * kBlock + threadIdx.x; s < n; s += (uint64_t) gridDim.x * kBlock) {
        const uint32_t x = (uint32_t) seeds[s * 3u], y = (uint32_t) seeds[s * 3u + 1u], z = (uint32_t) seeds[s * 3u + 2u];
        if (x >= g.nx || y >= g.ny || z >= g.nz) continue;   // (a negative coordinate is above any dim)
        if (!bits_has(g, bits, x, y, z)) continue;
        D[(z * g.ny + y) * g.nx + x] = 0u;
        if (flags) geo_flag_seed(g, x >> 6, y >> 3, z >> 3, geo_see_mask(x & 63u, y & 7u, z & 7u, g.w), flags, list, count);
    }
}

// The seeds of one word - a row of tile (tx, ty, tz) -, each lane with the see mask of its own (0: no seed): the masks or-ed over
// the wavefront, lane 0 wakes the tiles.
__device__ __forceinline__ void geo_wake_row(const GeoGrid &g, uint32_t tx, uint32_t ty, uint32_t tz, uint32_t see, uint32_t *flags, uint32_t *list,
                                             uint32_t *count)
{
    for (int d = 32; d >= 1; d >>= 1) see |= __shfl_xor(see, d);
    if ((threadIdx.x & 63u) == 0u) geo_flag_seed(g, tx, ty, tz, see, flags, list, count);
}

// O2V_HIP_CC_SEED_BORDER: D = 0 at the voxels of S on the six faces of the box
__global__ __launch_bounds__(kBlock) void k_geo_seed_border(GeoGrid g, const unsigned long long *__restrict__ bits, uint32_t *D, uint32_t *flags,
                                                            uint32_t *list, uint32_t *count)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t wx = at.wx, x = wx * 64u + lane, y = at.y, z = at.z;
        const bool seed = bits_on_face(g, x, y, z) && x < g.nx && ((bits[wi] >> lane) & 1ull);
        if (seed) D[(z * g.ny + y) * g.nx + x] = 0u;
        if (__ballot(seed) == 0ull || !flags) continue;
        geo_wake_row(g, wx, y >> 3, z >> 3, seed ? geo_see_mask(lane, y & 7u, z & 7u, g.w) : 0u, flags, list, count);   // (the word is one row of one tile)
    }
}

// One round: the tiles list[0, n_list), their flag words flags_cur; what they wake goes to flags_next, list_next and *count_next.
// sweeps (Count: O2V_HIP_FLAG_STAGE_TIMES) += the in-tile sweeps.
template <bool Count>
__global__ __launch_bounds__(kBlock) void k_geo_tiles(GeoGrid g, const unsigned long long *__restrict__ bits, uint32_t *D, const uint32_t *__restrict__ list,
                                                      uint32_t n_list, uint32_t *flags_cur, uint32_t *flags_next, uint32_t *list_next,
                                                      uint32_t *count_next, unsigned long long *sweeps)
{
    __shared__ uint32_t s_d[kGeoHalo];
    __shared__ uint64_t s_w[kCcTileRows];
    __shared__ uint32_t s_see;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x) {
        const uint32_t tile = list[li];
        uint32_t tx, ty, tz;
        bits_tile_at(g, g.tiles_y, tile, tx, ty, tz);
        const uint32_t x0 = tx * 64u, y0 = ty * 8u, z0 = tz * 8u;
        __syncthreads();   // (the last tile's words and distances are no longer read)
        if (threadIdx.x == 0) flags_cur[tile] = 0u, s_see = 0u;   // (nothing else touches this round's word in this launch)
        if (threadIdx.x < kCcTileRows) s_w[threadIdx.x] = bits_tile_word(g, bits, tx, ty, tz, threadIdx.x);
        // the tile and its halo: 100 rows of 66, kGeoInf outside the box (D holds it outside S)
        for (uint32_t row = wave; row < 100u; row += kBlock / 64u) {
            const uint32_t Y = y0 + row % 10u - 1u, Z = z0 + row / 10u - 1u;   // (-1 wraps to above any dim)
            const bool in_box = Y < g.ny && Z < g.nz;
            const uint32_t *const src = D + (in_box ? ((uint64_t) Z * g.ny + Y) * g.nx : 0ull);
            const uint32_t X = x0 + lane;
            s_d[row * kGeoRowStride + 1u + lane] = in_box && X < g.nx ? cc_load(src + X) : kGeoInf;
            if (lane < 2u) {
                const uint32_t Xe = lane ? x0 + 64u : x0 - 1u;
                s_d[row * kGeoRowStride + (lane ? 65u : 0u)] = in_box && Xe < g.nx ? cc_load(src + Xe) : kGeoInf;
            }
        }
        __syncthreads();
        // Sweeps in place: a read may see a neighbour's value of this sweep or of the last one, both upper bounds that some
        // path gives; the fixed point is the one of the header.
        uint32_t changed = 0, n_sweeps = 0;   // bit k: the voxel of row wave + 4 k decreased
        for (;;) {
            int any = 0;
            for (uint32_t k = 0; k < 16u; ++k) {
                const uint32_t row = wave + 4u * k;
                if (!((s_w[row] >> lane) & 1ull)) continue;
                uint32_t *const p = s_d + ((row >> 3) + 1u) * kGeoLayerStride + ((row & 7u) + 1u) * kGeoRowStride + 1u + lane;
                const uint32_t d = geo_relax(p, (int) kGeoRowStride, (int) kGeoLayerStride, g.w, g.max_distance);
                if (d < *p) *p = d, changed |= 1u << k, any = 1;
            }
            ++n_sweeps;
            if (!__syncthreads_or(any)) break;
        }
        // only this tile's voxels, and only those that decreased
        uint32_t see = 0;
        for (uint32_t k = 0; k < 16u; ++k) {
            if (!((changed >> k) & 1u)) continue;
            const uint32_t row = wave + 4u * k, y = row & 7u, z = row >> 3;
            cc_store(D + ((uint64_t) (z0 + z) * g.ny + (y0 + y)) * g.nx + (x0 + lane), s_d[(z + 1u) * kGeoLayerStride + (y + 1u) * kGeoRowStride + 1u + lane]);
            see |= geo_see_mask(lane, y, z, g.w);
        }
        for (int d = 32; d >= 1; d >>= 1) see |= __shfl_xor(see, d);
        if (lane == 0u && see) atomicOr(&s_see, see);
        __syncthreads();
        if (threadIdx.x < 27u && ((s_see >> threadIdx.x) & 1u)) {
            const uint32_t X = tx + (uint32_t) geo_dx((int) threadIdx.x), Y = ty + (uint32_t) geo_dy((int) threadIdx.x), Z = tz + (uint32_t) geo_dz((int) threadIdx.x);
            if (X < g.W && Y < g.tiles_y && Z < g.tiles_z) {
                const uint32_t t = (Z * g.tiles_y + Y) * g.W + X;
                __threadfence();   // the stores above before the flag (the next launch would see them anyway)
                if (atomicExch(flags_next + t, 1u) == 0u) list_next[atomicAdd(count_next, 1u)] = t;
            }
        }
        if (Count && threadIdx.x == 0) atomicAdd(sweeps, (unsigned long long) n_sweeps);
    }
}

// O2V_GEO_NO_TILES: one sweep over the whole grid; *changed = 1 if a distance decreased
__global__ __launch_bounds__(kBlock) void k_geo_sweep(GeoGrid g, const unsigned long long *__restrict__ bits, uint32_t *D, uint32_t *changed)
{
    const uint32_t lane = threadIdx.x & 63u;
    bool any = false;
    for (const uint64_t wi : bits_words(g)) {
        const unsigned long long w = bits[wi];
        if (!((w >> lane) & 1ull)) continue;
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z, i = (z * g.ny + y) * g.nx + x;
        const uint32_t d = geo_relax_grid(g, D, x, y, z);
        if (d < D[i]) atomicMin(D + i, d), any = true;
    }
    if (__ballot(any) != 0ull && lane == 0u) atomicOr(changed, 1u);
}

// dist(x, y, z) = D, -1 for kGeoInf and for anything above max_distance; *reached += the voxels with a distance
__global__ __launch_bounds__(kBlock) void k_geo_write(GeoGrid g, const uint32_t *D, int32_t *dist, uint64_t s0, uint64_t s1, uint64_t s2,
                                                      unsigned long long *reached)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long mine = 0;   // (the same in every lane of the wavefront)
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z;
        bool hit = false;
        if (x < g.nx) {
            const uint32_t d = D[(z * g.ny + y) * g.nx + x];   // (D may be dist itself: a lane reads its own element, then writes it)
            hit = d <= g.max_distance;
            dist[(uint64_t) x * s0 + (uint64_t) y * s1 + (uint64_t) z * s2] = hit ? (int32_t) d : -1;
        }
        mine += (unsigned long long) __popcll(__ballot(hit));
    }
    bits_add_wave_sums(mine, reached);
}

struct GeoTrace {
    uint32_t dims[3], w[3];
    uint64_t s[3];
};

// o2v_hip_geodesic_paths: a lane per target; latency-bound and tiny
__global__ __launch_bounds__(kBlock) void k_geo_trace(GeoTrace t, const int32_t *__restrict__ dist, const int32_t *__restrict__ targets, uint64_t n,
                                                      uint32_t max_len, int32_t *__restrict__ paths, int32_t *__restrict__ lengths)
{
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock)
        lengths[i] = geo_trace(dist, t.s[0], t.s[1], t.s[2], t.dims, t.w, targets[i * 3u], targets[i * 3u + 1u], targets[i * 3u + 2u], max_len,
                               paths + i * 3u * max_len);
}

#endif   // O2V_GEO_HOST
