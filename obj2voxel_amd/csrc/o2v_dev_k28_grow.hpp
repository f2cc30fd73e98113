// o2v_dev_k28_grow.hpp -- K28: seeded watershed, markers grown through a relief (o2v_hip_grow_dense).  Included from
// o2v_device.hip inside its anonymous namespace, after K20 (its offsets, see masks, tile flags and limits) and the pair table
// (I32View).
//
// The definition (include/o2v_hip.h, tests/grow_ref.py).  H is an int32 relief, S = { v : H[v] > 0 }; a voxel of S with M[v] > 0
// is a seed.  Every voxel of S gets a key (Q, T) - level and ticks -, better with a higher Q, then with a lower T.  A seed has
// (H, 0); a step of weight w from u to v turns (Q, T) into (H[v], 0) if H[v] < Q, else into (Q, min(T + w, 2^31 - 2)).  The best
// fixed point is unique and splits into three 32-bit fixed points, each final before the next starts:
//   level   Q(v) = max(seed ? H[v] : 0, max_u min(Q(u), H[v])), from 0, only rising;
//   ticks   T(v) = 0 for a seed or a voxel with a neighbour u of Q(u) > H[v] (a source), else the min over the neighbours u with
//           Q(u) == Q(v) of min(T(u) + w, 2^31 - 2), from kGeoInf, only falling;
//   label   a seed keeps M[v]; every other reached voxel takes the smallest L(u) over its tight neighbours - Q(u) > H[v], or Q(u)
//           == Q(v) and min(T(u) + w, cap) == T(v) -, from 0xffffffff, only falling.
// Q, T, L are uint32 arrays with linear index i = (z * ny + y) * nx + x: the caller's level, ticks and labels where those are
// contiguous, else scratch.  mask is 4 bytes per voxel of scratch: bit k (K20's offset order) says that the neighbour at offset k
// takes part in the voxel's relaxation - for the ticks the neighbours of equal level, for the labels the tight ones; 0 for a voxel
// that never changes (outside S, not reached, a seed, a source of the ticks).
//
//   k_grow_init      Q = H at the seeds, 0 elsewhere; the seeds' tiles and the tiles that see them listed for round 0 of the level.
//   k_grow_tiles<0>  level: a workgroup per listed tile of 64 x 8 x 8 voxels; Q with a halo of one voxel in LDS (66 x 10 x 10 uint32,
//                    26 400 bytes, 0 outside the box), the lane's 16 own max(H, 0) in registers; sweeps in place until nothing
//                    rose (__syncthreads_or); the voxels that rose are stored, the tiles that see them flagged and listed.
//   k_grow_between<false>   a lane per voxel: T = 0 at seeds and sources, kGeoInf elsewhere; the mask of the neighbours of equal level;
//                    every tile with a reached voxel listed for round 0 of the ticks.
//   k_grow_tiles<1>  ticks: T with halo in LDS (kGeoInf outside the box), the lane's 16 masks in registers; falling.
//   k_grow_between<true>    a lane per voxel: the mask of the tight neighbours; L = M at the seeds, 0xffffffff elsewhere; the tiles with a
//                    reached voxel listed for round 0 of the labels.
//   k_grow_tiles<2>  labels: L with halo in LDS (0xffffffff outside the box), the lane's 16 masks in registers; falling.
//   k_grow_sweep<P>  O2V_GROW_NO_TILES=1: a lane per voxel over the whole grid, the neighbours from global memory, a changed word
//                    per sweep; the host repeats it until a sweep changes nothing.  Same results: the cross-check and the baseline.
//   k_grow_write     labels / level / ticks through their strides: 0 / 0 / -1 outside S and where not reached; `reached` from one
//                    atomic per workgroup.
//
// Invariants (K20's).  A voxel's Q, T, L and mask are written only by the workgroup of its tile (k_grow_tiles), or by its own lane
// (the streaming passes and k_grow_sweep).  A tile is in a round's list at most once: the flag words of two rounds alternate, a tile
// clears its own word of the round that runs, its neighbours set its word of the round that follows.  Within a phase values move
// one way only, so a halo read that races with the neighbour's store reads a valid bound, and the neighbour's flag brings the tile
// back in a later launch.  A phase starts only after the one before it has reached its fixed point: the host has read an empty
// list (or a clear changed word).  No kernel waits for another workgroup; there is no persistent kernel and no round cap.

constexpr uint32_t kGrowCap = 0x7ffffffeu;        // where the ticks saturate
constexpr uint32_t kGrowNoLabel = 0xffffffffu;    // L of a voxel no label has reached (yet): above every label
// every T + w of a relaxation fits a uint32: T <= kGeoInf and w <= kGeoMaxWeight
static_assert((uint64_t) kGeoInf + kGeoMaxWeight <= 0xffffffffull && kGrowCap < kGeoInf && kGrowCap == kGeoMaxDistance, "T + w must not wrap");

#ifndef O2V_GROW_HOST
#define O2V_GROW_FN __device__ __forceinline__
O2V_GROW_FN uint32_t grow_load(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
O2V_GROW_FN void grow_store(uint32_t *p, uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
#endif

// ---- the lane bodies ----------------------------------------------------------------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_grow.py compiles this part for the host behind K20's plain part, with
// O2V_GROW_FN, grow_load and grow_store of its own, runs it tile by tile in a shuffled order and as whole-grid sweeps against the
// reference and checks that two changes are caught.)
//
// Every body looks at the voxel at p[0] of an array in which the neighbour at offset k is p[dz * sz + dy * sy + dx]: the tile with
// its halo in LDS (sy = 66, sz = 660: every neighbour has an element) or the whole grid (sy = nx, sz = nx * ny: `box` says which
// neighbours are in the box, grow_box_mask).  Only step kinds with a weight are looked at.

O2V_GROW_FN int64_t grow_off(int k, int64_t sy, int64_t sz) { return geo_dz(k) * sz + geo_dy(k) * sy + geo_dx(k); }

// bit k: the neighbour at offset k of voxel (x, y, z) is in the box
O2V_GROW_FN uint32_t grow_box_mask(const BitGrid &g, uint32_t x, uint32_t y, uint32_t z)
{
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        if (k == 13) continue;
        const uint32_t X = x + (uint32_t) geo_dx(k), Y = y + (uint32_t) geo_dy(k), Z = z + (uint32_t) geo_dz(k);   // (-1 wraps to above any dim)
        if (X < g.nx && Y < g.ny && Z < g.nz) m |= 1u << k;
    }
    return m;
}

// level: the new Q of a voxel of S with relief h > 0 (0 stands for "not in S" and "not reached" alike, so a neighbour's Q says
// everything about it)
O2V_GROW_FN uint32_t grow_level_relax(const uint32_t *q, int64_t sy, int64_t sz, const uint32_t w[3], uint32_t h, uint32_t box)
{
    uint32_t best = 0;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        if (k == 13 || !w[geo_axes(k) - 1] || !((box >> k) & 1u)) continue;
        const uint32_t c = grow_load(q + grow_off(k, sy, sz));
        best = c > best ? c : best;
    }
    best = best < h ? best : h;
    const uint32_t old = q[0];
    return best > old ? best : old;
}

// sources: T at the start of the ticks (0 for a seed and for a voxel with a neighbour of Q(u) > h, else kGeoInf) and *mask, the
// neighbours of equal level that the ticks relax over (0 where T is final from the start).  q[0] = 0: not reached.
O2V_GROW_FN uint32_t grow_sources(const uint32_t *q, int64_t sy, int64_t sz, const uint32_t w[3], uint32_t h, bool seed, uint32_t box, uint32_t *mask)
{
    const uint32_t own = q[0];
    uint32_t m = 0;
    bool source = seed;
    *mask = 0;
    if (!own) return kGeoInf;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        if (k == 13 || !w[geo_axes(k) - 1] || !((box >> k) & 1u)) continue;
        const uint32_t c = q[grow_off(k, sy, sz)];
#ifndef O2V_GROW_MUTATE_NO_RESET   // (test only: a descent does not restart the clock)
        source = source || c > h;
#endif
        if (c == own) m |= 1u << k;
    }
    if (source) return 0u;
    *mask = m;
    return kGeoInf;
}

// one step of the clock over a weight above 0
O2V_GROW_FN uint32_t grow_tick_step(uint32_t t, uint32_t wk)
{
    const uint32_t c = t + wk;
    return c < kGrowCap ? c : kGrowCap;
}

// ticks: the new T of a voxel with the mask of grow_sources
O2V_GROW_FN uint32_t grow_tick_relax(const uint32_t *t, int64_t sy, int64_t sz, const uint32_t w[3], uint32_t mask)
{
    uint32_t best = t[0];
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        if (k == 13 || !((mask >> k) & 1u)) continue;
        const uint32_t c = grow_tick_step(grow_load(t + grow_off(k, sy, sz)), w[geo_axes(k) - 1]);
        best = c < best ? c : best;
    }
    return best;
}

// tight: the neighbours whose step gives exactly the voxel's key; 0 for a seed and for a voxel that was not reached
O2V_GROW_FN uint32_t grow_tight_mask(const uint32_t *q, const uint32_t *t, int64_t sy, int64_t sz, const uint32_t w[3], uint32_t h, bool seed, uint32_t box)
{
    const uint32_t own_q = q[0], own_t = t[0];
    uint32_t m = 0;
    if (!own_q || seed) return 0u;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        const uint32_t wk = k == 13 ? 0u : w[geo_axes(k) - 1];
        if (!wk || !((box >> k) & 1u)) continue;
        const int64_t o = grow_off(k, sy, sz);
        const uint32_t c = q[o];
        if (c > h || (c == own_q && grow_tick_step(t[o], wk) == own_t)) m |= 1u << k;
    }
    return m;
}

// labels: the new L of a voxel with the mask of grow_tight_mask
O2V_GROW_FN uint32_t grow_label_relax(const uint32_t *l, int64_t sy, int64_t sz, uint32_t mask)
{
    uint32_t best = l[0];
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        if (k == 13 || !((mask >> k) & 1u)) continue;
        const uint32_t c = grow_load(l + grow_off(k, sy, sz));
        best = c < best ? c : best;
    }
    return best;
}

// One relaxation of phase P (0 level, 1 ticks, 2 labels) of the voxel at p[0]; own: max(H, 0) for the level, else the mask.
// 0 in own: the voxel never changes.
template <int P>
O2V_GROW_FN uint32_t grow_relax(const uint32_t *p, int64_t sy, int64_t sz, const uint32_t w[3], uint32_t own, uint32_t box)
{
    if (P == 0) return grow_level_relax(p, sy, sz, w, own, box);
    if (P == 1) return grow_tick_relax(p, sy, sz, w, own);
    return grow_label_relax(p, sy, sz, own);
}

// what a phase's array holds outside the box: the value that never wins
template <int P>
O2V_GROW_FN uint32_t grow_outside()
{
    return P == 0 ? 0u : P == 1 ? kGeoInf : kGrowNoLabel;
}

#ifdef O2V_GROW_MUTATE_LABEL_IN_KEY
// (test only, host only: the smallest label taken inside the comparison of the ticks instead of in a phase of its own.  One
// relaxation of the packed pair T << 32 | L of a reached voxel that is no seed: (0, L(u)) from a neighbour of Q(u) > h - bit k of
// `higher` -, (min(T(u) + w, cap), L(u)) from a neighbour of equal level - bit k of `same` -, the smallest of them and the old
// pair.  A neighbour's pair can fall from (3, 1) to (2, 7): what it gave while it held the 1 stays, so the step is not monotone
// and the result depends on the order of the visits.  tests/test_host_grow.py sees it differ from the reference.)
O2V_GROW_FN uint32_t grow_higher_mask(const uint32_t *q, int64_t sy, int64_t sz, const uint32_t w[3], uint32_t h, uint32_t box)
{
    uint32_t m = 0;
    for (int k = 0; k < 27; ++k) {
        if (k == 13 || !w[geo_axes(k) - 1] || !((box >> k) & 1u)) continue;
        if (q[grow_off(k, sy, sz)] > h) m |= 1u << k;
    }
    return m;
}

O2V_GROW_FN uint64_t grow_joint_relax(const uint64_t *p, int64_t sy, int64_t sz, const uint32_t w[3], uint32_t same, uint32_t higher)
{
    uint64_t best = p[0];
    for (int k = 0; k < 27; ++k) {
        if (k == 13 || !(((same | higher) >> k) & 1u)) continue;
        const uint64_t u = p[grow_off(k, sy, sz)];
        const uint32_t t = ((higher >> k) & 1u) ? 0u : grow_tick_step((uint32_t) (u >> 32), w[geo_axes(k) - 1]);
        const uint64_t c = (uint64_t) t << 32 | (uint32_t) u;
        best = c < best ? c : best;
    }
    return best;
}
#endif

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_GROW_HOST

constexpr uint32_t kGrowAllInBox = 0x7ffffffu;   // every neighbour has an element: the tile with its halo

// the tile of word (wx, y, z): a word is one row of one tile
__device__ __forceinline__ uint32_t grow_tile_of(const GeoGrid &g, const BitWord &at) { return ((at.z >> 3) * g.tiles_y + (at.y >> 3)) * g.W + at.wx; }

// Q = H at the seeds, 0 elsewhere; flags != null: the seeds' tiles and the tiles that see them go to round 0's list (a seed
// never rises, so no round would tell them)
__global__ __launch_bounds__(kBlock) void k_grow_init(GeoGrid g, I32View H, I32View M, uint32_t *Q, uint32_t *flags, uint32_t *list, uint32_t *count)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z;
        bool seed = false;
        if (x < g.nx) {
            const int32_t h = H.at(x, y, z);
            seed = h > 0 && M.at(x, y, z) > 0;
            Q[((uint64_t) z * g.ny + y) * g.nx + x] = seed ? (uint32_t) h : 0u;
        }
        if (__ballot(seed) == 0ull || !flags) continue;
        geo_wake_row(g, at.wx, y >> 3, z >> 3, seed ? geo_see_mask(lane, y & 7u, z & 7u, g.w) : 0u, flags, list, count);
    }
}

// One round of phase P: the tiles list[0, n_list), their flag words flags_cur; what they wake goes to flags_next, list_next and
// *count_next.  V: the phase's array (Q, T or L); own: the relief (P = 0) or the mask.  sweeps (Count) += the in-tile sweeps.
template <int P, bool Count>
__global__ __launch_bounds__(kBlock) void k_grow_tiles(GeoGrid g, I32View H, const uint32_t *__restrict__ mask, uint32_t *V, const uint32_t *__restrict__ list,
                                                       uint32_t n_list, uint32_t *flags_cur, uint32_t *flags_next, uint32_t *list_next, uint32_t *count_next,
                                                       unsigned long long *sweeps)
{
    __shared__ uint32_t s_v[kGeoHalo];
    __shared__ uint32_t s_see;
    const uint32_t outside = grow_outside<P>();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x) {
        const uint32_t tile = list[li];
        uint32_t tx, ty, tz;
        bits_tile_at(g, g.tiles_y, tile, tx, ty, tz);
        const uint32_t x0 = tx * 64u, y0 = ty * 8u, z0 = tz * 8u;
        __syncthreads();   // (the last tile's values are no longer read)
        if (threadIdx.x == 0) flags_cur[tile] = 0u, s_see = 0u;   // (nothing else touches this round's word in this launch)
        // the tile and its halo: 100 rows of 66
        for (uint32_t row = wave; row < 100u; row += kBlock / 64u) {
            const uint32_t Y = y0 + row % 10u - 1u, Z = z0 + row / 10u - 1u;   // (-1 wraps to above any dim)
            const bool in_box = Y < g.ny && Z < g.nz;
            const uint32_t *const src = V + (in_box ? ((uint64_t) Z * g.ny + Y) * g.nx : 0ull);
            const uint32_t X = x0 + lane;
            s_v[row * kGeoRowStride + 1u + lane] = in_box && X < g.nx ? grow_load(src + X) : outside;
            if (lane < 2u) {
                const uint32_t Xe = lane ? x0 + 64u : x0 - 1u;
                s_v[row * kGeoRowStride + (lane ? 65u : 0u)] = in_box && Xe < g.nx ? grow_load(src + Xe) : outside;
            }
        }
        // the lane's own 16 voxels, rows wave + 4 k: their relief or mask, 0 for "never changes" and outside the box
        uint32_t own[16];
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint32_t row = wave + 4u * k, x = x0 + lane, y = y0 + (row & 7u), z = z0 + (row >> 3);
            own[k] = 0u;
            if (x < g.nx && y < g.ny && z < g.nz) {
                if (P == 0) {
                    const int32_t h = H.at(x, y, z);
                    own[k] = h > 0 ? (uint32_t) h : 0u;
                } else {
                    own[k] = mask[((uint64_t) z * g.ny + y) * g.nx + x];
                }
            }
        }
        __syncthreads();
        // Sweeps in place: a read may see a neighbour's value of this sweep or of the last one, both bounds that some path gives.
        uint32_t changed = 0, n_sweeps = 0;   // bit k: the voxel of row wave + 4 k moved
        for (;;) {
            int any = 0;
            // (one body for the 16 voxels: the registers take a turn per voxel, so that own[0] is always this one's.  116 - 124
            // VGPRs, four workgroups a CU; 16 unrolled copies of the body take 144 for the ticks and the labels: three.)
#pragma unroll 1
            for (uint32_t k = 0; k < 16u; ++k) {
                const uint32_t mine = own[0];
#pragma unroll
                for (uint32_t j = 0; j < 15u; ++j) own[j] = own[j + 1u];
                own[15] = mine;
                if (!mine) continue;
                const uint32_t row = wave + 4u * k;
                uint32_t *const p = s_v + ((row >> 3) + 1u) * kGeoLayerStride + ((row & 7u) + 1u) * kGeoRowStride + 1u + lane;
                const uint32_t v = grow_relax<P>(p, (int64_t) kGeoRowStride, (int64_t) kGeoLayerStride, g.w, mine, kGrowAllInBox);
                if (v != *p) grow_store(p, v), changed |= 1u << k, any = 1;
            }
            ++n_sweeps;
            if (!__syncthreads_or(any)) break;
        }
        // only this tile's voxels, and only those that moved
        uint32_t see = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            if (!((changed >> k) & 1u)) continue;
            const uint32_t row = wave + 4u * k, y = row & 7u, z = row >> 3;
            grow_store(V + ((uint64_t) (z0 + z) * g.ny + (y0 + y)) * g.nx + (x0 + lane), s_v[(z + 1u) * kGeoLayerStride + (y + 1u) * kGeoRowStride + 1u + lane]);
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

// O2V_GROW_NO_TILES: one sweep of phase P over the whole grid; *changed = 1 if a value moved.  A lane writes its own voxel only.
template <int P>
__global__ __launch_bounds__(kBlock) void k_grow_sweep(GeoGrid g, I32View H, const uint32_t *__restrict__ mask, uint32_t *V, uint32_t *changed)
{
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t sy = g.nx, sz = (int64_t) g.nx * g.ny;
    bool any = false;
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z;
        if (x >= g.nx) continue;
        const uint64_t i = ((uint64_t) z * g.ny + y) * g.nx + x;
        uint32_t own;
        if (P == 0) {
            const int32_t h = H.at(x, y, z);
            own = h > 0 ? (uint32_t) h : 0u;
        } else {
            own = mask[i];
        }
        if (!own) continue;
        const uint32_t v = grow_relax<P>(V + i, sy, sz, g.w, own, P == 0 ? grow_box_mask(g, x, y, z) : 0u);
        if (v != V[i]) grow_store(V + i, v), any = true;
    }
    if (__ballot(any) != 0ull && lane == 0u) atomicOr(changed, 1u);
}

// Between the phases, a lane per voxel.  Tight = false: T and the mask of the ticks from the final Q.  Tight = true: the mask of
// the labels from the final Q and T, L = M at the seeds and kGrowNoLabel elsewhere.  flags != null: every tile with a reached
// voxel goes to round 0's list of the phase that follows.
template <bool Tight>
__global__ __launch_bounds__(kBlock) void k_grow_between(GeoGrid g, I32View H, I32View M, const uint32_t *__restrict__ Q, uint32_t *T, uint32_t *L, uint32_t *mask,
                                                         uint32_t *flags, uint32_t *list, uint32_t *count)
{
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t sy = g.nx, sz = (int64_t) g.nx * g.ny;
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z;
        bool reached = false;
        if (x < g.nx) {
            const uint64_t i = ((uint64_t) z * g.ny + y) * g.nx + x;
            reached = Q[i] != 0u;
            uint32_t m = 0, t = kGeoInf, l = kGrowNoLabel;
            if (reached) {
                const int32_t h = H.at(x, y, z), mk = M.at(x, y, z);   // (reached: h > 0)
                const uint32_t box = grow_box_mask(g, x, y, z);
                if (Tight) {
                    m = grow_tight_mask(Q + i, T + i, sy, sz, g.w, (uint32_t) h, mk > 0, box);
                    if (mk > 0) l = (uint32_t) mk;
                } else {
                    t = grow_sources(Q + i, sy, sz, g.w, (uint32_t) h, mk > 0, box, &m);
                }
            }
            mask[i] = m;
            if (Tight) L[i] = l;
            else T[i] = t;
        }
        if (flags && __ballot(reached) != 0ull && lane == 0u) geo_flag_tile(grow_tile_of(g, at), flags, list, count);
    }
}

// labels / level / ticks through their strides (level, ticks may be null): L / Q / T where the voxel was reached, else 0 / 0 / -1.
// Q, T, L may be the outputs themselves: a lane reads its own elements, then writes them.  *reached += the voxels with Q > 0.
__global__ __launch_bounds__(kBlock) void k_grow_write(GeoGrid g, const uint32_t *Q, const uint32_t *T, const uint32_t *L, int32_t *labels, uint64_t l0, uint64_t l1,
                                                       uint64_t l2, int32_t *level, uint64_t q0, uint64_t q1, uint64_t q2, int32_t *ticks, uint64_t t0, uint64_t t1,
                                                       uint64_t t2, unsigned long long *reached)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long mine = 0;   // (the same in every lane of the wavefront)
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z;
        bool hit = false;
        if (x < g.nx) {
            const uint64_t i = ((uint64_t) z * g.ny + y) * g.nx + x;
            const uint32_t q = Q[i], t = T[i], l = L[i];
            hit = q != 0u;
            labels[(uint64_t) x * l0 + (uint64_t) y * l1 + (uint64_t) z * l2] = hit ? (int32_t) l : 0;
            if (level) level[(uint64_t) x * q0 + (uint64_t) y * q1 + (uint64_t) z * q2] = (int32_t) q;
            if (ticks) ticks[(uint64_t) x * t0 + (uint64_t) y * t1 + (uint64_t) z * t2] = hit ? (int32_t) t : -1;
        }
        mine += (unsigned long long) __popcll(__ballot(hit));
    }
    bits_add_wave_sums(mine, reached);
}

#endif   // O2V_GROW_HOST
