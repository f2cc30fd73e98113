// o2v_dev_k22_thinning.hpp -- K22: skeletons of a dense grid by topological thinning (o2v_hip_thin_dense).  Included from
// o2v_device.hip inside its anonymous namespace, after K12 (whose classification it uses) and o2v_dev_bits.hpp (the bit grid,
// its words, tiles and walk).
//
// The definition (include/o2v_hip.h and DESIGN.md section 25 state the same words).  S is the set of a set grid; voxels outside
// the box are background.  Objects are 26-connected, the background is 6-connected.
//   Neighbourhood mask of a voxel: bit k = 9 (dz + 1) + 3 (dy + 1) + (dx + 1) is set where the neighbour is in S; k runs 0 ... 26
//   without 13.
//   C26(m) is the number of 26-connected components of the set bits of m.
//   C6(m): take the clear bits of m among the 18 positions that differ from the centre on at most two axes, connect them by
//   6-adjacency within these 18, count the components that hold a face neighbour.
//   Simple: a voxel is simple iff C26 == 1 && C6 == 1.
//   Border: a voxel of S is a border voxel if one of its six face neighbours is background.
//   Subfield: the subfield of a voxel is s = (x & 1) | (y & 1) << 1 | (z & 1) << 2, in box coordinates.  Two voxels of one
//   subfield are never 26-neighbours.
//   One iteration: B := the border voxels of S as it is now; for s = 0 ... 7 in turn, remove from S at once every voxel v that
//   is in subfield s, is in B, is not in `keep`, is simple and - in mode CURVE - has other than exactly one 26-neighbour in S,
//   all in the current S.  Iterations repeat until one removes nothing (that iteration counts), or until max_iterations have run.
//
//   k_cc_classify   (K12) the set into the bit grid `bits`; `keep` into a second one.
//   k_thin_border   B = S and not all six neighbours in S, by word shifts and the rows above and below, into a third bit grid;
//                   a thread per word, for the words of the tiles that run.
//   k_thin_substep  the hot kernel.  A workgroup reads the stamps of up to 32 tiles at a time, a thread each, lists those that run and
//                   takes them one by one, the whole workgroup on a tile of 64 x 8 x 8 voxels.  LDS holds the tile's 64 row words
//                   with a halo of one row in y and z and the neighbour words in x (10 x 10 rows x 3 words).  Only the 32 x 4 x 4
//                   voxels of subfield s are candidates: a lane per candidate, two rows per wavefront.  The 26-bit mask from nine
//                   shifts of row words; the cheap exits (no set neighbour; an end point in CURVE); then the simple test in
//                   registers, two floods over adjacency masks that are immediates once the loops are unrolled.  Removed bits are
//                   cleared in the LDS word and one lane per changed row stores the word.
//   the host        nine launches per iteration - border, then s = 0 ... 7 - and one read of "voxels removed so far".
//   k_thin_sweep    O2V_THIN_NO_TILES=1: a lane per voxel over the whole grid, masks from global memory.  Same bits: the
//                   cross-check and the baseline.
//   k_thin_write    dst from the bits: 1 / 0, or 1 + the number of 26-neighbours in the skeleton.
//
// Invariants.  A word of `bits` is written only by the workgroup of the tile that owns it (k_thin_substep) or by the wavefront
// that walks it (k_thin_sweep).  Sub-step s changes only bits of subfield s, and a candidate of subfield s reads only its 26
// neighbours, none of which is in subfield s: readers in other tiles never depend on a bit that this sub-step can change, so the
// update is in place and needs no second copy; a halo word read while its owner stores it is the same in every bit that is
// used.  Every sub-step is a pure function of the grid, so the result is the same bits on every run and under every schedule.
// When a tile runs: per tile two stamps, of the last odd and the last even iteration during which a voxel of the tile or of its
// one-voxel halo was removed, written by the removing tile for itself and the tiles that see the voxel.  A tile runs in every
// sub-step of iteration i if its stamps say i - 1 or i: a removal in a neighbour tile earlier in the same iteration counts (a
// one-voxel line across a tile border ends one voxel off without it).  A stamp written during the launch that reads it is of a
// removal in subfield s, which no candidate of that launch sees: the tile's result is the same whether it runs or not.
// No kernel waits for another workgroup, flag or lane; there is no round cap other than max_iterations; every loop ends because
// a voxel was removed or nothing was.

constexpr uint32_t kThinUltimate = 0u, kThinCurve = 1u;       // mode
constexpr uint32_t kThinDstMask = 0u, kThinDstDegree = 1u;    // dst_format
constexpr uint32_t kThinAll26 = 0x07ffdfffu;                  // bits 0 ... 26 without 13
constexpr uint32_t kThinFaces = 1u << 4 | 1u << 10 | 1u << 12 | 1u << 14 | 1u << 16 | 1u << 22;
constexpr uint32_t kThinCorners = 1u << 0 | 1u << 2 | 1u << 6 | 1u << 8 | 1u << 18 | 1u << 20 | 1u << 24 | 1u << 26;
constexpr uint32_t kThin18 = kThinAll26 & ~kThinCorners;      // the positions that differ from the centre on at most two axes
constexpr uint32_t kThinRowWords = 3u, kThinHaloRows = 100u;  // the tile in LDS: 10 (y) x 10 (z) rows of (left, own, right) words
constexpr uint32_t kThinChunk = 32u;                          // the most tiles whose stamps one workgroup of k_thin_substep reads at a time

#ifndef O2V_THIN_HOST
#define O2V_THIN_FN __device__ __forceinline__
// (a word of the set may be stored by its owner while a neighbour reads it: one 64-bit load, never a torn one)
O2V_THIN_FN uint64_t thin_load(const unsigned long long *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
#endif

// ---- the simple test, the masks, the tiles that see a voxel, when a tile runs ----------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_thinning.py compiles this part for the host, with an O2V_THIN_FN and a
// thin_load of its own, counts the simple masks, runs the sub-steps tile by tile in a shuffled order and as whole-grid sweeps
// against the reference, and checks that the wrong tile rule is caught.)

struct ThinGrid : BitGrid {
    uint32_t tiles_y, tiles_z;   // ceil(ny / 8), ceil(nz / 8); tiles along x: W
    uint32_t mode;               // kThinUltimate, kThinCurve
};

// The 27 positions of the 3^3 block by their coordinate along one axis: bit k of thin_at(a, d) is set where position k has
// offset d = -1, 0, 1 along axis a = 0 (x), 1 (y), 2 (z).
O2V_THIN_FN constexpr uint32_t thin_at(int a, int d)
{
    return (a == 0 ? 0x1249249u : a == 1 ? 0x01c0e07u : 0x00001ffu) << ((d + 1) * (a == 0 ? 1 : a == 1 ? 3 : 9));
}
O2V_THIN_FN constexpr int thin_d(int a, int k) { return a == 0 ? k % 3 - 1 : a == 1 ? k / 3 % 3 - 1 : k / 9 - 1; }
// ... within one step of position k along axis a
O2V_THIN_FN constexpr uint32_t thin_near(int a, int k)
{
    return thin_at(a, thin_d(a, k)) | (thin_d(a, k) <= 0 ? thin_at(a, thin_d(a, k) + 1) : 0u) | (thin_d(a, k) >= 0 ? thin_at(a, thin_d(a, k) - 1) : 0u);
}
O2V_THIN_FN constexpr uint32_t thin_same(int a, int k) { return thin_at(a, thin_d(a, k)); }

// the positions that are 26-adjacent to position k (the centre is none)
O2V_THIN_FN constexpr uint32_t thin_adj26(int k) { return thin_near(0, k) & thin_near(1, k) & thin_near(2, k) & kThinAll26 & ~(1u << k); }
// the positions among the 18 that are 6-adjacent to position k
O2V_THIN_FN constexpr uint32_t thin_adj6(int k)
{
    return ((thin_near(0, k) & thin_same(1, k) & thin_same(2, k)) | (thin_same(0, k) & thin_near(1, k) & thin_same(2, k)) |
            (thin_same(0, k) & thin_same(1, k) & thin_near(2, k))) & kThin18 & ~(1u << k);
}

// What the bits of `from` reach through the bits of `within` (from is part of within): by 26-adjacency, or (Six) by 6-adjacency.
// Once the loop over k is unrolled every adjacency mask is an immediate.  Ends: a sweep adds a bit or is the last.
template <bool Six>
O2V_THIN_FN uint32_t thin_flood(uint32_t from, uint32_t within)
{
    uint32_t cur = from;
    for (;;) {
        const uint32_t old = cur;
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            if (k == 13 || (Six && !((kThin18 >> k) & 1u))) continue;
            if ((cur >> k) & 1u) cur |= (Six ? thin_adj6(k) : thin_adj26(k)) & within;
        }
        if (cur == old) return cur;
    }
}

O2V_THIN_FN uint32_t thin_lowest(uint32_t m) { return m & (0u - m); }

O2V_THIN_FN uint32_t thin_c26(uint32_t m)
{
    uint32_t rest = m & kThinAll26, n = 0;
    for (; rest; ++n) rest &= ~thin_flood<false>(thin_lowest(rest), m & kThinAll26);
    return n;
}

O2V_THIN_FN uint32_t thin_c6(uint32_t m)
{
    const uint32_t clear = ~m & kThin18;
    uint32_t rest = clear & kThinFaces, n = 0;
    for (; rest; ++n) rest &= ~thin_flood<true>(thin_lowest(rest), clear);
    return n;
}

// C26 == 1 && C6 == 1, with one flood each: everything set is reached from the lowest set bit, every clear face from the
// lowest clear face.
O2V_THIN_FN bool thin_is_simple(uint32_t m)
{
    m &= kThinAll26;
    const uint32_t clear = ~m & kThin18, faces = clear & kThinFaces;
    if (!m || !faces) return false;
    if (thin_flood<false>(thin_lowest(m), m) != m) return false;
    return (thin_flood<true>(thin_lowest(faces), clear) & faces) == faces;
}

// is a voxel with mask m (in B, not in keep) removed
O2V_THIN_FN bool thin_removes(uint32_t m, uint32_t mode)
{
    m &= kThinAll26;
    if (!m || (mode == kThinCurve && !(m & (m - 1u)))) return false;   // the cheap exits: no set neighbour (C26 == 0); an end point
    return thin_is_simple(m);
}

// voxels x - 1, x, x + 1 (bits 0, 1, 2) of the row whose word is `own`, between the words `left` and `right`; x = 0 ... 63
O2V_THIN_FN uint32_t thin_row3(uint64_t left, uint64_t own, uint64_t right, uint32_t x)
{
    const uint32_t below = x ? (uint32_t) (own >> (x - 1u)) & 1u : (uint32_t) (left >> 63);
    const uint32_t above = x < 63u ? (uint32_t) (own >> (x + 1u)) & 1u : (uint32_t) right & 1u;
    return below | ((uint32_t) (own >> x) & 1u) << 1 | above << 2;
}

// The mask of voxel x (0 ... 63) of a row from nine row words: rows points at the (left, own, right) words of the voxel's row,
// the row at (dy, dz) lies kThinRowWords * (dy * sy + dz * sz) words from it.
O2V_THIN_FN uint32_t thin_mask_rows(const uint64_t *rows, int sy, int sz, uint32_t x)
{
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const uint64_t *const p = rows + (int) kThinRowWords * ((r % 3 - 1) * sy + (r / 3 - 1) * sz);
        m |= thin_row3(p[0], p[1], p[2], x) << (3 * r);
    }
    return m & kThinAll26;
}

// word wx of row (y, z) of the whole grid; 0 outside the box (-1 wraps to above any dim)
O2V_THIN_FN uint64_t thin_word(const BitGrid &g, const unsigned long long *bits, uint32_t wx, uint32_t y, uint32_t z)
{
    return wx < g.W && y < g.ny && z < g.nz ? thin_load(bits + bits_word_index(g, wx, y, z)) : 0ull;
}

// The same mask for voxel (x, y, z) of the whole grid (k_thin_sweep, k_thin_write).
O2V_THIN_FN uint32_t thin_mask_grid(const BitGrid &g, const unsigned long long *bits, uint32_t x, uint32_t y, uint32_t z)
{
    const uint32_t wx = x >> 6, b = x & 63u;
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const uint32_t Y = y + (uint32_t) (r % 3 - 1), Z = z + (uint32_t) (r / 3 - 1);
        const uint64_t left = b == 0u ? thin_word(g, bits, wx - 1u, Y, Z) : 0ull, right = b == 63u ? thin_word(g, bits, wx + 1u, Y, Z) : 0ull;
        m |= thin_row3(left, thin_word(g, bits, wx, Y, Z), right, b) << (3 * r);
    }
    return m & kThinAll26;
}

// B of one word: S and not all six neighbours in S, from the word, its two neighbours in x and the words above and below in y and z
O2V_THIN_FN uint64_t thin_border_word(uint64_t own, uint64_t left, uint64_t right, uint64_t ym, uint64_t yp, uint64_t zm, uint64_t zp)
{
    return own & ~(((own << 1) | (left >> 63)) & ((own >> 1) | (right << 63)) & ym & yp & zm & zp);
}

// ... of word wx of row (y, z) of the whole grid
O2V_THIN_FN uint64_t thin_border_at(const BitGrid &g, const unsigned long long *bits, uint32_t wx, uint32_t y, uint32_t z)
{
    return thin_border_word(thin_word(g, bits, wx, y, z), thin_word(g, bits, wx - 1u, y, z), thin_word(g, bits, wx + 1u, y, z),
                            thin_word(g, bits, wx, y - 1u, z), thin_word(g, bits, wx, y + 1u, z), thin_word(g, bits, wx, y, z - 1u),
                            thin_word(g, bits, wx, y, z + 1u));
}

// the candidates of subfield s in a word of row (y, z): the bits of its parity in x if the row has its parities in y and z
O2V_THIN_FN uint64_t thin_subfield_word(uint32_t s, uint32_t y, uint32_t z)
{
    if ((y & 1u) != ((s >> 1) & 1u) || (z & 1u) != ((s >> 2) & 1u)) return 0ull;
    return (s & 1u) ? 0xaaaaaaaaaaaaaaaaull : 0x5555555555555555ull;
}

// Which tiles see voxel (x, y, z) of a tile (0 ... 63, 0 ... 7, 0 ... 7), in the tile itself or in their halo: bit k for the tile at
// offset k (bit 13: the tile itself).  (Tiles outside the grid are the caller's to leave out.)
O2V_THIN_FN uint32_t thin_see_mask(uint32_t x, uint32_t y, uint32_t z)
{
    return (thin_at(0, 0) | (x == 0u ? thin_at(0, -1) : 0u) | (x == 63u ? thin_at(0, 1) : 0u)) &
           (thin_at(1, 0) | (y == 0u ? thin_at(1, -1) : 0u) | (y == 7u ? thin_at(1, 1) : 0u)) &
           (thin_at(2, 0) | (z == 0u ? thin_at(2, -1) : 0u) | (z == 7u ? thin_at(2, 1) : 0u));
}

// The rule for when a tile must run in (every sub-step of) iteration i = 1, 2, ...: a voxel of the tile or of its one-voxel halo
// was removed during iteration i - 1, or during iteration i so far.  stamp_last, stamp_this: the tile's stamps of the parities of
// i - 1 and of i - the last iteration of that parity with such a removal, 0 from the start, so every tile runs in iteration 1.
O2V_THIN_FN bool thin_tile_runs(uint32_t stamp_last, uint32_t stamp_this, uint32_t i)
{
#ifdef O2V_THIN_MUTATE_STALE_LIST
    (void) stamp_this;   // (test only: the tiles fixed at the start of the iteration from "something changed last iteration")
    return stamp_last == i - 1u;
#else
    return stamp_last == i - 1u || stamp_this == i;
#endif
}

// 32 bits to the even bits of 64
O2V_THIN_FN uint64_t thin_spread(uint32_t h)
{
    uint64_t v = h;
    v = (v | v << 16) & 0x0000ffff0000ffffull;
    v = (v | v << 8) & 0x00ff00ff00ff00ffull;
    v = (v | v << 4) & 0x0f0f0f0f0f0f0f0full;
    v = (v | v << 2) & 0x3333333333333333ull;
    return (v | v << 1) & 0x5555555555555555ull;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_THIN_HOST

// B for the words of the tiles that run in iteration `it` (All: for every word); a thread per word
template <bool All>
__global__ __launch_bounds__(kBlock) void k_thin_border(ThinGrid g, const unsigned long long *__restrict__ bits, const uint32_t *__restrict__ stamps,
                                                        uint32_t it, unsigned long long *__restrict__ border)
{
    const uint32_t tiles = g.W * g.tiles_y * g.tiles_z;   // (no more than the words)
    for (uint64_t wi = (uint64_t) blockIdx.x * kBlock + threadIdx.x; wi < g.words; wi += (uint64_t) gridDim.x * kBlock) {
        const BitWord at = bits_word_at(g, wi);
        if (!All) {
            const uint32_t tile = ((at.z >> 3) * g.tiles_y + (at.y >> 3)) * g.W + at.wx;
            if (!thin_tile_runs(stamps[((it - 1u) & 1u) * tiles + tile], stamps[(it & 1u) * tiles + tile], it)) continue;
        }
        border[wi] = thin_border_at(g, bits, at.wx, at.y, at.z);
    }
}

// Sub-step `sub` of iteration `it` for the tiles that run.  ctr[0] += the voxels removed; Count (O2V_HIP_FLAG_STAGE_TIMES):
// ctr[1] += the tiles that ran.
template <bool Count>
__global__ __launch_bounds__(kBlock) void k_thin_substep(ThinGrid g, uint32_t sub, uint32_t it, uint32_t per_chunk, unsigned long long *bits,
                                                         const unsigned long long *__restrict__ keep, const unsigned long long *__restrict__ border,
                                                         uint32_t *stamps, unsigned long long *ctr)
{
    static_assert(kBlock == 256u, "four wavefronts: two candidate rows each, twice");
    __shared__ uint64_t s_rows[kThinHaloRows * kThinRowWords];
    __shared__ uint64_t s_cand[kCcTileRows];
    __shared__ uint32_t s_list[kThinChunk];
    __shared__ uint32_t s_n, s_see, s_removed;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tiles = g.W * g.tiles_y * g.tiles_z, chunks = (tiles + per_chunk - 1u) / per_chunk;
    const uint32_t px = sub & 1u, py = (sub >> 1) & 1u, pz = (sub >> 2) & 1u;
    // A workgroup takes chunks of per_chunk tiles (at most kThinChunk; the host's choice), a thread per tile's stamps - tile =
    // thread * chunks + chunk, so that neighbouring tiles, which run together, go to different workgroups -, lists the tiles that
    // run and takes them one by one.  A thread decides for its tile alone (another tile may stamp it during the launch); the list
    // makes the workgroup take one way.
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        __syncthreads();   // (the last chunk's list is no longer read)
        if (threadIdx.x == 0) s_n = 0u;
        __syncthreads();
        const uint32_t mine_tile = threadIdx.x * chunks + chunk;
        if (threadIdx.x < per_chunk && mine_tile < tiles && thin_tile_runs(cc_load(stamps + ((it - 1u) & 1u) * tiles + mine_tile), cc_load(stamps + (it & 1u) * tiles + mine_tile), it))
            s_list[atomicAdd(&s_n, 1u)] = mine_tile;
        __syncthreads();
        const uint32_t n_list = s_n;
        for (uint32_t li = 0; li < n_list; ++li) {
            const uint32_t tile = s_list[li];
            __syncthreads();   // (the last tile's words are no longer read)
            if (threadIdx.x == 0) s_see = 0u, s_removed = 0u;
            uint32_t tx, ty, tz;
            bits_tile_at(g, g.tiles_y, tile, tx, ty, tz);
            const uint32_t y0 = ty * 8u, z0 = tz * 8u;
            for (uint32_t i = threadIdx.x; i < kThinHaloRows * kThinRowWords; i += kBlock) {
                const uint32_t row = i / kThinRowWords, c = i - row * kThinRowWords;
                s_rows[i] = thin_word(g, bits, tx + c - 1u, y0 + row % 10u - 1u, z0 + row / 10u - 1u);
            }
            bool any = false;
            if (threadIdx.x < kCcTileRows) {
                const uint32_t y = y0 + (threadIdx.x & 7u), z = z0 + (threadIdx.x >> 3);
                uint64_t c = 0;
                if (y < g.ny && z < g.nz && thin_subfield_word(sub, y, z)) {
                    const uint64_t wi = bits_word_index(g, tx, y, z);
                    c = border[wi] & bits[wi] & ~(keep ? keep[wi] : 0ull) & thin_subfield_word(sub, y, z);
                }
                s_cand[threadIdx.x] = c;
                any = c != 0ull;
            }
            if (!__syncthreads_or(any)) continue;   // no candidate in the tile
            if (Count && threadIdx.x == 0) atomicAdd(ctr + 1, 1ull);
            // a lane per candidate: 32 along x, two rows per wavefront, the 16 rows of the subfield in two turns
            uint32_t see = 0, n_removed = 0;
            for (uint32_t turn = 0; turn < 2u; ++turn) {
                const uint32_t c = turn * 8u + wave * 2u + (lane >> 5), y = 2u * (c & 3u) + py, z = 2u * (c >> 2) + pz, row = z * 8u + y;
                const uint32_t x = 2u * (lane & 31u) + px;
                uint64_t *const own = s_rows + ((z + 1u) * 10u + (y + 1u)) * kThinRowWords;
                bool removed = false;
                if ((s_cand[row] >> x) & 1ull) removed = thin_removes(thin_mask_rows(own, 1, 10, x), g.mode);
                const unsigned long long all = __ballot(removed);
                if (removed) see |= thin_see_mask(x, y, z);
                const uint32_t mine = (uint32_t) (all >> (lane & 32u));   // the row's 32 candidates
                if (mine && (lane & 31u) == 0u) {
                    const uint64_t w = own[1] & ~(thin_spread(mine) << px);
                    own[1] = w;
                    __atomic_store_n(bits + bits_word_index(g, tx, y0 + y, z0 + z), w, __ATOMIC_RELAXED);   // (a candidate's row is in the box)
                    n_removed += (uint32_t) __popc(mine);
                }
            }
            for (int d = 32; d >= 1; d >>= 1) see |= __shfl_xor(see, d);
            if (lane == 0u && see) atomicOr(&s_see, see);
            if (n_removed) atomicAdd(&s_removed, n_removed);
            __syncthreads();
            if (threadIdx.x < 27u && ((s_see >> threadIdx.x) & 1u)) {
                const uint32_t k = threadIdx.x;
                const uint32_t X = tx + (uint32_t) thin_d(0, (int) k), Y = ty + (uint32_t) thin_d(1, (int) k), Z = tz + (uint32_t) thin_d(2, (int) k);   // (-1 wraps)
                if (X < g.W && Y < g.tiles_y && Z < g.tiles_z) atomicMax(stamps + (it & 1u) * tiles + (Z * g.tiles_y + Y) * g.W + X, it);
            }
            if (threadIdx.x == 0 && s_removed) atomicAdd(ctr, (unsigned long long) s_removed);
        }
    }
}

// O2V_THIN_NO_TILES: sub-step `sub` over the whole grid, a wavefront per word, a lane per voxel, the masks from global memory
__global__ __launch_bounds__(kBlock) void k_thin_sweep(ThinGrid g, uint32_t sub, unsigned long long *bits, const unsigned long long *__restrict__ keep,
                                                       const unsigned long long *__restrict__ border, unsigned long long *ctr)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long mine = 0;   // (the same in every lane of the wavefront)
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint64_t field = thin_subfield_word(sub, at.y, at.z);
        if (!field) continue;
        const uint64_t w = bits[wi], cand = border[wi] & w & ~(keep ? keep[wi] : 0ull) & field;
        if (!cand) continue;
        bool removed = false;
        if ((cand >> lane) & 1ull) removed = thin_removes(thin_mask_grid(g, bits, at.wx * 64u + lane, at.y, at.z), g.mode);
        const unsigned long long all = __ballot(removed);
        if (all && lane == 0u) __atomic_store_n(bits + wi, w & ~all, __ATOMIC_RELAXED);
        mine += (unsigned long long) __popcll(all);
    }
    bits_add_wave_sums(mine, ctr);
}

// dst(x, y, z) = 1 in the skeleton (Degree: 1 + its 26-neighbours in the skeleton), 0 elsewhere; every voxel of the box
template <bool Degree>
__global__ __launch_bounds__(kBlock) void k_thin_write(ThinGrid g, const unsigned long long *__restrict__ bits, uint8_t *dst, uint64_t s0, uint64_t s1,
                                                       uint64_t s2)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane;
        if (x >= g.nx) continue;
        uint32_t v = (uint32_t) (bits[wi] >> lane) & 1u;
        if (Degree && v) v += (uint32_t) __popc(thin_mask_grid(g, bits, x, at.y, at.z));
        dst[(uint64_t) x * s0 + (uint64_t) at.y * s1 + (uint64_t) at.z * s2] = (uint8_t) v;
    }
}

#endif   // O2V_THIN_HOST
