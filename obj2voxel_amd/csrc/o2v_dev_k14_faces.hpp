// o2v_dev_k14_faces.hpp -- K14: the exposed voxel faces of a dense grid as coloured quads (o2v_hip_faces_count / _write).
// Included from o2v_device.hip inside its anonymous namespace, after K13 (whose slot -> word -> bit mapping and colour modes it
// uses; the classify kernel is K12's, the bit grid, its words and walk o2v_dev_bits.hpp's, the scans K6's).
//
// The set is classified once into the bit grid of o2v_dev_bits.hpp; its padding bits are 0, so that "outside the box is empty"
// needs no mask.  With a colour grid or a palette and MERGE_RUNS two more words per solid word say
// where a voxel has the colour of the voxel at x - 1 and at y - 1.  Everything after that works on those words alone.
//
// An item is (row, direction, word): item = ((z * ny + y) * 6 + d) * W + wx.  The start mask of an item - the exposed faces of
// direction d in that word that begin a quad - in ascending (item, bit) order is the contract's order key, so quad q is the q-th
// set start bit.
//
//   k_cc_classify (K12)   the only pass over the grid.
//   k_faces_same          GRID / PALETTE with MERGE_RUNS: a wavefront per word, a lane per voxel: the colour where the voxel is
//                         solid (256 contiguous bytes a load for a dense colour grid), the x comparison with the lane before,
//                         the y comparison with the same lane of the row before, two ballots -> same_x[wi], same_y[wi].
//   k_faces_count + k_fill_scan_blocks (K6)   a lane per item: start mask, popcount, the sum over the block of 256 items (at most
//                         2^14) -> boff[block]; the scan of the sums in place, boff[n_blocks] = the count (64-bit).
//   k_faces_write         a workgroup per block of items in turns: the start masks again (words from L2) and their exclusive scan
//                         into LDS; then a lane per quad: slot -> item (ga_find_word) -> bit (ga_select) -> run length by walking
//                         the continuation bits -> 48 bytes of corners, 24 of indices, 4 of colour, each lane's behind the
//                         lane's before, so a wavefront writes 64 x 48, 64 x 24 and 64 x 4 contiguous bytes.
// No atomics, no private segment: every order comes from the scans.

constexpr uint32_t kFaMergeNone = 0, kFaMergeRuns = 1, kFaMergeRects = 3;   // O2V_HIP_FACES_MERGE_*

#ifndef O2V_FA_HOST
#define O2V_FA_FN __device__ __forceinline__
O2V_FA_FN uint32_t fa_ctz64(uint64_t v) { return (uint32_t) __builtin_ctzll(v); }   // (v != 0)
#endif

// ---- words -> exposed faces -> starts of quads -> run lengths -> corners --------------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_faces.py compiles this part for the host behind the plain part of
// o2v_dev_bits.hpp, with O2V_FA_FN and fa_ctz64 of its own, and runs it against the reference.)

struct FaGrid : BitGrid {   // (words: at most 2^31 - 1)
    uint32_t merge;         // kFaMergeNone / kFaMergeRuns
    uint32_t colored;       // same_x / same_y exist (GRID or PALETTE with MERGE_RUNS); else all voxels are of one colour
    uint64_t items;         // 6 * words
    uint64_t n_blocks;      // of kBlock items
};

struct FaBits {
    const unsigned long long *solid, *same_x, *same_y;   // [z][y][W]; same_*: only if colored
};

// word (wx, y, z) of a [z][y][W] array; 0 outside the box
O2V_FA_FN uint64_t fa_word(const unsigned long long *a, const FaGrid &g, int64_t wx, int64_t y, int64_t z)
{
    if (wx < 0 || y < 0 || z < 0 || wx >= (int64_t) g.W || y >= (int64_t) g.ny || z >= (int64_t) g.nz) return 0;
    return a[((uint64_t) z * g.ny + (uint64_t) y) * g.W + (uint64_t) wx];
}

// the exposed faces of direction d (0 .. 5: -x, +x, -y, +y, -z, +z) in word (wx, y, z): solid & ~neighbour
O2V_FA_FN uint64_t fa_exposed(const unsigned long long *solid, const FaGrid &g, uint32_t d, int64_t wx, int64_t y, int64_t z)
{
    const uint64_t s = fa_word(solid, g, wx, y, z);
    if (!s) return 0;
    uint64_t n;
    if (d == 0u) n = s << 1 | fa_word(solid, g, wx - 1, y, z) >> 63;
    else if (d == 1u) n = s >> 1 | fa_word(solid, g, wx + 1, y, z) << 63;
    else if (d == 2u) n = fa_word(solid, g, wx, y - 1, z);
    else if (d == 3u) n = fa_word(solid, g, wx, y + 1, z);
    else if (d == 4u) n = fa_word(solid, g, wx, y, z - 1);
    else n = fa_word(solid, g, wx, y, z + 1);
    return s & ~n;
}

// of the exposed faces e = fa_exposed(d, wx, y, z): those that continue the run of the face before them - at x - 1 for d >= 2
// (the carry is the last face of the word before), at y - 1 for d < 2 - with a voxel of the same colour
O2V_FA_FN uint64_t fa_continues(const FaBits &b, const FaGrid &g, uint32_t d, int64_t wx, int64_t y, int64_t z, uint64_t e)
{
    if (g.merge == kFaMergeNone || !e) return 0;
    uint64_t c;
    if (d >= 2u) {
#ifdef O2V_FA_MUTATE_NO_CARRY
        const uint64_t carry = 0;   // (test only: the word before is ignored, so runs along x are cut at multiples of 64)
#else
        const uint64_t carry = (e & 1u) ? fa_exposed(b.solid, g, d, wx - 1, y, z) >> 63 : 0u;
#endif
        c = e & (e << 1 | carry);
        if (g.colored && c) c &= fa_word(b.same_x, g, wx, y, z);
    } else {
        c = e & fa_exposed(b.solid, g, d, wx, y - 1, z);
        if (g.colored && c) c &= fa_word(b.same_y, g, wx, y, z);
    }
    return c;
}

// the faces of item (d, wx, y, z) that begin a quad
O2V_FA_FN uint64_t fa_starts(const FaBits &b, const FaGrid &g, uint32_t d, int64_t wx, int64_t y, int64_t z)
{
    const uint64_t e = fa_exposed(b.solid, g, d, wx, y, z);
    return e & ~fa_continues(b, g, d, wx, y, z, e);
}

// the faces of the run that begins at `bit` of item (d, wx, y, z): the continuation bits behind it, to the end of its word by a
// count of trailing ones and then word by word along x (d >= 2), or row by row along y (d < 2)
O2V_FA_FN uint32_t fa_run_length(const FaBits &b, const FaGrid &g, uint32_t d, int64_t wx, int64_t y, int64_t z, uint32_t bit)
{
    if (g.merge == kFaMergeNone) return 1u;
    uint32_t n = 1u;
    if (d >= 2u) {
        const uint64_t c = fa_continues(b, g, d, wx, y, z, fa_exposed(b.solid, g, d, wx, y, z));
        const uint32_t ones = bit == 63u ? 0u : fa_ctz64(~(c >> (bit + 1u)));   // (the shift leaves zeros at the top)
        n += ones;
        if (bit + ones < 63u) return n;
        for (int64_t w = wx + 1; w < (int64_t) g.W; ++w) {
            const uint64_t cw = fa_continues(b, g, d, w, y, z, fa_exposed(b.solid, g, d, w, y, z));
            if (cw != ~0ull) return n + fa_ctz64(~cw);
            n += 64u;
        }
        return n;
    }
    uint64_t before = fa_exposed(b.solid, g, d, wx, y, z);
    for (int64_t r = y + 1; r < (int64_t) g.ny; ++r, ++n) {
        const uint64_t e = fa_exposed(b.solid, g, d, wx, r, z);
        if (!((e & before) >> bit & 1u)) break;
        if (g.colored && !(fa_word(b.same_y, g, wx, r, z) >> bit & 1u)) break;
        before = e;
    }
    return n;
}

// where item `item` is: direction, word of the row, row
O2V_FA_FN void fa_item_at(const FaGrid &g, uint64_t item, uint32_t &d, uint32_t &wx, uint32_t &y, uint32_t &z)
{
    const uint64_t rd = item / g.W, row = rd / 6u;
    wx = (uint32_t) (item - rd * g.W);
    d = (uint32_t) (rd - row * 6u);
    z = (uint32_t) (row / g.ny);
    y = (uint32_t) (row - (uint64_t) z * g.ny);
}

O2V_FA_FN uint32_t fa_pick(uint32_t axis, uint32_t vx, uint32_t vy, uint32_t vz) { return axis == 0u ? vx : axis == 1u ? vy : vz; }

// The four corners (x, y, z each) of the quad of direction d over the `len` faces from lattice voxel (x, y, z) (the origin
// included) along its run axis and `height` rows along its stack axis (K16: y for d = 4, 5, else z; 1 for a run): in the plane a = voxel[a] + s, spanning [u0, u1] x [v0, v1] with (u, v) the axes after a in
// cyclic order, as (u0, v0), (u1, v0), (u1, v1), (u0, v1) for s = 1 and (u0, v0), (u0, v1), (u1, v1), (u1, v0) for s = 0.
O2V_FA_FN void fa_quad(uint32_t d, uint32_t x, uint32_t y, uint32_t z, uint32_t len, uint32_t height, float out[12])
{
    const uint32_t a = d >> 1, s = d & 1u, u = a == 2u ? 0u : a + 1u, v = u == 2u ? 0u : u + 1u;
    const uint32_t hx = x + (d >= 2u ? len : 1u), hy = y + (d < 2u ? len : d >= 4u ? height : 1u), hz = z + (d < 4u ? height : 1u);
    const uint32_t plane = fa_pick(a, x, y, z) + s;
    const uint32_t u0 = fa_pick(u, x, y, z), u1 = fa_pick(u, hx, hy, hz), v0 = fa_pick(v, x, y, z), v1 = fa_pick(v, hx, hy, hz);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        // corner k: u1 for k = 1, 2 (s = 1) or k = 2, 3 (s = 0); v1 for k = 2, 3 (s = 1) or k = 1, 2 (s = 0)
        const bool mid = k == 1u || k == 2u, late = k >= 2u;
        const uint32_t cu = (s ? mid : late) ? u1 : u0, cv = (s ? late : mid) ? v1 : v0;
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) out[3u * k + c] = (float) (c == a ? plane : c == u ? cu : cv);
    }
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_FA_HOST

// same_x[wi] bit x: voxels x and x - 1 of the row are solid and of one colour; same_y[wi]: the same with the voxel at y - 1.
// (Only solid voxels are read: the bits are looked at only where both faces are exposed.)
template <uint32_t Mode>
__global__ __launch_bounds__(kBlock) void k_faces_same(FaGrid g, const unsigned long long *__restrict__ solid, GaColor col,
                                                       unsigned long long *__restrict__ same_x, unsigned long long *__restrict__ same_y)
{
    __shared__ uint32_t s_pal[Mode == kGaColorPalette ? 256 : 1];
    bits_palette_to_lds<Mode == kGaColorPalette>(col.palette, s_pal, true);
    const uint32_t lane = threadIdx.x & 63u;
    for (const uint64_t wi : bits_words(g)) {
        const uint64_t s = solid[wi];
        unsigned long long mx = 0, my = 0;
        if (s) {
            const BitWord at = bits_word_at(g, wi);
            const uint32_t wx = at.wx, x = wx * 64u + lane, y = at.y, z = at.z;   // (a solid bit is inside the box: the padding bits are 0)
            const uint64_t below = y ? solid[wi - g.W] : 0ull;
            const uint64_t left = s << 1 | (wx ? solid[wi - 1u] >> 63 : 0ull);
            const bool me = s >> lane & 1u;
            const uint32_t c = me ? ga_color_at<Mode>(col, s_pal, x, y, z) : 0u;
            uint32_t cl = __shfl_up(c, 1);
            if (lane == 0u && (s & left & 1u)) cl = ga_color_at<Mode>(col, s_pal, x - 1u, y, z);
            const bool both_y = (s & below) >> lane & 1u;
            const uint32_t cb = both_y ? ga_color_at<Mode>(col, s_pal, x, y - 1u, z) : 0u;
            mx = __ballot(((s & left) >> lane & 1u) && c == cl);
            my = __ballot(both_y && c == cb);
        }
        if (lane == 0u) same_x[wi] = mx, same_y[wi] = my;
    }
}

// The count of K14 and K16, a lane per item: block_sums[block] = the set bits of the start masks of the block's items.
// starts(item, d, wx, y, z): the start mask of an item below g.items.
template <class Starts>
__device__ __forceinline__ void fa_count_blocks(const FaGrid &g, unsigned long long *__restrict__ block_sums, Starts starts)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    for (uint64_t blk = blockIdx.x; blk < g.n_blocks; blk += gridDim.x) {
        const uint64_t item = blk * kBlock + threadIdx.x;
        uint64_t n = 0;
        if (item < g.items) {
            uint32_t d, wx, y, z;
            fa_item_at(g, item, d, wx, y, z);
            n = (uint64_t) __popcll(starts(item, d, wx, y, z));
        }
        uint64_t total;
        (void) fill_block_exscan64(n, s_wave, total);
        if (threadIdx.x == 0) block_sums[blk] = total;
    }
}

// block_sums[block] = the quads that begin in the block's items
__global__ __launch_bounds__(kBlock) void k_faces_count(FaGrid g, FaBits b, unsigned long long *__restrict__ block_sums)
{
    fa_count_blocks(g, block_sums, [&](uint64_t, uint32_t d, uint32_t wx, uint32_t y, uint32_t z) { return fa_starts(b, g, d, wx, y, z); });
}

// quad q: its corners p, its two triangles over the vertices 4 q .. 4 q + 3 (if faces is not null; 4 q + 3 is below 2^31: the
// host refuses more), its colour (if quad_argb is not null)
__device__ __forceinline__ void fa_store_quad(uint64_t q, const float p[12], uint32_t argb, float4 *__restrict__ positions, int2 *__restrict__ faces,
                                              uint32_t *__restrict__ quad_argb)
{
    positions[3u * q] = make_float4(p[0], p[1], p[2], p[3]);
    positions[3u * q + 1u] = make_float4(p[4], p[5], p[6], p[7]);
    positions[3u * q + 2u] = make_float4(p[8], p[9], p[10], p[11]);
    if (faces) {
        const int32_t v = (int32_t) (4u * q);
        faces[3u * q] = make_int2(v, v + 1);
        faces[3u * q + 1u] = make_int2(v + 2, v);
        faces[3u * q + 2u] = make_int2(v + 2, v + 3);
    }
    if (quad_argb) quad_argb[q] = argb;
}

// The write of K14 and K16, a workgroup per block of items in turns: the start masks again and their exclusive scan into LDS,
// then a lane per quad: slot -> item (ga_find_word) -> bit (ga_select) -> extents -> fa_store_quad.  starts: as the count took
// it; extents(d, wx, y, z, bit, len, height): the faces along the run axis and the rows along the stack axis of the quad that
// begins at `bit` of item (d, wx, y, z).
template <uint32_t Mode, class Starts, class Extents>
__device__ __forceinline__ void fa_write_blocks(const FaGrid &g, const unsigned long long *__restrict__ boff, uint32_t ox, uint32_t oy, uint32_t oz,
                                                const GaColor &col, float4 *__restrict__ positions, int2 *__restrict__ faces,
                                                uint32_t *__restrict__ quad_argb, Starts starts, Extents extents)
{
    __shared__ uint32_t s_pref[kBlock];
    __shared__ uint64_t s_start[kBlock];
    __shared__ uint64_t s_wave[kBlock / 64];
    __shared__ uint32_t s_pal[Mode == kGaColorPalette ? 256 : 1];
    static_assert(kBlock == 256u, "a lane per item of a block, ga_find_word over 256 prefixes");
    bits_palette_to_lds<Mode == kGaColorPalette>(col.palette, s_pal, false);   // (the first barrier below publishes it)
    for (uint64_t blk = blockIdx.x; blk < g.n_blocks; blk += gridDim.x) {
        const uint64_t base = boff[blk];
        const uint32_t cnt = (uint32_t) (boff[blk + 1] - base);   // at most 2^14
        if (!cnt) continue;                                       // (uniform over the workgroup)
        __syncthreads();                                          // (the arrays of the block before have been read)
        {
            const uint64_t item = blk * kBlock + threadIdx.x;
            uint64_t start = 0;
            if (item < g.items) {
                uint32_t d, wx, y, z;
                fa_item_at(g, item, d, wx, y, z);
                start = starts(item, d, wx, y, z);
            }
            uint64_t total;
            s_pref[threadIdx.x] = (uint32_t) fill_block_exscan64((uint64_t) __popcll(start), s_wave, total);   // (past the items: the block's count)
            s_start[threadIdx.x] = start;
        }
        __syncthreads();
        for (uint32_t slot = threadIdx.x; slot < cnt; slot += kBlock) {
            const uint32_t l = ga_find_word(s_pref, slot);
            const uint32_t bit = ga_select(s_start[l], slot - s_pref[l]);
            uint32_t d, wx, y, z, len, height;
            fa_item_at(g, blk * kBlock + l, d, wx, y, z);
            extents(d, wx, y, z, bit, len, height);
            const uint32_t x = wx * 64u + bit;
            float p[12];
            fa_quad(d, ox + x, oy + y, oz + z, len, height, p);
            fa_store_quad(base + slot, p, quad_argb ? ga_color_at<Mode>(col, s_pal, x, y, z) : 0u, positions, faces, quad_argb);
        }
    }
}

// quad q of the numbering -> positions[12 q ..], faces[6 q ..] (if not null), quad_argb[q] (if not null): the start masks
// computed again (words from L2), a run's length by walking the continuation bits
template <uint32_t Mode>
__global__ __launch_bounds__(kBlock) void k_faces_write(FaGrid g, FaBits b, const unsigned long long *__restrict__ boff, uint32_t ox, uint32_t oy,
                                                        uint32_t oz, GaColor col, float4 *__restrict__ positions, int2 *__restrict__ faces,
                                                        uint32_t *__restrict__ quad_argb)
{
    fa_write_blocks<Mode>(
        g, boff, ox, oy, oz, col, positions, faces, quad_argb,
        [&](uint64_t, uint32_t d, uint32_t wx, uint32_t y, uint32_t z) { return fa_starts(b, g, d, wx, y, z); },
        [&](uint32_t d, uint32_t wx, uint32_t y, uint32_t z, uint32_t bit, uint32_t &len, uint32_t &height) {
            len = fa_run_length(b, g, d, wx, y, z, bit), height = 1u;
        });
}

#endif   // O2V_FA_HOST
