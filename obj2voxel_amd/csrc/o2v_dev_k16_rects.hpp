// o2v_dev_k16_rects.hpp -- K16: equal runs of exposed voxel faces stacked into rectangles (O2V_HIP_FACES_MERGE_RECTS of
// o2v_hip_faces_count / _write).  Included from o2v_device.hip inside its anonymous namespace, after K14, whose words, items,
// start and continuation masks, run lengths and order it uses as they are.
//
// The stack axis of direction d is y for d = 4, 5 and z otherwise; the row before (y, z) is (y - 1, z) or (y, z - 1).  A run is
// stacked if the row before holds a run of its direction that begins at the same bit, has the same length and the same colour.
// A rectangle start is a run start that is not stacked, and rectangle q is the q-th set bit of the rectangle-start masks in
// K14's (item, bit) order.  This is not the sequential greedy mesher: the rule is a function of the set and the colours alone.
//
//   k_rects_same_z        GRID / PALETTE: k_faces_same for the z neighbour -> same_z[wi] (same_x, same_y are K14's).
//   k_rects_count + k_fill_scan_blocks (K6)   a lane per item: the stacked test of the item's run starts - for a run along x a
//                         walk over the words it covers, for the runs along y of a word all 64 bits at once row by row -, the
//                         rectangle-start mask kept in rstarts[item], its popcount summed over the block -> boff[block].
//   k_rects_write         K14's write over the kept masks: slot -> item -> bit -> run length (fa_run_length) and height: rows
//                         along the stack axis while the bit is a run start (fa_starts) and no rectangle start (the kept mask)
//                         -> corners over both extents (fa_quad).  The body and the stores are K14's (fa_write_blocks).
// The equality of a run with the one before it is tested once, in the count, by the lane of the run's item; the write of a
// rectangle of L x H faces costs L / 64 + H steps (L + H for d < 2).  No atomics, no private segment.

// ---- stacked runs -> rectangle starts -> heights --------------------------------------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_rects.py compiles this part for the host behind K14's.)

// the row before (y, z) along the stack axis of direction d; false if there is none
O2V_FA_FN bool rc_row_before(uint32_t d, int64_t &y, int64_t &z)
{
    if (d >= 4u) --y;
    else --z;
    return y >= 0 && z >= 0;
}

O2V_FA_FN uint64_t rc_continues(const FaBits &b, const FaGrid &g, uint32_t d, int64_t wx, int64_t y, int64_t z)
{
    return fa_continues(b, g, d, wx, y, z, fa_exposed(b.solid, g, d, wx, y, z));
}

// the run starts of item (d, wx, y, z) that are stacked on a run of the row before: same first bit, same length, same colour
O2V_FA_FN uint64_t rc_stacked(const FaBits &b, const unsigned long long *same_z, const FaGrid &g, uint32_t d, int64_t wx, int64_t y, int64_t z)
{
    int64_t py = y, pz = z;
    if (!rc_row_before(d, py, pz)) return 0;
    const uint64_t e = fa_exposed(b.solid, g, d, wx, y, z);
    if (!e) return 0;
    const uint64_t ep = fa_exposed(b.solid, g, d, wx, py, pz);
    if (!ep) return 0;
    const uint64_t c = fa_continues(b, g, d, wx, y, z, e), cp = fa_continues(b, g, d, wx, py, pz, ep);
    uint64_t cand = e & ~c & ep & ~cp;   // both rows begin a run here ...
    if (g.colored && cand) cand &= fa_word(d >= 4u ? b.same_y : same_z, g, wx, y, z);   // ... of one colour
#ifdef O2V_RC_MUTATE_NO_LENGTH
    return cand;   // (test only: the equality ignores the lengths)
#else
    if (!cand) return 0;
    if (d < 2u) {
        // runs along y, all bits of the word at once: a run and the one before it must continue or end together in every row
        uint64_t live = cand, before = e, before_p = ep;
        for (int64_t r = y + 1; live && r < (int64_t) g.ny; ++r) {
            const uint64_t er = fa_exposed(b.solid, g, d, wx, r, z), erp = fa_exposed(b.solid, g, d, wx, r, pz);
            uint64_t cr = er & before, crp = erp & before_p;
            if (g.colored && cr) cr &= fa_word(b.same_y, g, wx, r, z);
            if (g.colored && crp) crp &= fa_word(b.same_y, g, wx, r, pz);
            cand &= ~(live & (cr ^ crp));
            live &= cr & cand;
            before = er, before_p = erp;
        }
        return cand;   // (past the last row both end)
    }
    // runs along x: the continuation bits of both rows agree over (bit, bit + length], the bit behind the run included
    const uint64_t diff = c ^ cp;
    uint64_t out = 0;
    for (uint64_t m = cand; m; m &= m - 1u) {
        const uint32_t bit = fa_ctz64(m);
        const uint32_t ones = bit == 63u ? 0u : fa_ctz64(~(c >> (bit + 1u)));
        if (bit + ones < 63u) {   // the run ends inside the word: bits bit + 1 .. bit + ones + 1
            if (!(diff & ((2ull << ones) - 1u) << (bit + 1u))) out |= 1ull << bit;
            continue;
        }
        if (bit < 63u && (diff >> (bit + 1u))) continue;
        bool equal = true;   // (past the last word both end)
        for (int64_t w = wx + 1; w < (int64_t) g.W; ++w) {
            const uint64_t cw = rc_continues(b, g, d, w, y, z), cpw = rc_continues(b, g, d, w, py, pz);
            if (cw != ~0ull) {
                const uint32_t t = fa_ctz64(~cw);   // the run ends before bit t of this word
                equal = !((cw ^ cpw) & (t == 63u ? ~0ull : (2ull << t) - 1u));
                break;
            }
            if (cpw != ~0ull) {
                equal = false;
                break;
            }
        }
        if (equal) out |= 1ull << bit;
    }
    return out;
#endif
}

// the run starts of item (d, wx, y, z) that begin a rectangle
O2V_FA_FN uint64_t rc_rect_starts(const FaBits &b, const unsigned long long *same_z, const FaGrid &g, uint32_t d, int64_t wx, int64_t y, int64_t z)
{
    const uint64_t s = fa_starts(b, g, d, wx, y, z);
    return s ? s & ~rc_stacked(b, same_z, g, d, wx, y, z) : 0;
}

O2V_FA_FN uint64_t rc_item(const FaGrid &g, uint32_t d, int64_t wx, int64_t y, int64_t z)
{
    return (((uint64_t) z * g.ny + (uint64_t) y) * 6u + d) * g.W + (uint64_t) wx;
}

// the rows of the rectangle that begins at `bit` of item (d, wx, y, z): a row behind it belongs to it while the bit begins a run
// there that is no rectangle start (rstarts: the kept masks of all items) - by definition a run equal to the one before it
O2V_FA_FN uint32_t rc_height(const FaBits &b, const FaGrid &g, const unsigned long long *rstarts, uint32_t d, int64_t wx, int64_t y, int64_t z,
                             uint32_t bit)
{
    uint32_t h = 1u;
    for (;; ++h) {
        if (d >= 4u) ++y;
        else ++z;
        if (y >= (int64_t) g.ny || z >= (int64_t) g.nz) break;
        if (rstarts[rc_item(g, d, wx, y, z)] >> bit & 1u) break;
        if (!(fa_starts(b, g, d, wx, y, z) >> bit & 1u)) break;
    }
    return h;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_FA_HOST

// same_z[wi] bit x: voxels (x, y, z) and (x, y, z - 1) are solid and of one colour
template <uint32_t Mode>
__global__ __launch_bounds__(kBlock) void k_rects_same_z(FaGrid g, const unsigned long long *__restrict__ solid, GaColor col,
                                                         unsigned long long *__restrict__ same_z)
{
    __shared__ uint32_t s_pal[Mode == kGaColorPalette ? 256 : 1];
    bits_palette_to_lds<Mode == kGaColorPalette>(col.palette, s_pal, true);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t layer = (uint64_t) g.W * g.ny;
    for (const uint64_t wi : bits_words(g)) {
        const uint64_t both = wi >= layer ? solid[wi] & solid[wi - layer] : 0ull;
        unsigned long long mz = 0;
        if (both) {
            const BitWord at = bits_word_at(g, wi);
            const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z;   // (a solid bit is inside the box)
            const bool me = both >> lane & 1u;
            const uint32_t c = me ? ga_color_at<Mode>(col, s_pal, x, y, z) : 0u;
            const uint32_t cb = me ? ga_color_at<Mode>(col, s_pal, x, y, z - 1u) : 0u;
            mz = __ballot(me && c == cb);
        }
        if (lane == 0u) same_z[wi] = mz;
    }
}

// rstarts[item] = the item's rectangle starts; block_sums[block] = the rectangles that begin in the block's items
__global__ __launch_bounds__(kBlock) void k_rects_count(FaGrid g, FaBits b, const unsigned long long *__restrict__ same_z,
                                                        unsigned long long *__restrict__ rstarts, unsigned long long *__restrict__ block_sums)
{
    fa_count_blocks(g, block_sums, [&](uint64_t item, uint32_t d, uint32_t wx, uint32_t y, uint32_t z) {
        return rstarts[item] = rc_rect_starts(b, same_z, g, d, wx, y, z);
    });
}

// rectangle q of the numbering -> positions[12 q ..], faces[6 q ..] (if not null), quad_argb[q] (if not null): the kept masks,
// a run's length as K14 finds it and the height by rc_height
template <uint32_t Mode>
__global__ __launch_bounds__(kBlock) void k_rects_write(FaGrid g, FaBits b, const unsigned long long *__restrict__ rstarts,
                                                        const unsigned long long *__restrict__ boff, uint32_t ox, uint32_t oy, uint32_t oz, GaColor col,
                                                        float4 *__restrict__ positions, int2 *__restrict__ faces, uint32_t *__restrict__ quad_argb)
{
    fa_write_blocks<Mode>(
        g, boff, ox, oy, oz, col, positions, faces, quad_argb, [&](uint64_t item, uint32_t, uint32_t, uint32_t, uint32_t) { return (uint64_t) rstarts[item]; },
        [&](uint32_t d, uint32_t wx, uint32_t y, uint32_t z, uint32_t bit, uint32_t &len, uint32_t &height) {
            len = fa_run_length(b, g, d, wx, y, z, bit), height = rc_height(b, g, rstarts, d, wx, y, z, bit);
        });
}

#endif   // O2V_FA_HOST
