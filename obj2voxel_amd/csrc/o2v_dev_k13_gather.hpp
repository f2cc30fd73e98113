// o2v_dev_k13_gather.hpp -- K13: the solid voxels of a dense grid as (x, y, z, argb) records (o2v_hip_gather_count / _write /
// _save).  Included from o2v_device.hip inside its anonymous namespace, after K12 (whose classify kernel it uses) and
// o2v_dev_bits.hpp (the bit grid and its words).
//
// The set (include/o2v_hip.h) is classified once into the bit grid of o2v_dev_bits.hpp by K12's k_cc_classify (invert = 0).  Word
// wi holds the voxels of linear indices (wi / W) * nx + (wi % W) * 64 + bit,
// so the set bits in ascending (word, bit) order are the solid voxels in ascending linear index: record i is the i-th set bit.
//
//   k_cc_classify (K12)                    the only pass over the grid.
//   k_gather_count + k_fill_scan_blocks (K6)   a lane per word: popcount, exclusive scan over the block of 256 words
//                   (fill_block_exscan64) -> local[wi], the records of the block's words before wi (below 2^14); the block's
//                   sum -> boff[block]; the scan of the sums in place -> boff[block] = the records before the block (64-bit),
//                   boff[n_blocks] = the count.
//   k_gather_find   one workgroup: the block that holds record `first` - the last block b with boff[b] <= first - by a search
//                   with 256 probes a round over the block offsets (three rounds for 2^23 blocks) -> *b_first.
//   k_gather_write  lanes -> records, so a wavefront's stores cover 1 KiB contiguously: workgroups take the blocks from *b_first
//                   on in turns and leave at the first block that begins at or past first + n (one read).  A block's words,
//                   prefixes and word coordinates go to LDS; output slot -> word (search of the prefixes) -> bit (select the
//                   r-th set bit by popcounts) -> (x, y, z); then the colour (constant, colour grid, or palette[grid byte]) and
//                   one 16-byte store.  Occupancy comes from the kept bits only.
// No atomics, no private segment: every order comes from the scans.

constexpr uint32_t kGaFan = 256u;            // probes per round of the block search: a workgroup
constexpr uint32_t kGaColorConstant = 0, kGaColorGrid = 1, kGaColorPalette = 2;   // O2V_HIP_GATHER_COLOR_*

#ifndef O2V_GA_HOST
#define O2V_GA_FN __device__ __forceinline__
O2V_GA_FN uint32_t ga_popc64(uint64_t v) { return (uint32_t) __popcll(v); }
#endif

// ---- slot -> block -> word -> bit --------------------------------------------------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_gather.py compiles this part for the host, with O2V_GA_FN and ga_popc64
// of its own, and runs it against the reference.)

// The block search.  The block of record `slot` (below the count) is the last b in [0, n_blocks) with boff[b] <= slot; it is
// kept in [lo, hi) with boff[lo] <= slot.  A round probes lo + t * step for t = 0 .. kGaFan - 1; the probes that are in the
// interval and at or below the slot are the first c of them (boff rises, and probe 0 is lo itself), which narrows the
// interval to the step behind the last of those.
O2V_GA_FN uint64_t ga_step(uint64_t lo, uint64_t hi) { return (hi - lo + kGaFan - 1u) / kGaFan; }
O2V_GA_FN bool ga_probe_hit(const unsigned long long *boff, uint64_t lo, uint64_t hi, uint64_t step, uint32_t t, uint64_t slot)
{
    const uint64_t p = lo + (uint64_t) t * step;
#ifdef O2V_GA_MUTATE_SEARCH
    return p < hi && boff[p] <= slot + 1u;   // (test only: a range that begins at the last record of a block loses that block)
#else
    return p < hi && boff[p] <= slot;
#endif
}
O2V_GA_FN void ga_narrow(uint64_t &lo, uint64_t &hi, uint64_t step, uint32_t c)
{
    lo += (uint64_t) (c ? c - 1u : 0u) * step;
    if (lo + step < hi) hi = lo + step;
}

// the word of a block (its prefixes in pref, kBlock of them; past the grid: the block's count n) that holds slot < n: the last
// l with pref[l] <= slot
O2V_GA_FN uint32_t ga_find_word(const uint32_t *pref, uint32_t slot)
{
    uint32_t l = 0;
    for (uint32_t step = 128u; step; step >>= 1)
        if (pref[l + step] <= slot) l += step;
    return l;
}

// the position of the r-th set bit of m (r below its popcount)
O2V_GA_FN uint32_t ga_select(uint64_t m, uint32_t r)
{
    uint32_t p = 0;
    for (uint32_t width = 32u; width; width >>= 1) {
        const uint32_t c = ga_popc64((m >> p) & ((1ull << width) - 1ull));
        if (r >= c) {
            r -= c;
            p += width;
        }
    }
    return p;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_GA_HOST

struct GaGrid : BitGrid {   // (words: at most 2^31 - 1)
    uint64_t n_blocks;      // of kBlock words
};

struct GaColor {
    uint32_t argb;                 // CONSTANT
    const uint32_t *colors;        // GRID: element strides (x, y, z)
    uint64_t c0, c1, c2;
    const uint8_t *grid;           // PALETTE: the U8 grid, element strides (x, y, z), and the 256 colours (device memory)
    uint64_t s0, s1, s2;
    const uint32_t *palette;
};

// the colour of voxel (x, y, z); s_pal: the palette in LDS (PALETTE)
template <uint32_t Mode>
__device__ __forceinline__ uint32_t ga_color_at(const GaColor &col, const uint32_t *s_pal, uint32_t x, uint32_t y, uint32_t z)
{
    if (Mode == kGaColorGrid) return col.colors[(uint64_t) x * col.c0 + (uint64_t) y * col.c1 + (uint64_t) z * col.c2];
    if (Mode == kGaColorPalette) return s_pal[col.grid[(uint64_t) x * col.s0 + (uint64_t) y * col.s1 + (uint64_t) z * col.s2]];
    return col.argb;
}

// local[wi] = the records of the words of wi's block before wi; block_sums[block] = the block's records
__global__ __launch_bounds__(kBlock) void k_gather_count(const unsigned long long *__restrict__ bits, GaGrid g, uint32_t *__restrict__ local,
                                                         unsigned long long *__restrict__ block_sums)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    for (uint64_t b = blockIdx.x; b < g.n_blocks; b += gridDim.x) {
        const uint64_t wi = b * kBlock + threadIdx.x;
        const uint64_t n = wi < g.words ? (uint64_t) __popcll(bits[wi]) : 0u;
        uint64_t total;
        const uint64_t ex = fill_block_exscan64(n, s_wave, total);
        if (wi < g.words) local[wi] = (uint32_t) ex;
        if (threadIdx.x == 0) block_sums[b] = total;
    }
}

// *b_first = the block of record `first` (below the count)
__global__ __launch_bounds__(kBlock) void k_gather_find(const unsigned long long *__restrict__ boff, uint64_t n_blocks, uint64_t first,
                                                        unsigned long long *__restrict__ b_first)
{
    __shared__ uint32_t s_hits[kBlock / 64];
    uint64_t lo = 0, hi = n_blocks;
    while (hi - lo > 1u) {   // (uniform over the workgroup)
        const uint64_t step = ga_step(lo, hi);
        const unsigned long long m = __ballot(ga_probe_hit(boff, lo, hi, step, threadIdx.x, first));
        __syncthreads();   // (the counts of the round before have been read)
        if ((threadIdx.x & 63u) == 0u) s_hits[threadIdx.x >> 6] = (uint32_t) __popcll(m);
        __syncthreads();
        uint32_t c = 0;
#pragma unroll
        for (uint32_t w = 0; w < kBlock / 64u; ++w) c += s_hits[w];
        ga_narrow(lo, hi, step, c);
    }
    if (threadIdx.x == 0) *b_first = lo;
}

// records[i - first] = record i for first <= i < first + n (n > 0, first + n at most the count)
template <uint32_t Mode>
__global__ __launch_bounds__(kBlock) void k_gather_write(GaGrid g, const unsigned long long *__restrict__ bits, const uint32_t *__restrict__ local,
                                                         const unsigned long long *__restrict__ boff, const unsigned long long *__restrict__ b_first,
                                                         uint64_t first, uint64_t n, uint32_t ox, uint32_t oy, uint32_t oz, GaColor col,
                                                         uint4 *__restrict__ records)
{
    __shared__ uint32_t s_pref[kBlock];
    __shared__ uint64_t s_word[kBlock];
    __shared__ uint32_t s_x0[kBlock], s_yz[kBlock];   // the word's first x; y | z << 16 (both below 2^16)
    __shared__ uint32_t s_pal[Mode == kGaColorPalette ? 256 : 1];
    static_assert(kBlock == 256u, "a lane per word of a block");
    bits_palette_to_lds<Mode == kGaColorPalette>(col.palette, s_pal, false);   // (the first barrier below publishes it)
    const uint64_t end = first + n;
    for (uint64_t b = *b_first + blockIdx.x; b < g.n_blocks; b += gridDim.x) {
        const uint64_t base = boff[b];
        if (base >= end) break;   // (uniform over the workgroup; boff rises, so no later block has a record of the range)
        const uint64_t stop = boff[b + 1];
        const uint32_t cnt = (uint32_t) (stop - base);   // at most 2^14
        const uint32_t slot_lo = first <= base ? 0u : first - base < cnt ? (uint32_t) (first - base) : cnt;
        const uint32_t slot_hi = end < stop ? (uint32_t) (end - base) : cnt;
        if (slot_lo >= slot_hi) continue;   // (uniform)
        __syncthreads();                    // (the arrays of the block before have been read)
        {
            const uint64_t wi = b * kBlock + threadIdx.x;
            const bool in = wi < g.words;
            s_pref[threadIdx.x] = in ? local[wi] : cnt;   // (past the grid: no slot is below cnt)
            s_word[threadIdx.x] = in ? bits[wi] : 0ull;
            const BitWord at = bits_word_at(g, wi);   // (past the grid: coordinates that no slot reads)
            s_x0[threadIdx.x] = at.wx * 64u;
            s_yz[threadIdx.x] = at.y | at.z << 16;
        }
        __syncthreads();
        for (uint32_t slot = slot_lo + threadIdx.x; slot < slot_hi; slot += kBlock) {
            const uint32_t l = ga_find_word(s_pref, slot);
            const uint32_t x = s_x0[l] + ga_select(s_word[l], slot - s_pref[l]);
            const uint32_t yz = s_yz[l], y = yz & 0xffffu, z = yz >> 16;
            records[base + slot - first] = make_uint4(ox + x, oy + y, oz + z, ga_color_at<Mode>(col, s_pal, x, y, z));
        }
    }
}

#endif   // O2V_GA_HOST
