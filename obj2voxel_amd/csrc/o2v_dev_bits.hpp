// o2v_dev_bits.hpp -- the bit grid that K12, K13, K14, K16 and K20 read, and what they all do with it.  Included from
// o2v_device.hip inside its anonymous namespace, behind K11 and before K12.
//
// A classified set is one bit per voxel: 64-bit words along x, [z][y][W = ceil(nx / 64)], padding bits 0, written by K12's
// k_cc_classify.  Word wi = (z * ny + y) * W + wx holds the voxels x = wx * 64 + bit of row (y, z).  A tile is 64 x 8 x 8
// voxels - one word of each of 64 rows, row = ty + 8 tz within the tile -, tile = (tz * tiles_y + ty) * W + tx.

#ifndef O2V_BITS_HOST
#define O2V_BITS_FN __device__ __forceinline__
#endif

// ---- the layout: word <-> coordinates, membership, the faces of the box, tiles -----------------------------------------------
// (Plain C++ from here to the wavefronts: tests/test_host_bits.py compiles this part for the host with an O2V_BITS_FN of its
// own, and the host tests of K12, K14, K16 and K20 put it in front of their family's plain part.)

struct BitGrid {
    uint32_t nx, ny, nz, W;   // W = ceil(nx / 64) words per row
    uint64_t words;           // W * ny * nz
};

struct BitWord {
    uint32_t wx, y, z;   // the word's place in its row, the row
};

O2V_BITS_FN uint64_t bits_word_index(const BitGrid &g, uint32_t wx, uint32_t y, uint32_t z) { return ((uint64_t) z * g.ny + y) * g.W + wx; }

// Word wi (below g.words) -> (wx, y, z).  32-bit divisions are enough: every caller's host side refuses a grid whose words do
// not fit 31 bits - index_limits (K12, K20: at most 2^31 - 1 voxels, and a word holds at least one) and ga_grid (K13, K14, K16:
// at most kGaMaxWords = 2^31 - 1 words).  (wi is 64-bit where the walks count it.)
O2V_BITS_FN BitWord bits_word_at(const BitGrid &g, uint64_t wi)
{
    const uint32_t w32 = (uint32_t) wi, row = w32 / g.W, z = row / g.ny;
    return BitWord{w32 - row * g.W, row - z * g.ny, z};
}

// is voxel (x, y, z) of the box in the set
O2V_BITS_FN bool bits_has(const BitGrid &g, const unsigned long long *bits, uint32_t x, uint32_t y, uint32_t z)
{
    return ((bits[bits_word_index(g, x >> 6, y, z)] >> (x & 63u)) & 1ull) != 0ull;
}

// is (x, y, z) on one of the six faces of the box (x may lie in a word's padding: that is no face)
O2V_BITS_FN bool bits_on_face(const BitGrid &g, uint32_t x, uint32_t y, uint32_t z)
{
    return y == 0u || y == g.ny - 1u || z == 0u || z == g.nz - 1u || x == 0u || x == g.nx - 1u;
}

// tile -> (tx, ty, tz); tiles_y = ceil(ny / 8).  The tiles are no more than the words, so 32 bits again.
O2V_BITS_FN void bits_tile_at(const BitGrid &g, uint32_t tiles_y, uint32_t tile, uint32_t &tx, uint32_t &ty, uint32_t &tz)
{
    const uint32_t trow = tile / g.W;
    tx = tile - trow * g.W;
    tz = trow / tiles_y;
    ty = trow - tz * tiles_y;
}

// the word of row 0 .. 63 of tile (tx, ty, tz); 0 for a row outside the box
O2V_BITS_FN uint64_t bits_tile_word(const BitGrid &g, const unsigned long long *bits, uint32_t tx, uint32_t ty, uint32_t tz, uint32_t row)
{
    const uint32_t y = ty * 8u + (row & 7u), z = tz * 8u + (row >> 3);
    return y < g.ny && z < g.nz ? bits[bits_word_index(g, tx, y, z)] : 0ull;
}

// ---- wavefronts: the walk over the words, the sum of their counts, the palette ---------------------------------------------------
#ifndef O2V_BITS_HOST

// A wavefront per turn, the wavefronts of the grid in turns: for (const uint64_t i : WaveTurns{n}) runs i = this wavefront's
// index, then every (wavefronts of the grid)-th, below n - uniform over the wavefront.
struct WaveTurns {
    uint64_t n;
    struct Turn {
        uint64_t i, step;
        __device__ __forceinline__ uint64_t operator*() const { return i; }
        __device__ __forceinline__ void operator++() { i += step; }
        __device__ __forceinline__ bool operator!=(const Turn &end) const { return i < end.i; }
    };
    __device__ __forceinline__ Turn begin() const
    {
        return Turn{(uint64_t) blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6), (uint64_t) gridDim.x * (kBlock / 64u)};
    }
    __device__ __forceinline__ Turn end() const { return Turn{n, 0u}; }
};

// a wavefront per word of the grid, a lane per voxel of the word: for (const uint64_t wi : bits_words(g))
__device__ __forceinline__ WaveTurns bits_words(const BitGrid &g) { return WaveTurns{g.words}; }

// *total += the sum over the workgroup's wavefronts of `mine` (the same in every lane of a wavefront): one atomic per workgroup
__device__ __forceinline__ void bits_add_wave_sums(unsigned long long mine, unsigned long long *total)
{
    __shared__ unsigned long long s_sum[kBlock / 64];
    if ((threadIdx.x & 63u) == 0u) s_sum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (uint32_t w = 0; w < kBlock / 64u; ++w) sum += s_sum[w];
        if (sum) atomicAdd(total, sum);
    }
}

// The 256 colours of a palette into s_pal, a thread each (On: the kernel's colour mode reads a palette; else s_pal is one unused
// word).  barrier = false: the caller's next __syncthreads publishes them.
template <bool On>
__device__ __forceinline__ void bits_palette_to_lds(const uint32_t *__restrict__ palette, uint32_t *s_pal, bool barrier)
{
    static_assert(kBlock == 256u, "a thread per palette entry");
    if (!On) return;
    s_pal[threadIdx.x] = palette[threadIdx.x];
    if (barrier) __syncthreads();
}

#endif   // O2V_BITS_HOST
