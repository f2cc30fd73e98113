// o2v_dev_k10_surface.hpp -- K10: the level set of a dense float32 grid as an indexed triangle mesh, by surface nets
// (o2v_hip_surface_count / o2v_hip_surface_write).  Included from o2v_device.hip inside its anonymous namespace; compiled with
// -ffp-contract=off (o2v_math.h): a vertex is evaluated op by op in float32 exactly as include/o2v_hip.h writes it, so a numpy
// restatement reproduces every bit.
//
// The grid is cut into words of 64 samples along x: W = ceil(nx / 64) words per row (y, z), item = (z ny + y) W + w.  Cells
// and grid edges are filed under the item of their lowest sample, so one index space serves the signs, the active cells and
// the quads.  Per item the context keeps (20 bytes per 64 samples)
//   signs[item]    bit b: f(64 w + b, y, z) < level (0 past nx)
//   active[item]   bit b: cell (64 w + b, y, z) is active
//   local[item]    the active cells (low half) and quads (high half) of the items before it in its block of kBlock items
//   voff / qoff    per block: the vertices / quads of the blocks before it; one more entry: all of them
// Count:
//   k_surf_signs     the only pass over the field: a wavefront takes 64 consecutive x, one dword per lane, and its ballot is
//                    the sign word; kSurfInFlight words per wavefront are loaded before the first ballot
//   k_surf_count     a lane per item, on the sign words only: the masks of its active cells and of its crossing, interior
//                    edges along x, y, z from the words of the four rows (y, z) .. (y + 1, z + 1) by shifts, AND, OR, XOR; their
//                    popcounts scanned over the block
//   k_fill_scan_blocks (K6) twice: the block sums -> voff, qoff and the two totals the host reads
// Write (lanes -> outputs, so a wavefront's stores cover one contiguous range; a block without output leaves at once):
//   k_surf_vertices  a block's items in LDS; output slot -> item (search of the prefixes) -> bit (select by popcounts) -> the cell;
//                    its eight corners' signs from the kept words and values from the field (two samples along x in one
//                    load where the x stride is 1); 12 bytes per lane
//   k_surf_faces     the same for the quads; the four cells' numbers are voff + local + popcount(active below the bit);
//                    24 bytes per lane
// No atomics: every order comes from the scans.

constexpr uint32_t kSurfInFlight = 8;   // sign words a wavefront loads before its first ballot: 2 KiB per wavefront, 64 KiB per CU

struct SurfGrid {
    uint64_t s0, s1, s2;   // element strides of the field (x, y, z)
    uint32_t nx, ny, nz;
    uint32_t W;            // words per row
    uint64_t items;        // ny nz W
    uint64_t n_blocks;     // of kBlock items
    float level;
};

struct SurfItem {
    uint32_t w, j, k;
};

// rows = ny nz <= 2^32 (dims <= 65 536): a row index fits 32 bits; the items of any grid that fits a device do too
__device__ __forceinline__ SurfItem surf_item(const SurfGrid &g, uint64_t item)
{
    uint32_t row, w;
    if (g.items <= 0xffffffffull) {
        row = (uint32_t) item / g.W;
        w = (uint32_t) item - row * g.W;
    } else {
        const uint64_t r = item / g.W;
        row = (uint32_t) r;
        w = (uint32_t) (item - r * g.W);
    }
    const uint32_t k = row / g.ny;
    return SurfItem{w, row - k * g.ny, k};
}

__device__ __forceinline__ uint64_t surf_index(const SurfGrid &g, uint32_t w, uint32_t j, uint32_t k)
{
    return ((uint64_t) k * g.ny + j) * g.W + w;
}

__device__ __forceinline__ uint64_t surf_below(uint32_t bit) { return (1ull << bit) - 1ull; }   // (bit < 64)

// the word of the samples x + 1: `word` moved down by one, bit 0 of the next word of the row on top
__device__ __forceinline__ uint64_t surf_next(const unsigned long long *__restrict__ signs, const SurfGrid &g, uint64_t index, uint32_t w,
                                              uint64_t word)
{
    const uint64_t n = w + 1u < g.W ? signs[index + 1u] & 1ull : 0ull;
    return (word >> 1) | (n << 63);
}

struct SurfMasks {
    uint64_t in;          // the item's sign word
    uint64_t active;      // cells
    uint64_t qx, qy, qz;  // crossing edges from the sample along x, y, z with four cells around them
};

__device__ __forceinline__ SurfMasks surf_masks(const unsigned long long *__restrict__ signs, const SurfGrid &g, SurfItem it)
{
    SurfMasks m{};
    const uint64_t at = surf_index(g, it.w, it.j, it.k);
    const uint64_t r00 = signs[at];
    m.in = r00;
    const uint32_t x0 = it.w * 64u, cells = g.nx - 1u;
    const uint64_t mc = cells <= x0 ? 0ull : (cells - x0 >= 64u ? ~0ull : surf_below(cells - x0));   // x <= nx - 2
    const uint64_t mi = it.w == 0u ? mc & ~1ull : mc;                                                 // 1 <= x <= nx - 2
    const bool jc = it.j + 1u < g.ny, kc = it.k + 1u < g.nz;   // the row above / the layer above exists
    const bool ji = jc && it.j >= 1u, ki = kc && it.k >= 1u;   // 1 <= y <= ny - 2, 1 <= z <= nz - 2
    if (mc == 0ull || !(jc || kc)) return m;
    const uint64_t up = g.W, over = (uint64_t) g.W * g.ny;
    const uint64_t r10 = jc ? signs[at + up] : 0ull, r01 = kc ? signs[at + over] : 0ull;
    if (jc && kc) {
        const uint64_t r11 = signs[at + up + over];
        const uint64_t s00 = surf_next(signs, g, at, it.w, r00), s10 = surf_next(signs, g, at + up, it.w, r10);
        const uint64_t s01 = surf_next(signs, g, at + over, it.w, r01), s11 = surf_next(signs, g, at + up + over, it.w, r11);
        const uint64_t all = r00 & r10 & r01 & r11 & s00 & s10 & s01 & s11, any = r00 | r10 | r01 | r11 | s00 | s10 | s01 | s11;
        m.active = any & ~all & mc;
        if (ji && ki) m.qx = (r00 ^ s00) & mc;
    }
    if (jc && ki) m.qy = (r00 ^ r10) & mi;
    if (kc && ji) m.qz = (r00 ^ r01) & mi;
    return m;
}

// the position of the r-th set bit of m (r below its popcount)
__device__ __forceinline__ uint32_t surf_select(uint64_t m, uint32_t r)
{
    uint32_t p = 0;
#pragma unroll
    for (uint32_t width = 32; width; width >>= 1) {
        const uint32_t c = (uint32_t) __popcll((m >> p) & surf_below(width));
        if (r >= c) {
            r -= c;
            p += width;
        }
    }
    return p;
}

__global__ __launch_bounds__(kBlock) void k_surf_signs(const float *__restrict__ f, SurfGrid g, unsigned long long *__restrict__ signs)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t) blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6), n_waves = (uint64_t) gridDim.x * (kBlock / 64u);
    for (uint64_t first = wave * kSurfInFlight; first < g.items; first += n_waves * kSurfInFlight) {
        SurfItem it = surf_item(g, first);
        float v[kSurfInFlight];
#pragma unroll
        for (uint32_t u = 0; u < kSurfInFlight; ++u) {
            const uint32_t x = it.w * 64u + lane;
            v[u] = __builtin_nanf("");
            if (first + u < g.items && x < g.nx) v[u] = f[x * g.s0 + it.j * g.s1 + it.k * g.s2];
            if (++it.w == g.W) {
                it.w = 0;
                if (++it.j == g.ny) {
                    it.j = 0;
                    ++it.k;
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kSurfInFlight; ++u) {
            const unsigned long long m = __ballot(v[u] < g.level);
            if (lane == u && first + u < g.items) signs[first + u] = m;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_surf_count(const unsigned long long *__restrict__ signs, SurfGrid g,
                                                       unsigned long long *__restrict__ active, uint32_t *__restrict__ local,
                                                       unsigned long long *__restrict__ v_sums, unsigned long long *__restrict__ q_sums)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    for (uint64_t b = blockIdx.x; b < g.n_blocks; b += gridDim.x) {
        const uint64_t item = b * kBlock + threadIdx.x;
        uint64_t both = 0;   // vertices in the low half, quads in the high half: a block has at most 2^14 and 3 x 2^14
        if (item < g.items) {
            const SurfMasks m = surf_masks(signs, g, surf_item(g, item));
            active[item] = m.active;
            both = (uint64_t) __popcll(m.active) | (uint64_t) (__popcll(m.qx) + __popcll(m.qy) + __popcll(m.qz)) << 32;
        }
        uint64_t total;
        const uint64_t ex = fill_block_exscan64(both, s_wave, total);
        if (item < g.items) local[item] = (uint32_t) ex | (uint32_t) (ex >> 32) << 16;
        if (threadIdx.x == 0) {
            v_sums[b] = total & 0xffffffffull;
            q_sums[b] = total >> 32;
        }
    }
}

// the item of the block (its prefixes in s_pref, kBlock of them, past the grid: n) that holds output slot `slot` < n
__device__ __forceinline__ uint32_t surf_find(const uint32_t *s_pref, uint32_t slot)
{
    uint32_t l = 0;
#pragma unroll
    for (uint32_t step = kBlock / 2; step; step >>= 1)
        if (s_pref[l + step] <= slot) l += step;
    return l;
}

// t of a crossing edge from p to q
__device__ __forceinline__ float surf_t(float level, float fp, float fq)
{
    const float t = (level - fp) / (fq - fp);
    return t >= 0.f && t <= 1.f ? t : 0.5f;
}

// two consecutive samples along x
struct alignas(4) SurfPair {
    float lo, hi;
};

// UnitX: the x stride is 1, and a cell's two samples of a row come in one 8-byte load
template <bool UnitX>
__global__ __launch_bounds__(kBlock) void k_surf_vertices(const float *__restrict__ f, SurfGrid g, const unsigned long long *__restrict__ signs,
                                                          const unsigned long long *__restrict__ active, const uint32_t *__restrict__ local,
                                                          const unsigned long long *__restrict__ voff, uint32_t ox, uint32_t oy, uint32_t oz,
                                                          float *__restrict__ positions)
{
    __shared__ uint32_t s_pref[kBlock];
    __shared__ uint64_t s_mask[kBlock];
    for (uint64_t b = blockIdx.x; b < g.n_blocks; b += gridDim.x) {
        const uint64_t base = voff[b];
        const uint32_t n = (uint32_t) (voff[b + 1] - base);
        if (n == 0u) continue;   // (uniform over the block)
        __syncthreads();         // (the arrays of the block before have been read)
        {
            const uint64_t item = b * kBlock + threadIdx.x;
            s_pref[threadIdx.x] = item < g.items ? local[item] & 0xffffu : n;   // (past the grid: no slot is below n)
            s_mask[threadIdx.x] = item < g.items ? active[item] : 0ull;
        }
        __syncthreads();
        for (uint32_t slot = threadIdx.x; slot < n; slot += kBlock) {
            const uint32_t l = surf_find(s_pref, slot);
            const uint32_t bit = surf_select(s_mask[l], slot - s_pref[l]);
            const SurfItem it = surf_item(g, b * kBlock + l);
            const uint32_t i = it.w * 64u + bit;
            // the corners (a, b, c) at index a + 2 b + 4 c: inside from the kept words, values from the field
            bool in[8];
            float v[8];
            const uint64_t at = surf_index(g, it.w, it.j, it.k);
#pragma unroll
            for (uint32_t c = 0; c < 2; ++c)
#pragma unroll
                for (uint32_t bb = 0; bb < 2; ++bb) {
                    const uint64_t row = at + (bb ? g.W : 0u) + (c ? (uint64_t) g.W * g.ny : 0u);
                    const uint64_t word = signs[row];
                    in[2 * bb + 4 * c] = (word >> bit) & 1ull;
                    in[1 + 2 * bb + 4 * c] = (bit < 63u ? word >> (bit + 1u) : signs[row + 1u]) & 1ull;
                    const float *q = f + i * g.s0 + (it.j + bb) * g.s1 + (it.k + c) * g.s2;
                    if (UnitX) {
                        const SurfPair pair = *reinterpret_cast<const SurfPair *>(q);
                        v[2 * bb + 4 * c] = pair.lo;
                        v[1 + 2 * bb + 4 * c] = pair.hi;
                    } else {
                        v[2 * bb + 4 * c] = q[0];
                        v[1 + 2 * bb + 4 * c] = q[g.s0];
                    }
                }
            float sx = 0.f, sy = 0.f, sz = 0.f;
            uint32_t crossings = 0;
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) {   // x edges (0, b, c) - (1, b, c)
                const uint32_t p = 2 * (e & 1u) + 4 * (e >> 1);
                if (in[p] != in[p + 1]) {
                    sx = sx + surf_t(g.level, v[p], v[p + 1]);
                    sy = sy + (float) (e & 1u);
                    sz = sz + (float) (e >> 1);
                    ++crossings;
                }
            }
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) {   // y edges (a, 0, c) - (a, 1, c)
                const uint32_t p = (e & 1u) + 4 * (e >> 1);
                if (in[p] != in[p + 2]) {
                    sx = sx + (float) (e & 1u);
                    sy = sy + surf_t(g.level, v[p], v[p + 2]);
                    sz = sz + (float) (e >> 1);
                    ++crossings;
                }
            }
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) {   // z edges (a, b, 0) - (a, b, 1)
                const uint32_t p = (e & 1u) + 2 * (e >> 1);
                if (in[p] != in[p + 4]) {
                    sx = sx + (float) (e & 1u);
                    sy = sy + (float) (e >> 1);
                    sz = sz + surf_t(g.level, v[p], v[p + 4]);
                    ++crossings;
                }
            }
            const float n_f = (float) crossings;   // (at least 1: the cell is active by the same words)
            float *o = positions + (base + slot) * 3u;
            o[0] = ((float) (ox + i) + 0.5f) + sx / n_f;
            o[1] = ((float) (oy + it.j) + 0.5f) + sy / n_f;
            o[2] = ((float) (oz + it.k) + 0.5f) + sz / n_f;
        }
    }
}

// the number of the vertex of cell (i, j, k), which is active
__device__ __forceinline__ int32_t surf_vertex(const SurfGrid &g, const unsigned long long *__restrict__ active, const uint32_t *__restrict__ local,
                                               const unsigned long long *__restrict__ voff, uint32_t i, uint32_t j, uint32_t k)
{
    const uint64_t item = surf_index(g, i >> 6, j, k);
    return (int32_t) (voff[item / kBlock] + (local[item] & 0xffffu) + (uint32_t) __popcll(active[item] & surf_below(i & 63u)));
}

__global__ __launch_bounds__(kBlock) void k_surf_faces(SurfGrid g, const unsigned long long *__restrict__ signs,
                                                       const unsigned long long *__restrict__ active, const uint32_t *__restrict__ local,
                                                       const unsigned long long *__restrict__ voff, const unsigned long long *__restrict__ qoff,
                                                       int32_t *__restrict__ faces)
{
    __shared__ uint32_t s_pref[kBlock];
    __shared__ uint64_t s_in[kBlock], s_q[3][kBlock];
    for (uint64_t b = blockIdx.x; b < g.n_blocks; b += gridDim.x) {
        const uint64_t base = qoff[b];
        const uint32_t n = (uint32_t) (qoff[b + 1] - base);
        if (n == 0u) continue;   // (uniform over the block)
        __syncthreads();         // (the arrays of the block before have been read)
        {
            const uint64_t item = b * kBlock + threadIdx.x;
            SurfMasks m{};
            if (item < g.items) m = surf_masks(signs, g, surf_item(g, item));
            s_pref[threadIdx.x] = item < g.items ? local[item] >> 16 : n;
            s_in[threadIdx.x] = m.in;
            s_q[0][threadIdx.x] = m.qx;
            s_q[1][threadIdx.x] = m.qy;
            s_q[2][threadIdx.x] = m.qz;
        }
        __syncthreads();
        for (uint32_t slot = threadIdx.x; slot < n; slot += kBlock) {
            const uint32_t l = surf_find(s_pref, slot);
            const uint64_t qx = s_q[0][l], qy = s_q[1][l], qz = s_q[2][l];
            const uint32_t r = slot - s_pref[l];
            // quads in the order of (x, axis): the last bit with at most r quads below it, then the axes of that bit in turn
            uint32_t bit = 0, below = 0;
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1) {
                const uint64_t mask = surf_below(bit + step);
                const uint32_t c = (uint32_t) (__popcll(qx & mask) + __popcll(qy & mask) + __popcll(qz & mask));
                if (c <= r) {
                    bit += step;
                    below = c;
                }
            }
            uint32_t rem = r - below, ax = 0;
            const uint32_t has_x = (uint32_t) (qx >> bit) & 1u, has_y = (uint32_t) (qy >> bit) & 1u;
            if (has_x && rem == 0u) ax = 0;
            else if (has_y && rem == has_x) ax = 1;
            else ax = 2;
            const SurfItem it = surf_item(g, b * kBlock + l);
            const uint32_t c[3] = {it.w * 64u + bit, it.j, it.k};
            // u = (ax + 1) % 3, v = (ax + 2) % 3; the cells c - e_u - e_v, c - e_v, c, c - e_u
            const uint32_t du[3] = {ax == 2u, ax == 0u, ax == 1u}, dv[3] = {ax == 1u, ax == 2u, ax == 0u};
            const int32_t n0 = surf_vertex(g, active, local, voff, c[0] - du[0] - dv[0], c[1] - du[1] - dv[1], c[2] - du[2] - dv[2]);
            const int32_t n1 = surf_vertex(g, active, local, voff, c[0] - dv[0], c[1] - dv[1], c[2] - dv[2]);
            const int32_t n2 = surf_vertex(g, active, local, voff, c[0], c[1], c[2]);
            const int32_t n3 = surf_vertex(g, active, local, voff, c[0] - du[0], c[1] - du[1], c[2] - du[2]);
            const bool inside = (s_in[l] >> bit) & 1ull;
            int32_t *o = faces + (base + slot) * 6u;
            o[0] = o[3] = n0;
            o[1] = inside ? n1 : n3;
            o[2] = o[4] = n2;
            o[5] = inside ? n3 : n1;
        }
    }
}
