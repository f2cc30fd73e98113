// o2v_dev_k29_label_surface.hpp -- K29: the interfaces of a label grid as one indexed triangle mesh, by surface nets on labels
// (o2v_hip_label_surface_count / _write / _relax).  Included from o2v_device.hip inside its anonymous namespace, behind K10: the
// words, the prefixes, the search and the select are K10's (SurfGrid, surf_item, surf_find, surf_select, surf_vertex).  Compiled
// with -ffp-contract=off (o2v_math.h): the relaxation is evaluated op by op in float32 exactly as include/o2v_hip.h writes it.
//
// The extended lattice (the box, and one layer of label 0 around it if closed: E = 1) is cut into words of 64 samples along x, as
// K10 cuts its field: the SurfGrid here holds the extended dims, item = (z Y + y) W + w.  Per item the context keeps (36 bytes per
// 64 samples)
//   diff[0 .. 3)[item]  bit b: the label at x = 64 w + b differs from the one at x + 1, y + 1, z + 1 (0 where that is off the lattice);
//                       three arrays of `items` words behind each other
//   active[item]        bit b: cell (64 w + b, y, z) is active
//   local[item]         the active cells (low half) and quads (high half) of the items before it in its block of kBlock items
//   voff / qoff         per block: the vertices / quads of the blocks before it; one more entry: all of them
// Count:
//   k_lsf_classify_tile  the only pass over the labels: a workgroup loads a tile of 64 x 9 x 5 labels into LDS, its wavefronts ballot
//                    the three difference words of 8 x 4 rows out of it
//   k_lsf_classify   the same words without LDS (O2V_LSF_NO_TILE=1, the A/B): a wavefront takes 64 consecutive x, one label per lane
//                    with the ones at y + 1 and z + 1 (re-read through L2) and the one at x + 1 from the next lane; kLsfInFlight
//                    words per wavefront are loaded before the first ballot
//   k_lsf_count      a lane per item, on the difference words only: a cell is active if one of its 12 edges differs, the quads
//                    are the difference bits of the interior edges; their popcounts scanned over the block
//   k_fill_scan_blocks (K6) twice
// Write (lanes -> outputs, as K10's):
//   k_lsf_vertices   output slot -> item -> bit -> the cell; a link where one of the 4 edges of the shared face differs
//   k_lsf_faces      K10's, with the winding and the pair from the two labels of the edge (the only reads of the labels)
// Relax: k_lsf_centres, then k_lsf_relax once per iteration, a lane per vertex, from one buffer into the other (Jacobi).
// No atomics: every order comes from the scans.

constexpr uint32_t kLsfInFlight = 4;   // words a wavefront loads (three labels per lane each) before its first ballot

// the labels of the box, as the caller gave them; E: the layers of label 0 around it
struct LsfLabels {
    const void *p;
    uint64_t s0, s1, s2;   // element strides (x, y, z)
    uint32_t nx, ny, nz;
    uint32_t E;
};

// the label of the extended sample (xe, ye, ze) = box sample + E; 0 outside the box (a coordinate below 0 wraps to a large one)
template <bool I32>
__device__ __forceinline__ int32_t lsf_label(const LsfLabels &L, uint32_t xe, uint32_t ye, uint32_t ze)
{
    const uint32_t x = xe - L.E, y = ye - L.E, z = ze - L.E;
    if (x >= L.nx || y >= L.ny || z >= L.nz) return 0;
    const uint64_t at = x * L.s0 + y * L.s1 + z * L.s2;
    return I32 ? static_cast<const int32_t *>(L.p)[at] : (int32_t) static_cast<const uint8_t *>(L.p)[at];
}

// A row (ye, ze) of the extended lattice, the same for a whole wavefront (the callers make their wavefront's number a scalar, so
// this is scalar arithmetic): whether it lies in the box, and the element offset of its sample x = 0.
struct LsfRow {
    bool in;
    uint64_t at;
};

__device__ __forceinline__ LsfRow lsf_row(const LsfLabels &L, uint32_t ye, uint32_t ze)
{
    const uint32_t y = ye - L.E, z = ze - L.E;
    return LsfRow{y < L.ny && z < L.nz, y * L.s1 + z * L.s2};
}

// the label of the extended sample xe of the row; UnitX: the x stride is 1
template <bool I32, bool UnitX>
__device__ __forceinline__ int32_t lsf_row_label(const LsfLabels &L, const LsfRow &row, uint32_t xe)
{
    const uint32_t x = xe - L.E;
    if (!row.in || x >= L.nx) return 0;
    const uint64_t at = row.at + (UnitX ? (uint64_t) x : x * L.s0);
    return I32 ? static_cast<const int32_t *>(L.p)[at] : (int32_t) static_cast<const uint8_t *>(L.p)[at];
}

// the wavefront's number in its workgroup, as a scalar
__device__ __forceinline__ uint32_t lsf_wave() { return (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)); }

template <bool I32, bool UnitX>
__global__ __launch_bounds__(kBlock) void k_lsf_classify(LsfLabels L, SurfGrid g, unsigned long long *__restrict__ diff)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t) blockIdx.x * (kBlock / 64u) + lsf_wave(), n_waves = (uint64_t) gridDim.x * (kBlock / 64u);
    for (uint64_t first = wave * kLsfInFlight; first < g.items; first += n_waves * kLsfInFlight) {
        SurfItem it = surf_item(g, first);
        int32_t a[kLsfInFlight], ay[kLsfInFlight], az[kLsfInFlight], a64[kLsfInFlight];
        uint32_t ok[kLsfInFlight];   // bit 0, 1, 2: the neighbour at x + 1, y + 1, z + 1 is on the lattice
#pragma unroll
        for (uint32_t u = 0; u < kLsfInFlight; ++u) {
            const uint32_t x = it.w * 64u + lane;
            a[u] = ay[u] = az[u] = a64[u] = 0;
            ok[u] = 0;
            if (first + u < g.items) {   // (uniform over the wavefront)
                const LsfRow r = lsf_row(L, it.j, it.k);
                ok[u] = x < g.nx ? (x + 1u < g.nx ? 1u : 0u) | (it.j + 1u < g.ny ? 2u : 0u) | (it.k + 1u < g.nz ? 4u : 0u) : 0u;
                a[u] = lsf_row_label<I32, UnitX>(L, r, x);
                ay[u] = lsf_row_label<I32, UnitX>(L, lsf_row(L, it.j + 1u, it.k), x);
                az[u] = lsf_row_label<I32, UnitX>(L, lsf_row(L, it.j, it.k + 1u), x);
                if (lane == 63u) a64[u] = lsf_row_label<I32, UnitX>(L, r, x + 1u);
            }
            if (++it.w == g.W) {
                it.w = 0;
                if (++it.j == g.ny) {
                    it.j = 0;
                    ++it.k;
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kLsfInFlight; ++u) {
            int32_t ax = __shfl_down(a[u], 1);
            if (lane == 63u) ax = a64[u];
            const unsigned long long mx = __ballot(((ok[u] & 1u) != 0u) & (a[u] != ax));
            const unsigned long long my = __ballot(((ok[u] & 2u) != 0u) & (a[u] != ay[u]));
            const unsigned long long mz = __ballot(((ok[u] & 4u) != 0u) & (a[u] != az[u]));
            if (lane == u && first + u < g.items) {
                diff[first + u] = mx;
                diff[g.items + first + u] = my;
                diff[2u * g.items + first + u] = mz;
            }
        }
    }
}

// The same words from a tile in LDS: a workgroup takes one word along x, kLsfTileY rows and kLsfTileZ layers (one per wavefront),
// loads the labels of these and of the row, the layer and the sample behind them once - (9 x 5) / (8 x 4) = 1.4 reads per sample, all
// issued before the first is used - and every wavefront ballots its layer's rows out of LDS.  (k_lsf_classify reads every sample three
// times, two of them through L2.)
constexpr uint32_t kLsfTileY = 8, kLsfTileZ = kBlock / 64u;

template <bool I32, bool UnitX>
__global__ __launch_bounds__(kBlock) void k_lsf_classify_tile(LsfLabels L, SurfGrid g, uint32_t tiles_y, uint64_t tiles, unsigned long long *__restrict__ diff)
{
    constexpr uint32_t RY = kLsfTileY + 1u, RZ = kLsfTileZ + 1u, kRows = RY * RZ;
    __shared__ int32_t s_a[kRows][65];   // [rz * RY + ry][x]: column 64 is the first sample of the next word
    const uint32_t lane = threadIdx.x & 63u, wv = lsf_wave();
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // t = (tz * tiles_y + ty) * W + w
        uint32_t w, row;
        if (tiles <= 0xffffffffull) {
            row = (uint32_t) t / g.W;
            w = (uint32_t) t - row * g.W;
        } else {
            const uint64_t r = t / g.W;   // (rows of tiles: below 2^32 by the limits on the dims)
            row = (uint32_t) r;
            w = (uint32_t) (t - r * g.W);
        }
        const uint32_t tz = row / tiles_y, j0 = (row - tz * tiles_y) * kLsfTileY, k0 = tz * kLsfTileZ, x0 = w * 64u;
        __syncthreads();   // (the tile of the turn before has been read)
        // (a fixed number of turns, so that the loop unrolls and every load is issued before the first is waited for)
        constexpr uint32_t kTurns = (kRows + kBlock / 64u - 1u) / (kBlock / 64u);
        int32_t v[kTurns], v64 = 0;
#pragma unroll
        for (uint32_t i = 0; i < kTurns; ++i) {
            const uint32_t at = wv + i * (kBlock / 64u), rz = at / RY, ry = at - rz * RY;
            v[i] = at < kRows ? lsf_row_label<I32, UnitX>(L, lsf_row(L, j0 + ry, k0 + rz), x0 + lane) : 0;
        }
        if (threadIdx.x < kRows) {   // (the first 45 lanes of the workgroup: a row each)
            const uint32_t rz = threadIdx.x / RY, ry = threadIdx.x - rz * RY;
            v64 = lsf_row_label<I32, UnitX>(L, lsf_row(L, j0 + ry, k0 + rz), x0 + 64u);
        }
#pragma unroll
        for (uint32_t i = 0; i < kTurns; ++i) {
            const uint32_t at = wv + i * (kBlock / 64u);
            if (at < kRows) s_a[at][lane] = v[i];
        }
        if (threadIdx.x < kRows) s_a[threadIdx.x][64] = v64;
        __syncthreads();
        const uint32_t k = k0 + wv, x = x0 + lane;
        if (k >= g.nz) continue;   // (uniform over the wavefront; the barriers are passed by all at the loop's head)
        unsigned long long mine[3] = {0ull, 0ull, 0ull};
#pragma unroll
        for (uint32_t ry = 0; ry < kLsfTileY; ++ry) {
            const uint32_t j = j0 + ry, at = wv * RY + ry;
            const int32_t a = s_a[at][lane], ax = s_a[at][lane + 1u], ay = s_a[at + 1u][lane], az = s_a[at + RY][lane];   // (no branch: four reads in flight)
            const unsigned long long mx = __ballot((x + 1u < g.nx) & (a != ax));
            const unsigned long long my = __ballot((x < g.nx) & (j + 1u < g.ny) & (a != ay));
            const unsigned long long mz = __ballot((x < g.nx) & (k + 1u < g.nz) & (a != az));
            if (lane == ry) mine[0] = mx, mine[1] = my, mine[2] = mz;
        }
        if (lane < kLsfTileY && j0 + lane < g.ny) {
            const uint64_t at = surf_index(g, w, j0 + lane, k);
            diff[at] = mine[0];
            diff[g.items + at] = mine[1];
            diff[2u * g.items + at] = mine[2];
        }
    }
}

struct LsfMasks {
    uint64_t active;      // cells
    uint64_t qx, qy, qz;  // differing edges from the sample along x, y, z with four cells around them
};

// Active: the cells too (nine more words); else the quads alone, from the item's own three words
template <bool Active>
__device__ __forceinline__ LsfMasks lsf_masks(const unsigned long long *__restrict__ diff, const SurfGrid &g, SurfItem it)
{
    LsfMasks m{};
    const unsigned long long *const dx = diff, *const dy = diff + g.items, *const dz = diff + 2u * g.items;
    const uint64_t at = surf_index(g, it.w, it.j, it.k);
    const uint32_t x0 = it.w * 64u, cells = g.nx - 1u;
    const uint64_t mc = cells <= x0 ? 0ull : (cells - x0 >= 64u ? ~0ull : surf_below(cells - x0));   // x <= nx - 2
    const uint64_t mi = it.w == 0u ? mc & ~1ull : mc;                                                 // 1 <= x <= nx - 2
    const bool jc = it.j + 1u < g.ny, kc = it.k + 1u < g.nz;   // the row above / the layer above exists
    const bool ji = jc && it.j >= 1u, ki = kc && it.k >= 1u;   // 1 <= y <= ny - 2, 1 <= z <= nz - 2
    if (mc == 0ull) return m;
    const uint64_t x00 = dx[at], y00 = dy[at], z00 = dz[at];   // (y00 is 0 without a row above, z00 without a layer above)
    if (ji && ki) m.qx = x00 & mc;
    if (ki) m.qy = y00 & mi;
    if (ji) m.qz = z00 & mi;
    if (Active && jc && kc) {
        const uint64_t up = g.W, over = (uint64_t) g.W * g.ny;
        const uint64_t y01 = dy[at + over], z10 = dz[at + up];
        // the 12 edges of the cell at its lowest sample s: x edges at s, s + e_y, s + e_z, s + e_y + e_z; y edges at s, s + e_x,
        // s + e_z, s + e_x + e_z; z edges at s, s + e_x, s + e_y, s + e_x + e_y
        const uint64_t any = x00 | dx[at + up] | dx[at + over] | dx[at + up + over] | y00 | surf_next(dy, g, at, it.w, y00) | y01 |
                             surf_next(dy, g, at + over, it.w, y01) | z00 | surf_next(dz, g, at, it.w, z00) | z10 | surf_next(dz, g, at + up, it.w, z10);
        m.active = any & mc;
    }
    return m;
}

__global__ __launch_bounds__(kBlock) void k_lsf_count(const unsigned long long *__restrict__ diff, SurfGrid g, unsigned long long *__restrict__ active,
                                                      uint32_t *__restrict__ local, unsigned long long *__restrict__ v_sums,
                                                      unsigned long long *__restrict__ q_sums)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    for (uint64_t b = blockIdx.x; b < g.n_blocks; b += gridDim.x) {
        const uint64_t item = b * kBlock + threadIdx.x;
        uint64_t both = 0;   // vertices in the low half, quads in the high half: a block has at most 2^14 and 3 x 2^14
        if (item < g.items) {
            const LsfMasks m = lsf_masks<true>(diff, g, surf_item(g, item));
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

// bit `bit` (at most 64: bit 0 of the row's next word, 0 past the row) of the word at `row`, the item's word w
__device__ __forceinline__ uint32_t lsf_bit(const unsigned long long *__restrict__ d, const SurfGrid &g, uint64_t row, uint32_t w, uint32_t bit)
{
    if (bit < 64u) return (uint32_t) (d[row] >> bit) & 1u;
    return w + 1u < g.W ? (uint32_t) d[row + 1u] & 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void k_lsf_vertices(SurfGrid g, uint32_t E, const unsigned long long *__restrict__ diff,
                                                         const unsigned long long *__restrict__ active, const uint32_t *__restrict__ local,
                                                         const unsigned long long *__restrict__ voff, int32_t *__restrict__ cells,
                                                         int32_t *__restrict__ links)
{
    __shared__ uint32_t s_pref[kBlock];
    __shared__ uint64_t s_mask[kBlock];
    const unsigned long long *const dx = diff, *const dy = diff + g.items, *const dz = diff + 2u * g.items;
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
            const uint32_t i = it.w * 64u + bit, j = it.j, k = it.k;
            // (the cell is active: the row above and the layer above exist)
            const uint64_t at = surf_index(g, it.w, j, k), up = g.W, over = (uint64_t) g.W * g.ny;
            const uint32_t x00 = lsf_bit(dx, g, at, it.w, bit), x10 = lsf_bit(dx, g, at + up, it.w, bit);
            const uint32_t x01 = lsf_bit(dx, g, at + over, it.w, bit), x11 = lsf_bit(dx, g, at + up + over, it.w, bit);
            const uint32_t y00 = lsf_bit(dy, g, at, it.w, bit), y00n = lsf_bit(dy, g, at, it.w, bit + 1u);
            const uint32_t y01 = lsf_bit(dy, g, at + over, it.w, bit), y01n = lsf_bit(dy, g, at + over, it.w, bit + 1u);
            const uint32_t z00 = lsf_bit(dz, g, at, it.w, bit), z00n = lsf_bit(dz, g, at, it.w, bit + 1u);
            const uint32_t z10 = lsf_bit(dz, g, at + up, it.w, bit), z10n = lsf_bit(dz, g, at + up, it.w, bit + 1u);
            // a link: the neighbouring cell exists and one of the 4 edges of the shared face differs
            const bool xm = i >= 1u && (y00 | y01 | z00 | z10), xp = i + 2u < g.nx && (y00n | y01n | z00n | z10n);
            const bool ym = j >= 1u && (x00 | x01 | z00 | z00n), yp = j + 2u < g.ny && (x10 | x11 | z10 | z10n);
            const bool zm = k >= 1u && (x00 | x10 | y00 | y00n), zp = k + 2u < g.nz && (x01 | x11 | y01 | y01n);
            int32_t *c = cells + (base + slot) * 3u;
            c[0] = (int32_t) i - (int32_t) E;
            c[1] = (int32_t) j - (int32_t) E;
            c[2] = (int32_t) k - (int32_t) E;
            int32_t *o = links + (base + slot) * 6u;
            o[0] = xm ? surf_vertex(g, active, local, voff, i - 1u, j, k) : -1;
            o[1] = xp ? surf_vertex(g, active, local, voff, i + 1u, j, k) : -1;
            o[2] = ym ? surf_vertex(g, active, local, voff, i, j - 1u, k) : -1;
            o[3] = yp ? surf_vertex(g, active, local, voff, i, j + 1u, k) : -1;
            o[4] = zm ? surf_vertex(g, active, local, voff, i, j, k - 1u) : -1;
            o[5] = zp ? surf_vertex(g, active, local, voff, i, j, k + 1u) : -1;
        }
    }
}

template <bool I32>
__global__ __launch_bounds__(kBlock) void k_lsf_faces(LsfLabels L, SurfGrid g, const unsigned long long *__restrict__ diff,
                                                      const unsigned long long *__restrict__ active, const uint32_t *__restrict__ local,
                                                      const unsigned long long *__restrict__ voff, const unsigned long long *__restrict__ qoff,
                                                      int32_t *__restrict__ faces, int32_t *__restrict__ pairs)
{
    __shared__ uint32_t s_pref[kBlock];
    __shared__ uint64_t s_q[3][kBlock];
    for (uint64_t b = blockIdx.x; b < g.n_blocks; b += gridDim.x) {
        const uint64_t base = qoff[b];
        const uint32_t n = (uint32_t) (qoff[b + 1] - base);
        if (n == 0u) continue;   // (uniform over the block)
        __syncthreads();         // (the arrays of the block before have been read)
        {
            const uint64_t item = b * kBlock + threadIdx.x;
            LsfMasks m{};
            if (item < g.items) m = lsf_masks<false>(diff, g, surf_item(g, item));
            s_pref[threadIdx.x] = item < g.items ? local[item] >> 16 : n;
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
            const int32_t lc = lsf_label<I32>(L, c[0], c[1], c[2]);
            const int32_t lq = lsf_label<I32>(L, c[0] + (ax == 0u), c[1] + (ax == 1u), c[2] + (ax == 2u));
            const bool larger = lc > lq;   // the normal points from the larger label to the smaller
            int32_t *o = faces + (base + slot) * 6u;
            o[0] = o[3] = n0;
            o[1] = larger ? n1 : n3;
            o[2] = o[4] = n2;
            o[5] = larger ? n3 : n1;
            int32_t *p = pairs + (base + slot) * 2u;
            p[0] = larger ? lc : lq;
            p[1] = larger ? lq : lc;
        }
    }
}

// ---- the relaxation ----------------------------------------------------------------------------------------------------------

// component c of the centre of a cell: (float) (origin + cell + 1), exact for the cells of a counted grid
__device__ __forceinline__ float lsf_centre(uint32_t o, int32_t cell) { return (float) ((int64_t) o + cell + 1); }

// p_0: a lane per component
__global__ __launch_bounds__(kBlock) void k_lsf_centres(const int32_t *__restrict__ cells, uint32_t n, uint32_t ox, uint32_t oy, uint32_t oz,
                                                        float *__restrict__ p)
{
    const uint64_t total = 3ull * n;
    for (uint64_t e = (uint64_t) blockIdx.x * kBlock + threadIdx.x; e < total; e += (uint64_t) gridDim.x * kBlock) {
        const uint32_t c = (uint32_t) (e % 3u);
        p[e] = lsf_centre(c == 0u ? ox : c == 1u ? oy : oz, cells[e]);
    }
}

// p_{t + 1} from p_t, a lane per vertex; a link below 0 or from n on is no link and is not followed
__global__ __launch_bounds__(kBlock) void k_lsf_relax(const int32_t *__restrict__ cells, const int32_t *__restrict__ links, uint32_t n, uint32_t ox,
                                                      uint32_t oy, uint32_t oz, float relaxation, float reach, const float *__restrict__ pin,
                                                      float *__restrict__ pout)
{
    for (uint64_t v = (uint64_t) blockIdx.x * kBlock + threadIdx.x; v < n; v += (uint64_t) gridDim.x * kBlock) {
        int32_t link[6];
#pragma unroll
        for (uint32_t d = 0; d < 6; ++d) link[d] = links[v * 6u + d];
        const float px = pin[v * 3u], py = pin[v * 3u + 1u], pz = pin[v * 3u + 2u];
        float sx = 0.f, sy = 0.f, sz = 0.f;
        uint32_t m = 0;
#pragma unroll
        for (uint32_t d = 0; d < 6; ++d)
            if ((uint32_t) link[d] < n) {
                const float *q = pin + (uint64_t) (uint32_t) link[d] * 3u;
                sx = sx + q[0];
                sy = sy + q[1];
                sz = sz + q[2];
                ++m;
            }
        float rx = px, ry = py, rz = pz;
        if (m) {
            const float m_f = (float) m;
            const float cx = lsf_centre(ox, cells[v * 3u]), cy = lsf_centre(oy, cells[v * 3u + 1u]), cz = lsf_centre(oz, cells[v * 3u + 2u]);
            rx = px + relaxation * (sx / m_f - px);
            ry = py + relaxation * (sy / m_f - py);
            rz = pz + relaxation * (sz / m_f - pz);
            rx = fminf(fmaxf(rx, cx - reach), cx + reach);
            ry = fminf(fmaxf(ry, cy - reach), cy + reach);
            rz = fminf(fmaxf(rz, cz - reach), cz + reach);
        }
        pout[v * 3u] = rx;
        pout[v * 3u + 1u] = ry;
        pout[v * 3u + 2u] = rz;
    }
}
