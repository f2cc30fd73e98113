// o2v_dev_k12_components.hpp -- K12: connected components and flood fill of a dense grid (o2v_hip_components_dense /
// o2v_hip_flood_dense).  Included from o2v_device.hip inside its anonymous namespace, after K11 (whose reader it uses) and
// o2v_dev_bits.hpp (the bit grid, its words, tiles and walk).
//
// The set S (include/o2v_hip.h) is classified once into the bit grid of o2v_dev_bits.hpp; every later pass reads these bits.  A
// voxel's linear index is i = (z * ny + y) * nx + x, below 2^31; P[i] is its
// parent, P[i] <= i, a root has P[i] == i.  Hooking always puts the larger root under the smaller, so the root of a finished
// component is its smallest linear index and the numbering of the header falls out of a prefix count over the root flags.
//
//   k_cc_classify   the only pass over the grid: a lane reads 16 voxels along x through K11's ray_read16 (one 16-byte load for
//                   U8, four for F32 where rows are aligned), four lanes make a word (two xor-shuffles); INVERT complements
//                   inside the box.
//   k_cc_tiles      a workgroup per tile of 64 x 8 x 8 voxels (one word per row, 64 rows): the words and 4096 32-bit local labels in
//                   LDS (512 + 16 384 bytes, and a word).  A voxel starts at the first voxel of its x-run (bit operations on the word), then
//                   every adjacent pair of runs inside the tile is united in LDS (cc_union on ds_min_rtn_u32) - a union-find
//                   needs no sweeps "until stable".  P[i] = the global index of the tile-local root.  No global atomics.
//                   (32-bit labels, not 16-bit: LDS has no 16-bit atomic min, and 16.5 KB per workgroup still leaves the CU's
//                   eight workgroups their room.)
//   k_cc_seams      a wavefront per word, a lane per voxel: only pairs that leave the tile - along y and z where the row is on
//                   a tile face, along x at lanes 0 and 63 - are united in global memory: both roots by path halving,
//                   atomicMin of the smaller into the larger root's parent, again from the value returned if that was no
//                   root any more.  No lock, no wait on another lane: every loop ends because an index strictly decreases.
//                   All = true (O2V_CC_NO_TILES=1): P[i] = i (k_cc_init) and every adjacent pair goes through here.
//   k_cc_flatten    P[i] = root(i); the root flags of a word by ballot.
//   k_cc_count + k_fill_scan_blocks (K6)   popcounts of the root words -> per-word prefix, block offsets, the total (count).
//   k_cc_labels     labels = rank(root) + 1, or 0.
//   k_cc_seed_list / k_cc_seed_border / k_cc_flood_out   flood: a flag bit per root, at the root's own bit position; values[..]
//                   to out; `reached` from one atomic per workgroup.
// Which pairs are looked at: a voxel looks back - at x - 1 in its row and at the four neighbour rows (dy, dz) = (-1, 0), (0, -1),
// (-1, -1), (1, -1) with dx = 0 and, where the connectivity allows the offset, dx = -1 / +1 - so each unordered pair is seen once.
// Pairs that the runs already connect are left out (cc_visits): with dx = 0 unless it is the first voxel of the overlap of
// the two runs, with dx = -1 / +1 only where dx = 0 is not in S and the voxel's own run does not continue that way.

constexpr uint32_t kCcTileRows = 64u, kCcTileVoxels = 4096u;   // a tile: 64 (x) x 8 (y) x 8 (z); row = ty + 8 tz

#ifndef O2V_CC_HOST
#define O2V_CC_FN __device__ __forceinline__
O2V_CC_FN uint32_t cc_load(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
O2V_CC_FN void cc_store(uint32_t *p, uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
O2V_CC_FN uint32_t cc_min(uint32_t *p, uint32_t v) { return atomicMin(p, v); }
O2V_CC_FN uint32_t cc_clz64(uint64_t v) { return (uint32_t) __clzll((long long) v); }
#endif

// ---- the union-find and the adjacency ----------------------------------------------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_components.py compiles this part for the host, with O2V_CC_FN, cc_load,
// cc_store, cc_min and cc_clz64 of its own, runs it tile by tile against the reference and checks that two changes are caught.)

struct CcGrid : BitGrid {
    uint32_t tiles_y, tiles_z;   // ceil(ny / 8), ceil(nz / 8); tiles along x: W
    uint32_t conn;               // 6, 18 or 26
};

struct CcRow {
    uint64_t w;        // the row's word
    uint32_t lo, hi;   // the bits of x = -1 and x = 64 relative to the word (0 where that is outside what the pass looks at)
};
struct CcVisit {
    uint64_t c, l, r;   // bit x: the voxel x of `me` is united with the voxel x, x - 1, x + 1 of the neighbour row
};

O2V_CC_FN uint32_t cc_index(const CcGrid &g, uint32_t x, uint32_t y, uint32_t z) { return (z * g.ny + y) * g.nx + x; }

// the four neighbour rows a voxel looks back at, and whether the connectivity has them (dx = 0) and their diagonals (dx = -1, +1)
O2V_CC_FN int cc_pair_dy(int k) { return k == 1 ? 0 : k == 3 ? 1 : -1; }
O2V_CC_FN int cc_pair_dz(int k) { return k == 0 ? 0 : -1; }
O2V_CC_FN bool cc_pair_on(uint32_t conn, int k) { return k < 2 || conn >= 18u; }
O2V_CC_FN bool cc_pair_diag(uint32_t conn, int k) { return k < 2 ? conn >= 18u : conn == 26u; }

// the first voxel of the x-run of voxel x within its word
O2V_CC_FN uint32_t cc_run_start(uint64_t w, uint32_t x)
{
    const uint64_t gaps = ~w & ((1ull << x) - 1ull);   // the voxels below x that are not in S
    return gaps ? 64u - cc_clz64(gaps) : 0u;
}

O2V_CC_FN CcVisit cc_visits(const CcRow &me, const CcRow &n, bool diag, int k)
{
    const uint64_t me_l = me.w << 1 | me.lo, me_r = me.w >> 1 | (uint64_t) me.hi << 63;   // bit x: x - 1 / x + 1 of the row is in S
    const uint64_t n_l = n.w << 1 | n.lo, n_r = n.w >> 1 | (uint64_t) n.hi << 63;
    CcVisit v;
    v.c = me.w & n.w & ~(me_l & n_l);
    v.l = diag ? me.w & ~n.w & n_l & ~me_l : 0ull;
    v.r = diag ? me.w & ~n.w & n_r & ~me_r : 0ull;
#ifdef O2V_CC_MUTATE_DROP_DIAGONAL
    if (k == 3) v.r = 0ull;   // (test only: the offset (+1, +1, -1) left out)
#endif
    (void) k;
    return v;
}

// the root of i, with path halving: every store puts an ancestor, so a smaller index, in place of a parent
O2V_CC_FN uint32_t cc_find(uint32_t *P, uint32_t i)
{
    for (;;) {
        const uint32_t p = cc_load(P + i);
        if (p == i) return i;
        const uint32_t gp = cc_load(P + p);
        if (gp == p) return p;
        cc_store(P + i, gp);
        i = gp;
    }
}

// the root of i, nothing stored
O2V_CC_FN uint32_t cc_root(const uint32_t *P, uint32_t i)
{
    for (;;) {
        const uint32_t p = cc_load(P + i);
        if (p == i) return i;
        i = p;
    }
}

// Unites the sets of a and b.  The atomic min either hooks a root (it returns the root itself) or meets an element that
// another lane has hooked in the meantime: whatever it leaves there is smaller, and its former parent - the value returned -
// still has to be united with b.  a + b strictly decreases from turn to turn.  Returns the turns that met no root.
O2V_CC_FN uint32_t cc_union(uint32_t *P, uint32_t a, uint32_t b)
{
    for (uint32_t retries = 0;; ++retries) {
        a = cc_find(P, a);
        b = cc_find(P, b);
        if (a == b) return retries;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
#ifdef O2V_CC_MUTATE_HOOK_LARGER
        const uint32_t old = cc_max(P + b, a);   // (test only: the smaller root under the larger)
        if (old == b) return retries;
        b = old;
#else
        const uint32_t old = cc_min(P + a, b);
        if (old == a) return retries;
        a = old;
#endif
    }
}

// -- the tile pass, per lane: s_w the tile's 64 row words (0 for rows outside the box), lab its 4096 local labels, l = row * 64 + x

O2V_CC_FN void cc_tile_init(const uint64_t *s_w, uint32_t *lab, uint32_t row, uint32_t x)
{
    const uint64_t w = s_w[row];
    if ((w >> x) & 1ull) lab[row * 64u + x] = row * 64u + cc_run_start(w, x);
}

O2V_CC_FN void cc_tile_merge(uint32_t conn, const uint64_t *s_w, uint32_t *lab, uint32_t row, uint32_t x)
{
    const CcRow me = {s_w[row], 0u, 0u};
    if (!((me.w >> x) & 1ull)) return;
    const int ty = (int) (row & 7u), tz = (int) (row >> 3);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!cc_pair_on(conn, k)) continue;
        const int Y = ty + cc_pair_dy(k), Z = tz + cc_pair_dz(k);
        if ((uint32_t) Y >= 8u || (uint32_t) Z >= 8u) continue;   // (a seam)
        const uint32_t nrow = (uint32_t) (Y + 8 * Z);
        const CcRow n = {s_w[nrow], 0u, 0u};
        if (!n.w) continue;
        const CcVisit v = cc_visits(me, n, cc_pair_diag(conn, k), k);
        const uint32_t l = row * 64u + x, nb = nrow * 64u + x;
        if ((v.c >> x) & 1ull) (void) cc_union(lab, l, nb);
        if ((v.l >> x) & 1ull) (void) cc_union(lab, l, nb - 1u);
        if ((v.r >> x) & 1ull) (void) cc_union(lab, l, nb + 1u);
    }
}

// P[i] = the global index of the tile-local root ((x0, y0, z0): the tile's first voxel); local and global order agree in a tile
O2V_CC_FN void cc_tile_out(const CcGrid &g, const uint64_t *s_w, uint32_t *lab, uint32_t *P, uint32_t x0, uint32_t y0, uint32_t z0,
                           uint32_t row, uint32_t x)
{
    if (!((s_w[row] >> x) & 1ull)) return;
    const uint32_t root = cc_find(lab, row * 64u + x), rrow = root >> 6;
    P[cc_index(g, x0 + x, y0 + (row & 7u), z0 + (row >> 3))] = cc_index(g, x0 + (root & 63u), y0 + (rrow & 7u), z0 + (rrow >> 3));
}

// -- the seams, per lane: voxel x of word wx of row (y, z)

O2V_CC_FN CcRow cc_grid_row(const CcGrid &g, const uint64_t *bits, uint32_t wx, int y, int z)
{
    CcRow r = {0ull, 0u, 0u};
    if ((uint32_t) y >= g.ny || (uint32_t) z >= g.nz) return r;
    const uint64_t *row = bits + bits_word_index(g, 0u, (uint32_t) y, (uint32_t) z);
    r.w = row[wx];
    r.lo = wx > 0u ? (uint32_t) (row[wx - 1u] >> 63) : 0u;
    r.hi = wx + 1u < g.W ? (uint32_t) (row[wx + 1u] & 1ull) : 0u;
    return r;
}

struct CcCount {
    uint32_t unions, retries;   // the pairs handed to cc_union, its turns that met no root
};

// All = false: the pairs that leave the voxel's tile.  All = true: every pair.
template <bool All>
O2V_CC_FN CcCount cc_seam(const CcGrid &g, const uint64_t *bits, uint32_t *P, uint32_t wx, uint32_t y, uint32_t z, uint32_t x)
{
    CcCount n = {0u, 0u};
    const CcRow me = cc_grid_row(g, bits, wx, (int) y, (int) z);
    if (!((me.w >> x) & 1ull)) return n;
    const uint32_t i = cc_index(g, wx * 64u + x, y, z);
    if (All ? (((me.w << 1 | me.lo) >> x) & 1ull) != 0ull : (x == 0u && me.lo != 0u)) {
        ++n.unions;
        n.retries += cc_union(P, i, i - 1u);
    }
    const uint32_t ty = y & 7u, tz = z & 7u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!cc_pair_on(g.conn, k)) continue;
        const int dy = cc_pair_dy(k), dz = cc_pair_dz(k);
        const int Y = (int) y + dy, Z = (int) z + dz;
        if ((uint32_t) Y >= g.ny || (uint32_t) Z >= g.nz) continue;
        const bool cross = All || (dy < 0 && ty == 0u) || (dy > 0 && ty == 7u) || (dz < 0 && tz == 0u);
        const bool diag = cc_pair_diag(g.conn, k);
        if (!cross && !diag) continue;
        const CcRow nb = cc_grid_row(g, bits, wx, Y, Z);
        CcVisit v = cc_visits(me, nb, diag, k);
        if (!cross) v.c = 0ull, v.l &= 1ull, v.r &= 1ull << 63;   // (inside the tile's rows only x - 1 of lane 0 and x + 1 of lane 63 leave it)
        const uint32_t j = cc_index(g, wx * 64u + x, (uint32_t) Y, (uint32_t) Z);
        if ((v.c >> x) & 1ull) ++n.unions, n.retries += cc_union(P, i, j);
        if ((v.l >> x) & 1ull) ++n.unions, n.retries += cc_union(P, i, j - 1u);
        if ((v.r >> x) & 1ull) ++n.unions, n.retries += cc_union(P, i, j + 1u);
    }
    return n;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_CC_HOST

// the word of the root r and the bit below which its rank within the word is counted
__device__ __forceinline__ uint64_t cc_root_word(const CcGrid &g, uint32_t r, uint32_t &bit)
{
    const uint32_t row = r / g.nx, x = r - row * g.nx;
    bit = x & 63u;
    return (uint64_t) row * g.W + (x >> 6);
}

template <uint32_t Format, bool Vec>
__global__ __launch_bounds__(kBlock) void k_cc_classify(RaySource src, BitGrid g, uint32_t invert, unsigned long long *__restrict__ bits)
{
    const uint32_t lane = threadIdx.x & 63u, q = lane & 3u, j = lane >> 2;
    for (const uint64_t grp : WaveTurns{(g.words + 15u) / 16u}) {   // a wavefront takes 16 words
        const uint64_t wi = grp * 16u + j;
        uint32_t b = 0;
        if (wi < g.words) {
            const BitWord at = bits_word_at(g, wi);
            const uint32_t x0 = at.wx * 64u + q * 16u;
            if (x0 < g.nx) {
                const uint32_t n = min(16u, g.nx - x0);
                b = ray_read16<Format, Vec>(src, (uint64_t) at.y * src.s1 + (uint64_t) at.z * src.s2, x0, n);
                if (invert) b = ~b & ((1u << n) - 1u);
            }
        }
        unsigned long long w = (unsigned long long) b << (16u * q);
        w |= __shfl_xor(w, 1);
        w |= __shfl_xor(w, 2);
        if (q == 0u && wi < g.words) bits[wi] = w;
    }
}

__global__ __launch_bounds__(kBlock) void k_cc_tiles(CcGrid g, const unsigned long long *__restrict__ bits, uint32_t *__restrict__ P)
{
    __shared__ uint64_t s_w[kCcTileRows];
    __shared__ uint32_t s_lab[kCcTileVoxels];
    __shared__ uint32_t s_any;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tiles = g.W * g.tiles_y * g.tiles_z;   // (no more than the words)
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        uint32_t tx, ty, tz;
        bits_tile_at(g, g.tiles_y, tile, tx, ty, tz);
        __syncthreads();   // (the last tile's words and labels are no longer read)
        if (threadIdx.x < kCcTileRows) {
            const uint64_t w = s_w[threadIdx.x] = bits_tile_word(g, bits, tx, ty, tz, threadIdx.x);
            const unsigned long long any = __ballot(w != 0ull);   // (the 64 rows are the first wavefront's lanes)
            if (threadIdx.x == 0) s_any = any != 0ull;
        }
        __syncthreads();
        if (!s_any) continue;   // an empty tile
        for (uint32_t row = wave; row < kCcTileRows; row += kBlock / 64u) cc_tile_init(s_w, s_lab, row, lane);
        __syncthreads();
        for (uint32_t row = wave; row < kCcTileRows; row += kBlock / 64u) cc_tile_merge(g.conn, s_w, s_lab, row, lane);
        __syncthreads();
        for (uint32_t row = wave; row < kCcTileRows; row += kBlock / 64u) cc_tile_out(g, s_w, s_lab, P, tx * 64u, ty * 8u, tz * 8u, row, lane);
    }
}

// O2V_CC_NO_TILES: every voxel of S its own root
__global__ __launch_bounds__(kBlock) void k_cc_init(CcGrid g, const unsigned long long *__restrict__ bits, uint32_t *__restrict__ P)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        if ((bits[wi] >> lane) & 1ull) {
            const uint32_t i = cc_index(g, at.wx * 64u + lane, at.y, at.z);
            P[i] = i;
        }
    }
}

// ctr[0] += the pairs handed to cc_union, ctr[1] += the atomic mins that met no root (Count: O2V_HIP_FLAG_STAGE_TIMES)
template <bool All, bool Count>
__global__ __launch_bounds__(kBlock) void k_cc_seams(CcGrid g, const unsigned long long *bits, uint32_t *P, unsigned long long *ctr)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t unions = 0, retries = 0;
    for (const uint64_t wi : bits_words(g)) {
        if (bits[wi] == 0ull) continue;
        const BitWord at = bits_word_at(g, wi);
        const CcCount n = cc_seam<All>(g, reinterpret_cast<const uint64_t *>(bits), P, at.wx, at.y, at.z, lane);
        unions += n.unions, retries += n.retries;
    }
    if (Count) {
        for (int d = 32; d >= 1; d >>= 1) unions += __shfl_xor(unions, d), retries += __shfl_xor(retries, d);
        if (lane == 0u && unions) atomicAdd(ctr, (unsigned long long) unions);
        if (lane == 0u && retries) atomicAdd(ctr + 1, (unsigned long long) retries);
    }
}

// P[i] = the root of i; roots (if not null): bit x of word wi says that voxel is a root
__global__ __launch_bounds__(kBlock) void k_cc_flatten(CcGrid g, const unsigned long long *__restrict__ bits, uint32_t *P, unsigned long long *__restrict__ roots)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (const uint64_t wi : bits_words(g)) {
        const unsigned long long w = bits[wi];
        bool is_root = false;
        if ((w >> lane) & 1ull) {
            const BitWord at = bits_word_at(g, wi);
            const uint32_t i = cc_index(g, at.wx * 64u + lane, at.y, at.z), r = cc_root(P, i);
            if (r != i) cc_store(P + i, r);
            is_root = r == i;
        }
        const unsigned long long m = __ballot(is_root);
        if (roots && lane == 0u) roots[wi] = m;
    }
}

// local[wi] = the roots in the words of wi's block before wi; block_sums[block] = the block's roots
__global__ __launch_bounds__(kBlock) void k_cc_count(const unsigned long long *__restrict__ roots, uint64_t words, uint32_t *__restrict__ local,
                                                     unsigned long long *__restrict__ block_sums)
{
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint64_t wi = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n = wi < words ? (uint32_t) __popcll(roots[wi]) : 0u;
    uint32_t total;
    const uint32_t ex = block_exscan(n, s_wave, total);
    if (wi < words) local[wi] = ex;
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// labels(x, y, z) = 1 + the rank of the voxel's root, 0 outside S.  P may be the labels themselves (contiguous labels): a lane
// reads its own parent - a root, after k_cc_flatten - and nothing else of P.
__global__ __launch_bounds__(kBlock) void k_cc_labels(CcGrid g, const unsigned long long *__restrict__ bits, const uint32_t *P,
                                                      const unsigned long long *__restrict__ roots, const uint32_t *__restrict__ local,
                                                      const unsigned long long *__restrict__ block_offsets, int32_t *labels, uint64_t s0, uint64_t s1,
                                                      uint64_t s2)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z;
        if (x >= g.nx) continue;
        int32_t label = 0;
        if ((bits[wi] >> lane) & 1ull) {
            uint32_t bit;
            const uint64_t rw = cc_root_word(g, P[cc_index(g, x, y, z)], bit);
            label = (int32_t) (block_offsets[rw / kBlock] + local[rw] + (uint32_t) __popcll(roots[rw] & ((1ull << bit) - 1ull))) + 1;
        }
        labels[(uint64_t) x * s0 + (uint64_t) y * s1 + (uint64_t) z * s2] = label;
    }
}

__device__ __forceinline__ void cc_flag_root(const CcGrid &g, uint32_t root, unsigned long long *flags)
{
    uint32_t bit;
    const uint64_t rw = cc_root_word(g, root, bit);
    if (!((flags[rw] >> bit) & 1ull)) atomicOr(flags + rw, 1ull << bit);   // (a plain read first: a component's seeds set one bit)
}

// the listed seeds (after k_cc_flatten: P[i] is the root)
__global__ __launch_bounds__(kBlock) void k_cc_seed_list(CcGrid g, const unsigned long long *__restrict__ bits, const uint32_t *__restrict__ P,
                                                         const int32_t *__restrict__ seeds, uint64_t n, unsigned long long *flags)
{
    for (uint64_t s = (uint64_t) blockIdx.x * kBlock + threadIdx.x; s < n; s += (uint64_t) gridDim.x * kBlock) {
        const int32_t x = seeds[s * 3u], y = seeds[s * 3u + 1u], z = seeds[s * 3u + 2u];
        if ((uint32_t) x >= g.nx || (uint32_t) y >= g.ny || (uint32_t) z >= g.nz) continue;
        if (!bits_has(g, bits, (uint32_t) x, (uint32_t) y, (uint32_t) z)) continue;
        cc_flag_root(g, P[cc_index(g, (uint32_t) x, (uint32_t) y, (uint32_t) z)], flags);
    }
}

// O2V_HIP_CC_SEED_BORDER: the voxels of S on the six faces of the box
__global__ __launch_bounds__(kBlock) void k_cc_seed_border(CcGrid g, const unsigned long long *__restrict__ bits, const uint32_t *__restrict__ P,
                                                           unsigned long long *flags)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z;
        if (bits_on_face(g, x, y, z) && x < g.nx && ((bits[wi] >> lane) & 1ull)) cc_flag_root(g, P[cc_index(g, x, y, z)], flags);
    }
}

// out(x, y, z) = v0 in S with a seed in the component, v1 in S without, v2 outside S; *reached += the voxels that got v0
__global__ __launch_bounds__(kBlock) void k_cc_flood_out(CcGrid g, const unsigned long long *__restrict__ bits, const uint32_t *__restrict__ P,
                                                         const unsigned long long *__restrict__ flags, uint32_t v0, uint32_t v1, uint32_t v2,
                                                         uint8_t *__restrict__ out, uint64_t s0, uint64_t s1, uint64_t s2, unsigned long long *reached)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long mine = 0;   // (the same in every lane of the wavefront)
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z;
        bool hit = false;
        uint32_t v = v2;
        if (x < g.nx && ((bits[wi] >> lane) & 1ull)) {
            uint32_t bit;
            const uint64_t rw = cc_root_word(g, P[cc_index(g, x, y, z)], bit);
            hit = ((flags[rw] >> bit) & 1ull) != 0ull;
            v = hit ? v0 : v1;
        }
        if (x < g.nx) out[(uint64_t) x * s0 + (uint64_t) y * s1 + (uint64_t) z * s2] = (uint8_t) v;
        mine += (unsigned long long) __popcll(__ballot(hit));
    }
    bits_add_wave_sums(mine, reached);
}

#endif   // O2V_CC_HOST
