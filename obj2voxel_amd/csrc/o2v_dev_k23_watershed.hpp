// o2v_dev_k23_watershed.hpp -- K23: the watershed basins of a relief, merged by persistence (o2v_hip_watershed_dense).  Included
// from o2v_device.hip inside its anonymous namespace, after K12 (CcGrid, cc_index, cc_root_word, k_cc_count), K22 and the pair table.
//
// The definition (include/o2v_hip.h, tests/watershed_ref.py).  H is an int32 relief, S = { v : H[v] > 0 }, i(v) = (z * ny + y) * nx
// + x the linear index (below 2^31), K(v) = (H[v], i(v)) the key, compared lexicographically: a strict total order.  For v in S
// take the neighbour u in S (6, 18 or 26 neighbours) of greatest key; parent(v) = u if K(u) > K(v), else v is a peak.  Keys rise
// along parents, so the parents are a forest and basin(v) is the peak v reaches.  Two basins are adjacent where a voxel of one
// has a neighbour in the other; their saddle is the maximum over such pairs of min(H[u], H[v]).  The adjacent pairs, sorted by
// (saddle descending, smaller peak index, larger peak index), are walked with a union-find over the peaks whose classes are
// represented by their peak of greatest key: a pair that joins two classes kills the one whose representative p has the smaller
// key, pers(p) = H[p] - saddle, partner(p) = the other representative.  final(p) = p if pers(p) >= min_depth, else
// final(partner(p)); the label of v is 1 + the rank of final(basin(v)) among the surviving peaks in ascending index.
//
//   k_ws_ascent_tiles  a workgroup per K12 tile of 64 x 8 x 8 voxels: the relief with a one-voxel halo in LDS (66 x 10 x 10 int32,
//                      26 400 bytes; max(H, 0), 0 outside the box), a lane per voxel takes the greatest of the packed keys
//                      (uint64) H << 31 | i of its neighbours, then follows the parents inside the tile in LDS (one word per
//                      voxel, 16 384 bytes: the local index of a parent in the tile, or bit 31 and the global index where the
//                      path leaves the tile or ends in a peak; nothing is stored while lanes follow).  P[i] = the tile's exit
//                      or the peak, i itself for a peak, 0xFFFFFFFF outside S.
//   k_ws_ascent        O2V_WS_NO_TILES=1: the same choice with the neighbours from global memory, P[i] = the parent.
//   k_ws_flatten       P[i] = the peak of i (ws_root), as k_cc_flatten does it: a lane walks its parents and stores its own entry
//                      only, so every value a racing lane can read is an ancestor or the peak and later walks are shortened;
//                      every loop ends because a key rises; the peak flags of a word by ballot.
//   k_cc_count + k_fill_scan_blocks (K12, K6)   ranks of the peaks in ascending index.
//   k_ws_peaks         the peaks' indices and heights, by rank, for the host.
//   k_ws_pairs         (min_depth > 0, two peaks or more) a voxel looks back at its 3, 9 or 13 earlier neighbours, so every
//                      unordered pair is seen once; where the peaks differ, key (smaller peak) << 32 | larger peak and value
//                      min(H[u], H[v]) go into the pair table (pt_slot) and its 32-bit values: atomicMax where a plain read finds
//                      the value below.  A probe run without a place sets the overflow word: the host doubles the table, clears
//                      it and runs this stage again.
//   k_pt_list<uint32_t, 1>   the table's entries as a list (any order: the host sorts).  Only the set of distinct pairs and their
//                      maxima leaves the stage, whatever the table's size and the order of insertion.
//   ws_merge           on the host (plain C++): the sort, the elder-rule union-find, the final chains, label_of_rank.
//   k_ws_labels        labels = label_of_rank[rank(P[v])] (rank + 1 without a merge), 0 outside S, through the strides.
// No kernel waits for another workgroup, flag or lane.

constexpr uint32_t kWsOutside = 0xffffffffu;                 // P of a voxel outside S
constexpr uint32_t kWsHaloX = 66u, kWsHaloY = 10u, kWsHaloZ = 10u, kWsHalo = kWsHaloX * kWsHaloY * kWsHaloZ;
constexpr uint32_t kWsExit = 0x80000000u;                    // an LDS word that holds a global index: a peak, or the parent outside the tile
constexpr uint32_t kWsTableMaxLog2 = 40u;

#ifndef O2V_WS_HOST
#define O2V_WS_FN __device__ __forceinline__
O2V_WS_FN uint32_t ws_load(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
O2V_WS_FN void ws_store(uint32_t *p, uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
O2V_WS_FN void ws_max32(uint32_t *p, uint32_t v) { (void) atomicMax(p, v); }
#endif

// ---- the key, the offsets, the ascent, the follow, the table, the merge ----------------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_watershed.py compiles this part for the host behind the pair table's, with
// O2V_WS_FN, ws_load, ws_store and ws_max32 of its own, runs it tile by tile in a shuffled order against the reference and checks
// that a change is caught.)

// The 26 offsets in ascending (dz, dy, dx) order, k = 0 .. 26 without 13: K20's order.  k < 13: the neighbour's index is smaller.
O2V_WS_FN int ws_dx(int k) { return k % 3 - 1; }
O2V_WS_FN int ws_dy(int k) { return k / 3 % 3 - 1; }
O2V_WS_FN int ws_dz(int k) { return k / 9 - 1; }
O2V_WS_FN bool ws_offset_on(uint32_t conn, int k)
{
#ifdef O2V_WS_MUTATE_DROP_DIAGONAL
    if (k == 8) return false;   // (test only: the offset (+1, +1, -1) left out)
#endif
    const uint32_t axes = (uint32_t) (ws_dx(k) != 0) + (uint32_t) (ws_dy(k) != 0) + (uint32_t) (ws_dz(k) != 0);
    return k != 13 && axes <= pt_max_axes(conn);
}

// K(v) packed: H in 1 .. 2^31 - 1, i below 2^31
O2V_WS_FN uint64_t ws_key(int32_t h, uint32_t i) { return (uint64_t) (uint32_t) h << 31 | i; }

// the index of the neighbour of voxel i at offset k (inside the box); sy = nx, sz = nx * ny
O2V_WS_FN uint32_t ws_neighbour(uint32_t i, int k, uint32_t sy, uint32_t sz)
{
    return (uint32_t) ((int64_t) i + ws_dx(k) + (int64_t) ws_dy(k) * sy + (int64_t) ws_dz(k) * sz);
}

// The ascent of voxel i with relief h > 0: the offset k of its parent, or -1 for a peak.  hn(k): the relief of the neighbour at
// offset k, 0 or less where it is outside the box or S.  Ascent by value, not by slope: a diagonal
// neighbour counts like a face neighbour.
template <typename Hn>
O2V_WS_FN int ws_ascent_step(uint32_t conn, int32_t h, uint32_t i, uint32_t sy, uint32_t sz, Hn &&hn)
{
    uint64_t best = ws_key(h, i);
    int at = -1;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        if (!ws_offset_on(conn, k)) continue;
        const int32_t v = hn(k);
        if (v <= 0) continue;
        const uint64_t key = ws_key(v, ws_neighbour(i, k, sy, sz));
        if (key > best) best = key, at = k;
    }
    return at;
}

// The LDS word of voxel (lx, ly, lz) of a tile, global index i, whose ascent took offset k (-1: a peak): the local index
// (lz * 8 + ly) * 64 + lx of a parent inside the tile, else kWsExit | the global index of the peak or of the parent outside.
O2V_WS_FN uint32_t ws_tile_word(int k, uint32_t lx, uint32_t ly, uint32_t lz, uint32_t i, uint32_t sy, uint32_t sz)
{
    if (k < 0) return kWsExit | i;
    const uint32_t X = lx + (uint32_t) ws_dx(k), Y = ly + (uint32_t) ws_dy(k), Z = lz + (uint32_t) ws_dz(k);   // (-1 wraps above any side)
    if (X < 64u && Y < 8u && Z < 8u) return (Z * 8u + Y) * 64u + X;
    return kWsExit | ws_neighbour(i, k, sy, sz);
}

// Where the path from local voxel l leaves the tile or ends: keys rise along it, so it ends.  Nothing is stored.
O2V_WS_FN uint32_t ws_follow(const uint32_t *q, uint32_t l)
{
    uint32_t w = q[l];
    while (!(w & kWsExit)) w = q[w];
    return w & ~kWsExit;
}

// The peak of i: a peak is its own parent.  Nothing is stored: k_ws_flatten's lanes store their own entry only - a halving store
// into an ancestor's entry could land behind that voxel's own last store and leave it short of its peak.
O2V_WS_FN uint32_t ws_root(const uint32_t *P, uint32_t i)
{
    for (;;) {
        const uint32_t p = ws_load(P + i);
        if (p == i) return i;
        i = p;
    }
}

// (key, value) into the pair table of 2^log2 slots (pt_slot): the value of a key becomes the maximum of what was inserted for
// it.  Returns 1 if the key took a free slot, 0 if it was there, -1 if the probe run found neither (the table has to grow).
template <typename Cas>
O2V_WS_FN int ws_table_insert(unsigned long long *keys, uint32_t *vals, uint32_t log2, uint64_t key, uint32_t val, Cas &&cas)
{
    bool fresh;
    const uint64_t slot = pt_slot(keys, log2, key, cas, fresh);
    if (slot == kPtNoPlace) return -1;
    if (ws_load(vals + slot) < val) ws_max32(vals + slot, val);   // (a plain read first: a pair's voxels mostly repeat its maximum)
    return fresh ? 1 : 0;
}

// The merge, on the host.  The n peaks by rank (ascending index) with their heights, the m distinct adjacent pairs in any order
// (keys of peak indices, saddles).  label_of_rank[r] = 1 + the rank of final(peak r) among the survivors; returns the survivors.
inline uint32_t ws_merge(uint32_t n, const uint32_t *peak_index, const int32_t *peak_h, uint64_t m, const unsigned long long *pair_keys,
                         const uint32_t *pair_vals, uint32_t min_depth, int32_t *label_of_rank)
{
    struct Pair {
        uint32_t saddle, a, b;   // ranks a < b
    };
    std::vector<Pair> pairs(m);
    const auto rank_of = [&](uint32_t index) { return (uint32_t) (std::lower_bound(peak_index, peak_index + n, index) - peak_index); };
    for (uint64_t e = 0; e < m; ++e) pairs[e] = Pair{pair_vals[e], rank_of((uint32_t) (pair_keys[e] >> 32)), rank_of((uint32_t) pair_keys[e])};
    std::sort(pairs.begin(), pairs.end(), [](const Pair &p, const Pair &q) {
        return p.saddle != q.saddle ? p.saddle > q.saddle : p.a != q.a ? p.a < q.a : p.b < q.b;
    });
    // a class is the tree under its representative, the peak of greatest key; rep[p] == p for a representative, and partner = rep
    std::vector<uint32_t> rep(n);
    std::vector<uint64_t> pers(n, ~0ull);   // (never killed: above any min_depth)
    for (uint32_t p = 0; p < n; ++p) rep[p] = p;
    const auto find = [&](uint32_t p) {
        while (rep[p] != p) p = rep[p] = rep[rep[p]];
        return p;
    };
    std::vector<uint32_t> partner(n);
    for (const Pair &e : pairs) {
        uint32_t p = find(e.a), q = find(e.b);
        if (p == q) continue;
        if (peak_h[p] != peak_h[q] ? peak_h[p] > peak_h[q] : p > q) std::swap(p, q);   // p: the smaller key (ranks order as indices do), killed
        pers[p] = (uint64_t) (uint32_t) peak_h[p] - e.saddle;
        partner[p] = q;
        rep[p] = q;
    }
    // final(p): along the partners while pers < min_depth; the chain ends because keys rise.  fin[p] == n: not yet known.
    std::vector<uint32_t> fin(n, n), chain;
    for (uint32_t p = 0; p < n; ++p) {
        uint32_t f = p;
        chain.clear();
        while (fin[f] == n && pers[f] < (uint64_t) min_depth) chain.push_back(f), f = partner[f];
        f = fin[f] == n ? f : fin[f];
        fin[f] = f;
        for (const uint32_t c : chain) fin[c] = f;
    }
    std::vector<uint32_t> before(n + 1u, 0u);   // the survivors of rank below r
    for (uint32_t p = 0; p < n; ++p) before[p + 1u] = before[p] + (fin[p] == p ? 1u : 0u);
    for (uint32_t p = 0; p < n; ++p) label_of_rank[p] = (int32_t) (before[fin[p]] + 1u);
    return before[n];
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
#ifndef O2V_WS_HOST

__global__ __launch_bounds__(kBlock) void k_ws_ascent_tiles(CcGrid g, I32View H, uint32_t *__restrict__ P)
{
    __shared__ int32_t s_h[kWsHalo];            // 26 400 bytes: [10 z][10 y][66 x], max(H, 0)
    __shared__ uint32_t s_q[kCcTileVoxels];     // 16 384 bytes: ws_tile_word
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tiles = g.W * g.tiles_y * g.tiles_z, sy = g.nx, sz = g.nx * g.ny;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        uint32_t tx, ty, tz;
        bits_tile_at(g, g.tiles_y, tile, tx, ty, tz);
        const uint32_t x0 = tx * 64u, y0 = ty * 8u, z0 = tz * 8u;
        __syncthreads();   // (the last tile's words are no longer read)
        for (uint32_t e = threadIdx.x; e < kWsHalo; e += kBlock) {
            const uint32_t r = e / kWsHaloX, hx = e - r * kWsHaloX, hz = r / kWsHaloY, hy = r - hz * kWsHaloY;
            const uint32_t x = x0 + hx - 1u, y = y0 + hy - 1u, z = z0 + hz - 1u;   // (-1 wraps above any dim)
            const int32_t v = x < g.nx && y < g.ny && z < g.nz ? H.at(x, y, z) : 0;
            s_h[e] = v > 0 ? v : 0;
        }
        __syncthreads();
        for (uint32_t row = wave; row < kCcTileRows; row += kBlock / 64u) {
            const uint32_t ly = row & 7u, lz = row >> 3, x = x0 + lane, y = y0 + ly, z = z0 + lz;
            if (x >= g.nx || y >= g.ny || z >= g.nz) continue;
            const uint32_t c = ((lz + 1u) * kWsHaloY + ly + 1u) * kWsHaloX + lane + 1u, i = cc_index(g, x, y, z);
            const int32_t h = s_h[c];
            if (h <= 0) continue;
            const int k = ws_ascent_step(g.conn, h, i, sy, sz, [&](int n) { return s_h[(int) c + ws_dx(n) + ws_dy(n) * (int) kWsHaloX + ws_dz(n) * (int) (kWsHaloX * kWsHaloY)]; });
            s_q[row * 64u + lane] = ws_tile_word(k, lane, ly, lz, i, sy, sz);
        }
        __syncthreads();
        for (uint32_t row = wave; row < kCcTileRows; row += kBlock / 64u) {
            const uint32_t ly = row & 7u, lz = row >> 3, x = x0 + lane, y = y0 + ly, z = z0 + lz;
            if (x >= g.nx || y >= g.ny || z >= g.nz) continue;
            const bool in = s_h[((lz + 1u) * kWsHaloY + ly + 1u) * kWsHaloX + lane + 1u] > 0;
            P[cc_index(g, x, y, z)] = in ? ws_follow(s_q, row * 64u + lane) : kWsOutside;
        }
    }
}

// O2V_WS_NO_TILES: the neighbours from global memory, P[i] = the parent
__global__ __launch_bounds__(kBlock) void k_ws_ascent(CcGrid g, I32View H, uint32_t *__restrict__ P)
{
    const uint32_t lane = threadIdx.x & 63u, sy = g.nx, sz = g.nx * g.ny;
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z;
        if (x >= g.nx) continue;
        const uint32_t i = cc_index(g, x, y, z);
        const int32_t h = H.at(x, y, z);
        if (h <= 0) {
            P[i] = kWsOutside;
            continue;
        }
        const int k = ws_ascent_step(g.conn, h, i, sy, sz, [&](int n) {
            const uint32_t X = x + (uint32_t) ws_dx(n), Y = y + (uint32_t) ws_dy(n), Z = z + (uint32_t) ws_dz(n);
            return X < g.nx && Y < g.ny && Z < g.nz ? H.at(X, Y, Z) : 0;
        });
        P[i] = k < 0 ? i : ws_neighbour(i, k, sy, sz);
    }
}

// P[i] = the peak of i; peaks: bit x of word wi says that voxel is a peak
__global__ __launch_bounds__(kBlock) void k_ws_flatten(CcGrid g, uint32_t *P, unsigned long long *__restrict__ peaks)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane;
        bool is_peak = false;
        if (x < g.nx) {
            const uint32_t i = cc_index(g, x, at.y, at.z);
            if (ws_load(P + i) != kWsOutside) {
                const uint32_t r = ws_root(P, i);
                if (r != i) ws_store(P + i, r);
                is_peak = r == i;
            }
        }
        const unsigned long long m = __ballot(is_peak);
        if (lane == 0u) peaks[wi] = m;
    }
}

// the rank of peak r among the peaks in ascending index
__device__ __forceinline__ uint32_t ws_rank(const CcGrid &g, uint32_t r, const unsigned long long *__restrict__ peaks, const uint32_t *__restrict__ local,
                                            const unsigned long long *__restrict__ block_offsets)
{
    uint32_t bit;
    const uint64_t rw = cc_root_word(g, r, bit);
    return (uint32_t) block_offsets[rw / kBlock] + local[rw] + (uint32_t) __popcll(peaks[rw] & ((1ull << bit) - 1ull));
}

// index[rank] and height[rank] of every peak
__global__ __launch_bounds__(kBlock) void k_ws_peaks(CcGrid g, I32View H, const unsigned long long *__restrict__ peaks, const uint32_t *__restrict__ local,
                                                     const unsigned long long *__restrict__ block_offsets, uint32_t *__restrict__ index,
                                                     int32_t *__restrict__ height)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (const uint64_t wi : bits_words(g)) {
        const unsigned long long w = peaks[wi];
        if (!((w >> lane) & 1ull)) continue;
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, rank = (uint32_t) block_offsets[wi / kBlock] + local[wi] + (uint32_t) __popcll(w & ((1ull << lane) - 1ull));
        index[rank] = cc_index(g, x, at.y, at.z);
        height[rank] = H.at(x, at.y, at.z);
    }
}

// ctr[0]: overflow, ctr[1] += the distinct pairs (the slots taken), ctr[2] += the boundary pairs seen (Count: O2V_HIP_FLAG_STAGE_TIMES)
template <bool Count>
__global__ __launch_bounds__(kBlock) void k_ws_pairs(CcGrid g, I32View H, const uint32_t *__restrict__ P, unsigned long long *keys, uint32_t *vals,
                                                     uint32_t log2, unsigned long long *ctr)
{
    const uint32_t lane = threadIdx.x & 63u, sy = g.nx, sz = g.nx * g.ny;
    uint32_t seen = 0, fresh = 0;
    bool overflow = false;
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z;
        if (x >= g.nx) continue;
        const uint32_t i = cc_index(g, x, y, z), mine = P[i];
        if (mine == kWsOutside) continue;
        int32_t h = 0;
#pragma unroll
        for (int k = 0; k < 13; ++k) {
            if (!ws_offset_on(g.conn, k)) continue;
            const uint32_t X = x + (uint32_t) ws_dx(k), Y = y + (uint32_t) ws_dy(k), Z = z + (uint32_t) ws_dz(k);
            if (X >= g.nx || Y >= g.ny || Z >= g.nz) continue;
            const uint32_t other = P[ws_neighbour(i, k, sy, sz)];
            if (other == kWsOutside || other == mine) continue;
            if (!h) h = H.at(x, y, z);
            const int32_t hn = H.at(X, Y, Z);
            const int got = ws_table_insert(keys, vals, log2, pt_key(mine, other), (uint32_t) (h < hn ? h : hn), PtCas{});
            ++seen, fresh += got > 0 ? 1u : 0u, overflow |= got < 0;
        }
    }
    if (overflow) ctr[0] = 1ull;   // (every writer stores the same word)
    for (int d = 32; d >= 1; d >>= 1) fresh += __shfl_xor(fresh, d);
    if (lane == 0u && fresh) atomicAdd(ctr + 1, (unsigned long long) fresh);
    if (Count) {
        for (int d = 32; d >= 1; d >>= 1) seen += __shfl_xor(seen, d);
        if (lane == 0u && seen) atomicAdd(ctr + 2, (unsigned long long) seen);
    }
}

// labels(x, y, z) = label_of_rank[the rank of the voxel's peak] (rank + 1 where there is no table), 0 outside S
__global__ __launch_bounds__(kBlock) void k_ws_labels(CcGrid g, const uint32_t *__restrict__ P, const unsigned long long *__restrict__ peaks,
                                                      const uint32_t *__restrict__ local, const unsigned long long *__restrict__ block_offsets,
                                                      const int32_t *__restrict__ label_of_rank, int32_t *__restrict__ labels, uint64_t s0, uint64_t s1, uint64_t s2)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (const uint64_t wi : bits_words(g)) {
        const BitWord at = bits_word_at(g, wi);
        const uint32_t x = at.wx * 64u + lane, y = at.y, z = at.z;
        if (x >= g.nx) continue;
        const uint32_t p = P[cc_index(g, x, y, z)];
        int32_t label = 0;
        if (p != kWsOutside) {
            const uint32_t rank = ws_rank(g, p, peaks, local, block_offsets);
            label = label_of_rank ? label_of_rank[rank] : (int32_t) (rank + 1u);
        }
        labels[(uint64_t) x * s0 + (uint64_t) y * s1 + (uint64_t) z * s2] = label;
    }
}

#endif   // O2V_WS_HOST
