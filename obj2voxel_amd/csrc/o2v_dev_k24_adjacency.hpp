// o2v_dev_k24_adjacency.hpp -- K24: the region adjacency of a label grid (o2v_hip_adjacency_count / _write): per pair of labels
// a < b that touch a row of 5 int64 - the face, edge-only and corner-only contacts, and with a values grid V the maximum over the
// contacts of min(V[u], V[v]) and the minimum of max(V[u], V[v]).  Included from o2v_device.hip inside its anonymous namespace,
// after K23; it takes the chunk (LsVec, ls_value, ls_shift_up, ls_diff, ls_lane) and the read (ls_read, ls_load1) of K19 and the
// table in global memory of o2v_dev_pair_table.hpp (pt_key, pt_hash, pt_slot, k_pt_list, I32View).
//
//   k_adj_init             the keys of the table in global memory: ~0 (free); its rows: 0, 0, 0, kAdjNoMax, kAdjNoMin.
//   k_adj_pairs<Format, Connectivity, Values, Vec>   the one pass.  K19's cut of the rows: chunks of 16 bytes along x (4 int32 or
//                          16 uint8), a lane per chunk, a wavefront 64 chunks that follow each other, a workgroup a range of its own.
//                          A voxel looks back at its 3, 9 or 13 earlier neighbours - (-1, 0, 0), (., -1, 0), (., ., -1) - so every
//                          contact is seen once: the chunk's own row and the rows (y-1, z), (y-1, z-1), (y, z-1), (y+1, z-1), each
//                          with the element before and behind the chunk where the connectivity asks for them (adj_chunk_contacts:
//                          a "differs" mask per row and x offset, its bits are the contacts).  An interior chunk - every mask 0 -
//                          leaves after the compares.  A lane merges what it finds while the pair stays the same (AdjPending,
//                          adj_merge); a pending pair is flushed when the key changes and at the chunk's end - there by one lane
//                          for the wavefront if all its pending pairs are one pair.  A flush goes into a table per workgroup in
//                          LDS, open-addressed by the key a << 32 | b (adj_find_slot: kAdjSlots slots, kAdjProbes probes, a slot
//                          is claimed by a 64-bit compare-and-swap), with 64-bit LDS add / max / min; a flush that finds no slot goes
//                          to the table in global memory (adj_to_global: pt_slot, five accumulators a slot), and so does every
//                          flush with table = 0 (O2V_ADJ_NO_TABLE=1).  At its end the workgroup adds its occupied slots to the
//                          global table.  A probe run there that finds no slot sets the overflow word: the host doubles the
//                          table and runs the pass again.
//   k_pt_list<long long, 5>   the global table's occupied slots as a list, any order, counted; without values columns 3 and 4 are 0.
// Every column is an integer sum, maximum or minimum, so the table does not depend on any order.  No private segment.

constexpr uint32_t kAdjCols = 5;                                      // O2V_HIP_ADJ_COLUMNS
constexpr uint32_t kAdjFace = 0, kAdjEdge = 1, kAdjCorner = 2, kAdjHigh = 3, kAdjLow = 4;
constexpr long long kAdjNoMax = -(1ll << 40), kAdjNoMin = 1ll << 40;  // columns 3 and 4 before any contact (a value is an int32)
#ifndef O2V_ADJ_SLOT_BITS
#define O2V_ADJ_SLOT_BITS 9
#endif
constexpr uint32_t kAdjSlotBits = O2V_ADJ_SLOT_BITS, kAdjSlots = 1u << kAdjSlotBits;   // slots of a workgroup's table: 24 KiB of LDS
constexpr uint32_t kAdjProbes = 16;                                   // slots a flush looks at before it goes to global memory
constexpr uint32_t kAdjNoSlot = ~0u;
constexpr uint32_t kAdjTableMaxLog2 = 36u;
constexpr uint32_t kAdjRows = 5;                                      // own, (y-1, z), (y-1, z-1), (y, z-1), (y+1, z-1)

#ifndef O2V_ADJ_HOST
#define O2V_ADJ_FN __host__ __device__ __forceinline__
#endif

// ---- contacts: the chunk's rows, the class, the pending pair, the probes of the table in LDS ------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_adjacency.py compiles this part for the host behind K19's and the pair
// table's, with O2V_ADJ_FN of its own, and runs it chunk by chunk against the reference.)

// The rows a chunk of n elements at x0 looks at.  row[r]: 0 its own, 1 (y-1, z), 2 (y-1, z-1), 3 (y, z-1), 4 (y+1, z-1); have: bit r,
// the row lies in the box; before[r] / behind[r]: the element at x0 - 1 / x0 + n of row r, read where has_before / has_behind.
struct AdjChunk {
    LsVec row[kAdjRows];
    int32_t before[kAdjRows], behind[kAdjRows];
    uint32_t have, n;
    bool has_before, has_behind;
};

// The element before a chunk at x = 0 is no neighbour: it is the last of another row.
O2V_ADJ_FN bool adj_has_before(uint32_t x0)
{
#ifdef O2V_ADJ_MUTATE_WRAP_BEFORE
    return true;   // (test only: the element before linear index x0 is taken whatever row it lies in)
#else
    return x0 > 0u;
#endif
}
O2V_ADJ_FN bool adj_has_behind(uint32_t x0, uint32_t n, uint32_t nx) { return x0 + n < nx; }

// dy, dz of row r against the chunk's own
O2V_ADJ_FN int adj_row_dy(uint32_t r) { return r == 0u || r == 3u ? 0 : r == 4u ? 1 : -1; }
O2V_ADJ_FN int adj_row_dz(uint32_t r) { return r >= 2u ? -1 : 0; }
// The class of a contact: the axes on which the two voxels differ - 1 a face, 2 an edge only, 3 a corner only.
O2V_ADJ_FN uint32_t adj_class(int dx, int dy, int dz) { return (uint32_t) (dx != 0) + (uint32_t) (dy != 0) + (uint32_t) (dz != 0); }
// Row r is read at connectivity conn; its elements before and behind the chunk are.
O2V_ADJ_FN bool adj_row_on(uint32_t conn, uint32_t r) { return adj_class(0, adj_row_dy(r), adj_row_dz(r)) <= pt_max_axes(conn); }
O2V_ADJ_FN bool adj_ends_on(uint32_t conn, uint32_t r) { return adj_class(1, adj_row_dy(r), adj_row_dz(r)) <= pt_max_axes(conn); }

// The chunk moved down by one element: element j is element j + 1 of v, the last element of a full chunk is `behind`.  (A chunk
// that is not full ends its row: nothing is behind it.)
template <uint32_t Format>
O2V_ADJ_FN LsVec adj_shift_down(const LsVec &v, int32_t behind)
{
    if (Format == kLsI32) return LsVec{{v.w[1], v.w[2], v.w[3], (uint32_t) behind}};
    return LsVec{{v.w[0] >> 8 | v.w[1] << 24, v.w[1] >> 8 | v.w[2] << 24, v.w[2] >> 8 | v.w[3] << 24, v.w[3] >> 8 | ((uint32_t) behind & 0xffu) << 24}};
}

// ls_diff, with the common case - the same 16 bytes - first
template <uint32_t Format>
O2V_ADJ_FN uint32_t adj_diff(const LsVec &a, const LsVec &b)
{
    if (!((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2]) | (a.w[3] ^ b.w[3]))) return 0u;
    return ls_diff<Format>(a, b);
}

// Bit j of masks[3 r + dx + 1]: element j of the chunk and its neighbour in row r at x offset dx are both in the box, are counted
// at this connectivity and hold different values.  Returns the masks' union: 0 for an interior chunk.
template <uint32_t Format, uint32_t Conn>
O2V_ADJ_FN uint32_t adj_chunk_masks(const AdjChunk &c, uint32_t masks[3u * kAdjRows])
{
    const uint32_t all = (1u << c.n) - 1u;
    uint32_t any = 0;
#pragma unroll
    for (uint32_t r = 0; r < kAdjRows; ++r)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            uint32_t m = 0;
            const bool earlier = r > 0u || dx < 0;
            if (earlier && adj_class(dx, adj_row_dy(r), adj_row_dz(r)) <= pt_max_axes(Conn) && ((c.have >> r) & 1u)) {
                const uint32_t valid = dx < 0 ? (c.has_before ? all : all & ~1u) : dx > 0 ? (c.has_behind ? all : all >> 1) : all;
                const LsVec other = dx < 0 ? ls_shift_up<Format>(c.row[r], c.before[r]) : dx > 0 ? adj_shift_down<Format>(c.row[r], c.behind[r]) : c.row[r];
                m = adj_diff<Format>(c.row[0], other) & valid;
            }
            masks[3u * r + (uint32_t) (dx + 1)] = m;
            any |= m;
        }
    return any;
}

O2V_ADJ_FN uint32_t adj_all_if(bool on) { return 0u - (uint32_t) on; }   // all bits, or none

// The value of the neighbour of element j in row r at x offset dx.
template <uint32_t Format>
O2V_ADJ_FN int32_t adj_neighbour_value(const AdjChunk &c, uint32_t r, int dx, uint32_t j)
{
    LsVec v{{0u, 0u, 0u, 0u}};   // (masks, no indexed register: r is the caller's loop variable)
    uint32_t before = 0, behind = 0;
#pragma unroll
    for (uint32_t q = 0; q < kAdjRows; ++q) {
        const uint32_t on = adj_all_if(q == r);
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) v.w[i] |= c.row[q].w[i] & on;
        before |= (uint32_t) c.before[q] & on, behind |= (uint32_t) c.behind[q] & on;
    }
    if (dx < 0 && j == 0u) return (int32_t) before;
    if (dx > 0 && j + 1u == ls_lane<Format>()) return (int32_t) behind;
    return ls_value<Format>(v, (uint32_t) ((int) j + dx));
}

// A value takes part: lo <= v <= n_labels (lo: 0 or 1, n_labels below 2^31 - 1).
O2V_ADJ_FN bool adj_counted(int32_t v, uint32_t lo, uint32_t n_labels) { return v >= (int32_t) lo && (uint32_t) v <= n_labels; }
O2V_ADJ_FN bool adj_outside(int32_t v, uint32_t n_labels) { return v < 0 || (uint32_t) v > n_labels; }

// The contacts of a chunk (masks: adj_chunk_masks' with a union that is not 0): emit(j, r, dx, a, b, cls) per contact between
// element j, of value a, and its neighbour in row r at x offset dx, of value b != a.
template <uint32_t Format, typename Emit>
O2V_ADJ_FN void adj_chunk_contacts(const AdjChunk &c, const uint32_t masks[3u * kAdjRows], Emit &&emit)
{
#pragma nounroll
    for (uint32_t k = 0; k < 3u * kAdjRows; ++k) {   // (one copy of the caller's code: this is not the common path)
        uint32_t m = 0;
#pragma unroll
        for (uint32_t i = 0; i < 3u * kAdjRows; ++i) m |= masks[i] & adj_all_if(i == k);   // (no indexed register)
        const uint32_t r = k / 3u;
        const int dx = (int) (k - 3u * r) - 1;
        const uint32_t cls = adj_class(dx, adj_row_dy(r), adj_row_dz(r));
        for (; m; m &= m - 1u) {
            const uint32_t j = (uint32_t) __builtin_ctz(m);
            emit(j, r, dx, ls_value<Format>(c.row[0], j), adj_neighbour_value<Format>(c, r, dx, j), cls);
        }
    }
}

// What a lane holds back while the pair stays the same: the pair's key, its contacts by class, the two passes.
struct AdjPending {
    uint64_t key;
    uint32_t cnt[3];
    long long hi, lo;
};

O2V_ADJ_FN void adj_pending_clear(AdjPending &p) { p.key = kPtEmpty, p.cnt[0] = p.cnt[1] = p.cnt[2] = 0u, p.hi = kAdjNoMax, p.lo = kAdjNoMin; }

// One contact of class cls of the pair `key` (values va, vb of the two voxels where with_values) into the pending pair;
// flush(pending) first where the pair changes.
template <typename Flush>
O2V_ADJ_FN void adj_merge(AdjPending &p, uint64_t key, uint32_t cls, bool with_values, int32_t va, int32_t vb, Flush &&flush)
{
    if (p.key != key) {
        if (p.key != kPtEmpty) flush(p);
        adj_pending_clear(p);
        p.key = key;
    }
    p.cnt[0] += cls == 1u ? 1u : 0u, p.cnt[1] += cls == 2u ? 1u : 0u, p.cnt[2] += cls == 3u ? 1u : 0u;
    if (with_values) {
        const long long m = va < vb ? va : vb, M = va < vb ? vb : va;
        p.hi = m > p.hi ? m : p.hi;
        p.lo = M < p.lo ? M : p.lo;
    }
}

// What a pending pair adds to its row: add(column, value) / raise(column, value) / lower(column, value) are the caller's sum,
// maximum and minimum.
template <typename Add, typename Raise, typename Lower>
O2V_ADJ_FN void adj_apply(const AdjPending &p, bool with_values, Add &&add, Raise &&raise, Lower &&lower)
{
    if (p.cnt[0]) add(kAdjFace, (uint64_t) p.cnt[0]);
    if (p.cnt[1]) add(kAdjEdge, (uint64_t) p.cnt[1]);
    if (p.cnt[2]) add(kAdjCorner, (uint64_t) p.cnt[2]);
    if (with_values) raise(kAdjHigh, p.hi), lower(kAdjLow, p.lo);
}

O2V_ADJ_FN long long adj_init_value(uint32_t column) { return column == kAdjHigh ? kAdjNoMax : column == kAdjLow ? kAdjNoMin : 0; }

// The slot of `key` in a workgroup's table of kAdjSlots keys (kPtEmpty: free), claimed if it has none yet: linear probing from
// the key's hash, kAdjNoSlot if none of kAdjProbes slots is the key's or free.  cas(p, expected, desired) returns what *p held.
template <typename Cas>
O2V_ADJ_FN uint32_t adj_find_slot(unsigned long long *keys, uint64_t key, Cas &&cas)
{
    uint32_t h = (uint32_t) pt_hash(key, kAdjSlotBits);
    for (uint32_t i = 0; i < kAdjProbes && i < kAdjSlots; ++i, h = (h + 1u) & (kAdjSlots - 1u)) {
        uint64_t seen = *(volatile unsigned long long *) (keys + h);
        if (seen == kPtEmpty) seen = cas(keys + h, kPtEmpty, key);
        if (seen == kPtEmpty || seen == key) return h;
    }
    return kAdjNoSlot;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_ADJ_HOST

struct AdjGrid {
    uint32_t n[3];
    uint32_t n_labels, lo;     // the labels lo ... n_labels take part
    uint32_t cpr;              // chunks per row
    uint32_t chunks;           // cpr * n[1] * n[2], at most the voxels: below 2^31
    uint32_t groups, per_wg;   // groups of kBlock chunks; groups per workgroup
    uint32_t table;            // 1: the table in LDS; 0: every flush to global memory
    uint32_t log2;             // the global table has 2^log2 slots
    uint32_t count;            // 1: the flushes are counted (O2V_HIP_FLAG_STAGE_TIMES)
};

// ctr: [0] overflow, [1] voxels outside [0, n_labels], [2] flushes into LDS, [3] flushes to global memory, [4] listed pairs, [5] slots taken
constexpr uint32_t kAdjCtrs = 8;

__global__ __launch_bounds__(kBlock) void k_adj_init(unsigned long long *__restrict__ keys, long long *__restrict__ rows, uint64_t slots)
{
    const uint64_t n = slots * kAdjCols, step = (uint64_t) gridDim.x * kBlock;
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
        rows[i] = adj_init_value((uint32_t) (i % kAdjCols));
        if (i < slots) keys[i] = kPtEmpty;
    }
}

// What a pending pair, or a slot of a workgroup's table, holds of the pair `key` - its contacts by class (a workgroup's sums pass
// 2^32) and its two passes - into the global table; false: no slot (overflow).
__device__ __forceinline__ bool adj_to_global(uint64_t key, uint64_t faces, uint64_t edges, uint64_t corners, bool with_values, long long hi, long long lo,
                                              unsigned long long *keys, long long *rows, uint32_t log2, uint32_t &n_fresh)
{
    bool fresh;
    const uint64_t slot = pt_slot(keys, log2, key, PtCas{}, fresh);
    n_fresh += fresh ? 1u : 0u;
    if (slot == kPtNoPlace) return false;
    long long *const row = rows + slot * kAdjCols;
    if (faces) atomicAdd(reinterpret_cast<unsigned long long *>(row + kAdjFace), (unsigned long long) faces);
    if (edges) atomicAdd(reinterpret_cast<unsigned long long *>(row + kAdjEdge), (unsigned long long) edges);
    if (corners) atomicAdd(reinterpret_cast<unsigned long long *>(row + kAdjCorner), (unsigned long long) corners);
    if (with_values) {   // (a plain read first: a pair's contacts mostly repeat its passes)
        if (*(volatile long long *) (row + kAdjHigh) < hi) atomicMax(row + kAdjHigh, hi);
        if (*(volatile long long *) (row + kAdjLow) > lo) atomicMin(row + kAdjLow, lo);
    }
    return true;
}

template <uint32_t Format, uint32_t Conn, bool Values, bool Vec>
__global__ __launch_bounds__(kBlock) void k_adj_pairs(RaySource src, I32View V, AdjGrid g, unsigned long long *keys, long long *rows, unsigned long long *ctr)
{
    constexpr uint32_t K = ls_lane<Format>();
    __shared__ unsigned long long s_key[kAdjSlots];
    __shared__ long long s_tab[kAdjSlots * kAdjCols];
    if (g.table) {
        for (uint32_t i = threadIdx.x; i < kAdjSlots; i += kBlock) s_key[i] = kPtEmpty;
        for (uint32_t i = threadIdx.x; i < kAdjSlots * kAdjCols; i += kBlock) s_tab[i] = adj_init_value(i % kAdjCols);
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g0 = blockIdx.x * g.per_wg, g1 = min(g.groups, g0 + g.per_wg);
    unsigned long long n_outside = 0;
    uint32_t to_lds = 0, to_global = 0, n_fresh = 0;
    bool overflow = false;
    const auto flush = [&](const AdjPending &p) {
        const uint32_t slot = g.table ? adj_find_slot(s_key, p.key, PtCas{}) : kAdjNoSlot;
        const bool in_lds = slot != kAdjNoSlot;
        to_lds += in_lds ? 1u : 0u, to_global += in_lds ? 0u : 1u;   // (both sums in both branches: the counters stay in registers)
        if (in_lds) {
            long long *const row = s_tab + slot * kAdjCols;
            adj_apply(p, Values, [&](uint32_t c, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long *>(row + c), (unsigned long long) v); },
                      [&](uint32_t c, long long v) { atomicMax(row + c, v); }, [&](uint32_t c, long long v) { atomicMin(row + c, v); });
        } else {
            overflow |= !adj_to_global(p.key, p.cnt[0], p.cnt[1], p.cnt[2], Values, p.hi, p.lo, keys, rows, g.log2, n_fresh);
        }
    };
    for (uint32_t gi = g0; gi < g1; ++gi) {
        const uint64_t c64 = (uint64_t) gi * kBlock + threadIdx.x;
        AdjPending pend;
        adj_pending_clear(pend);
        if (c64 < g.chunks) {
            const uint32_t ci = (uint32_t) c64, row = ci / g.cpr, x0 = (ci - row * g.cpr) * K, z = row / g.n[1], y = row - z * g.n[1];
            AdjChunk c;
            c.n = min(K, g.n[0] - x0);
            c.has_before = adj_has_before(x0), c.has_behind = adj_has_behind(x0, c.n, g.n[0]);
            c.have = 1u | (y > 0u ? 2u : 0u) | (y > 0u && z > 0u ? 4u : 0u) | (z > 0u ? 8u : 0u) | (z > 0u && y + 1u < g.n[1] ? 16u : 0u);
#pragma unroll
            for (uint32_t r = 0; r < kAdjRows; ++r) {
                c.row[r] = LsVec{{0u, 0u, 0u, 0u}}, c.before[r] = c.behind[r] = 0;
                if (!adj_row_on(Conn, r) || !((c.have >> r) & 1u)) continue;
                const uint64_t at = (uint64_t) (uint32_t) ((int) y + adj_row_dy(r)) * src.s1 + (uint64_t) (uint32_t) ((int) z + adj_row_dz(r)) * src.s2;
                c.row[r] = ls_read<Format, Vec>(src, at, x0, c.n);
                if (r == 0u || adj_ends_on(Conn, r)) {
                    if (c.has_before) c.before[r] = ls_load1<Format>(src, at, x0 - 1u);
                    if (c.has_behind && r > 0u) c.behind[r] = ls_load1<Format>(src, at, x0 + c.n);
                }
            }
            // the voxels that are in no row of K19's table either
            if (Format == kLsI32 || g.n_labels < 255u) {
#pragma unroll
                for (uint32_t j = 0; j < K; ++j) n_outside += j < c.n && adj_outside(ls_value<Format>(c.row[0], j), g.n_labels) ? 1u : 0u;
            }
            uint32_t masks[3u * kAdjRows];
            if (adj_chunk_masks<Format, Conn>(c, masks)) {
                adj_chunk_contacts<Format>(c, masks, [&](uint32_t j, uint32_t r, int dx, int32_t a, int32_t b, uint32_t cls) {
                    if (!adj_counted(a, g.lo, g.n_labels) || !adj_counted(b, g.lo, g.n_labels)) return;
                    int32_t va = 0, vb = 0;
                    if (Values) {
                        const uint32_t x = x0 + j;
                        va = V.at(x, y, z);
                        vb = V.at((uint32_t) ((int) x + dx), (uint32_t) ((int) y + adj_row_dy(r)), (uint32_t) ((int) z + adj_row_dz(r)));
                    }
                    adj_merge(pend, pt_key((uint32_t) a, (uint32_t) b), cls, Values, va, vb, flush);
                });
            }
        }
        // the chunk's end: if every pending pair of the wavefront is one pair, one lane flushes their sum
        const bool has = pend.key != kPtEmpty;
        const unsigned long long with = __ballot(has);
        if (!with) continue;
        const uint32_t first = (uint32_t) __builtin_ctzll(with);
        const uint64_t key0 = (uint64_t) __shfl((unsigned long long) pend.key, (int) first);
        if (__popcll(with) > 1 && !__ballot(has && pend.key != key0)) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {   // (a chunk has at most 16 x 13 contacts: the wavefront's sums fit 32 bits)
                pend.cnt[0] += __shfl_xor(pend.cnt[0], d), pend.cnt[1] += __shfl_xor(pend.cnt[1], d), pend.cnt[2] += __shfl_xor(pend.cnt[2], d);
                if (Values) {
                    const long long hi = __shfl_xor(pend.hi, d), lo = __shfl_xor(pend.lo, d);
                    pend.hi = hi > pend.hi ? hi : pend.hi, pend.lo = lo < pend.lo ? lo : pend.lo;
                }
            }
            pend.key = key0;
            if (lane == first) flush(pend);
        } else if (has) {
            flush(pend);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n_outside += __shfl_xor(n_outside, d);
    if (lane == 0u && n_outside) atomicAdd(ctr + 1, n_outside);
    if (g.table) {
        __syncthreads();
        for (uint32_t slot = threadIdx.x; slot < kAdjSlots; slot += kBlock) {
            const uint64_t key = s_key[slot];
            if (key == kPtEmpty) continue;
            const long long *const row = s_tab + slot * kAdjCols;
            overflow |= !adj_to_global(key, (uint64_t) row[kAdjFace], (uint64_t) row[kAdjEdge], (uint64_t) row[kAdjCorner], Values, row[kAdjHigh], row[kAdjLow], keys, rows,
                                       g.log2, n_fresh);
        }
    }
    if (overflow) ctr[0] = 1ull;   // (every writer stores the same word)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n_fresh += __shfl_xor(n_fresh, d);
    if (lane == 0u && n_fresh) atomicAdd(ctr + 5, (unsigned long long) n_fresh);
    if (g.count) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) to_lds += __shfl_xor(to_lds, d), to_global += __shfl_xor(to_global, d);
        if (lane == 0u && to_lds) atomicAdd(ctr + 2, (unsigned long long) to_lds);
        if (lane == 0u && to_global) atomicAdd(ctr + 3, (unsigned long long) to_global);
    }
}

#endif   // O2V_ADJ_HOST
