// o2v_dev_k19_label_stats.hpp -- K19: per-label statistics of a dense label grid (o2v_hip_label_stats): per value L of the grid a
// row of 17 int64 - the voxel count, the bounding box, the sums of the coordinates and of their products, the exposed faces.
// Included from o2v_device.hip inside its anonymous namespace, after K18; it reads the grid through K11's ray_read16_raw.
//
//   k_ls_init              every element of the table: 0, and the empty box (min 2^31 - 1, max -1) where the box is asked for; the
//                          counter of the voxels outside [0, n_labels] cleared.
//   k_label_stats<Format, Vec, Faces>   the one pass over the grid.  The rows of the box are cut into chunks of 16 bytes along x
//                          (4 int32 or 16 uint8, kLsLane), numbered row by row; a lane takes a chunk, a wavefront 64 chunks that
//                          follow each other, a workgroup a range of its own of such groups (neighbouring voxels, the same few
//                          labels).  A lane turns its chunk into runs (label, x0, len): the bits of `starts` are where a value
//                          differs from the one before it.  The run a chunk ends with and the run the next chunk begins with are
//                          one run if they have one label and lie in one row (ls_joins): a segmented inclusive scan over the
//                          wavefront (ls_scan_step, six shuffle steps) adds the lengths - and the faces - of such chains up, and the
//                          lane in which a chain ends adds it once.  A run costs what a voxel costs: its columns are closed forms
//                          (ls_apply_run).  Where it goes: a table per workgroup in LDS, open-addressed by label (ls_find_slot:
//                          kLsSlots slots, kLsProbes probes, a slot is claimed by a compare-and-swap of its key), with 64-bit LDS
//                          add / min / max; a run that finds no slot within the probes goes to the table in global memory with
//                          64-bit atomics, and so does every run with table = 0 (O2V_LS_NO_TABLE=1).  At its end the workgroup
//                          adds its occupied slots to global memory.  Faces: the variant also reads the rows at y +- 1 and z +- 1
//                          and the elements before and behind the chunk; a run's faces are the popcounts of six "differs" masks
//                          under the run's bits.
// Every column is an integer sum, minimum or maximum, so the table does not depend on any order.  No private segment.

constexpr uint32_t kLsI32 = 0, kLsU8 = 1;                                        // O2V_HIP_LABELS_*
constexpr uint32_t kLsBox = 1, kLsSums = 2, kLsMoments = 4, kLsFaces = 8;        // O2V_HIP_STATS_*
constexpr uint32_t kLsCols = 17;                                                 // O2V_HIP_STATS_COLUMNS
constexpr uint32_t kLsCount = 0, kLsMin = 1, kLsMax = 4, kLsSum = 7, kLsMoment = 10, kLsFace = 16;   // the first column of each group
constexpr long long kLsEmptyMin = 0x7fffffffll, kLsEmptyMax = -1;                // the box of a row without voxels
constexpr uint32_t kLsSlotBits = 7, kLsSlots = 1u << kLsSlotBits;                // slots of a workgroup's table: 17 KiB of LDS
constexpr uint32_t kLsProbes = 8;                                                // slots a run looks at before it goes to global memory
constexpr int32_t kLsEmptyKey = -1;                                              // (a label that is counted is >= 0)
constexpr uint32_t kLsNoSlot = ~0u;

#ifndef O2V_LS_HOST
#define O2V_LS_FN __host__ __device__ __forceinline__
#endif

// ---- runs: a chunk's values, the closed forms, the joining rule, the slot probe ------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_label_stats.py compiles this part for the host, with O2V_LS_FN of its own,
// and runs it against the reference.)

// The 16 bytes of a chunk: element j in bits [8 E j, 8 E (j + 1)), E = 4 (I32) or 1 (U8); zero behind the chunk's last element.
struct LsVec {
    uint32_t w[4];
};

template <uint32_t Format> constexpr uint32_t ls_lane() { return Format == kLsI32 ? 4u : 16u; }   // elements of a chunk

// Element j of a chunk (any j below ls_lane: selects, no indexed register).
template <uint32_t Format>
O2V_LS_FN int32_t ls_value(const LsVec &v, uint32_t j)
{
    const uint32_t q = Format == kLsI32 ? j : j >> 2;
    const uint32_t word = q == 0u ? v.w[0] : q == 1u ? v.w[1] : q == 2u ? v.w[2] : v.w[3];
    return Format == kLsI32 ? (int32_t) word : (int32_t) ((word >> (8u * (j & 3u))) & 0xffu);
}

// The chunk moved up by one element: element j is element j - 1 of v, element 0 is `before`.
template <uint32_t Format>
O2V_LS_FN LsVec ls_shift_up(const LsVec &v, int32_t before)
{
    if (Format == kLsI32) return LsVec{{(uint32_t) before, v.w[0], v.w[1], v.w[2]}};
    return LsVec{{v.w[0] << 8 | ((uint32_t) before & 0xffu), v.w[1] << 8 | v.w[0] >> 24, v.w[2] << 8 | v.w[1] >> 24, v.w[3] << 8 | v.w[2] >> 24}};
}

// Bit j: element j of a differs from element j of b.
template <uint32_t Format>
O2V_LS_FN uint32_t ls_diff(const LsVec &a, const LsVec &b)
{
    uint32_t m = 0;
    if (Format == kLsI32) {
        m = (uint32_t) (a.w[0] != b.w[0]) | (uint32_t) (a.w[1] != b.w[1]) << 1 | (uint32_t) (a.w[2] != b.w[2]) << 2 | (uint32_t) (a.w[3] != b.w[3]) << 3;
    } else {
        const uint32_t x[4] = {a.w[0] ^ b.w[0], a.w[1] ^ b.w[1], a.w[2] ^ b.w[2], a.w[3] ^ b.w[3]};
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) m |= (uint32_t) ((x[j >> 2] >> (8u * (j & 3u)) & 0xffu) != 0u) << j;
    }
    return m;
}

// The starts of the runs of a chunk of n >= 1 elements: bit 0, and bit j where element j differs from element j - 1.
template <uint32_t Format>
O2V_LS_FN uint32_t ls_starts(const LsVec &v, uint32_t n)
{
    return (ls_diff<Format>(v, ls_shift_up<Format>(v, 0)) | 1u) & ((1u << n) - 1u);
}

// What a run adds to its label's row: len voxels from (X0, Y, Z) along x, global coordinates below 2^16, with `faces` exposed
// faces.  add(column, value) / lower(column, value) / raise(column, value) are the caller's sum, minimum and maximum.  The sums
// over x = X0 ... X0 + len - 1 are closed forms: sum x = len X0 + len (len - 1) / 2, sum x^2 = len X0^2 + X0 len (len - 1) +
// (len - 1) len (2 len - 1) / 6; y and z are the row's.  Every term is below 2^48.
template <typename Add, typename Lower, typename Raise>
O2V_LS_FN void ls_apply_run(uint32_t which, uint64_t X0, uint64_t len, uint64_t Y, uint64_t Z, uint64_t faces, Add &&add, Lower &&lower, Raise &&raise)
{
    add(kLsCount, len);
    if (which & kLsBox) {
        lower(kLsMin, X0), lower(kLsMin + 1u, Y), lower(kLsMin + 2u, Z);
        raise(kLsMax, X0 + len - 1u), raise(kLsMax + 1u, Y), raise(kLsMax + 2u, Z);
    }
    const uint64_t pairs = len * (len - 1u);     // (even)
    const uint64_t sx = len * X0 + pairs / 2u;
    if (which & kLsSums) add(kLsSum, sx), add(kLsSum + 1u, len * Y), add(kLsSum + 2u, len * Z);
    if (which & kLsMoments) {
#ifdef O2V_LS_MUTATE_NO_SQUARES_TERM
        const uint64_t squares = 0;   // (test only: the run's own sum of squares left out)
#else
        const uint64_t squares = pairs * (2u * len - 1u) / 6u;
#endif
        add(kLsMoment, len * X0 * X0 + X0 * pairs + squares), add(kLsMoment + 1u, len * Y * Y), add(kLsMoment + 2u, len * Z * Z);
        add(kLsMoment + 3u, Y * sx), add(kLsMoment + 4u, Z * sx), add(kLsMoment + 5u, len * Y * Z);
    }
    if (which & kLsFaces) add(kLsFace, faces);
}

// What an element of the table holds before any run: the empty box where the box is asked for, else 0.
O2V_LS_FN long long ls_init_value(uint32_t column, uint32_t which)
{
    if (!(which & kLsBox) || column < kLsMin || column >= kLsSum) return 0;
    return column < kLsMax ? kLsEmptyMin : kLsEmptyMax;
}

// The joining rule: the run a chunk ends with (its label, its row) and the run the next chunk begins with are one run.
O2V_LS_FN bool ls_joins(int32_t prev_label, uint32_t prev_row, int32_t label, uint32_t row) { return prev_label == label && prev_row == row; }

// A chain's length (at most 64 x 16) and faces (at most six per voxel) in one word, so that one scan adds both.
O2V_LS_FN uint32_t ls_pack(uint32_t len, uint32_t faces) { return len | faces << 16; }
O2V_LS_FN uint32_t ls_len(uint32_t packed) { return packed & 0xffffu; }
O2V_LS_FN uint32_t ls_faces(uint32_t packed) { return packed >> 16; }

// One step of the inclusive segmented scan over the lanes: (v, head) of a lane takes in (pv, phead) of the lane d before it
// (d = 1, 2, 4 ... 32, lanes below d left as they are).  head: the lane's chain begins in it.
O2V_LS_FN void ls_scan_step(uint32_t &v, bool &head, uint32_t pv, bool phead)
{
    if (!head) v += pv, head = phead;
}

O2V_LS_FN uint32_t ls_hash(int32_t label) { return ((uint32_t) label * 0x9e3779b1u) >> (32u - kLsSlotBits); }

// The slot of `label` in a table of kLsSlots keys (kLsEmptyKey: free), claimed if it has none yet: linear probing from the
// label's hash, kLsNoSlot if none of kLsProbes slots is the label's or free.  cas(p, expected, desired) returns what *p held.
template <typename Cas>
O2V_LS_FN uint32_t ls_find_slot(int32_t *keys, int32_t label, Cas &&cas)
{
    uint32_t h = ls_hash(label);
    for (uint32_t i = 0; i < kLsProbes; ++i, h = (h + 1u) & (kLsSlots - 1u)) {
        int32_t seen = *(volatile int32_t *) (keys + h);
        if (seen == kLsEmptyKey) seen = cas(keys + h, kLsEmptyKey, label);
        if (seen == kLsEmptyKey || seen == label) return h;
    }
    return kLsNoSlot;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_LS_HOST

struct LsGrid {
    uint32_t n[3], o[3];       // the box and its origin
    uint32_t n_labels, which;
    uint32_t cpr;              // chunks per row
    uint32_t chunks;           // cpr * n[1] * n[2], at most the voxels: below 2^31
    uint32_t groups, per_wg;   // groups of kBlock chunks; groups per workgroup
    uint32_t table;            // 1: the table in LDS; 0: every run to global memory
};

__global__ __launch_bounds__(kBlock) void k_ls_init(long long *__restrict__ table, uint64_t rows, uint32_t which, unsigned long long *__restrict__ outside)
{
    const uint64_t n = rows * kLsCols, step = (uint64_t) gridDim.x * kBlock;
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += step) table[i] = ls_init_value((uint32_t) (i % kLsCols), which);
    if (blockIdx.x == 0 && threadIdx.x == 0) *outside = 0;
}

template <uint32_t Format>
__device__ __forceinline__ int32_t ls_load1(const RaySource &src, uint64_t at, uint32_t x)
{
    if (Format == kLsI32) return static_cast<const int32_t *>(src.p)[at + (uint64_t) x * src.s0];
    return (int32_t) static_cast<const uint8_t *>(src.p)[at + (uint64_t) x * src.s0];
}

template <uint32_t Format, bool Vec>
__device__ __forceinline__ LsVec ls_read(const RaySource &src, uint64_t at, uint32_t x0, uint32_t n)
{
    const uint4 v = ray_read16_raw<Format == kLsI32 ? 4u : 1u, Vec>(src, at, x0, n);
    return LsVec{{v.x, v.y, v.z, v.w}};
}

// A run added to `row`, its label's 17 columns in LDS or in global memory (the address space is the caller's).
__device__ __forceinline__ void ls_add_run(long long *row, uint32_t which, uint64_t X0, uint64_t len, uint64_t Y, uint64_t Z, uint64_t faces)
{
    ls_apply_run(which, X0, len, Y, Z, faces,
                 [&](uint32_t c, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long *>(row + c), (unsigned long long) v); },
                 [&](uint32_t c, uint64_t v) { atomicMin(row + c, (long long) v); }, [&](uint32_t c, uint64_t v) { atomicMax(row + c, (long long) v); });
}

template <uint32_t Format, bool Vec, bool Faces>
__global__ __launch_bounds__(kBlock) void k_label_stats(RaySource src, LsGrid g, long long *__restrict__ table, unsigned long long *__restrict__ outside)
{
    constexpr uint32_t K = ls_lane<Format>();
    __shared__ int32_t s_key[kLsSlots];
    __shared__ long long s_tab[kLsSlots * kLsCols];
    if (g.table) {
        for (uint32_t i = threadIdx.x; i < kLsSlots; i += kBlock) s_key[i] = kLsEmptyKey;
        for (uint32_t i = threadIdx.x; i < kLsSlots * kLsCols; i += kBlock) s_tab[i] = ls_init_value(i % kLsCols, g.which);
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g0 = blockIdx.x * g.per_wg, g1 = min(g.groups, g0 + g.per_wg);   // (g0 <= groups < 2^23)
    unsigned long long n_outside = 0;
    for (uint32_t gi = g0; gi < g1; ++gi) {
        const uint64_t c64 = (uint64_t) gi * kBlock + threadIdx.x;
        const bool active = c64 < g.chunks;
        uint32_t row = 0, x0 = 0, y = 0, z = 0, n = 0, starts = 0, last = 0, tail = 0;
        uint32_t diff[6] = {0u, 0u, 0u, 0u, 0u, 0u};   // Faces: bit j, the neighbour of element j at x - 1, x + 1, y - 1, y + 1, z - 1, z + 1 differs
        int32_t first_label = 0, last_label = 0;
        LsVec v{{0u, 0u, 0u, 0u}};
        if (active) {
            const uint32_t c = (uint32_t) c64;
            row = c / g.cpr;
            x0 = (c - row * g.cpr) * K;
            z = row / g.n[1], y = row - z * g.n[1];
            n = min(K, g.n[0] - x0);
            const uint64_t at = (uint64_t) y * src.s1 + (uint64_t) z * src.s2;
            v = ls_read<Format, Vec>(src, at, x0, n);
            const uint32_t all = (1u << n) - 1u;
            if (Faces) {
                const bool before = x0 > 0u, behind = x0 + n < g.n[0];
                const uint32_t d = ls_diff<Format>(v, ls_shift_up<Format>(v, before ? ls_load1<Format>(src, at, x0 - 1u) : 0));
                diff[0] = (before ? d : d | 1u) & all;
                const bool end_differs = !behind || ls_load1<Format>(src, at, x0 + n) != ls_value<Format>(v, n - 1u);
                diff[1] = ((d >> 1) & (all >> 1)) | (uint32_t) end_differs << (n - 1u);
                diff[2] = y > 0u ? ls_diff<Format>(v, ls_read<Format, Vec>(src, at - src.s1, x0, n)) & all : all;
                diff[3] = y + 1u < g.n[1] ? ls_diff<Format>(v, ls_read<Format, Vec>(src, at + src.s1, x0, n)) & all : all;
                diff[4] = z > 0u ? ls_diff<Format>(v, ls_read<Format, Vec>(src, at - src.s2, x0, n)) & all : all;
                diff[5] = z + 1u < g.n[2] ? ls_diff<Format>(v, ls_read<Format, Vec>(src, at + src.s2, x0, n)) & all : all;
                starts = (d | 1u) & all;
            } else {
                starts = ls_starts<Format>(v, n);
            }
            last = 31u - (uint32_t) __builtin_clz(starts);   // where the chunk's last run begins
            first_label = ls_value<Format>(v, 0u), last_label = ls_value<Format>(v, last);
            uint32_t f = 0;
            if (Faces) {
                const uint32_t m = all & ~((1u << last) - 1u);
#pragma unroll
                for (uint32_t k = 0; k < 6u; ++k) f += (uint32_t) __builtin_popcount(diff[k] & m);
            }
            tail = ls_pack(n - last, f);
        }
        // the chains: the chunk's first run is the run the chunk before ends with; a chunk of one run passes the chain on
        const int32_t prev_label = __shfl_up(last_label, 1);
        const uint32_t prev_row = __shfl_up(row, 1);
        const bool joined = active && lane > 0u && ls_joins(prev_label, prev_row, first_label, row);
        const bool single = starts == 1u;
        uint32_t sv = tail;
        bool head = !(single && joined);
#pragma unroll
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const uint32_t pv = __shfl_up(sv, d);
            const bool phead = __shfl_up((int) head, d) != 0;
            if (lane >= d) ls_scan_step(sv, head, pv, phead);
        }
        const uint32_t before = __shfl_up(sv, 1);                              // the chain that ends with the chunk before
        const bool goes_on = __shfl_down((int) joined, 1) != 0 && lane < 63u;   // the chunk's last run is the next chunk's first
        if (active) {
            const uint64_t Y = (uint64_t) g.o[1] + y, Z = (uint64_t) g.o[2] + z;
            for (uint32_t m = starts; m;) {
                const uint32_t s = (uint32_t) __builtin_ctz(m);
                m &= m - 1u;
                const uint32_t e = m ? (uint32_t) __builtin_ctz(m) : n;
                if (!m && goes_on) break;
                uint32_t len = e - s, faces = 0;
                if (Faces) {
                    const uint32_t rm = ((1u << e) - 1u) & ~((1u << s) - 1u);
#pragma unroll
                    for (uint32_t k = 0; k < 6u; ++k) faces += (uint32_t) __builtin_popcount(diff[k] & rm);
                }
                if (s == 0u && single) len = ls_len(sv), faces = ls_faces(sv);             // (the scan has added the chain before it)
                else if (s == 0u && joined) len += ls_len(before), faces += ls_faces(before);
                const int32_t label = ls_value<Format>(v, s);
                if (label < 0 || (uint32_t) label > g.n_labels) {
                    n_outside += len;
                    continue;
                }
                const uint64_t X0 = (uint64_t) g.o[0] + x0 + e - len;
                const uint32_t slot = g.table ? ls_find_slot(s_key, label, [](int32_t *p, int32_t expected, int32_t desired) { return atomicCAS(p, expected, desired); })
                                              : kLsNoSlot;
                if (slot != kLsNoSlot)
                    ls_add_run(s_tab + slot * kLsCols, g.which, X0, len, Y, Z, faces);
                else
                    ls_add_run(table + (uint64_t) (uint32_t) label * kLsCols, g.which, X0, len, Y, Z, faces);
            }
        }
    }
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) n_outside += __shfl_xor(n_outside, (int) d);
    if (lane == 0u && n_outside) atomicAdd(outside, n_outside);
    if (g.table) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < kLsSlots * kLsCols; i += kBlock) {
            const uint32_t slot = i / kLsCols, c = i - slot * kLsCols;
            const int32_t label = s_key[slot];
            const long long val = s_tab[i];
            if (label == kLsEmptyKey || val == ls_init_value(c, g.which)) continue;
            long long *const dst = table + (uint64_t) (uint32_t) label * kLsCols + c;
            if (c >= kLsMin && c < kLsMax) atomicMin(dst, val);
            else if (c >= kLsMax && c < kLsSum) atomicMax(dst, val);
            else atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long) val);
        }
    }
}

#endif   // O2V_LS_HOST
