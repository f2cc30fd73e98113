// o2v_dev_pair_table.hpp -- the table of unordered pairs of 31-bit ids that K23 (adjacent basins) and K24 (labels that touch)
// fill in global memory.  Included from o2v_device.hip inside its anonymous namespace, before K23.
//
// A slot is a 64-bit key, (smaller id) << 32 | larger id, ~0 while it is free (no pair: ids are below 2^31); what a slot
// accumulates beside its key - K23's saddle, K24's five columns - is the family's own array, indexed by the slot.  Open
// addressing: the slot of a key is its hash, the next slots in turn; a free slot is claimed by a 64-bit compare-and-swap.  A
// probe run of kPtProbeLimit slots (or the whole table) that finds neither the key nor a free slot reports kPtNoPlace: the
// family's pass sets its overflow word, and the host doubles the table and runs the pass again (pt_grow, o2v_dev_host_args.hpp).

#ifndef O2V_PT_HOST
#define O2V_PT_FN __host__ __device__ __forceinline__
#endif

// ---- the table: the key, the hash, the probe run, the first size --------------------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_pair_table.py compiles this part for the host with an O2V_PT_FN of its
// own, and the host tests of K23 and K24 put it in front of their family's plain part.)

constexpr uint64_t kPtEmpty = ~0ull, kPtNoPlace = ~0ull;          // a free slot; pt_slot: the probe run found no place
constexpr uint32_t kPtProbeLimit = 128u, kPtMinLog2 = 10u;        // slots a probe run looks at; log2 of the smallest first size

O2V_PT_FN uint64_t pt_key(uint32_t a, uint32_t b) { return a < b ? (uint64_t) a << 32 | b : (uint64_t) b << 32 | a; }
// The first slot of a key's probe run in a table of 2^log2 slots: the product's top log2 bits.  (Two shifts, so that a table of
// one slot shifts by no 64 bits; a test of log2 in its place cost k_adj_pairs 3 % of its time - DESIGN.md section 28.)
O2V_PT_FN uint64_t pt_hash(uint64_t key, uint32_t log2) { return (key * 0x9e3779b97f4a7c15ull) >> 1 >> (63u - log2); }

// The axes on which two voxels that count as neighbours at connectivity 6 / 18 / 26 may differ: 1 / 2 / 3.
O2V_PT_FN uint32_t pt_max_axes(uint32_t conn) { return conn == 6u ? 1u : conn == 18u ? 2u : 3u; }

// The slot of `key` in the table of 2^log2 keys, claimed if it has none yet; kPtNoPlace if the probe run found neither - the
// table has to grow.  cas(p, expected, desired) returns what *p held.  fresh: this call took a free slot for the key.
template <typename Cas>
O2V_PT_FN uint64_t pt_slot(unsigned long long *keys, uint32_t log2, uint64_t key, Cas &&cas, bool &fresh)
{
    fresh = false;
    const uint64_t mask = (1ull << log2) - 1ull, run = mask + 1ull < kPtProbeLimit ? mask + 1ull : kPtProbeLimit;
    uint64_t slot = pt_hash(key, log2);
    for (uint64_t n = 0; n < run; ++n, slot = (slot + 1ull) & mask) {
        uint64_t cur = *(volatile unsigned long long *) (keys + slot);   // (a plain read first: most keys are there already)
        if (cur == kPtEmpty) {
            cur = cas(keys + slot, kPtEmpty, key);
            if (cur == kPtEmpty) cur = key, fresh = true;
        }
        if (cur == key) return slot;
    }
    return kPtNoPlace;
}

// log2 of the table's first size for `ids` ids that can occur: 16 slots an id (a region in three dimensions touches a handful
// of others), 2^kPtMinLog2 at least, 2^first_max_log2 at most - more only after an overflow.  forced > 0 (a test hook of the
// family) is taken as it is, up to max_log2.
O2V_PT_FN uint32_t pt_first_log2(uint64_t ids, int forced, uint32_t first_max_log2, uint32_t max_log2)
{
    if (forced > 0) return (uint32_t) forced < max_log2 ? (uint32_t) forced : max_log2;
    uint32_t log2 = kPtMinLog2;
    while (log2 < first_max_log2 && (1ull << log2) < 16u * ids) ++log2;
    return log2;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_PT_HOST

// the kernels' cas: pt_slot(keys, log2, key, PtCas{}, fresh)
struct PtCas {
    __device__ __forceinline__ uint64_t operator()(unsigned long long *p, uint64_t expected, uint64_t desired) const { return (uint64_t) atomicCAS(p, (unsigned long long) expected, (unsigned long long) desired); }
};

// an int32 grid as K23 and K24 read it: the caller's pointer and element strides
struct I32View {
    const int32_t *p;
    uint64_t s0, s1, s2;
    __device__ __forceinline__ int32_t at(uint32_t x, uint32_t y, uint32_t z) const { return p[(uint64_t) x * s0 + (uint64_t) y * s1 + (uint64_t) z * s2]; }
};

// The occupied slots as a list - keys, and per key its slot's Cols values, 0 from column kept_cols on -, in any order; *n counts them.
template <typename T, uint32_t Cols>
__global__ __launch_bounds__(kBlock) void k_pt_list(const unsigned long long *__restrict__ keys, const T *__restrict__ vals, uint64_t slots, uint32_t kept_cols,
                                                    unsigned long long *__restrict__ list_keys, T *__restrict__ list_vals, unsigned long long *n)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = ((uint64_t) blockIdx.x * kBlock + (threadIdx.x & ~63u)); base < slots; base += (uint64_t) gridDim.x * kBlock) {
        const uint64_t s = base + lane;
        const unsigned long long key = s < slots ? keys[s] : kPtEmpty;
        const unsigned long long taken = __ballot(key != kPtEmpty);
        if (!taken) continue;
        unsigned long long first = 0;
        if (lane == 0u) first = atomicAdd(n, (unsigned long long) __popcll(taken));
        first = __shfl(first, 0);
        if (key != kPtEmpty) {
            const uint64_t at = first + (uint64_t) __popcll(taken & ((1ull << lane) - 1ull));
            list_keys[at] = key;
#pragma unroll
            for (uint32_t c = 0; c < Cols; ++c) list_vals[at * Cols + c] = c < kept_cols ? vals[s * Cols + c] : 0;
        }
    }
}

#endif   // O2V_PT_HOST
