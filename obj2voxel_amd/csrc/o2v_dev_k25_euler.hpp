// o2v_dev_k25_euler.hpp -- K25: the cell counts of a label grid (o2v_hip_euler_stats): per value L of the grid a row of 7 int64 -
// its voxels, the faces, edges and vertices of the unit lattice that touch one of them (closed-in), and the faces, edges and
// vertices whose incident voxels all hold L (inner).  Euler numbers, intrinsic volumes and the exposed faces are sums of these.
// Included from o2v_device.hip inside its anonymous namespace, after K24; it takes the chunk (LsVec, ls_value, ls_diff, ls_lane)
// and the read (ls_read, ls_load1) of K19.
//
//   k_eu_init              every element of the table 0; the counter of the voxels outside [0, n_labels] cleared.
//   k_euler<Format, Vec>   the one pass.  The 2x2x2 window at lattice vertex v = (vx, vy, vz) holds the voxels at v + {-1, 0}^3 and
//                          owns v, the three edges from v towards +x, +y, +z, the three faces they span and the cube at v.  The rows
//                          of the vertex lattice (nx + 1 windows, (ny + 1)(nz + 1) rows) are cut into chunks of K windows along x
//                          (K = 4 int32 or 16 uint8: 16 bytes of a voxel row), numbered row by row; a lane takes a chunk, a
//                          wavefront 64 chunks that follow each other, a workgroup a range of its own.  A lane reads the four voxel
//                          rows (vy - 1, vy) x (vz - 1, vz) at x0 ... x0 + K - 1 (16-byte loads where the layout allows) and the one
//                          element before them - the last element of the lane before it, a load of its own in lane 0 only.  Rows and
//                          elements outside the box are not read.  A chunk that lies inside one label (eu_uniform: word compares)
//                          is a run of K windows, K x (1, 3, 3, 1, 3, 3, 1); a chain of runs of one label in lanes that follow each
//                          other (eu_joins, eu_chain: two ballots) is added once, by its first lane.  Any other chunk takes its distinct labels one after the other (eu_next): per label eight
//                          masks, bit w of E[b] says that position b of window w holds the label (eu_label_masks: one ls_diff
//                          per row), and the seven columns are popcounts of ORs (closed-in) and ANDs (inner) of these masks under
//                          the cells' incidence masks (eu_columns) - the chunk's windows at once, no walk.  Where a row goes: a
//                          table per workgroup in LDS, open-addressed by label (eu_find_slot: kEuSlots slots, kEuProbes probes, a
//                          slot is claimed by a compare-and-swap of its key), with 64-bit LDS adds; a row that finds no slot goes
//                          to the table in global memory with 64-bit atomic adds, and so does every row with table = 0
//                          (O2V_EU_NO_TABLE=1).  At its end the workgroup adds its occupied slots to global memory.
// Every column is an integer sum, so the table does not depend on any order.  No private segment; no workgroup waits for another.

constexpr uint32_t kEuCols = 7;                                                  // O2V_HIP_EULER_COLUMNS
constexpr uint32_t kEuVoxels = 0, kEuFaces = 1, kEuEdges = 2, kEuVertices = 3, kEuInnerFaces = 4, kEuInnerEdges = 5, kEuInnerVertices = 6;
#ifndef O2V_EU_SLOT_BITS
#define O2V_EU_SLOT_BITS 8
#endif
constexpr uint32_t kEuSlotBits = O2V_EU_SLOT_BITS, kEuSlots = 1u << kEuSlotBits;   // slots of a workgroup's table: 15 KiB of LDS
constexpr uint32_t kEuProbes = 8;                                                // slots a row looks at before it goes to global memory
constexpr uint32_t kEuNoSlot = ~0u;
constexpr uint32_t kEuRows = 4;                                                  // voxel rows of a chunk: r = j + 2 k is (vy - 1 + j, vz - 1 + k)
// Position b = i + 2 j + 4 k of a window is the voxel at (vx - 1 + i, vy - 1 + j, vz - 1 + k).  The positions incident to the cells
// that the window owns: the vertex, the edges towards +x, +y, +z, the faces xy, xz, yz, the cube.
constexpr uint32_t kEuVertexMask = 0xffu, kEuEdgeMask[3] = {0xaau, 0xccu, 0xf0u}, kEuFaceMask[3] = {0x88u, 0xa0u, 0xc0u}, kEuCubeMask = 0x80u;

#ifndef O2V_EU_HOST
#define O2V_EU_FN __host__ __device__ __forceinline__
#ifdef O2V_EU_MUTATE_WRAP_ROW_END
#error "O2V_EU_MUTATE_WRAP_ROW_END is for the host test only: the kernel would read behind the grid's last row"
#endif
#endif

// ---- windows: a chunk's rows, a label's masks, the columns, the run, the slot probe ---------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_topology.py compiles this part for the host behind K19's, with O2V_EU_FN
// of its own, and runs it chunk by chunk and wavefront by wavefront against the reference.)

// The windows x0 ... x0 + nw - 1 of a lattice row and what they see.  row[r]: the elements x0 ... x0 + n - 1 of voxel row r, zero
// behind them; before[r]: its element x0 - 1, read where has_before; have: bit r, row r lies in the box.
struct EuChunk {
    LsVec row[kEuRows];
    int32_t before[kEuRows];
    uint32_t have, n, nw;
    bool has_before;
};

// The windows of the chunk at x0 (a row has nx + 1), and the voxels at x0 ... that lie in the box: the window at vx = nx has none.
O2V_EU_FN uint32_t eu_windows(uint32_t x0, uint32_t nx, uint32_t K) { return nx + 1u - x0 < K ? nx + 1u - x0 : K; }
O2V_EU_FN uint32_t eu_voxels(uint32_t x0, uint32_t nx, uint32_t K)
{
#ifdef O2V_EU_MUTATE_WRAP_ROW_END
    return eu_windows(x0, nx, K);   // (test only: the window at vx = nx takes the element behind the row, the next row's first)
#else
    return nx - x0 < K ? nx - x0 : K;
#endif
}
// Bit r: voxel row r = j + 2 k of the lattice row (vy, vz), (vy - 1 + j, vz - 1 + k), lies in the box.
O2V_EU_FN uint32_t eu_rows_in_box(uint32_t vy, uint32_t vz, uint32_t ny, uint32_t nz)
{
    const uint32_t lo_y = vy > 0u, hi_y = vy < ny, lo_z = vz > 0u, hi_z = vz < nz;
    return (lo_y & lo_z) | (hi_y & lo_z) << 1 | (lo_y & hi_z) << 2 | (hi_y & hi_z) << 3;
}

// 16 bytes that hold `label` in every element.
template <uint32_t Format>
O2V_EU_FN LsVec eu_splat(int32_t label)
{
    const uint32_t w = Format == kLsI32 ? (uint32_t) label : ((uint32_t) label & 0xffu) * 0x01010101u;
    return LsVec{{w, w, w, w}};
}

// The last element of a full chunk: the element before the next one.
template <uint32_t Format>
O2V_EU_FN int32_t eu_last(const LsVec &v) { return Format == kLsI32 ? (int32_t) v.w[3] : (int32_t) (v.w[3] >> 24); }

// Bit w of E[b]: position b of window w lies in the box and holds `label`.
template <uint32_t Format>
O2V_EU_FN void eu_label_masks(const EuChunk &c, int32_t label, uint32_t E[8])
{
    const LsVec lv = eu_splat<Format>(label);
    const uint32_t valid = (1u << c.n) - 1u, windows = (1u << c.nw) - 1u;
#pragma unroll
    for (uint32_t r = 0; r < kEuRows; ++r) {
        const bool on = (c.have >> r) & 1u;
        const uint32_t cur = on ? ~ls_diff<Format>(c.row[r], lv) & valid : 0u;
        const uint32_t first = on && c.has_before && c.before[r] == label ? 1u : 0u;
        E[2u * r] = (cur << 1 | first) & windows;
        E[2u * r + 1u] = cur & windows;
    }
}

// The configuration of a label in window w: bit b, position b holds it.
O2V_EU_FN uint32_t eu_config(const uint32_t E[8], uint32_t w)
{
    uint32_t c = 0;
#pragma unroll
    for (uint32_t b = 0; b < 8u; ++b) c |= ((E[b] >> w) & 1u) << b;
    return c;
}

// What a configuration adds to the seven columns, four bits a column (3 at most): a cell is closed-in if one of its incident
// positions holds the label, inner if all do.
O2V_EU_FN uint32_t eu_increments(uint32_t config)
{
    uint32_t closed_faces = 0, closed_edges = 0, inner_faces = 0, inner_edges = 0;
#pragma unroll
    for (uint32_t a = 0; a < 3u; ++a) {
        closed_faces += (config & kEuFaceMask[a]) != 0u, inner_faces += (config & kEuFaceMask[a]) == kEuFaceMask[a];
        closed_edges += (config & kEuEdgeMask[a]) != 0u, inner_edges += (config & kEuEdgeMask[a]) == kEuEdgeMask[a];
    }
    return (uint32_t) ((config & kEuCubeMask) != 0u) << (4u * kEuVoxels) | closed_faces << (4u * kEuFaces) | closed_edges << (4u * kEuEdges) |
           (uint32_t) ((config & kEuVertexMask) != 0u) << (4u * kEuVertices) | inner_faces << (4u * kEuInnerFaces) | inner_edges << (4u * kEuInnerEdges) |
           (uint32_t) (config == kEuVertexMask) << (4u * kEuInnerVertices);
}

// The same for all windows of a chunk at once: the sums over w of eu_increments(eu_config(E, w)) as popcounts.
O2V_EU_FN void eu_columns(const uint32_t E[8], uint32_t col[kEuCols])
{
    const auto pc = [](uint32_t m) { return (uint32_t) __builtin_popcount(m); };
    col[kEuVoxels] = pc(E[7]);
    col[kEuFaces] = pc(E[3] | E[7]) + pc(E[5] | E[7]) + pc(E[6] | E[7]);
    col[kEuEdges] = pc(E[1] | E[3] | E[5] | E[7]) + pc(E[2] | E[3] | E[6] | E[7]) + pc(E[4] | E[5] | E[6] | E[7]);
    col[kEuVertices] = pc(E[0] | E[1] | E[2] | E[3] | E[4] | E[5] | E[6] | E[7]);
    col[kEuInnerFaces] = pc(E[3] & E[7]) + pc(E[5] & E[7]) + pc(E[6] & E[7]);
    col[kEuInnerEdges] = pc(E[1] & E[3] & E[5] & E[7]) + pc(E[2] & E[3] & E[6] & E[7]) + pc(E[4] & E[5] & E[6] & E[7]);
    col[kEuInnerVertices] = pc(E[0] & E[1] & E[2] & E[3] & E[4] & E[5] & E[6] & E[7]);
}

// What a run of len windows of one label adds: len x (1, 3, 3, 1, 3, 3, 1).
O2V_EU_FN void eu_run_columns(uint32_t len, uint32_t col[kEuCols])
{
    col[kEuVoxels] = col[kEuVertices] = col[kEuInnerVertices] = len;
    col[kEuFaces] = col[kEuEdges] = col[kEuInnerFaces] = col[kEuInnerEdges] = 3u * len;
}

// The chunk lies inside one label: a full chunk of four rows in the box, every element and the ones before them one value.
template <uint32_t Format>
O2V_EU_FN bool eu_uniform(const EuChunk &c, int32_t &label)
{
    label = c.before[0];
    if (c.have != 15u || !c.has_before || c.n != ls_lane<Format>()) return false;
    const uint32_t w = eu_splat<Format>(label).w[0];
    uint32_t differs = 0;
#pragma unroll
    for (uint32_t r = 0; r < kEuRows; ++r)
        differs |= (uint32_t) (c.before[r] != label) | (c.row[r].w[0] ^ w) | (c.row[r].w[1] ^ w) | (c.row[r].w[2] ^ w) | (c.row[r].w[3] ^ w);
    return differs == 0u;
}

// The joining rule: a run goes on the run of the lane before it if the two have one label (whatever rows they lie in: a run adds
// sums only).  A chain of such runs is added once, by the lane it begins in.
O2V_EU_FN bool eu_joins(bool prev_run, int32_t prev_label, int32_t label) { return prev_run && prev_label == label; }

// The runs of the chain that begins in `lane`.  runs, heads: bit l, lane l of the wavefront holds a run / a run that joins none.
O2V_EU_FN uint32_t eu_chain(uint64_t runs, uint64_t heads, uint32_t lane)
{
    const uint64_t on = lane < 63u ? (runs & ~heads) >> (lane + 1u) : 0ull;   // the lanes behind it that go on a chain: ones up to its end
    return 1u + (uint32_t) __builtin_ctzll(~on);                              // (the top lane + 1 bits of `on` are 0)
}

// What a chunk has still to take: todo[r], the elements of row r; before, bit r: the element before row r.
template <uint32_t Format>
O2V_EU_FN void eu_todo_init(const EuChunk &c, uint32_t todo[kEuRows], uint32_t &before)
{
#pragma unroll
    for (uint32_t r = 0; r < kEuRows; ++r) todo[r] = (c.have >> r) & 1u ? (1u << c.n) - 1u : 0u;
    before = c.has_before ? c.have : 0u;
}

// The next label of a chunk: the value of the first element that no label before it has taken, which is taken off; false: none left.
template <uint32_t Format>
O2V_EU_FN bool eu_next(const EuChunk &c, uint32_t todo[kEuRows], uint32_t &before, int32_t &label)
{
    bool found = false;
#pragma unroll
    for (uint32_t r = 0; r < kEuRows; ++r)
        if (!found && todo[r]) {
            const uint32_t j = (uint32_t) __builtin_ctz(todo[r]);
            label = ls_value<Format>(c.row[r], j), todo[r] &= todo[r] - 1u, found = true;
        }
#pragma unroll
    for (uint32_t r = 0; r < kEuRows; ++r)
        if (!found && ((before >> r) & 1u)) label = c.before[r], before &= ~(1u << r), found = true;
    return found;
}

// The elements that `label` has taken (E: its masks) are off the list.
O2V_EU_FN void eu_taken(const uint32_t E[8], uint32_t todo[kEuRows], uint32_t &before)
{
#pragma unroll
    for (uint32_t r = 0; r < kEuRows; ++r) todo[r] &= ~E[2u * r + 1u], before &= ~((E[2u * r] & 1u) << r);
}

// A value that has a row: 0 <= v <= n_labels (n_labels below 2^31 - 1).
O2V_EU_FN bool eu_counted(int32_t v, uint32_t n_labels) { return v >= 0 && (uint32_t) v <= n_labels; }

O2V_EU_FN uint32_t eu_hash(int32_t label) { return ((uint32_t) label * 0x9e3779b1u) >> (32u - kEuSlotBits); }

// The slot of `label` in a table of kEuSlots keys (kLsEmptyKey: free), claimed if it has none yet: linear probing from the
// label's hash, kEuNoSlot if none of kEuProbes slots is the label's or free.  cas(p, expected, desired) returns what *p held.
template <typename Cas>
O2V_EU_FN uint32_t eu_find_slot(int32_t *keys, int32_t label, Cas &&cas)
{
    uint32_t h = eu_hash(label);
    for (uint32_t i = 0; i < kEuProbes && i < kEuSlots; ++i, h = (h + 1u) & (kEuSlots - 1u)) {
        int32_t seen = *(volatile int32_t *) (keys + h);
        if (seen == kLsEmptyKey) seen = cas(keys + h, kLsEmptyKey, label);
        if (seen == kLsEmptyKey || seen == label) return h;
    }
    return kEuNoSlot;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_EU_HOST

struct EuGrid {
    uint32_t n[3];
    uint32_t n_labels;
    uint32_t cpr;              // chunks per lattice row: ceil((nx + 1) / K)
    uint32_t rows_y;           // ny + 1: lattice rows per lattice plane
    uint32_t chunks;           // cpr * (ny + 1) * (nz + 1): below 2^32 (o2v_dev_host_k25_euler.hpp)
    uint32_t groups, per_wg;   // groups of kBlock chunks; groups per workgroup
    uint32_t table;            // 1: the table in LDS; 0: every row to global memory
};

__global__ __launch_bounds__(kBlock) void k_eu_init(long long *__restrict__ table, uint64_t rows, unsigned long long *__restrict__ outside)
{
    const uint64_t n = rows * kEuCols, step = (uint64_t) gridDim.x * kBlock;
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += step) table[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) *outside = 0;
}

// The columns of a label added to `row`, its seven int64 in LDS or in global memory (the address space is the caller's).
__device__ __forceinline__ void eu_add_row(long long *row, const uint32_t col[kEuCols])
{
#pragma unroll
    for (uint32_t c = 0; c < kEuCols; ++c)
        if (col[c]) atomicAdd(reinterpret_cast<unsigned long long *>(row + c), (unsigned long long) col[c]);
}

template <uint32_t Format, bool Vec>
__global__ __launch_bounds__(kBlock) void k_euler(RaySource src, EuGrid g, long long *__restrict__ table, unsigned long long *__restrict__ outside)
{
    constexpr uint32_t K = ls_lane<Format>();
    __shared__ int32_t s_key[kEuSlots];
    __shared__ long long s_tab[kEuSlots * kEuCols];
    if (g.table) {
        for (uint32_t i = threadIdx.x; i < kEuSlots; i += kBlock) s_key[i] = kLsEmptyKey;
        for (uint32_t i = threadIdx.x; i < kEuSlots * kEuCols; i += kBlock) s_tab[i] = 0;
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g0 = blockIdx.x * g.per_wg, g1 = min(g.groups, g0 + g.per_wg);   // (g0 <= groups < 2^24)
    unsigned long long n_outside = 0;
    const auto add = [&](int32_t label, const uint32_t col[kEuCols]) {
        const uint32_t slot = g.table ? eu_find_slot(s_key, label, [](int32_t *p, int32_t expected, int32_t desired) { return atomicCAS(p, expected, desired); })
                                      : kEuNoSlot;
        if (slot != kEuNoSlot)
            eu_add_row(s_tab + slot * kEuCols, col);
        else
            eu_add_row(table + (uint64_t) (uint32_t) label * kEuCols, col);
    };
    for (uint32_t gi = g0; gi < g1; ++gi) {
        const uint64_t c64 = (uint64_t) gi * kBlock + threadIdx.x;
        const bool active = c64 < g.chunks;
        EuChunk c;
        c.have = c.n = c.nw = 0u, c.has_before = false;
#pragma unroll
        for (uint32_t r = 0; r < kEuRows; ++r) c.row[r] = LsVec{{0u, 0u, 0u, 0u}}, c.before[r] = 0;
        uint32_t x0 = 0, vy = 0, vz = 0;
        if (active) {
            const uint32_t ci = (uint32_t) c64, lrow = ci / g.cpr;
            x0 = (ci - lrow * g.cpr) * K;
            vz = lrow / g.rows_y, vy = lrow - vz * g.rows_y;
            c.n = eu_voxels(x0, g.n[0], K), c.nw = eu_windows(x0, g.n[0], K);
            c.has_before = x0 > 0u;
            c.have = eu_rows_in_box(vy, vz, g.n[1], g.n[2]);
            if (c.n) {
#pragma unroll
                for (uint32_t r = 0; r < kEuRows; ++r)
                    if ((c.have >> r) & 1u) c.row[r] = ls_read<Format, Vec>(src, (uint64_t) (vy - 1u + (r & 1u)) * src.s1 + (uint64_t) (vz - 1u + (r >> 1)) * src.s2, x0, c.n);
            }
        }
        // the element before a chunk is the last of the chunk before it, which the lane before holds: it lies in the same lattice
        // row (x0 > 0) and is full; lane 0 reads it
#pragma unroll
        for (uint32_t r = 0; r < kEuRows; ++r) {
            const int32_t prev = __shfl_up(eu_last<Format>(c.row[r]), 1);
            if (c.has_before && ((c.have >> r) & 1u))
                c.before[r] = lane > 0u ? prev : ls_load1<Format>(src, (uint64_t) (vy - 1u + (r & 1u)) * src.s1 + (uint64_t) (vz - 1u + (r >> 1)) * src.s2, x0 - 1u);
        }
        // the runs: chunks inside one label; a chain of them over lanes that follow each other is added once, by its first lane
        int32_t run_label = 0;
        const bool run = active && eu_uniform<Format>(c, run_label);
        const int32_t prev_label = __shfl_up(run_label, 1);
        const bool prev_run = __shfl_up((int) run, 1) != 0;
        const bool head = run && !(lane > 0u && eu_joins(prev_run, prev_label, run_label));
        const unsigned long long runs = __ballot(run), heads = __ballot(head);
        if (run) {
            if (head) {
                const uint32_t len = eu_chain(runs, heads, lane) * K;
                if (eu_counted(run_label, g.n_labels)) {
                    uint32_t col[kEuCols];
                    eu_run_columns(len, col);
                    add(run_label, col);
                } else {
                    n_outside += len;
                }
            }
        } else if (active) {
            uint32_t todo[kEuRows], before;
            eu_todo_init<Format>(c, todo, before);
            int32_t label = 0;
            while (eu_next<Format>(c, todo, before, label)) {
                uint32_t E[8];
                eu_label_masks<Format>(c, label, E);
                eu_taken(E, todo, before);
                if (!eu_counted(label, g.n_labels)) {
                    n_outside += (uint32_t) __builtin_popcount(E[7]);
                    continue;
                }
                uint32_t col[kEuCols];
                eu_columns(E, col);
                add(label, col);
            }
        }
    }
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) n_outside += __shfl_xor(n_outside, (int) d);
    if (lane == 0u && n_outside) atomicAdd(outside, n_outside);
    if (g.table) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < kEuSlots * kEuCols; i += kBlock) {
            const uint32_t slot = i / kEuCols, c = i - slot * kEuCols;
            const int32_t label = s_key[slot];
            const long long val = s_tab[i];
            if (label == kLsEmptyKey || val == 0) continue;
            atomicAdd(reinterpret_cast<unsigned long long *>(table + (uint64_t) (uint32_t) label * kEuCols + c), (unsigned long long) val);
        }
    }
}

#endif   // O2V_EU_HOST
