// o2v_dev_k26_octree.hpp -- K26: the sparse voxel octree of a dense grid (o2v_hip_octree_build / _write / _lookup / _to_dense).
// Included from o2v_device.hip inside its anonymous namespace, behind K17 (after K12, whose classify kernel it uses, K6, whose
// block scan it uses, and o2v_dev_bits.hpp, the bit grid it reads).
//
// The definition is in include/o2v_hip.h: the root cube [0, 2^D)^3 on the global lattice, a cell of level l an aligned cube of
// side 2^(D - l), per stored cell of level l < D the masks `valid` (children that hold a solid voxel) and `full` (children that
// are solid throughout), nodes level by level in (parent, octant) order.
//
//   k_cc_classify (K12)   the only pass over the grid: the set as the bit grid of the box.
//   k_oct_leaves          a lane per cell of level D - 1 that the box touches: the 2^3 block's bits from the four rows it meets,
//                         aligned to the global lattice (an odd origin makes a block straddle bit pairs and, at x = 63 | 64,
//                         words) -> pyr[D - 1][cell] = valid | full << 8 (full = valid there).
//   k_oct_up              a lane per cell of level l < D - 1: its eight children's entries of level l + 1 -> its own.  Both count
//                         the cells of their level that are nodes - non-empty and, in a collapsed tree, not full - (a sum: the
//                         atomics decide no order), which the host reads to size the node arrays and the launches.
//   k_oct_root            node 0 from the one cell of level 0.
//   per level, top down, over the stored nodes only (their number stays on the device; the launch is sized by the bound):
//   k_oct_count + k_fill_scan_blocks (K6)   popcount of `stored` (of `valid` at level D - 1) per node, exclusive scan over the block of
//                         256 nodes, the scan of the block sums -> the number of nodes of the next level (of listed voxels).
//   k_oct_children        first_child = the next level's offset + the node's prefix (-1 without stored children; at level D - 1 the
//                         prefix alone: the voxel index), and each stored child's corner and entry, read from the pyramid, at
//                         first_child + rank.
//   k_oct_lookup          a lane per point: the descent.  k_oct_dense: a lane per aligned 2^3 block of the box: one descent to
//                         level D - 1, whose `valid` answers eight voxels.
// The per-level arrays of the pyramid are box-sized: 2 bytes per touched cell, 1/4 byte per voxel at level D - 1 and 2/7 in all.
// No float, no private segment, no LDS beyond the block scan's four words; the same bits on every run.

constexpr uint32_t kOctMaxDepth = 16u;
constexpr uint32_t kOctEmpty = 0u, kOctFull = 1u, kOctDown = 2u, kOctCorrupt = 3u;   // what a step of the descent finds

#ifndef O2V_OCT_HOST
#define O2V_OCT_FN __device__ __forceinline__
#define O2V_OCT_HD __host__ __device__ __forceinline__   // (what the host side plans the levels with)
O2V_OCT_FN uint32_t oct_popc(uint32_t v) { return (uint32_t) __popc(v); }
#endif

// ---- cells, bit pairs, the descent ------------------------------------------------------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_octree.py compiles this part for the host behind the plain part of
// o2v_dev_bits.hpp, with O2V_OCT_FN, O2V_OCT_HD and oct_popc of its own, and runs it against the reference.)

// The cells of one level that the box origin + [0, dims) touches, s = D - l the binary logarithm of their side: cell c0 + i along
// an axis for i below n; `first`: where the level's entries begin in the pyramid.  origin + dims is at most 2^16.
struct OctLevel {
    uint32_t c0[3], n[3];
    uint64_t cells, first;
};

O2V_OCT_HD uint32_t oct_cell_lo(uint32_t origin, uint32_t s) { return origin >> s; }
O2V_OCT_HD uint32_t oct_cell_n(uint32_t origin, uint32_t dim, uint32_t s) { return ((origin + dim - 1u) >> s) - (origin >> s) + 1u; }

// cell index -> (i, j, k) within the level (x fastest); the cells of a level are no more than the voxels, below 2^31
O2V_OCT_FN void oct_cell_at(const OctLevel &L, uint32_t c, uint32_t &i, uint32_t &j, uint32_t &k)
{
    const uint32_t row = c / L.n[0];
    i = c - row * L.n[0];
    k = row / L.n[1];
    j = row - k * L.n[1];
}

// Bits x0 and x0 + 1 of row (y, z) of the box, x0 in [-1, nx - 1] (box coordinates; a position outside the row is empty): bit 0
// and bit 1 of the result.  The padding bits of a row's last word are 0, so one word answers both unless x0 is bit 63 of its word.
O2V_OCT_FN uint32_t oct_row_pair(const BitGrid &g, const unsigned long long *bits, int32_t x0, uint32_t y, uint32_t z)
{
    const uint64_t row = bits_word_index(g, 0u, y, z);
    if (x0 < 0) return x0 == -1 ? (uint32_t) (bits[row] & 1ull) << 1 : 0u;
    if ((uint32_t) x0 >= g.nx) return 0u;
    const uint32_t wx = (uint32_t) x0 >> 6, b = (uint32_t) x0 & 63u;
    uint32_t pair = (uint32_t) (bits[row + wx] >> b) & 3u;
    if (b == 63u && wx + 1u < g.W) pair |= (uint32_t) (bits[row + wx + 1u] & 1ull) << 1;
    return pair;
}

// The mask of the aligned 2^3 block (gx, gy, gz) of the global lattice (voxels 2 g + d): bit dx + 2 dy + 4 dz
O2V_OCT_FN uint32_t oct_block_mask(const BitGrid &g, const unsigned long long *bits, uint32_t ox, uint32_t oy, uint32_t oz, uint32_t gx, uint32_t gy,
                                   uint32_t gz)
{
    const int32_t x0 = (int32_t) (2u * gx) - (int32_t) ox;
    uint32_t mask = 0;
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t y = 2u * gy + (r & 1u) - oy, z = 2u * gz + (r >> 1) - oz;   // (below the origin: wraps past any ny, nz)
        if (y < g.ny && z < g.nz) mask |= oct_row_pair(g, bits, x0, y, z) << (2u * r);
    }
    return mask;
}

// the entry valid | full << 8 of a cell from its eight children's entries (0 for a child outside the box)
O2V_OCT_FN uint32_t oct_merge(const uint32_t child[8])
{
    uint32_t valid = 0, full = 0;
    for (uint32_t o = 0; o < 8u; ++o) {
        valid |= (uint32_t) ((child[o] & 0xffu) != 0u) << o;
        full |= (uint32_t) ((child[o] >> 8) == 0xffu) << o;
    }
    return valid | full << 8;
}

// A tree as the queries take it: the caller's arrays of n_nodes entries.
struct OctTree {
    const uint8_t *valid, *full;
    const int32_t *first_child;
    uint32_t n_nodes, depth, collapsed;
};

// the octant of (x, y, z) in a cell whose children have side 2^s
O2V_OCT_FN uint32_t oct_octant(uint32_t x, uint32_t y, uint32_t z, uint32_t s)
{
#ifdef O2V_OCT_MUTATE_SWAP_YZ
    return ((x >> s) & 1u) | ((z >> s) & 1u) << 1 | ((y >> s) & 1u) << 2;   // (test only: the octant bits of y and z exchanged)
#else
    return ((x >> s) & 1u) | ((y >> s) & 1u) << 1 | ((z >> s) & 1u) << 2;
#endif
}

O2V_OCT_FN uint32_t oct_rank(uint32_t mask, uint32_t o) { return oct_popc(mask & ((1u << o) - 1u)); }
O2V_OCT_FN uint32_t oct_stored(uint32_t valid, uint32_t full, uint32_t collapsed) { return collapsed ? valid & ~full & 0xffu : valid; }

// One step at node i of a level below D - 1 towards octant o.  kOctDown: i is the child.  Nothing is read outside [0, n_nodes).
O2V_OCT_FN uint32_t oct_step(const OctTree &t, uint32_t &i, uint32_t o)
{
    const uint32_t v = t.valid[i], f = t.full[i];
    if (!((v >> o) & 1u)) return kOctEmpty;
    if (t.collapsed && ((f >> o) & 1u)) return kOctFull;
    const int32_t fc = t.first_child[i];
    if (fc < 0) return kOctCorrupt;
    const uint64_t c = (uint64_t) (uint32_t) fc + oct_rank(oct_stored(v, f, t.collapsed), o);
    if (c >= t.n_nodes) return kOctCorrupt;
    i = (uint32_t) c;
    return kOctDown;
}

// The descent to (x, y, z): out = (solid, level, node, voxel_index) as include/o2v_hip.h defines them; at most D steps.
O2V_OCT_FN void oct_descend(const OctTree &t, int32_t x, int32_t y, int32_t z, int32_t out[4])
{
    const int32_t side = (int32_t) (1u << t.depth);
    out[0] = 0, out[1] = out[2] = out[3] = -1;
    if (x < 0 || y < 0 || z < 0 || x >= side || y >= side || z >= side) return;
    uint32_t i = 0;
    for (uint32_t l = 0; l + 1u < t.depth; ++l) {
        const uint32_t code = oct_step(t, i, oct_octant((uint32_t) x, (uint32_t) y, (uint32_t) z, t.depth - 1u - l));
        if (code == kOctDown) continue;
        if (code == kOctCorrupt) {
            out[1] = -2;
            return;
        }
        out[0] = code == kOctFull ? 1 : 0, out[1] = (int32_t) l, out[2] = (int32_t) i;
        return;
    }
    const uint32_t o = oct_octant((uint32_t) x, (uint32_t) y, (uint32_t) z, 0u), v = t.valid[i];
    out[1] = (int32_t) t.depth - 1, out[2] = (int32_t) i;
    if (!((v >> o) & 1u)) return;
    out[0] = 1;
    out[3] = (int32_t) ((uint32_t) t.first_child[i] + oct_rank(v, o));
}

// The eight voxels of the aligned 2^3 block at (x, y, z) (even, inside the root cube) as a mask, bit dx + 2 dy + 4 dz: one
// descent to level D - 1.  A corrupt tree gives 0.
O2V_OCT_FN uint32_t oct_block(const OctTree &t, uint32_t x, uint32_t y, uint32_t z)
{
    uint32_t i = 0;
    for (uint32_t l = 0; l + 1u < t.depth; ++l) {
        const uint32_t code = oct_step(t, i, oct_octant(x, y, z, t.depth - 1u - l));
        if (code == kOctDown) continue;
        return code == kOctFull ? 0xffu : 0u;
    }
    return t.valid[i];
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------
#ifndef O2V_OCT_HOST

// The counters of a build, 64-bit words on the device and, twice, on the host: the cells that are nodes per level (from the pyramid), the stored nodes per
// level (from the scans), their first node per level, the listed voxels.
constexpr uint32_t kOctBound = 0u, kOctCount = 17u, kOctFirst = 34u, kOctVoxels = 51u, kOctMeta = 64u;

// The node arrays of a build in the context's scratch, `cap` entries each.
struct OctNodes {
    uint8_t *valid, *full;
    int32_t *first_child, *coords;   // coords: [cap][3]
    uint64_t cap;
};

// The lanes of this wavefront whose cell (entry: valid | full << 8; 0 for a lane without a cell) is a stored node below the root:
// non-empty and, in a collapsed tree, not full - its ancestors are then non-empty and not full too, so the sum over a level is
// its node count.  The same in every lane.
__device__ __forceinline__ uint32_t oct_wave_stored(uint32_t entry, uint32_t collapsed)
{
    return (uint32_t) __popcll(__ballot((entry & 0xffu) != 0u && !(collapsed && (entry >> 8) == 0xffu)));
}

// *bound += a wavefront's count of all its turns: one atomic per wavefront of the launch, not per turn - two million adds to one
// address made the pyramid at 1024^3 take 20 ms, not 1
__device__ __forceinline__ void oct_add_wave_count(uint32_t count, unsigned long long *bound)
{
    if ((threadIdx.x & 63u) == 0u && count) atomicAdd(bound, (unsigned long long) count);
}

// pyr[cell] of level D - 1 from the bit grid; *bound += the cells that are nodes
__global__ __launch_bounds__(kBlock) void k_oct_leaves(const unsigned long long *__restrict__ bits, BitGrid g, uint32_t ox, uint32_t oy, uint32_t oz,
                                                       OctLevel L, uint32_t collapsed, uint16_t *__restrict__ pyr, unsigned long long *__restrict__ bound)
{
    uint32_t stored = 0;
    for (uint64_t base = (uint64_t) blockIdx.x * kBlock; base < L.cells; base += (uint64_t) gridDim.x * kBlock) {   // (uniform over the workgroup)
        const uint64_t c = base + threadIdx.x;
        uint32_t mask = 0;
        if (c < L.cells) {
            uint32_t i, j, k;
            oct_cell_at(L, (uint32_t) c, i, j, k);
            mask = oct_block_mask(g, bits, ox, oy, oz, L.c0[0] + i, L.c0[1] + j, L.c0[2] + k);
            pyr[L.first + c] = (uint16_t) (mask | mask << 8);
        }
        stored += oct_wave_stored(mask | mask << 8, collapsed);
    }
    oct_add_wave_count(stored, bound);
}

// pyr[cell] of level l from the entries of level l + 1 (Lc); *bound += the cells that are nodes
__global__ __launch_bounds__(kBlock) void k_oct_up(uint16_t *__restrict__ pyr, OctLevel Lc, OctLevel L, uint32_t collapsed,
                                                   unsigned long long *__restrict__ bound)
{
    uint32_t stored = 0;
    for (uint64_t base = (uint64_t) blockIdx.x * kBlock; base < L.cells; base += (uint64_t) gridDim.x * kBlock) {
        const uint64_t c = base + threadIdx.x;
        uint32_t entry = 0;
        if (c < L.cells) {
            uint32_t i, j, k, child[8];
            oct_cell_at(L, (uint32_t) c, i, j, k);
#pragma unroll
            for (uint32_t o = 0; o < 8u; ++o) {
                // (a child below the child level's first cell wraps past any n)
                const uint32_t ci = 2u * (L.c0[0] + i) + (o & 1u) - Lc.c0[0], cj = 2u * (L.c0[1] + j) + ((o >> 1) & 1u) - Lc.c0[1],
                               ck = 2u * (L.c0[2] + k) + (o >> 2) - Lc.c0[2];
                const bool in = ci < Lc.n[0] && cj < Lc.n[1] && ck < Lc.n[2];
                child[o] = in ? pyr[Lc.first + ((uint64_t) ck * Lc.n[1] + cj) * Lc.n[0] + ci] : 0u;
            }
            entry = oct_merge(child);
            pyr[L.first + c] = (uint16_t) entry;
        }
        stored += oct_wave_stored(entry, collapsed);
    }
    oct_add_wave_count(stored, bound);
}

// node 0: the one cell of level 0
__global__ void k_oct_root(const uint16_t *__restrict__ pyr, uint64_t first, OctNodes nd, unsigned long long *__restrict__ meta)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint32_t e = pyr[first];
    nd.valid[0] = (uint8_t) (e & 0xffu), nd.full[0] = (uint8_t) (e >> 8);
    nd.coords[0] = nd.coords[1] = nd.coords[2] = 0;
    meta[kOctCount] = 1u, meta[kOctFirst] = 0u;
}

// the stored children of a node of level l (of depth D): at level D - 1 its voxels
__device__ __forceinline__ uint32_t oct_node_children(const OctNodes &nd, uint64_t node, bool leaf, uint32_t collapsed)
{
    const uint32_t v = nd.valid[node];
    return leaf ? v : oct_stored(v, nd.full[node], collapsed);
}

// first_child[node] = the children of the nodes of its block of 256 before it; block_sums[b] = the block's children, for every block
// of the launch's bound (past the level's nodes: 0)
__global__ __launch_bounds__(kBlock) void k_oct_count(OctNodes nd, const unsigned long long *__restrict__ meta, uint32_t l, uint32_t leaf, uint32_t collapsed,
                                                      uint64_t n_blocks, unsigned long long *__restrict__ block_sums)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    const uint64_t n = meta[kOctCount + l], first = meta[kOctFirst + l];
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint64_t i = b * kBlock + threadIdx.x;
        const bool in = i < n && first + i < nd.cap;
        const uint64_t cnt = in ? (uint64_t) __popc(oct_node_children(nd, first + i, leaf != 0u, collapsed)) : 0u;
        uint64_t total;
        const uint64_t ex = fill_block_exscan64(cnt, s_wave, total);
        if (in) nd.first_child[first + i] = (int32_t) ex;
        if (threadIdx.x == 0) block_sums[b] = total;
    }
}

// first_child of the nodes of level l and, below level D - 1, their stored children's corners and entries (Lc: level l + 1, cells of
// side 2^sc); meta: the next level's first node
__global__ __launch_bounds__(kBlock) void k_oct_children(OctNodes nd, unsigned long long *__restrict__ meta, uint32_t l, uint32_t leaf, uint32_t collapsed,
                                                         uint64_t n_blocks, const unsigned long long *__restrict__ boff, const uint16_t *__restrict__ pyr,
                                                         OctLevel Lc, uint32_t sc)
{
    const uint64_t n = meta[kOctCount + l], first = meta[kOctFirst + l], next = first + n;
    if (blockIdx.x == 0 && threadIdx.x == 0) meta[kOctFirst + l + 1u] = next;   // (entry 17 of the firsts: the nodes in all)
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint64_t i = b * kBlock + threadIdx.x, node = first + i;
        if (i >= n || node >= nd.cap) continue;
        const uint64_t before = boff[b] + (uint64_t) (uint32_t) nd.first_child[node];
        if (leaf) {
            nd.first_child[node] = (int32_t) before;
            continue;
        }
        const uint32_t stored = oct_node_children(nd, node, false, collapsed);
        nd.first_child[node] = stored ? (int32_t) (next + before) : -1;
        const int32_t x = nd.coords[3u * node], y = nd.coords[3u * node + 1u], z = nd.coords[3u * node + 2u];
        uint32_t rank = 0;
        for (uint32_t o = 0; o < 8u; ++o) {
            if (!((stored >> o) & 1u)) continue;
            const uint64_t child = next + before + rank++;
            if (child >= nd.cap) continue;   // (never: the capacity is the sum of the levels' bounds)
            const uint32_t cx = (uint32_t) x + ((o & 1u) << sc), cy = (uint32_t) y + (((o >> 1) & 1u) << sc), cz = (uint32_t) z + ((o >> 2) << sc);
            const uint32_t ci = (cx >> sc) - Lc.c0[0], cj = (cy >> sc) - Lc.c0[1], ck = (cz >> sc) - Lc.c0[2];
            const bool in = ci < Lc.n[0] && cj < Lc.n[1] && ck < Lc.n[2];   // (always: the child holds a voxel of the box)
            const uint32_t e = in ? pyr[Lc.first + ((uint64_t) ck * Lc.n[1] + cj) * Lc.n[0] + ci] : 0u;
            nd.valid[child] = (uint8_t) (e & 0xffu), nd.full[child] = (uint8_t) (e >> 8);
            nd.coords[3u * child] = (int32_t) cx, nd.coords[3u * child + 1u] = (int32_t) cy, nd.coords[3u * child + 2u] = (int32_t) cz;
        }
    }
}

// out[p] = the descent to points[p]
__global__ __launch_bounds__(kBlock) void k_oct_lookup(OctTree t, const int32_t *__restrict__ points, uint64_t n, int32_t *__restrict__ out)
{
    for (uint64_t p = (uint64_t) blockIdx.x * kBlock + threadIdx.x; p < n; p += (uint64_t) gridDim.x * kBlock) {
        int32_t r[4];
        oct_descend(t, points[3u * p], points[3u * p + 1u], points[3u * p + 2u], r);
        out[4u * p] = r[0], out[4u * p + 1u] = r[1], out[4u * p + 2u] = r[2], out[4u * p + 3u] = r[3];
    }
}

// The box origin + [0, n) as aligned 2^3 blocks: block b0 + i along an axis for i below nb.
struct OctDense {
    uint32_t o[3], n[3], b0[3], nb[3];
    uint64_t blocks;
    uint64_t s0, s1, s2;   // element strides of out (x, y, z)
};

// out(x, y, z) = 1 where the descent is solid, 0 elsewhere: a lane per block, neighbouring lanes neighbouring pairs of a row
__global__ __launch_bounds__(kBlock) void k_oct_dense(OctTree t, OctDense d, uint8_t *__restrict__ out)
{
    const uint32_t side = 1u << t.depth;
    for (uint64_t b = (uint64_t) blockIdx.x * kBlock + threadIdx.x; b < d.blocks; b += (uint64_t) gridDim.x * kBlock) {
        const uint64_t row = b / d.nb[0];
        const uint32_t i = (uint32_t) (b - row * d.nb[0]), k = (uint32_t) (row / d.nb[1]), j = (uint32_t) (row - (uint64_t) k * d.nb[1]);
        const uint32_t x = 2u * (d.b0[0] + i), y = 2u * (d.b0[1] + j), z = 2u * (d.b0[2] + k);   // (origin + dims is at most 2^32: no wrap)
        const uint32_t mask = x < side && y < side && z < side ? oct_block(t, x, y, z) : 0u;
#pragma unroll
        for (uint32_t o = 0; o < 8u; ++o) {
            const uint32_t lx = x + (o & 1u) - d.o[0], ly = y + ((o >> 1) & 1u) - d.o[1], lz = z + (o >> 2) - d.o[2];   // (below the origin: wraps past n)
            if (lx < d.n[0] && ly < d.n[1] && lz < d.n[2]) out[(uint64_t) lx * d.s0 + (uint64_t) ly * d.s1 + (uint64_t) lz * d.s2] = (uint8_t) ((mask >> o) & 1u);
        }
    }
}

#endif   // O2V_OCT_HOST
