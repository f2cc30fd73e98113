// o2v_dev_k30_dag.hpp -- K30: the sparse voxel DAG of an octree (o2v_hip_octree_dag_build / _write / _lookup / _to_dense).
// Included from o2v_device.hip inside its anonymous namespace, behind K26 (whose octant, rank and stored-mask functions and whose
// box of 2^3 blocks it uses; K6's block scan comes with it).
//
// The definition is in include/o2v_hip.h: two nodes of one level are equal if their valid masks, their full masks and, one by one,
// their stored children are; a class is numbered by its smallest member; per child pointer the listed voxels under the earlier
// siblings (`skip`), so that the descent still finds a voxel's slot.  Bottom up, a group of launches per level, no host wait between:
//
//   level D - 1: the key is `valid` alone.
//   k_dag_leaf_min        a wavefront per contiguous run of nodes: per turn it reduces the lanes that bring a value it has not seen
//                         to one lane per value (the lowest: indices rise with the lane) and that lane alone touches the table of 256
//                         smallest indices - after a read, so that an index that would not lower the entry issues no atomic.
//   k_dag_leaf_rep        rep[i] = table[valid[i]].
//   levels above: the key is valid, full and the classes of the stored children, which the level below has finalised.
//   k_dag_insert          a lane per node into an open-addressing table of node indices (a slot's key is read through the node it
//                         names): an empty slot is claimed by compare-and-swap, a slot of an equal key lowered by atomicMin - after
//                         a read: a lane whose index is not below what it read issues nothing -, a slot of another key passed.  The
//                         lanes of a wavefront whose key equals that of its first lane leave the insert to that lane (the all-equal
//                         level: a wavefront brings one candidate, not 64).  A stored child outside the next level raises the flag
//                         and keeps the node out of the table: the index is checked before it is used.
//   k_dag_find            rep[i] = the slot of i's key: the smallest index of the class, whatever the slots' positions.
//   every level:
//   k_dag_flags + k_fill_scan_blocks (K6)   the exclusive scan of rep[i] == i: the rank of a class within its level, and their number.
//   k_dag_ids             cls[i] = rank of rep[i] (with a bit for the representatives), listed[i] = the listed voxels under the node,
//                         and the stored children of the representatives counted: the pointers of the level.
//   the host reads the flag and the counts, sizes the DAG's arrays, and per level:
//   k_dag_ptr_count + k_fill_scan_blocks    the exclusive scan of the representatives' stored children: first_child.
//   k_dag_emit            a lane per representative: its DAG node, and per stored child its class and the listed voxels before it.
//   k_dag_lookup          a lane per point: the descent.  k_dag_dense: a lane per aligned 2^3 block of the box, as k_oct_dense.
// Integers only, wave64, no private segment, no LDS beyond the block scan's four words; the same bits on every run: the atomics
// decide which slot a class lands in, never which index represents it.

constexpr uint32_t kDagEmpty = 0xffffffffu;    // a table entry that no node has claimed (and above every index)
constexpr uint32_t kDagRepBit = 0x80000000u;   // in cls: the node represents its class
constexpr uint32_t kDagIdMask = 0x7fffffffu;
constexpr uint32_t kDagBadTree = 1u, kDagTableFull = 2u;   // the bits of the flag

// ---- keys, the child-range check, the descent ----------------------------------------------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_dag.py compiles this part for the host behind the plain part of
// o2v_dev_k26_octree.hpp and runs it against the reference.)

// The nodes of one level of the tree while it is merged: node i of the level is entry first + i of the tree's arrays; cls: per tree
// node its class within its level (low 31 bits), final for the levels below this one.  [lo, hi): the next level's nodes.
struct DagLevel {
    const uint8_t *valid, *full;
    const int32_t *first_child;
    const uint32_t *cls;
    uint64_t first, lo, hi;
    uint32_t collapsed;
};

// The stored children first_child ... first_child + n_stored - 1 of a node all lie in [lo, hi): the next level of a tree of these
// level counts.  A node without stored children passes whatever its first_child holds.
O2V_OCT_FN bool dag_child_range_ok(int32_t first_child, uint32_t n_stored, uint64_t lo, uint64_t hi)
{
    if (n_stored == 0u) return true;
    return first_child >= 0 && (uint64_t) (uint32_t) first_child >= lo && (uint64_t) (uint32_t) first_child + n_stored <= hi;
}

// what two equal nodes share besides their children
O2V_OCT_FN uint32_t dag_key_head(uint32_t valid, uint32_t full)
{
#ifdef O2V_DAG_MUTATE_IGNORE_FULL
    return valid;   // (test only: equality that does not look at `full`)
#else
    return valid | full << 8;
#endif
}

O2V_OCT_FN uint32_t dag_mix(uint32_t h, uint32_t v)
{
    h = (h ^ v) * 0x9e3779b1u;
    return h ^ h >> 15;
}

// The key of node i of the level (its child range checked): the hash ...
O2V_OCT_FN uint32_t dag_key_hash(const DagLevel &L, uint32_t i)
{
    const uint32_t v = L.valid[L.first + i], f = L.full[L.first + i], n = oct_popc(oct_stored(v, f, L.collapsed));
    uint32_t h = dag_mix(0x2545f491u, dag_key_head(v, f));
    const uint32_t *const c = L.cls + (n ? (uint32_t) L.first_child[L.first + i] : 0u);
    for (uint32_t r = 0; r < n; ++r) h = dag_mix(h, c[r] & kDagIdMask);
    return h ^ h >> 13;
}

// ... and equality with node j's
O2V_OCT_FN bool dag_key_equal(const DagLevel &L, uint32_t i, uint32_t j)
{
    const uint32_t vi = L.valid[L.first + i], fi = L.full[L.first + i], vj = L.valid[L.first + j], fj = L.full[L.first + j];
    if (dag_key_head(vi, fi) != dag_key_head(vj, fj)) return false;
    const uint32_t n = oct_popc(oct_stored(vi, fi, L.collapsed));
    if (n != oct_popc(oct_stored(vj, fj, L.collapsed))) return false;   // (only where the head leaves `full` out)
    if (n == 0u) return true;
    const uint32_t *const a = L.cls + (uint32_t) L.first_child[L.first + i], *const b = L.cls + (uint32_t) L.first_child[L.first + j];
    for (uint32_t r = 0; r < n; ++r)
        if ((a[r] & kDagIdMask) != (b[r] & kDagIdMask)) return false;
    return true;
}

// A DAG as the queries take it: the caller's arrays of n_nodes and n_pointers entries.  skips: the voxel index is asked for and skip
// is there (a DAG without pointers has nothing to skip: see dag_skips).
struct OctDag {
    const uint8_t *valid, *full;
    const int32_t *first_child, *child, *skip;
    uint32_t n_nodes, n_pointers, depth, collapsed, skips;
};

O2V_OCT_HD uint32_t dag_skips(const int32_t *skip, uint64_t n_pointers) { return skip || n_pointers == 0u ? 1u : 0u; }

// One step at node i of a level below D - 1 towards octant o.  kOctDown: i is the child and acc has its skip.  Nothing is read
// outside the n_nodes and n_pointers entries.
O2V_OCT_FN uint32_t dag_step(const OctDag &d, uint32_t &i, uint32_t &acc, uint32_t o)
{
    const uint32_t v = d.valid[i], f = d.full[i];
    if (!((v >> o) & 1u)) return kOctEmpty;
    if (d.collapsed && ((f >> o) & 1u)) return kOctFull;
    const int32_t fc = d.first_child[i];
    if (fc < 0) return kOctCorrupt;
    const uint64_t e = (uint64_t) (uint32_t) fc + oct_rank(oct_stored(v, f, d.collapsed), o);
    if (e >= d.n_pointers) return kOctCorrupt;
    const int32_t c = d.child[e];
    if (c < 0 || (uint32_t) c >= d.n_nodes) return kOctCorrupt;
    if (d.skips) acc += (uint32_t) d.skip[e];
    i = (uint32_t) c;
    return kOctDown;
}

// The descent to (x, y, z): out = (solid, level, node, voxel_index) as include/o2v_hip.h defines them; at most D steps.
O2V_OCT_FN void dag_descend(const OctDag &d, int32_t x, int32_t y, int32_t z, int32_t out[4])
{
    const int32_t side = (int32_t) (1u << d.depth);
    out[0] = 0, out[1] = out[2] = out[3] = -1;
    if (x < 0 || y < 0 || z < 0 || x >= side || y >= side || z >= side) return;
    uint32_t i = 0, acc = 0;
    for (uint32_t l = 0; l + 1u < d.depth; ++l) {
        const uint32_t at = i, code = dag_step(d, i, acc, oct_octant((uint32_t) x, (uint32_t) y, (uint32_t) z, d.depth - 1u - l));
        if (code == kOctDown) continue;
        if (code == kOctCorrupt) {
            out[1] = -2;
            return;
        }
        out[0] = code == kOctFull ? 1 : 0, out[1] = (int32_t) l, out[2] = (int32_t) at;
        return;
    }
    const uint32_t o = oct_octant((uint32_t) x, (uint32_t) y, (uint32_t) z, 0u), v = d.valid[i];
    out[1] = (int32_t) d.depth - 1, out[2] = (int32_t) i;
    if (!((v >> o) & 1u)) return;
    out[0] = 1;
    if (d.skips) out[3] = (int32_t) (acc + oct_rank(v, o));
}

// The eight voxels of the aligned 2^3 block at (x, y, z) (even, inside the root cube) as a mask, bit dx + 2 dy + 4 dz: one
// descent to level D - 1, without the skips.  Corrupt arrays give 0.
O2V_OCT_FN uint32_t dag_block(const OctDag &d, uint32_t x, uint32_t y, uint32_t z)
{
    OctDag t = d;
    t.skips = 0u;
    uint32_t i = 0, acc = 0;
    for (uint32_t l = 0; l + 1u < t.depth; ++l) {
        const uint32_t code = dag_step(t, i, acc, oct_octant(x, y, z, t.depth - 1u - l));
        if (code == kOctDown) continue;
        return code == kOctFull ? 0xffu : 0u;
    }
    return t.valid[i];
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------
#ifndef O2V_OCT_HOST

// The counters of a build, 64-bit words: the classes per level, the pointers per level (summed, then from the scans), the flag.
constexpr uint32_t kDagCount = 0u, kDagPtr = 16u, kDagPtrScan = 32u, kDagFlag = 48u, kDagMeta = 56u;

// What a build keeps per tree node (cls, listed) and per node of its widest level (num: the block-local scans).
struct DagWork {
    uint32_t *cls, *listed, *num;
};

// The DAG's arrays in the context's scratch.
struct DagOut {
    uint8_t *valid, *full;
    int32_t *first_child, *child, *skip;
    uint64_t nodes, pointers;
};

__device__ __forceinline__ uint32_t dag_peek(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// tab[v] = the smallest i with valid[first + i] == v (tab: 256 entries of kDagEmpty on entry)
__global__ __launch_bounds__(kBlock) void k_dag_leaf_min(const uint8_t *__restrict__ valid, uint64_t first, uint32_t n, uint32_t *__restrict__ tab)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t) blockIdx.x * kBlock + threadIdx.x) >> 6, waves = (uint64_t) gridDim.x * (kBlock / 64u);
    const uint64_t per = (((uint64_t) n + waves - 1u) / waves + 63u) & ~63ull;   // a wavefront's run: indices rise with its turns
    const uint64_t lo = wave * per, hi = lo + per < n ? lo + per : n;
    uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;   // the values this wavefront has brought to the table: 256 bits, the same in every lane
    for (uint64_t base = lo; base < hi; base += 64u) {
        const uint64_t i = base + lane;
        const uint32_t v = i < hi ? valid[first + i] : 0u;
        const uint64_t word = v < 64u ? s0 : v < 128u ? s1 : v < 192u ? s2 : s3;
        bool fresh = i < hi && !((word >> (v & 63u)) & 1ull);
        for (uint64_t todo = __ballot(fresh); todo; todo = __ballot(fresh)) {
            const uint32_t leader = (uint32_t) __ffsll((unsigned long long) todo) - 1u;
            const uint32_t cur = (uint32_t) __shfl((int) v, (int) leader, 64);
            if (lane == leader && (uint32_t) i < dag_peek(tab + cur)) atomicMin(tab + cur, (uint32_t) i);
            const uint64_t bit = 1ull << (cur & 63u);
            s0 |= cur < 64u ? bit : 0ull, s1 |= cur >= 64u && cur < 128u ? bit : 0ull, s2 |= cur >= 128u && cur < 192u ? bit : 0ull, s3 |= cur >= 192u ? bit : 0ull;
            fresh = fresh && v != cur;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_dag_leaf_rep(const uint8_t *__restrict__ valid, uint64_t first, uint32_t n, const uint32_t *__restrict__ tab,
                                                         uint32_t *__restrict__ cls)
{
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) cls[first + i] = tab[valid[first + i]];
}

// whether node i of the level may be keyed: its stored children lie in the next level
__device__ __forceinline__ bool dag_node_ok(const DagLevel &L, uint32_t i)
{
    const uint32_t v = L.valid[L.first + i], f = L.full[L.first + i];
    return dag_child_range_ok(L.first_child[L.first + i], oct_popc(oct_stored(v, f, L.collapsed)), L.lo, L.hi);
}

// every node of the level into the table (tab: mask + 1 entries of kDagEmpty on entry)
__global__ __launch_bounds__(kBlock) void k_dag_insert(DagLevel L, uint32_t n, uint32_t *__restrict__ tab, uint32_t mask, unsigned long long *__restrict__ flag)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t) blockIdx.x * kBlock; base < n; base += (uint64_t) gridDim.x * kBlock) {   // (uniform over the workgroup)
        const uint32_t i = (uint32_t) (base + threadIdx.x);
        const bool ok = base + threadIdx.x < n && dag_node_ok(L, i);
        if (base + threadIdx.x < n && !ok) atomicOr(flag, (unsigned long long) kDagBadTree);
        // the lanes whose key is that of the wavefront's first lane leave the insert to it: its index is the smallest of them
        const uint64_t active = __ballot(ok);
        const uint32_t leader = active ? (uint32_t) __ffsll((unsigned long long) active) - 1u : 0u;
        const uint32_t li = (uint32_t) __shfl((int) i, (int) leader, 64);   // (an ok lane has an ok leader)
        if (ok && (lane == leader || !dag_key_equal(L, i, li))) {
            uint32_t h = dag_key_hash(L, i) & mask, probe = 0;
            for (; probe <= mask; ++probe, h = (h + 1u) & mask) {
                uint32_t cur = dag_peek(tab + h);
                if (cur == kDagEmpty) {
                    cur = atomicCAS(tab + h, kDagEmpty, i);
                    if (cur == kDagEmpty) break;
                }
                if (cur == i || dag_key_equal(L, i, cur)) {
                    if (i < cur) atomicMin(tab + h, i);   // (cur: what was read.  Not below it: no atomic)
                    break;
                }
            }
            if (probe > mask) atomicOr(flag, (unsigned long long) kDagTableFull);   // (never: the table has twice the level's nodes)
        }
    }
}

// cls[first + i] = the smallest index of i's class, read from the slot of its key
__global__ __launch_bounds__(kBlock) void k_dag_find(DagLevel L, uint32_t n, const uint32_t *__restrict__ tab, uint32_t mask, uint32_t *__restrict__ cls,
                                                     unsigned long long *__restrict__ flag)
{
    for (uint64_t p = (uint64_t) blockIdx.x * kBlock + threadIdx.x; p < n; p += (uint64_t) gridDim.x * kBlock) {
        const uint32_t i = (uint32_t) p;
        uint32_t rep = i;
        if (dag_node_ok(L, i)) {
            uint32_t h = dag_key_hash(L, i) & mask, probe = 0;
            for (; probe <= mask; ++probe, h = (h + 1u) & mask) {
                const uint32_t cur = tab[h];
                if (cur == kDagEmpty) break;
                if (cur == i || dag_key_equal(L, i, cur)) {
                    rep = cur;
                    break;
                }
            }
            if (rep == i && tab[h] != i) atomicOr(flag, (unsigned long long) kDagTableFull);   // (never: k_dag_insert has put the key there)
        }
        cls[L.first + i] = rep;
    }
}

// num[i] = the representatives of its block of 256 before node i; block_sums[b] = the block's representatives
__global__ __launch_bounds__(kBlock) void k_dag_flags(const uint32_t *__restrict__ cls, uint64_t first, uint32_t n, uint64_t n_blocks,
                                                      uint32_t *__restrict__ num, unsigned long long *__restrict__ block_sums)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint64_t i = b * kBlock + threadIdx.x;
        const uint64_t cnt = i < n && cls[first + i] == (uint32_t) i ? 1u : 0u;
        uint64_t total;
        const uint64_t ex = fill_block_exscan64(cnt, s_wave, total);
        if (i < n) num[i] = (uint32_t) ex;
        if (threadIdx.x == 0) block_sums[b] = total;
    }
}

// the stored children of node i of the level as the DAG sees them: none at level D - 1
__device__ __forceinline__ uint32_t dag_node_stored(const DagLevel &L, uint32_t i, uint32_t leaf)
{
    return leaf ? 0u : oct_stored(L.valid[L.first + i], L.full[L.first + i], L.collapsed);
}

// cls[first + i] = the rank of i's class (kDagRepBit: i represents it); listed[first + i]; *pointers += the representatives' stored children
__global__ __launch_bounds__(kBlock) void k_dag_ids(DagLevel L, uint32_t n, uint32_t leaf, const uint32_t *__restrict__ num,
                                                    const unsigned long long *__restrict__ boff, DagWork w, unsigned long long *__restrict__ pointers)
{
    uint32_t mine = 0;
    for (uint64_t base = (uint64_t) blockIdx.x * kBlock; base < n; base += (uint64_t) gridDim.x * kBlock) {
        const uint32_t i = (uint32_t) (base + threadIdx.x);
        if (base + threadIdx.x >= n) continue;
        const uint32_t rep = w.cls[L.first + i], v = L.valid[L.first + i];
        uint32_t listed = oct_popc(v);
        if (!leaf) {
            const uint32_t stored = dag_node_stored(L, i, 0u), cnt = oct_popc(stored);
            listed = 0;
            if (cnt && dag_node_ok(L, i)) {
                const uint32_t fc = (uint32_t) L.first_child[L.first + i];
                for (uint32_t r = 0; r < cnt; ++r) listed += w.listed[fc + r];
            }
            if (rep == i) mine += cnt;
        }
        w.listed[L.first + i] = listed;
        w.cls[L.first + i] = ((uint32_t) boff[rep / kBlock] + num[rep]) | (rep == i ? kDagRepBit : 0u);
    }
    for (int d = 32; d >= 1; d >>= 1) mine += (uint32_t) __shfl_xor((int) mine, d, 64);
    if ((threadIdx.x & 63u) == 0u && mine) atomicAdd(pointers, (unsigned long long) mine);   // (a sum: the atomics decide no order)
}

// num[i] = the stored children of the representatives of its block before node i; block_sums[b] = the block's
__global__ __launch_bounds__(kBlock) void k_dag_ptr_count(DagLevel L, uint32_t n, uint64_t n_blocks, uint32_t *__restrict__ num,
                                                          unsigned long long *__restrict__ block_sums)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint64_t i = b * kBlock + threadIdx.x;
        const uint64_t cnt = i < n && (L.cls[L.first + i] & kDagRepBit) ? (uint64_t) oct_popc(dag_node_stored(L, (uint32_t) i, 0u)) : 0u;
        uint64_t total;
        const uint64_t ex = fill_block_exscan64(cnt, s_wave, total);
        if (i < n) num[i] = (uint32_t) ex;
        if (threadIdx.x == 0) block_sums[b] = total;
    }
}

// The DAG nodes of the level's representatives, from node0 on, and (above level D - 1) their pointers, from ptr0 on: the class of
// each stored child (next0: the next level's first DAG node) and the listed voxels under the stored children before it.
__global__ __launch_bounds__(kBlock) void k_dag_emit(DagLevel L, uint32_t n, uint32_t leaf, const uint32_t *__restrict__ num,
                                                     const unsigned long long *__restrict__ boff, const uint32_t *__restrict__ listed, uint64_t node0,
                                                     uint64_t next0, uint64_t ptr0, DagOut out)
{
    for (uint64_t p = (uint64_t) blockIdx.x * kBlock + threadIdx.x; p < n; p += (uint64_t) gridDim.x * kBlock) {
        const uint32_t i = (uint32_t) p, c = L.cls[L.first + i];
        if (!(c & kDagRepBit)) continue;
        const uint64_t m = node0 + (c & kDagIdMask);
        if (m >= out.nodes) continue;   // (never: the arrays are sized by the counts of these very classes)
        out.valid[m] = L.valid[L.first + i], out.full[m] = L.full[L.first + i];
        const uint32_t cnt = oct_popc(dag_node_stored(L, i, leaf));
        if (!cnt || !dag_node_ok(L, i)) {
            out.first_child[m] = -1;
            continue;
        }
        const uint64_t e0 = ptr0 + boff[i / kBlock] + num[i];
        const uint32_t fc = (uint32_t) L.first_child[L.first + i];
        out.first_child[m] = (int32_t) e0;
        uint32_t before = 0;
        for (uint32_t r = 0; r < cnt; ++r) {
            if (e0 + r < out.pointers) out.child[e0 + r] = (int32_t) (next0 + (L.cls[fc + r] & kDagIdMask)), out.skip[e0 + r] = (int32_t) before;
            before += listed[fc + r];
        }
    }
}

// out[p] = the descent to points[p]
__global__ __launch_bounds__(kBlock) void k_dag_lookup(OctDag d, const int32_t *__restrict__ points, uint64_t n, int32_t *__restrict__ out)
{
    for (uint64_t p = (uint64_t) blockIdx.x * kBlock + threadIdx.x; p < n; p += (uint64_t) gridDim.x * kBlock) {
        int32_t r[4];
        dag_descend(d, points[3u * p], points[3u * p + 1u], points[3u * p + 2u], r);
        out[4u * p] = r[0], out[4u * p + 1u] = r[1], out[4u * p + 2u] = r[2], out[4u * p + 3u] = r[3];
    }
}

// out(x, y, z) = 1 where the descent is solid, 0 elsewhere: a lane per block of the box (K26's OctDense)
__global__ __launch_bounds__(kBlock) void k_dag_dense(OctDag t, OctDense d, uint8_t *__restrict__ out)
{
    const uint32_t side = 1u << t.depth;
    for (uint64_t b = (uint64_t) blockIdx.x * kBlock + threadIdx.x; b < d.blocks; b += (uint64_t) gridDim.x * kBlock) {
        const uint64_t row = b / d.nb[0];
        const uint32_t i = (uint32_t) (b - row * d.nb[0]), k = (uint32_t) (row / d.nb[1]), j = (uint32_t) (row - (uint64_t) k * d.nb[1]);
        const uint32_t x = 2u * (d.b0[0] + i), y = 2u * (d.b0[1] + j), z = 2u * (d.b0[2] + k);   // (origin + dims is at most 2^32: no wrap)
        const uint32_t mask = x < side && y < side && z < side ? dag_block(t, x, y, z) : 0u;
#pragma unroll
        for (uint32_t o = 0; o < 8u; ++o) {
            const uint32_t lx = x + (o & 1u) - d.o[0], ly = y + ((o >> 1) & 1u) - d.o[1], lz = z + (o >> 2) - d.o[2];   // (below the origin: wraps past n)
            if (lx < d.n[0] && ly < d.n[1] && lz < d.n[2]) out[(uint64_t) lx * d.s0 + (uint64_t) ly * d.s1 + (uint64_t) lz * d.s2] = (uint8_t) ((mask >> o) & 1u);
        }
    }
}

#endif   // O2V_OCT_HOST
