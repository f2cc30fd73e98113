// o2v_dev_k31_treeray.hpp -- K31: rays through a sparse voxel octree or DAG (o2v_hip_octree_raycast / o2v_hip_octree_dag_raycast).
// Included from o2v_device.hip inside its anonymous namespace, behind K11 (whose Ray, ray_T, ray_step and ray_advance it uses
// unchanged), K26 (OctTree, oct_step) and K30 (OctDag, dag_step); compiled with -ffp-contract=off like K11.
//
// The definition is in include/o2v_hip.h: the walk of o2v_hip_raycast over the solid set of the descent, the root cube [0, 2^D)^3 on
// the global lattice, everything outside it empty.  The caller's arrays are walked in place: no snapshot, no scratch.
//
//   tree_walk<Src, Stack>   a ray per lane.  Outside the root cube it is K11's entry: the greatest entry event of the axes on which the
//                           ray is still outside, with the "gone" tests.  Inside, it descends for the cell the ray stands in.  An
//                           empty octant of a node of level l is an empty aligned block of side 2^(D - 1 - l): ray_advance takes
//                           the ray to the block's least exit event, exactly as K11 leaves an empty 4^3, 16^3 or 64^3 block - a
//                           step that the descent calls corrupt is such an octant too.  A full octant of a collapsed tree is a hit
//                           where the ray stands.  At level D - 1 the node's `valid` byte is the 2^3 block: the fine walk runs on
//                           it in registers until the ray leaves the block.  The DAG source adds the skips on the way down, so the
//                           voxel index of the hit is there when the walk ends.
//   Stack = false           (O2V_TREERAY_NO_STACK=1) every event descends again from the root.
//   Stack = true            the ray keeps (node, skips) of its ancestors per level and restarts from the deepest common ancestor of
//                           the old and the new cell, found from the highest differing bit of their coordinates.  The stack is
//                           indexed by a run-time level, so it lives in LDS as [level][lane]: 8 bytes per entry, (D - 1) * 8 * 256
//                           bytes of dynamic LDS a block, at most 30 KB; lane-contiguous, so a wavefront's access is one row.
//   k_tree_cast<Src, Stack> k_ray_cast's prologue and epilogue (validity, 1 / d, the outputs) around tree_walk, and the voxel index.
// wave64, 256 threads, no private segment.  Both variants give the same bits: the stack only changes where a descent starts.

// ---- the walk ------------------------------------------------------------------------------------------------------------
// (Plain C++ from here to the cast kernel: tests/test_host_treeray.py compiles this part for the host behind K11's walk part and the
// plain parts of K26 and K30, and holds it against the reference there, with the mutation below as well.)

// What a ray remembers of an ancestor: the node and, for a DAG, the skips added on the way to it.
struct alignas(8) TreeRayEntry {   // (one 8-byte LDS access)
    uint32_t node, acc;
};

// A lane's stack: entry (l - 1) * stride is its ancestor of level l, 1 <= l <= D - 1 (level 0 is node 0 with no skips).
struct TreeRayStack {
    TreeRayEntry *p;
    uint32_t stride;
};

// The two sources of a walk: the step of the descent, the 2^3 block of a node of level D - 1, the slot of one of its voxels.
struct TreeRayOct {
    OctTree t;
    __device__ __forceinline__ uint32_t depth() const { return t.depth; }
    __device__ __forceinline__ uint32_t step(uint32_t &i, uint32_t &, uint32_t o) const { return oct_step(t, i, o); }
    __device__ __forceinline__ uint32_t block(uint32_t i) const { return t.valid[i]; }
    __device__ __forceinline__ int32_t slot(uint32_t i, uint32_t, uint32_t v, uint32_t o) const { return (int32_t) ((uint32_t) t.first_child[i] + oct_rank(v, o)); }
};

struct TreeRayDag {
    OctDag d;
    __device__ __forceinline__ uint32_t depth() const { return d.depth; }
    __device__ __forceinline__ uint32_t step(uint32_t &i, uint32_t &acc, uint32_t o) const { return dag_step(d, i, acc, o); }
    __device__ __forceinline__ uint32_t block(uint32_t i) const { return d.valid[i]; }
    __device__ __forceinline__ int32_t slot(uint32_t, uint32_t acc, uint32_t v, uint32_t o) const { return d.skips ? (int32_t) (acc + oct_rank(v, o)) : -1; }
};

// the position of the highest set bit of v != 0
__device__ __forceinline__ uint32_t treeray_top_bit(uint32_t v) { return 31u - (uint32_t) __builtin_clz(v); }

// true: r.c is solid, entered at r.T through r.face, and slot is its voxel index (-1 inside a full cell or without skips)
// The entry from outside the cube, the choice of E and the second "gone" test are ray_walk's of o2v_dev_k11_raycast.hpp line by line
// (its box being [0, 2^D)^3 here): the two must change together, since the equality with RayCaster bit for bit rests on them.
template <class Src, bool Stack>
__device__ __forceinline__ bool tree_walk(Ray &r, double tmax, const Src &src, const TreeRayStack &st, int32_t &slot)
{
    const uint32_t D = src.depth();
    const int32_t side = (int32_t) (1u << D);
    // the stack holds the ancestors of levels 1 ... top of the cell (px, py, pz)
    uint32_t top = 0;
    int32_t px = 0, py = 0, pz = 0;
    slot = -1;
    for (;;) {
        const int32_t cx = r.c[0], cy = r.c[1], cz = r.c[2];
        const bool in = (uint32_t) cx < (uint32_t) side && (uint32_t) cy < (uint32_t) side && (uint32_t) cz < (uint32_t) side;
        int32_t x[3], lim[3];   // per axis: the plane of its event; the plane the search ends at
        bool takes[3];          // the axis has an event
        if (in) {
            uint32_t l = 0, i = 0, acc = 0;
            if (Stack && top != 0u) {
                // the deepest level at which the old and the new cell have one ancestor: above their highest differing bit
                const uint32_t diff = (uint32_t) ((cx ^ px) | (cy ^ py) | (cz ^ pz));
                const uint32_t shared = diff ? D - 1u - treeray_top_bit(diff) : D - 1u;   // (both inside the cube: the bit is below D)
                l = shared < top ? shared : top;
                if (l != 0u) {
                    const TreeRayEntry e = st.p[(l - 1u) * st.stride];
                    i = e.node, acc = e.acc;
                }
            }
            uint32_t code = kOctDown;
            for (; l + 1u < D; ++l) {
                code = src.step(i, acc, oct_octant((uint32_t) cx, (uint32_t) cy, (uint32_t) cz, D - 1u - l));
                if (code != kOctDown) break;
                if (Stack) st.p[l * st.stride] = TreeRayEntry{i, acc};   // (level l + 1)
            }
            if (Stack) top = l, px = cx, py = cy, pz = cz;
            if (code == kOctFull) return true;
            if (code == kOctDown) {
                // level D - 1: the fine walk on the node's 2^3 block
                const uint32_t v = src.block(i);
                const int32_t bx = cx >> 1, by = cy >> 1, bz = cz >> 1;
                for (;;) {
                    if ((r.c[0] >> 1) != bx || (r.c[1] >> 1) != by || (r.c[2] >> 1) != bz) break;
                    const uint32_t o = oct_octant((uint32_t) r.c[0], (uint32_t) r.c[1], (uint32_t) r.c[2], 0u);
                    if ((v >> o) & 1u) {
                        slot = src.slot(i, acc, v, o);
                        return true;
                    }
                    if (!ray_step(r, tmax)) return false;
                }
                continue;
            }
            // an empty (or corrupt) octant of level l: the aligned block of side 2^k around the cell is empty
#ifdef O2V_TREERAY_MUTATE_BLOCK_SHIFT
            const uint32_t k = D - l;        // (test only: the block taken one level too large)
#else
            const uint32_t k = D - 1u - l;
#endif
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                x[b] = lim[b] = ((r.c[b] >> k) + (r.s[b] > 0 ? 1 : 0)) << k;
                takes[b] = r.s[b] != 0;
            }
        } else {
            bool gone = false;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const bool below = r.c[b] < 0, above = r.c[b] >= side;
                gone = gone || (r.s[b] > 0 ? above : r.s[b] < 0 ? below : (below || above));   // left on this axis for good
                takes[b] = (r.s[b] > 0 && below) || (r.s[b] < 0 && above);
                x[b] = r.s[b] > 0 ? 0 : side;     // the plane it enters through
                lim[b] = r.s[b] > 0 ? side : 0;   // the plane it leaves through
            }
            if (gone) return false;
        }
        // E: inside, the least of the block's exit events; outside, the greatest of the entry events still ahead
        double TE = 0.0;
        int aE = -1;
        int32_t xE = 0;
#pragma unroll
        for (int b = 0; b < 3; ++b)
            if (takes[b]) {
                const double Tb = ray_T(r, b, x[b]);
                const bool better = in ? (Tb < TE || (!kRayTieLowestAxis && Tb == TE)) : (Tb > TE || (kRayTieLowestAxis && Tb == TE));
                if (aE < 0 || better) TE = Tb, aE = b, xE = x[b];
            }
        if (aE < 0 || TE > tmax) return false;
        if (!in) {
            // an axis whose exit plane comes before E has left the cube before the ray is inside on every axis
            bool gone = false;
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (b != aE && r.s[b] != 0) {
                    const double Tl = ray_T(r, b, lim[b]);
                    gone = gone || Tl < TE || (Tl == TE && (kRayTieLowestAxis ? b < aE : b > aE));
                }
            if (gone) return false;
        }
        ray_advance(r, TE, aE, xE, lim);
    }
}

// ---- the cast kernel ---------------------------------------------------------------------------------------------------------
#ifndef O2V_OCT_HOST

constexpr uint32_t kTreeRayEntryBytes = 8u;
static_assert(sizeof(TreeRayEntry) == kTreeRayEntryBytes, "the stack's entries are two words");

template <class Src, bool Stack>
__global__ __launch_bounds__(kBlock) void k_tree_cast(const float *__restrict__ origins, const float *__restrict__ directions, uint64_t n, float t_max, Src src,
                                                      int32_t *__restrict__ hit, float *__restrict__ t_out, int32_t *__restrict__ voxel_index)
{
    extern __shared__ TreeRayEntry s_treeray[];   // [level 1 ... D - 1][lane of the block]: only with Stack
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Ray r;
    bool valid = true;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const float of = origins[i * 3u + b], df = directions[i * 3u + b];
        valid = valid && isfinite(of) && isfinite(df) && fabsf(of) <= 4194304.f;
        r.o[b] = (double) of;
        r.d[b] = (double) df;
    }
    int32_t out[4] = {-1, -1, -1, -2}, slot = -1;
    float t = __builtin_nanf("");
    if (valid) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            r.s[b] = r.d[b] > 0.0 ? 1 : r.d[b] < 0.0 ? -1 : 0;
            r.inv[b] = r.s[b] != 0 ? 1.0 / r.d[b] : 0.0;
            r.c[b] = (int32_t) floor(r.o[b]);
            r.nxt[b] = r.c[b] + (r.s[b] > 0 ? 1 : 0);
        }
        r.T = 0.0;
        r.face = -1;
        const TreeRayStack st{s_treeray + threadIdx.x, kBlock};
        if (tree_walk<Src, Stack>(r, (double) t_max, src, st, slot)) {
            out[0] = r.c[0], out[1] = r.c[1], out[2] = r.c[2], out[3] = r.face;
            t = (float) r.T;
        } else {
            out[3] = -1;
            slot = -1;
            t = __builtin_inff();
        }
    }
    if ((reinterpret_cast<uintptr_t>(hit) & 15u) == 0u)
        reinterpret_cast<int4 *>(hit)[i] = make_int4(out[0], out[1], out[2], out[3]);
    else
        hit[i * 4u] = out[0], hit[i * 4u + 1u] = out[1], hit[i * 4u + 2u] = out[2], hit[i * 4u + 3u] = out[3];
    t_out[i] = t;
    if (voxel_index) voxel_index[i] = slot;
}

#endif   // O2V_OCT_HOST
