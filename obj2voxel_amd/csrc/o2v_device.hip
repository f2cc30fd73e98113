// o2v_device.hip -- the MI355X (gfx950) voxelization pipeline behind include/o2v_hip.h.
//
// Replaces, for one GPU's z-slab of the grid, the reference's chunk loop (src/obj2voxel.cpp:467-520) and
// Voxelizer::voxelize (src/voxelization.cpp:480-526).  Written for CDNA4: 64-wide wavefronts, LDS-staged leaf
// geometry and work queues, register-resident clip stacks, 32- and 64-bit atomics on dense (bricked) HBM grids of per-cell
// counters / maxima.  No MFMA: the path is float32 VALU + HBM/atomic traffic.
//
// Stages (one HIP stream; the replay tiers fork onto three auxiliary streams; kernels in o2v_dev_k*.hpp):
//   K0  k_bounds / k_setup     mesh bounds (obj2voxel.cpp:180-200) and mesh transform (obj2voxel.cpp:370-402)
//   K1  k_expand_roots         transform (obj2voxel.cpp:202-224), alignment test (voxelization.cpp:335-347),
//       k_expand_nodes         exact LIFO subdivision (voxelization.cpp:349-379) done breadth-first with an
//                              order key that reproduces the reference's processing order,
//       k_expand_big           tiles of <= 256 candidate voxels for large leaves
//   K2  k_voxelize<UV>         AABB walk + plane cull (voxelization.cpp:426-472) + six-plane clip by triangle
//                              splitting (voxelization.cpp:175-331,383-424).  A hit either goes straight into the
//                              64-bit max grid (MAX strategy, unsplit triangle: one atomicMax) or is
//                              appended to the hit pool and counted in its cell (atomicAdd on the dense grid -> rank)
//   K5  k_scan_flags/_bricks   reads the dirty bricks of the dense grid, compacts occupied cells, turns the
//                              per-cell counts into offsets (counting sort); k_scatter places the pooled hits
//   K3  k_resolve + tiers      per occupied cell: orders the hits like the reference's sequential loops
//                              (sub-voxel, triangle index, leaf order), replays insertWeighted
//                              (voxelization.cpp:56-63,466-468) and moveUvBufferIntoVoxels (:513-526) with
//                              MAX / BLEND, then packs (x, y, z, argb) (obj2voxel.cpp:279-297);
//       k_pick / k_emit_max    direct MAX path: winner colours of textured meshes; the 64-bit max grid -> records
//   K6  k_fill_*               O2V_HIP_FLAG_FILL_INTERIOR: parity crossings per column of the pass box, prefix XOR along z,
//                              the surface cells removed, interior records appended behind the surface records
//   K7  k_gather_tris, k_dense_* device-resident input (positions + faces) and dense output grids; outside the pipeline
//   K8  k_dist_*               o2v_hip_distance_dense: exact squared distance / SDF of a label grid; its header holds the row
//                              scan and the envelope that K15 and K21 run too (dt_*); outside the pipeline
//   K9  k_meshdist_*           o2v_hip_mesh_distance_dense: narrow-band distance to the triangles, signed by K6's parity set;
//                              outside the pipeline
//   K10 k_surf_*               o2v_hip_surface_count / _write: the level set of a float32 grid as an indexed mesh (surface
//                              nets); outside the pipeline
//   K11 k_ray_*                o2v_hip_raycast_build / o2v_hip_raycast: rays through a dense grid, a hierarchical walk over
//                              bit-packed occupancy; outside the pipeline
//   K12 k_cc_*                 o2v_hip_components_dense / o2v_hip_flood_dense: connected components and flood fill of a dense
//                              grid, a union-find over its voxels ; outside the pipeline
//   K13 k_gather_*             o2v_hip_gather_count / _write / _save: the solid voxels of a dense grid as (x, y, z, argb)
//                              records, in ranges, and as a voxel file; outside the pipeline
//   K14 k_faces_*              o2v_hip_faces_count / _write: the exposed voxel faces of a dense grid as coloured quads, merged
//                              into runs; outside the pipeline
//   K15 k_near_*               o2v_hip_nearest_dense: the nearest seed voxel of every voxel (K8's passes with the seed's
//                              coordinates as payload) and its value spread over the grid; outside the pipeline
//   K16 k_rects_*              O2V_HIP_FACES_MERGE_RECTS of K14's calls: equal runs of neighbouring rows stacked into
//                              rectangles; outside the pipeline
//   K17 k_downsample           o2v_hip_downsample: blocks of f^3 voxels of a dense grid merged into one coarse voxel each;
//                              outside the pipeline
//   K18 k_cross_*              o2v_hip_crossings_dense: signed crossing numbers of the triangles along x, y and z rays, from
//                              both ends of every line (K6's exact column test, keeping the sign); outside the pipeline
//   K19 k_label_stats          o2v_hip_label_stats: per value of a label grid its voxel count, bounding box, coordinate sums,
//                              second moments and exposed faces, one pass of runs into a table in LDS; outside the pipeline
//   K20 k_geo_*                o2v_hip_geodesic_dense / o2v_hip_geodesic_paths: shortest path lengths through the set of a dense
//                              grid, a relaxation tile by tile in LDS, round by round; the walk back; outside the pipeline
//   K21 k_thick_*              o2v_hip_thickness_dense: local thickness, opening and erosion by a ball - two of K8's distance
//                              transforms, a pruned list of ball centres, an atomicMax per ball voxel; outside the pipeline
//   K22 k_thin_*               o2v_hip_thin_dense: skeletons by topological thinning - eight subfields per iteration, a 26-voxel
//                              bit test per border voxel, tile by tile in LDS, in place on the bit grid; outside the pipeline
//   K23 k_ws_*                 o2v_hip_watershed_dense: watershed basins of an int32 relief by steepest ascent of a packed key, the
//                              adjacent basins through the pair table, merged by persistence on the host; outside the pipeline
//   K24 k_adj_*                o2v_hip_adjacency_count / _write: which labels of a label grid touch - per pair the face, edge and
//                              corner contacts and the two passes of a values grid, one pass of K19's chunks into a table in LDS
//                              and the pair table, sorted on the host; outside the pipeline
//   K26 k_oct_*              o2v_hip_octree_build / _write / _lookup / _to_dense: the sparse voxel octree of a dense grid - a
//                              pyramid of (valid, full) masks bottom-up, the nodes level by level top-down by scans, the descent
//                              per point and per 2^3 block; outside the pipeline
//   K27 k_open_*               o2v_hip_openness: in how many of D integer directions a voxel sees out of the grid - K11's masks built
//                              into scratch of its own, the targets compacted into a list, a lane per target walking one direction
//                              at a time in 32-bit integers, empty 4^3 / 16^3 / 64^3 blocks left in one exact skip; outside the pipeline
//   K28 k_grow_*               o2v_hip_grow_dense: seeded watershed - markers grown through an int32 relief by three fixed points (level,
//                              ticks, label), each K20's relaxation tile by tile in LDS, round by round, with a streaming pass that
//                              writes the next one's neighbour masks in between; outside the pipeline
//   K30 k_dag_*                o2v_hip_octree_dag_build / _write / _lookup / _to_dense: equal subtrees of an octree merged level by
//                              level, bottom up - a table of 256 smallest indices at level D - 1, an open-addressing table of node
//                              indices above, the classes ranked by scans -, the descent with per-pointer skips; outside the pipeline
//       k_pt_list              o2v_dev_pair_table.hpp: the table of id pairs in global memory of K23 and K24, its occupied slots as a list
//   plan k_zhist               o2v_hip_plan_slabs: predicted hits per z layer -> work-balanced slabs for N GPUs
// With the direct MAX path K1's counters reach the host while K2 runs, and only the stages that have work are enqueued
// behind it.  N > 1 GPUs: o2v_hip_voxelize_sharded (bounds / work-histogram passes sharded over the ranks, RCCL).
//
// Compile with -ffp-contract=off (see o2v_math.h).
#include "o2v_math.h"

#include "../../include/o2v_hip.h"
#include "o2v_comm.hpp"
#include "o2v_device_internal.hpp"
#include "o2v_io.hpp"

#ifndef O2V_BUILD_ID
#define O2V_BUILD_ID "unknown"  // the Makefile passes the hash of the device sources
#endif

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

using namespace o2v;

namespace {

#include "o2v_dev_common.hpp"
#include "o2v_dev_arith.hpp"
#include "o2v_dev_k0_bounds_plan.hpp"
#include "o2v_dev_k1_expand.hpp"
#include "o2v_dev_k2_voxelize.hpp"
#include "o2v_dev_k5_scan_scatter.hpp"
#include "o2v_dev_k3_resolve.hpp"
#include "o2v_dev_k6_fill.hpp"
#include "o2v_dev_k7_dense.hpp"
#include "o2v_dev_k9_mesh_distance.hpp"
#include "o2v_dev_k10_surface.hpp"
#include "o2v_dev_k11_raycast.hpp"
#include "o2v_dev_k8_distance.hpp"   // (behind K11: its seed test reads a set grid, K11's RaySource and kRay* formats)
#include "o2v_dev_bits.hpp"           // (the bit grid of K12, K13, K14, K16 and K20)
#include "o2v_dev_k12_components.hpp"
#include "o2v_dev_k13_gather.hpp"
#include "o2v_dev_k14_faces.hpp"
#include "o2v_dev_k16_rects.hpp"
#include "o2v_dev_k15_nearest.hpp"
#include "o2v_dev_k17_downsample.hpp"
#include "o2v_dev_k26_octree.hpp"      // (behind K12 and K6: the bit grid, the classify kernel, the block scan)
#include "o2v_dev_k30_dag.hpp"         // (behind K26: its octants, ranks and stored masks, its box of 2^3 blocks)
#include "o2v_dev_k31_treeray.hpp"     // (behind K11, K26 and K30: K11's ray and its advance, the steps of the two descents)
#include "o2v_dev_k27_openness.hpp"    // (behind K11: it walks the masks that k_ray_build makes)
#include "o2v_dev_k18_crossings.hpp"
#include "o2v_dev_k19_label_stats.hpp"
#include "o2v_dev_k20_geodesic.hpp"
#include "o2v_dev_k21_thickness.hpp"
#include "o2v_dev_k22_thinning.hpp"
#include "o2v_dev_pair_table.hpp"      // (the table of id pairs in global memory of K23 and K24)
#include "o2v_dev_k23_watershed.hpp"   // (behind K12: its grid, index and prefix count)
#include "o2v_dev_k24_adjacency.hpp"   // (behind K19: its chunk and its reads)
#include "o2v_dev_k25_euler.hpp"       // (behind K19: its chunk and its reads)
#include "o2v_dev_k28_grow.hpp"        // (behind K20 and the pair table: the offsets, see masks and tile flags; I32View)
#include "o2v_dev_k29_label_surface.hpp"   // (behind K10 and K6: its words, prefixes, search and select; the block scan)

}  // namespace

// ---- host side: context, buffers, launch sequence ------------------------------------------------------------

namespace {

// An array the context owns: device memory, or page-locked host memory (Pinned).  `cap` counts elements and is set only once
// its allocation succeeded; the memory is freed with the array.  Grown with grow / grow_keep (below), emptied with release.
template <typename T, bool Pinned = false>
struct DevArray {
    T *ptr = nullptr;
    uint64_t cap = 0;

    DevArray() = default;
    DevArray(DevArray &&o) noexcept : ptr(std::exchange(o.ptr, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevArray &operator=(DevArray &&o) noexcept { return std::swap(ptr, o.ptr), std::swap(cap, o.cap), *this; }
    ~DevArray() { (void) release(); }

    hipError_t release()
    {
        const hipError_t e = !ptr ? hipSuccess : Pinned ? hipHostFree(ptr) : hipFree(ptr);
        ptr = nullptr;
        cap = 0;
        return e;
    }
    // n elements in place of what the array held (which is lost)
    hipError_t alloc(uint64_t n)
    {
        if (const hipError_t e = release(); e != hipSuccess) return e;
        void *q = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, n * sizeof(T));
        if (e == hipSuccess) ptr = static_cast<T *>(q), cap = n;
        return e;
    }
};
template <typename T> using PinnedArray = DevArray<T, true>;

// An event and a stream the context owns, like its arrays: destroyed with it, read as the HIP handle they hold, made by the
// create calls (nothing if the handle exists).
struct Event {
    hipEvent_t h = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Event &operator=(Event &&o) noexcept { return std::swap(h, o.h), *this; }
    ~Event() { if (h) (void) hipEventDestroy(h); }
    operator hipEvent_t() const { return h; }
    // An event that is only ever used to read a time: without the system-scope fence a default event performs when it is
    // recorded (cache write-back and invalidation in the middle of the pass; nothing on the host reads device memory on its
    // strength).  Measured: the six stage events of a pass cost 0.009 ms less this way (bench headline, O2V_HIP_FLAG_STAGE_TIMES).
    hipError_t create_timing() { return h ? hipSuccess : hipEventCreateWithFlags(&h, hipEventDisableSystemFence); }
    // an event that only makes a stream or the host wait
    hipError_t create_sync() { return h ? hipSuccess : hipEventCreateWithFlags(&h, hipEventDisableTiming); }
};
struct Stream {
    hipStream_t h = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Stream &operator=(Stream &&o) noexcept { return std::swap(h, o.h), *this; }
    ~Stream() { if (h) (void) hipStreamDestroy(h); }
    operator hipStream_t() const { return h; }
    hipError_t create() { return h ? hipSuccess : hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
};

// Timing events around the N stages of a call and the stages' device times (ms) of the last call that finished.  mark(i) is
// where stage i begins (mark(N): where the last one ends); the first mark(0) creates the events, unless create did.
template <int N>
struct StageTimes {
    Event ev[N + 1];
    float ms[N] = {};

    hipError_t create()
    {
        for (Event &e : ev)
            if (const hipError_t r = e.create_timing(); r != hipSuccess) return r;
        return hipSuccess;
    }
    hipError_t mark(int i, hipStream_t s)
    {
        if (i == 0)
            if (const hipError_t r = create(); r != hipSuccess) return r;
        return hipEventRecord(ev[i], s);
    }
    // the time from mark(i) to mark(j), once the stream has passed mark(j)
    hipError_t elapsed(int i, int j, float &out_ms) const { return hipEventElapsedTime(&out_ms, ev[i], ev[j]); }
    // once the stream has passed mark(N)
    hipError_t finish()
    {
        for (int i = 0; i < N; ++i)
            if (const hipError_t r = elapsed(i, i + 1, ms[i]); r != hipSuccess) return r;
        return hipSuccess;
    }
    int read(float out_ms[N]) const
    {
        if (!out_ms) return O2V_HIP_ERR_BAD_ARGUMENT;
        std::copy(ms, ms + N, out_ms);
        return O2V_HIP_OK;
    }
};

constexpr uint64_t kStageTriangles = 1u << 16;  // per staging block: 2.25 MiB of vertices, 5 MiB with every optional array

// one page-locked staging block of the streamed upload (o2v_hip_begin / commit / end_triangles)
struct StageBlock {
    PinnedArray<float> verts, uvs, colors;
    PinnedArray<uint32_t> types;
    PinnedArray<int32_t> texids;
    o2v_hip_staging view() const { return {verts.ptr, uvs.ptr, types.ptr, colors.ptr, texids.ptr, verts.ptr ? kStageTriangles : 0u}; }
};

bool env_on(const char *name) { const char *e = std::getenv(name); return e && e[0] == '1'; }
int env_int(const char *name, int unset) { const char *e = std::getenv(name); return e ? std::atoi(e) : unset; }

// The environment switches that o2v_device.hip reads, all in one place.  They are read when a Switches is made - once at the
// entry of every C-ABI call that uses them (read_switches) - and handed down: the tests change them between the calls of one
// process.  O2V_DEBUG_SYNC (debug_sync_level: the launch macros) and O2V_INIT_TIMES (o2v_hip_create) are read where they are
// used.  A flag is on with the value 1.
struct Switches {
    bool exact_clip = env_on("O2V_EXACT_CLIP");                // user-facing: the clip kernel without its work-removal logic
    bool no_direct_max = env_on("O2V_NO_DIRECT_MAX");          // A/B: the MAX strategy through the general sort-and-replay route
    bool no_occupancy_only = env_on("O2V_NO_OCCUPANCY_ONLY");  // A/B: material-less meshes through the weighted routes
    bool no_crop = env_on("O2V_NO_CROP");                      // A/B: grids for the whole cube (grid_box)
    bool no_root_bypass = env_on("O2V_NO_ROOT_BYPASS");        // A/B: occupancy only, every leaf through its Leaf / Tile records
    bool count_roots = env_on("O2V_COUNT_ROOTS");              // A/B: k_count_roots ahead of k_expand_roots on the whole grid too
    bool no_count_roots = env_on("O2V_NO_COUNT_ROOTS");        // A/B: never k_count_roots
    bool no_solo_roots = env_on("O2V_NO_SOLO_ROOTS");          // A/B: k_expand_roots in every pass
    bool force_solo_roots = env_on("O2V_TEST_FORCE_SOLO_ROOTS");  // test hook: solo roots whatever the extent hint says
    bool all_launches = env_on("O2V_ALL_LAUNCHES");            // A/B: no launch left out on the strength of the upload's hints
    bool no_slabs = env_on("O2V_NO_SLABS");                    // A/B: no new hit slabs, every hit pooled
    bool ray_no_skip = env_on("O2V_RAY_NO_SKIP");              // A/B: k_ray_cast walks every fine cell, no empty block is skipped
    bool open_no_skip = env_on("O2V_OPEN_NO_SKIP");            // A/B: k_open_walk walks every fine cell, no empty block is skipped
    bool treeray_no_stack = env_on("O2V_TREERAY_NO_STACK");    // A/B: k_tree_cast keeps no ancestors in LDS, every event descends again from the root
    bool cc_no_tiles = env_on("O2V_CC_NO_TILES");              // A/B: no k_cc_tiles, every adjacent pair is united in global memory
    bool cross_no_tile = env_on("O2V_CROSS_NO_TILE");          // A/B: no k_cross_prefix_tile, a lane per line stores along the ray
    bool ls_no_table = env_on("O2V_LS_NO_TABLE");              // A/B: k_label_stats without its table in LDS, every run to global memory
    bool geo_no_tiles = env_on("O2V_GEO_NO_TILES");            // A/B: no k_geo_tiles, whole-grid sweeps with atomic mins in global memory
    bool grow_no_tiles = env_on("O2V_GROW_NO_TILES");          // A/B: no k_grow_tiles, every phase by whole-grid sweeps with the neighbours from global memory
    bool thin_no_tiles = env_on("O2V_THIN_NO_TILES");          // A/B: no k_thin_substep, every sub-step a whole-grid sweep with the masks from global memory
    bool ws_no_tiles = env_on("O2V_WS_NO_TILES");              // A/B: no k_ws_ascent_tiles, every voxel's neighbours from global memory and P[i] = the parent
    int ws_table_log2 = env_int("O2V_WS_TABLE_LOG2", 0);       // test hook: the pair table of K23 starts with 2^k slots (if > 0; else sized from the peaks)
    bool adj_no_table = env_on("O2V_ADJ_NO_TABLE");            // A/B: k_adj_pairs without its table in LDS, every flush to global memory
    bool eu_no_table = env_on("O2V_EU_NO_TABLE");              // A/B: k_euler without its table in LDS, every row to global memory
    bool lsf_no_tile = env_on("O2V_LSF_NO_TILE");              // A/B: k_lsf_classify, every label's neighbours at y + 1 and z + 1 re-read through L2, no tile in LDS
    int adj_table_log2 = env_int("O2V_ADJ_TABLE_LOG2", 0);     // test hook: the pair table of K24 starts with 2^k slots (if > 0; else sized from the labels)
    bool tiny_buffers = env_on("O2V_TEST_TINY_BUFFERS");       // test hook: minimal first capacities (every grow -> re-run path)
    bool block_list = env_on("O2V_TEST_BLOCK_LIST");           // test hook: the slab's block list for a mesh of any size
    int resolve_wgs_per_cu = env_int("O2V_RESOLVE_WGS_PER_CU", 0);  // A/B: workgroups per CU of resolve tier 1 (if > 0; else 2)
    bool force_collectives = env_on("O2V_TEST_FORCE_COLLECTIVES");  // test hook: a sharded run of one rank runs the collectives
    int fail_rank = env_int("O2V_TEST_FAIL_RANK", -1);         // test hook: this rank fails before the collectives
};
Switches read_switches() { return Switches{}; }

// The grid a _count call counted, by which its _write knows its own: the pointer, format, strides, dims and level of the call.
// The level is compared bit for bit, whatever the format reads of it.
struct GridKey {
    const void *p = nullptr;
    uint32_t format = 0;
    uint64_t strides[3] = {};
    uint32_t dims[3] = {};
    float level = 0.f;

    GridKey() = default;
    GridKey(const void *p_, uint32_t format_, const uint64_t strides_[3], const uint32_t dims_[3], float level_) : p(p_), format(format_), level(level_)
    {
        std::copy(strides_, strides_ + 3, strides);
        std::copy(dims_, dims_ + 3, dims);
    }
    bool operator==(const GridKey &o) const
    {
        return p == o.p && format == o.format && std::equal(strides, strides + 3, o.strides) && std::equal(dims, dims + 3, o.dims) &&
               std::memcmp(&level, &o.level, sizeof(float)) == 0;
    }
};

}  // namespace

struct o2v_hip_ctx {
    int device = 0;
    int num_cus = 256;
    Stream stream;
    StageTimes<5> pass_times;                    // the stages of a pass; made at once: k_voxelize's dispatch records events 2, 3 (O2V_LAUNCH_K2)
    StageTimes<1> coll_times;                    // sharded planning: around a collective
    DevArray<unsigned long long> d_counts;       // per-rank voxel counts (all-gathered), world entries
    PinnedArray<unsigned long long> h_counts;
    DevArray<uint32_t> d_status;                 // sharded runs: "this rank is ready" word, max-reduced over the ranks
    PinnedArray<uint32_t> h_status;
    std::string err;

    // inputs
    DevArray<float> d_verts, d_uvs, d_colors;
    DevArray<uint32_t> d_types;
    DevArray<int32_t> d_texids;
    uint64_t n_tris = 0;
    // streamed upload (o2v_hip_begin / commit / end_triangles): two page-locked staging blocks, filled in turn
    StageBlock stage[2];
    Event ev_stage[2];
    int stage_cur = 0;
    uint64_t stream_count = 0;
    uint32_t stream_arrays = 0;
    std::vector<DevArray<uint8_t>> retired;  // device arrays replaced by larger ones while a streamed upload was in flight
    bool any_textured = false;
    DevArray<DevTexture> d_textures;
    std::vector<DevArray<uint8_t>> d_texpix;
    uint32_t n_textures = 0;

    // work buffers (grown on demand)
    DevArray<Counters> d_ctr;
    PinnedArray<Counters> h_ctr;
    bool stage_events = false;  // this call records an event between the stages of a pass (O2V_HIP_FLAG_STAGE_TIMES)
    uint64_t no_pool_key = 0;   // (key + 1 of) the mesh and settings whose last pass pooled no hits (run_pass: k_mark_bricks left out)
    bool marked_bricks = false, mark_missing = false; // the current pass listed its bricks before k_voxelize
    bool skip_big = false;      // no leaf of the uploaded mesh can have more than four tiles (its largest triangle's extent): k_expand_big left out
    bool poisoned = false;      // a collective of a sharded run is stuck on the stream (time limit passed): o2v_hip_destroy must not wait for it
    bool ctr_clean = false;     // d_ctr was zeroed (k_init) behind the last pass and nothing has touched it since
    Stream aux[3];                    // the cooperative resolve tiers run beside tier 1
    Event ev_fork, ev_sorted, ev_join[3];
    DevArray<unsigned long long> d_zhist;        // kPlanBins, o2v_hip_plan_slabs
    PinnedArray<unsigned long long> h_zhist;
    DevArray<float2> d_zrange;                   // z extent per 256 triangles, written by the slab plan
    DevArray<unsigned long long> d_plan_gather;  // sharded runs: one record per rank (k_pack_plan), all-gathered
    DevArray<float> d_zrange_xform;              // the transform they were computed with (12 floats)
    DevArray<uint32_t> d_block_list;             // the blocks of 256 triangles that meet the slab (k_list_blocks)
    uint32_t *d_block_count = nullptr;           // ... their number: a word of d_ctr
    DevArray<uint32_t> d_need_list;              // k_count_roots: the blocks k_expand_roots still has to walk
    bool lean_roots = false;          // this call: k_count_roots ahead of k_expand_roots (choose_routes)
    bool solo_roots = false;          // this call: no k_expand_roots at all, k_voxelize_occ counts the root leaves itself (plan_rounds)
    uint64_t solo_refused_key = 0;    // the mesh and settings for which a solo pass found a triangle that needs k_expand_roots
    float mesh_bounds_hint[6] = {0, 0, 0, 0, 0, 0};  // bounds of the uploaded mesh, k_bounds' own result at the upload (or another rank's,
                                                     // TriHints): they place the dense grids (grid_box), scale the estimates from the
                                                     // hints (mesh_scale) and, on the occupancy-only route, are the bounds of the pass
                                                     // itself (host_transform, o2v_hip_voxelize: no k_bounds, no k_setup)
    uint64_t bounds_generation = ~0ull;              // ... valid while this equals tri_generation (ctx_finish_triangles sets it, whatever
                                                     // replaces or appends triangles clears it)
    float max_tri_extent = -1.f;                     // largest triangle extent of the uploaded mesh: bounds the number of subdivision
                                                     // rounds (-1: unknown)
    uint32_t ext_hist[256] = {};                     // k_tri_extent: the uploaded mesh's triangles by the binary exponent of their extent
                                                     // (grid_modes: is the 64-bit max grid worth its memory?)
    uint64_t tri_generation = 0, zrange_generation = ~0ull;  // the extents belong to the triangles of that upload
    DevArray<Leaf> d_leaves;
    DevArray<Tile> d_tiles;
    DevArray<BigLeaf> d_big;
    DevArray<Node> d_nodes[2];
    DevArray<uint2> d_jobq;  // k_voxelize's job queues: VoxShape::queue records per workgroup
    DevArray<HitRec> d_pool;
    DevArray<SortedRec> d_sorted;  // (read through SortedView: 24 or 16 bytes per record)
    uint32_t sorted_stride = 6;
    DevArray<Occ> d_occ;
    DevArray<uint4> d_out;
    DevArray<uint32_t> d_list_lane8, d_list_lane16, d_list_w64, d_list_lane, d_list_mid, d_list_long, d_list_big, d_list_huge;
    DevArray<uint64_t> d_scratch_key;  // tier-4 resolve scratch, allocated on first need
    DevArray<uint32_t> d_scratch_idx;

    // dense grid of list heads for this context's slab
    DevArray<uint32_t> d_grid;
    DevArray<uint8_t> d_brick_dirty;    // one flag per brick (padded to 16 bytes)
    DevArray<uint32_t> d_dirty_list;    // dirty brick ids of the current run
    DevArray<uint32_t> d_brick_slab;    // per brick: its place in that list = the number of its hit slab (Params::brick_slab)
    DevArray<uint32_t> d_slabs;         // cap_slabs() x kInlineHits x 64 hit records (slabs_stride dwords each)
    uint32_t slabs_stride = 0;
    uint64_t want_slabs_next = 0;       // the brick list of the last pass (+ 1/8): what the slabs are grown to at the next call
    uint64_t slabs_wanted_at_grant = 0; // what was asked for when the slabs were last allocated (they may have got less: the memory was short)
    DevArray<PickRec> d_pick_extra;     // textured MAX: {cell, key, argb} of the cells resolved by replay (6 words each)
    DevArray<uint8_t> d_maxgrid;        // direct MAX path: one 64-bit cell per output voxel (same bricked layout), or one byte
    DevArray<uint8_t> d_dirty_max;      // ... its dirty-brick flags and list
    DevArray<uint32_t> d_dirty_list_max;
    Event ev_k1;                        // after K1: its counters decide which stages follow k_voxelize
    // solid fill (O2V_HIP_FLAG_FILL_INTERIOR, K6): allocated by the first call that asks for it
    DevArray<uint32_t> d_fill_bits;              // toggle bitmap of the pass box, [z-word][y][x]
    DevArray<unsigned long long> d_fill_ends;    // per triangle: inclusive end of its (triangle, column) items
    DevArray<unsigned long long> d_fill_blocks;  // per block of kBlock triangles: its items' offset
    DevArray<unsigned long long> d_fill_chunks;  // per chunk of kFillChunk bitmap words: its records' offset
    DevArray<unsigned long long> d_fill_ctr;     // [0] items, [1] interior voxels, [2] the mesh's top (f2ord of its largest z)
    PinnedArray<unsigned long long> h_fill_ctr;
    StageTimes<1> fill_times;                    // of the stage (O2V_HIP_FLAG_STAGE_TIMES)
    bool maxgrid_dirty = false;
    bool grid_dirty = false;
    // K7 (o2v_hip_set_triangles_device, o2v_hip_write_dense, o2v_hip_voxels_box): flags and sums, allocated on first use
    DevArray<DenseCtr> d_dense;
    PinnedArray<DenseCtr> h_dense;
    // K8 (o2v_hip_distance_dense): the envelope stacks, grown on demand; the times of the three passes
    DevArray<uint2> d_dist_stack;
    StageTimes<3> dist_times;
    // K15 (o2v_hip_nearest_dense): its envelope stacks are K8's (d_dist_stack); the times of its three passes
    StageTimes<3> near_times;
    // K9 (o2v_hip_mesh_distance_dense): sample-space vertices, per-tile counters, offsets and triangle lists, grown on demand;
    // the times of the three stages
    DevArray<float> d_md_sv;
    DevArray<uint32_t> d_md_counts, d_md_lists;
    DevArray<unsigned long long> d_md_first, d_md_blocks, d_md_ctr;
    PinnedArray<unsigned long long> h_md_ctr;
    StageTimes<3> md_times;
    // K10 (o2v_hip_surface_count / _write): per word of 64 samples its sign bits, active cells and block-local prefixes, per
    // block of words the vertex and quad offsets, grown on demand; the grid they were counted for; the times of the four stages
    DevArray<unsigned long long> d_sf_signs, d_sf_active, d_sf_voff, d_sf_qoff;
    DevArray<uint32_t> d_sf_local;
    PinnedArray<unsigned long long> h_sf_ctr;
    StageTimes<4> sf_times;
    struct SurfaceCount {
        bool valid = false;
        GridKey key;   // (the field; format 0)
        uint64_t vertices = 0, quads = 0;
    } sf;
    // K11 (o2v_hip_raycast_build / o2v_hip_raycast): the snapshot of the last build - the words of the 4^3 bricks, then of the
    // 16^3 and the 64^3 blocks, in one array - and its identity; the times of the last build and the last cast
    DevArray<unsigned long long> d_ray_masks;
    StageTimes<1> ray_build_times, ray_cast_times;
    struct RaySnapshot {
        bool valid = false;
        uint32_t dims[3] = {}, origin[3] = {};
        uint64_t generation = 0;   // counts the builds, refused ones included
    } ray;

    // K12 (o2v_hip_components_dense / o2v_hip_flood_dense): the bits of the set, the root flags (labels) or seed flags (flood),
    // the per-word prefixes and block offsets of the root count, the parents where they cannot live in the caller's labels, grown
    // on demand; [0] unions, [1] retries, [2] reached; the times of the five stages and the two counters of the last call
    DevArray<unsigned long long> d_cc_bits, d_cc_flags, d_cc_boff, d_cc_ctr;
    DevArray<uint32_t> d_cc_local, d_cc_parent;
    PinnedArray<unsigned long long> h_cc_ctr;
    StageTimes<5> cc_times;
    uint64_t cc_counters[2] = {};

    // K13 (o2v_hip_gather_count / _write / _save): the bits of the set, the per-word prefixes, the block offsets (+ the count)
    // and the block of a range's first record, grown on demand; the grid they were counted for; the two record buffers and
    // page-locked batches of _save (allocated by its first call); the times of the three stages
    DevArray<unsigned long long> d_ga_bits, d_ga_boff, d_ga_first;
    DevArray<uint32_t> d_ga_local;
    PinnedArray<unsigned long long> h_ga_ctr;
    DevArray<uint4> d_ga_rec[2];
    PinnedArray<uint32_t> h_ga_rec[2];
    Event ev_ga_rec[2];
    StageTimes<3> ga_times;
    struct GatherCount {
        bool valid = false;
        GridKey key;
        uint64_t total = 0;
    } ga;
    // K13 and K14, O2V_HIP_GATHER_COLOR_PALETTE: the palette of the call that is running (upload_palette), allocated on first use
    DevArray<uint32_t> d_palette;
    PinnedArray<uint32_t> h_palette;

    // K14 (o2v_hip_faces_count / _write): the bits of the set, the same-colour bits along x and y (GRID / PALETTE with
    // MERGE_RUNS) and the block offsets (+ the count), grown on demand; what they were counted for; the times of the three
    // stages
    DevArray<unsigned long long> d_fa_bits, d_fa_same_x, d_fa_same_y, d_fa_boff;
    PinnedArray<unsigned long long> h_fa_ctr;
    StageTimes<3> fa_times;
    // K16 (O2V_HIP_FACES_MERGE_RECTS): the same-colour bits along z (GRID / PALETTE) and the kept rectangle-start masks, a
    // word per item; grown only by a count with that merge mode
    DevArray<unsigned long long> d_rc_same_z, d_rc_starts;
    struct FacesCount {
        bool valid = false;
        GridKey key;
        const void *colors = nullptr;
        uint32_t merge = 0, color_mode = 0, argb = 0;
        uint64_t color_strides[3] = {};
        uint32_t palette[256] = {};
        uint64_t total = 0;
    } fa;
    // K17 (o2v_hip_downsample): no scratch; the time of the one launch
    StageTimes<1> ds_times;
    // K18 (o2v_hip_crossings_dense): the delta grid of the box ([w][line]) and the totals per line of the axis in work, per
    // triangle the inclusive end of its (triangle, line) items, per block of kBlock triangles its items' offset, the number of
    // items, grown on demand; the times of the three axes
    DevArray<int32_t> d_cr_delta, d_cr_totals;
    DevArray<unsigned long long> d_cr_ends, d_cr_blocks, d_cr_ctr;
    StageTimes<3> cr_times;
    // K19 (o2v_hip_label_stats): the number of voxels outside [0, n_labels]; the times of the initialisation and of the pass
    DevArray<unsigned long long> d_ls_ctr;
    PinnedArray<unsigned long long> h_ls_ctr;
    StageTimes<2> ls_times;
    // K20 (o2v_hip_geodesic_dense / o2v_hip_geodesic_paths): the bits of the set; per tile its flag words of two rounds and its
    // places in the two rounds' lists ([4][tiles]); the distances where they cannot live in the caller's dist; [0] in-tile
    // sweeps, [1] reached, then as uint32 the two lists' lengths and the changed word; grown on demand; the times of the four
    // stages and the four counters of the last call
    DevArray<unsigned long long> d_geo_bits, d_geo_ctr;
    DevArray<uint32_t> d_geo_tiles, d_geo_dist;
    PinnedArray<unsigned long long> h_geo_ctr;
    StageTimes<4> geo_times;
    uint64_t geo_counters[4] = {};
    // K21 (o2v_hip_thickness_dense): the depth grid where the caller passes none, the block offsets (+ the count) and the list
    // of the kept ball centres, [0] candidates, [2] ball voxels visited, grown on demand; the envelope stacks are K8's
    // (d_dist_stack); the cover table of the last cap, on the device and page-locked; the times of the five stages and the
    // three counters of the last call
    DevArray<int32_t> d_thick_depth, d_thick_list;
    DevArray<unsigned long long> d_thick_boff, d_thick_ctr;
    PinnedArray<unsigned long long> h_thick_ctr;
    DevArray<uint32_t> d_thick_table;
    PinnedArray<uint32_t> h_thick_table;
    uint32_t thick_table_cap = 0;
    StageTimes<5> thick_times;
    uint64_t thick_counters[3] = {};
    // K22 (o2v_hip_thin_dense): the bits of the set, of its border voxels and of `keep` ([2 or 3][words]); per tile its stamps of
    // the last odd and the last even iteration with a removal in view ([2][tiles]); [0] voxels removed, [1] tile turns; grown on
    // demand; the times of the three stages and the four counters of the last call
    DevArray<unsigned long long> d_thin_bits, d_thin_ctr;
    DevArray<uint32_t> d_thin_stamps;
    PinnedArray<unsigned long long> h_thin_ctr;
    StageTimes<3> thin_times;
    uint64_t thin_counters[4] = {};
    // K23 (o2v_hip_watershed_dense): a parent per voxel, the peak bits with their prefixes and block offsets (+ the count), [0]
    // overflow, [1] distinct pairs, [2] boundary pairs seen, [3] listed pairs - fixed by the box; the peaks' indices and heights
    // ([2][peaks]), label_of_rank, the pair table's keys and values and its entries as a list (keys, then values), on the device
    // and page-locked - grown with the data; the times of the five stages and the six counters of the last call
    DevArray<uint32_t> d_ws_parent, d_ws_local, d_ws_peaks, d_ws_vals;
    DevArray<unsigned long long> d_ws_flags, d_ws_boff, d_ws_ctr, d_ws_keys, d_ws_list;
    DevArray<int32_t> d_ws_lab;
    PinnedArray<unsigned long long> h_ws_ctr, h_ws_list;
    PinnedArray<uint32_t> h_ws_peaks;
    PinnedArray<int32_t> h_ws_lab;
    StageTimes<5> ws_times;
    uint64_t ws_counters[6] = {};
    // K28 (o2v_hip_grow_dense): the neighbour masks (4 bytes a voxel); Q, T and L where they cannot live in the caller's level,
    // ticks and labels; per tile its flag words of two rounds and its places in the two rounds' lists ([4][tiles]); [0 .. 2] the
    // in-tile sweeps per phase, [3] reached, then as uint32 the two lists' lengths and the changed word; grown on demand; the
    // times of the seven stages and the nine counters of the last call
    DevArray<uint32_t> d_grow_mask, d_grow_q, d_grow_t, d_grow_l, d_grow_tiles;
    DevArray<unsigned long long> d_grow_ctr;
    PinnedArray<unsigned long long> h_grow_ctr;
    StageTimes<7> grow_times;
    uint64_t grow_counters[9] = {};
    // K24 (o2v_hip_adjacency_count / _write): the pair table's keys and rows ([slots], [slots][5]); [0] overflow, [1] voxels outside,
    // [2] flushes into LDS, [3] flushes to global memory, [4] listed pairs, [5] slots taken; the list - keys [m] and rows [m][5] as
    // the table gives them, then pairs [m][2] and rows sorted by key - on the device and page-locked (both orders); grown with the
    // data; the times of the four stages and the four counters of the last count, whether one stands, and its pairs
    DevArray<unsigned long long> d_adj_keys, d_adj_ctr, d_adj_list;
    DevArray<long long> d_adj_rows;
    PinnedArray<unsigned long long> h_adj_ctr, h_adj_list;
    StageTimes<4> adj_times;
    uint64_t adj_counters[4] = {};
    uint64_t adj_pairs = 0;
    bool adj_counted = false;
    // K25 (o2v_hip_euler_stats): the number of voxels outside [0, n_labels]; the times of the initialisation and of the pass
    DevArray<unsigned long long> d_eu_ctr;
    PinnedArray<unsigned long long> h_eu_ctr;
    StageTimes<2> eu_times;
    // K26 (o2v_hip_octree_build / _write): the bits of the set, the pyramid (an entry valid | full << 8 per touched cell, level by
    // level), the counters (kOctMeta words) and the block offsets of a level's scan - fixed by the box; the node arrays - grown with
    // the data; what the last build was made of; the times of classify, pyramid and order (events 0 - 2 and 3 - 4 of oct_times:
    // the host waits between them) and of the last write
    DevArray<unsigned long long> d_oct_bits, d_oct_meta, d_oct_boff;
    DevArray<uint16_t> d_oct_pyr;
    DevArray<uint8_t> d_oct_valid, d_oct_full;
    DevArray<int32_t> d_oct_first, d_oct_coords;
    PinnedArray<unsigned long long> h_oct_meta;
    StageTimes<4> oct_times;
    StageTimes<1> oct_write_times;
    struct OctreeBuild {
        bool valid = false;
        GridKey key;
        uint32_t origin[3] = {}, depth = 0, flags = 0;
        uint64_t nodes = 0, voxels = 0;
    } oct;
    // K30 (o2v_hip_octree_dag_build / _write): per tree node its class and its listed voxels, per node of the widest level the
    // block-local scans, the table of node indices (at least the 256 entries of level D - 1), the block offsets of a level's scan
    // and the counters (kDagMeta words) - fixed by the level counts; the DAG's arrays - grown with the data; what the last build
    // made; the times of level D - 1, the levels above and the output (events 0 - 2 and 3 - 4 of dag_times: the host waits between
    // them) and of the last write
    DevArray<uint32_t> d_dag_cls, d_dag_listed, d_dag_num, d_dag_tab;
    DevArray<unsigned long long> d_dag_boff, d_dag_meta;
    DevArray<uint8_t> d_dag_valid, d_dag_full;
    DevArray<int32_t> d_dag_first, d_dag_child, d_dag_skip;
    PinnedArray<unsigned long long> h_dag_meta;
    StageTimes<4> dag_times;
    StageTimes<1> dag_write_times;
    struct DagBuild {
        bool valid = false;
        uint64_t nodes = 0, pointers = 0;
    } dag;
    // K31 (o2v_hip_octree_raycast / o2v_hip_octree_dag_raycast): no scratch - the caller's arrays are walked in place; the time of the last cast
    StageTimes<1> treeray_times;
    // K27 (o2v_hip_openness): the three levels of masks of its own (a RayCaster's snapshot is not touched), the counters (targets
    // counted, targets listed), the direction table (nine words per direction) on both sides, the list of the targets' linear
    // indices - grown with the data; the times of build, targets and walk
    DevArray<unsigned long long> d_open_masks, d_open_ctr;
    PinnedArray<unsigned long long> h_open_ctr;
    DevArray<uint32_t> d_open_dirs, d_open_list;
    PinnedArray<uint32_t> h_open_dirs;
    StageTimes<3> open_times;
    // K29 (o2v_hip_label_surface_count / _write / _relax): per word of 64 extended samples its three difference words (x, y, z: one
    // array, three parts), active cells and block-local prefixes, per block of words the vertex and quad offsets; the second
    // position buffer of the relaxation - all grown on demand; the grid they were counted for; the times of the five stages
    DevArray<unsigned long long> d_lsf_diff, d_lsf_active, d_lsf_voff, d_lsf_qoff;
    DevArray<uint32_t> d_lsf_local;
    DevArray<float> d_lsf_pos;
    PinnedArray<unsigned long long> h_lsf_ctr;
    StageTimes<5> lsf_times;
    SurfaceCount lsf;   // (the labels; format | flags << 8)

    // results of the last run
    uint64_t n_vox = 0;
    bool last_ran_general = true;  // the last pass enqueued the counting sort + replay stages
    bool force_general = false;    // ... must do so whatever K1's counters say (set if the shortcut's premise did not hold)
    bool last_direct = false;  // the last run used the 64-bit max grid: occ[] / sorted[] do not describe every voxel
    o2v_hip_timings timings = {};
    o2v_hip_stats stats = {};
    float xform[12] = {};
    uint64_t dbg[16] = {};  // Counters::dbg of the last run (instrumented builds only)

    // O2V_HIP_FLAG_KERNEL_TIMES: an event pair around every launch of a pass
    struct KernelBracket {
        const char *name = nullptr;
        StageTimes<1> times;
    };
    std::vector<KernelBracket> ktimes;
    size_t ktimes_used = 0;
    bool ktimes_on = false;
    std::vector<o2v_hip_kernel_time> kernel_times;  // of the last run: one entry per kernel name

    // hit slabs held, in slabs of the current record size
    uint32_t cap_slabs() const { return slabs_stride ? (uint32_t) (d_slabs.cap / ((uint64_t) kInlineHits * kBrickCells * slabs_stride)) : 0u; }
};

namespace {

#define O2V_CHECK(expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) {                                                                           \
            ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_);                                 \
            return e_ == hipErrorOutOfMemory ? O2V_HIP_ERR_OUT_OF_MEMORY : O2V_HIP_ERR_HIP;               \
        }                                                                                                 \
    } while (0)

constexpr uint64_t kMaxRecords = 0xfffffff0ull;  // the arrays whose capacity goes into Params (32-bit)
constexpr uint64_t kNoLimit = ~0ull;

// Room for `want` elements; what the array held is lost if it has to grow.
template <typename T, bool P>
int grow(o2v_hip_ctx *ctx, DevArray<T, P> &a, uint64_t want, uint64_t max_records = kMaxRecords)
{
    if (want <= a.cap && a.ptr) return O2V_HIP_OK;
    if (want > max_records) {
        ctx->err = "device buffer would exceed 2^32 records";
        return O2V_HIP_ERR_LIMIT;
    }
    O2V_CHECK(a.alloc(want));
    return O2V_HIP_OK;
}

// Keeps an array the stream may still be reading until o2v_hip_end_triangles has waited for the stream; `a` is left empty.
template <typename T>
void retire(o2v_hip_ctx *ctx, DevArray<T> &a)
{
    if (a.ptr) ctx->retired.emplace_back().ptr = reinterpret_cast<uint8_t *>(std::exchange(a.ptr, nullptr));  // (freed as bytes)
    a.cap = 0;
}

// Room for `need` elements in an array that already holds `have` valid ones (copied over on the stream if it has to move).
template <typename T>
int grow_keep(o2v_hip_ctx *ctx, DevArray<T> &a, uint64_t have, uint64_t need, uint64_t floor_elems)
{
    if (a.ptr && need <= a.cap) return O2V_HIP_OK;
    // (floor_elems: room for 2^20 triangles from the start, so that a streamed mesh does not pay for a chain of allocations
    // and device-to-device moves)
    DevArray<T> bigger;
    O2V_CHECK(bigger.alloc(std::max<uint64_t>(std::max<uint64_t>(need, 2 * a.cap), floor_elems)));
    if (a.ptr && have) O2V_CHECK(hipMemcpyAsync(bigger.ptr, a.ptr, have * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    retire(ctx, a);
    a = std::move(bigger);
    return O2V_HIP_OK;
}

// O2V_DEBUG_SYNC=1: synchronise and log after every launch (locates a faulting or hanging kernel); the resolve tiers
// then run on one stream.  O2V_DEBUG_SYNC=2: the same, but the tiers keep their own streams (device-wide sync).
int debug_sync_level()
{
    static const int level = [] {
        const char *e = std::getenv("O2V_DEBUG_SYNC");
        return e && (e[0] == '1' || e[0] == '2') ? e[0] - '0' : 0;
    }();
    return level;
}
bool debug_sync_enabled() { return debug_sync_level() != 0; }
#define O2V_STAGE(name)                                                          \
    do {                                                                         \
        if (debug_sync_enabled()) {                                              \
            std::fprintf(stderr, "[o2v] launched %s ...", name);                 \
            std::fflush(stderr);                                                 \
            hipError_t e_ = debug_sync_level() == 2 ? hipDeviceSynchronize() : hipStreamSynchronize(s); \
            std::fprintf(stderr, " %s\n", hipGetErrorString(e_));                \
        }                                                                        \
    } while (0)

// One kernel launch.  Within o2v_hip_voxelize with O2V_HIP_FLAG_KERNEL_TIMES (KernelTimesScope) the launch is bracketed by two
// events on the stream it goes to (o2v_hip_get_kernel_times; the brackets cost a few microseconds per launch, so bench.py
// times its steps without the flag and collects the per-kernel times in extra steps).
#define O2V_LAUNCH(name, stream, ...)                                            \
    do {                                                                         \
        const int kt_ = ktime_begin(ctx, name, stream);                          \
        hipLaunchKernelGGL(__VA_ARGS__);                                         \
        if (kt_ >= 0) (void) ctx->ktimes[(size_t) kt_].times.mark(1, stream);   \
        O2V_STAGE(name);                                                         \
    } while (0)

// k_voxelize's launch: without the stage events (the default) its duration is still measured, by two events that ride on the
// kernel's own dispatch (hipExtLaunchKernelGGL: the start and end times of that dispatch).  Measured on the bench headline, per
// step: these two 0.004 - 0.006 ms together, an event recorded on the stream between two kernels ~0.004 ms each - the six of
// O2V_HIP_FLAG_STAGE_TIMES 0.02 - 0.025 ms of a 0.5 ms step (profiles/r05/NOTES.md).
#define O2V_LAUNCH_K2(name, kernel, grid, block, ...)                                                               \
    do {                                                                                                            \
        if (ctx->stage_events || ctx->ktimes_on) O2V_LAUNCH(name, s, kernel, grid, block, 0, s, __VA_ARGS__);       \
        else {                                                                                                      \
            hipExtLaunchKernelGGL(kernel, grid, block, 0, s, ctx->pass_times.ev[2], ctx->pass_times.ev[3], 0,           \
                                  __VA_ARGS__);                                                                     \
            O2V_STAGE(name);                                                                                        \
        }                                                                                                           \
    } while (0)

int ktime_begin(o2v_hip_ctx *ctx, const char *name, hipStream_t stream)
{
    if (!ctx->ktimes_on) return -1;
    if (ctx->ktimes_used == ctx->ktimes.size()) ctx->ktimes.emplace_back();
    o2v_hip_ctx::KernelBracket &b = ctx->ktimes[ctx->ktimes_used];
    b.name = name;
    if (b.times.mark(0, stream) != hipSuccess) return -1;
    return (int) ctx->ktimes_used++;
}

float ord2f_host(uint32_t o)
{
    const uint32_t b = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// The mesh's scale as the estimates from the upload's hints see it: the longest axis of the bounds in effect (the caller's,
// or the mesh's own) and the norm of the unit transform (its largest absolute row sum) - the mesh transform's scale is
// norm x S / longest axis (obj2voxel.cpp:370-402).  Each caller combines them in its own order of operations: the estimates
// feed thresholds.
struct MeshScale {
    float max_axis, unit_norm;
};
MeshScale mesh_scale(const o2v_hip_ctx *ctx, const o2v_hip_params *params)
{
    const float *b = params->bounds_known ? params->bounds : ctx->mesh_bounds_hint;
    MeshScale m;
    m.max_axis = std::max(b[3] - b[0], std::max(b[4] - b[1], b[5] - b[2]));
    m.unit_norm = 0.f;
    for (int i = 0; i < 3; ++i)
        m.unit_norm = std::max(m.unit_norm, std::fabs((float) params->unit_transform[i * 3]) + std::fabs((float) params->unit_transform[i * 3 + 1]) +
                                                std::fabs((float) params->unit_transform[i * 3 + 2]));
    return m;
}

// Which runs take the occupancy-only mode (Params::occupancy_only) and the direct MAX path: decided in one place, for the
// run itself (choose_routes) and for the memory estimate of o2v_hip_max_slab_layers (1 byte per cell against 4 + 8).
struct GridModes {
    bool use_uv, exact_clip, occupancy_only, direct_max;
};
GridModes grid_modes(const o2v_hip_ctx *ctx, const o2v_hip_params *params, const Switches &sw)
{
    GridModes g;
    g.use_uv = ctx->d_uvs.ptr && ctx->any_textured;
    g.exact_clip = (params->flags & O2V_HIP_FLAG_EXACT_CLIP) || sw.exact_clip;
    // occupancy-only mode: no triangle has a material, so the result is the set of hit voxels, all white, with either
    // strategy.  Not in exact mode: the fast-vs-exact comparison covers this shortcut too.
    g.occupancy_only = !ctx->d_types.ptr && !g.use_uv && !g.exact_clip && !sw.no_direct_max && !sw.no_occupancy_only;
    // Direct MAX path: MAX strategy; with textured triangles in its "pick" variant
    g.direct_max = (params->strategy == 0u || g.occupancy_only) && !sw.no_direct_max;
    // ... unless most of the mesh will be subdivided anyway: the direct path then stays unused (direct_active() on the device:
    // at most half of the triangles subdivided) while its 64-bit grid takes two thirds of the grids' memory - 29 GB of 43 for the
    // reference README's 8192^3 showcase (19 k large triangles), allocated and zeroed for nothing.  Estimated from the
    // triangles' extents, known since the upload (k_tri_extent): a triangle 16 voxels or more across is subdivided as a rule
    // (a voxel box of 512 cells and more, voxelization.cpp:357-361, unless it is a sliver or axis-aligned).  Either way the
    // result is the same; only which route computes it, and what it needs of the device, changes.
    if (g.direct_max && !g.occupancy_only && ctx->max_tri_extent >= 0.f && ctx->n_tris) {
        const MeshScale m = mesh_scale(ctx, params);
        const uint32_t ss = params->supersampling ? params->supersampling : 1u;
        const float voxels_per_unit = m.unit_norm * (float) (params->resolution * ss) / m.max_axis;
        if (m.max_axis > 0.f && std::isfinite(voxels_per_unit) && voxels_per_unit > 0.f) {
            uint64_t large = 0;
            for (uint32_t e = 1; e < 255; ++e)   // bin e: extents in [2^(e-127), 2^(e-126))
                if (std::ldexp(1.0f, (int) e - 127) * voxels_per_unit >= 16.0f) large += ctx->ext_hist[e];
            large += ctx->ext_hist[255];          // (infinite / NaN extents: such triangles are subdivided until they vanish)
            if (large * 4 > ctx->n_tris * 3) g.direct_max = false;
        }
    }
    return g;
}

// The memory of a dense grid per brick: its cells, and beside them the brick's dirty flag, its entry in the dirty-brick list
// and - the counter grid - the number of its hit slab (Params::brick_slab).  The allocations (ensure_count_grid,
// ensure_max_grid) and the estimate of o2v_hip_max_slab_layers both follow it.
enum class Grid { counter, max64, occupancy };
struct GridBytes {
    uint64_t cells, flag, list, slab;
    uint64_t side() const { return flag + list + slab; }
    uint64_t total() const { return cells + side(); }
};
GridBytes grid_bytes(Grid g)
{
    const uint64_t cell = g == Grid::counter ? sizeof(uint32_t) : g == Grid::max64 ? sizeof(unsigned long long) : 1u;
    return GridBytes{kBrickCells * cell, 1u, sizeof(uint32_t), g == Grid::counter ? sizeof(uint32_t) : 0u};
}

// The part of the output grid the dense grids are allocated for: the mesh's voxel bounding box, not the G^3 cube - the
// reference's VoxelMap only ever holds the chunks the mesh touches (util.hpp:179-208), and a long thin model at a high
// resolution (the reference README's showcase: r = 8192) fills a small fraction of the cube.  From the bounds of the
// uploaded mesh (known since the upload: ctx->mesh_bounds_hint) and the same transform k_setup computes on the device
// (compute_mesh_transform of the bounds in effect: the caller's, or the mesh's own): the eight corners of the mesh's box,
// transformed, one voxel of margin either side, in output space rounded outwards to whole bricks in x and y and cut to
// the slab in z.  A mesh whose bounds are unknown or not finite gets the whole cube.  O2V_NO_CROP=1: always the cube (A/B).
struct GridBox {
    uint32_t lo[3], hi[3];  // output space, [lo, hi); lo[0], lo[1] multiples of the brick edge
    bool empty;             // the slab does not meet the mesh's box: nothing to voxelize
};

// The bounds in effect of a call where the host knows them - the caller's, else the upload's while they belong to the uploaded
// triangles (ctx->bounds_generation) - and the mesh transform from them: compute_mesh_transform gives the same floats on the host
// as in k_setup (-ffp-contract=off; o2v_math.h).  Computed once per call: grid_box places the grids with it, and on the
// occupancy-only route the kernels get it as an argument (Params::xform; o2v_hip_voxelize).
struct HostTransform {
    bool have = false;    // bounds[] and a are set
    bool finite = false;  // ... and all six bounds are finite
    float bounds[6] = {};
    Affine a{};
};
bool upload_bounds_valid(const o2v_hip_ctx *ctx) { return ctx->bounds_generation == ctx->tri_generation; }
HostTransform host_transform(const o2v_hip_ctx *ctx, const o2v_hip_params *params, uint32_t S)
{
    HostTransform t;
    const float *e = params->bounds_known ? params->bounds : upload_bounds_valid(ctx) ? ctx->mesh_bounds_hint : nullptr;
    if (!e || ctx->n_tris == 0) return t;
    t.have = t.finite = true;
    for (int i = 0; i < 6; ++i) {
        t.bounds[i] = e[i];
        t.finite &= std::isfinite(e[i]);
    }
    t.a = compute_mesh_transform(V3{e[0], e[1], e[2]}, V3{e[3], e[4], e[5]}, S, params->unit_transform);
    return t;
}

GridBox grid_box(const o2v_hip_ctx *ctx, const o2v_hip_params *params, const Switches &sw, const HostTransform &xf, uint32_t ss, uint32_t z0,
                 uint32_t z1)
{
    const uint32_t G = params->resolution, S = G * ss;
    GridBox b{{0u, 0u, z0}, {G, G, z1}, false};
    // (an x / y tile of the grid, o2v_hip_params::x_begin; 0, 0: the whole axis)
    if (params->x_begin || params->x_end) {
        b.lo[0] = params->x_begin;
        b.hi[0] = std::min(params->x_end, G);
    }
    if (params->y_begin || params->y_end) {
        b.lo[1] = params->y_begin;
        b.hi[1] = std::min(params->y_end, G);
    }
    if (b.lo[0] >= b.hi[0] || b.lo[1] >= b.hi[1]) b.empty = true;
    if (sw.no_crop || !upload_bounds_valid(ctx) || !xf.have) return b;
    const float *h = ctx->mesh_bounds_hint;
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(h[i])) return b;
    const Affine &a = xf.a;  // (of the bounds in effect: the caller's, or the mesh's own)
    double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
    for (int corner = 0; corner < 8; ++corner) {
        const V3 t = affine_apply(a, V3{h[(corner & 1) ? 3 : 0], h[(corner & 2) ? 4 : 1], h[(corner & 4) ? 5 : 2]});
        const float c[3] = {t.x, t.y, t.z};
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(c[k])) return b;
            mn[k] = std::min<double>(mn[k], c[k]);
            mx[k] = std::max<double>(mx[k], c[k]);
        }
    }
    for (int k = 0; k < 3; ++k) {
        // sample space: [floor(min) - 1, floor(max) + 2), within [0, S) (a negative coordinate is voxel 0 on the device)
        const double lo_s = std::min<double>(std::max<double>(std::floor(mn[k]) - 1.0, 0.0), (double) S);
        const double hi_s = std::min<double>(std::max<double>(std::floor(mx[k]) + 2.0, 0.0), (double) S);
        uint32_t lo_o = (uint32_t) lo_s / ss, hi_o = ((uint32_t) hi_s + ss - 1u) / ss;
        if (k < 2) lo_o &= ~(kBrickX - 1u);  // (kBrickX == kBrickY)
        b.lo[k] = std::max(b.lo[k], lo_o);
        b.hi[k] = std::min(b.hi[k], hi_o);
        if (b.lo[k] >= b.hi[k]) b.empty = true;
    }
    return b;
}
static_assert(kBrickX == kBrickY, "grid_box aligns x and y alike");

// K0 and K1 of a pass: bounds and transform, the slab's block list, the root triangles and the subdivision rounds.  Returns in
// `block_list` the list of blocks of 256 triangles that meet the slab (null: every block).
int launch_expand(o2v_hip_ctx *ctx, const Params &p, const Switches &sw, uint32_t n_rounds, uint32_t *&block_list)
{
    hipStream_t s = ctx->stream;
    Counters *const ctr = ctx->d_ctr.ptr;
    const uint32_t persistent = (uint32_t) ctx->num_cus * 8u;
    if (ctx->stage_events) O2V_CHECK(ctx->pass_times.mark(0, s));
    // (the counters were zeroed behind the previous pass, off its critical path, unless something else used them since)
    if (!ctx->ctr_clean) O2V_LAUNCH("k_init", s, k_init, dim3(1), dim3(64), 0, s, ctr, kPassCounterWords);
    ctx->ctr_clean = false;
    if (!p.bounds_known) {
        // one workgroup per CU: every workgroup ends with six atomics on the same six words, which serialise (1024
        // workgroups: 43 us for 31 MB, 256: 24 us)
        O2V_LAUNCH("k_bounds", s, k_bounds, dim3((uint32_t) std::min<uint64_t>((uint64_t) ctx->num_cus, (p.n_tris * 9 / 12 + kBoundsBlock) / kBoundsBlock)),
                           dim3(kBoundsBlock), 0, s, ctx->d_verts.ptr, p.n_tris * 9, ctr);
    }
    // (letting the last workgroup of k_bounds compute the transform - one launch less - was measured: the stage 0.021 -> 0.027 ms)
    // (occupancy only with the bounds in effect on the host: the transform is in p already, o2v_hip_voxelize - neither launch)
    if (!p.xform_known) O2V_LAUNCH("k_setup", s, k_setup, dim3(1), dim3(64), 0, s, ctr, p);
    if (ctx->stage_events) O2V_CHECK(ctx->pass_times.mark(1, s));

    // After a slab plan the z extent of every block of 256 triangles is known: a slab that is not the whole grid visits only
    // the blocks that meet it (on N GPUs ~1/N of the list, compacted by k_list_blocks).
    const bool have_zrange = ctx->zrange_generation == ctx->tri_generation;
    const uint64_t n_tri_blocks = (p.n_tris + kBlock - 1) / kBlock;
    block_list = nullptr;
    const uint64_t list_above = sw.block_list ? 0ull : 256ull;
    if (have_zrange && (p.zs0 != 0 || p.zs1 < p.S) && n_tri_blocks > list_above && ctx->d_block_list.ptr && ctx->d_block_list.cap >= n_tri_blocks) {
        block_list = ctx->d_block_list.ptr;
        // (the list's counter is a word of the pass's counters: zero since k_init)
        O2V_LAUNCH("k_list_blocks", s, k_list_blocks, dim3((uint32_t) std::min<uint64_t>((uint64_t) ctx->num_cus * 4u, (n_tri_blocks + kBlock - 1) / kBlock)),
                           dim3(kBlock), 0, s, ctx->d_zrange.ptr, ctx->d_zrange_xform.ptr, ctr, block_list, ctx->d_block_count, p);
    }
    // (root_bypass: most super-blocks of three sub-batches are only read and counted - fewer workgroups with several super-blocks
    // each keep the loads of the next one in flight behind the current one's arithmetic)
    // (a slab visits the listed blocks only - how many is known on the device; the slab's share of z, and a third more, is the
    // estimate here: too many workgroups cost this kernel as much again, 0.033 -> 0.06 - 0.08 ms on a slab of the 8-GPU weak job)
    uint64_t walked_blocks = n_tri_blocks;
    if (block_list && p.S) walked_blocks = std::min<uint64_t>(n_tri_blocks, (uint64_t) ((double) n_tri_blocks * (double) (p.zs1 - p.zs0) / (double) p.S * 1.33) + 64u);
    uint64_t root_wgs = p.root_bypass ? std::max<uint64_t>((uint64_t) ctx->num_cus * 2u, walked_blocks / 6u) : (p.n_tris + kBlock - 1) / kBlock;
    const uint32_t *k1_list = block_list, *k1_count = ctx->d_block_count;
    // (solo roots: every root triangle is a leaf of one tile or misses the slab, plan_rounds - nothing for K1 to write, and what
    // it would count k_voxelize_occ counts)
    if (!p.solo_roots && ctx->lean_roots && p.root_bypass) {
        // a tessellated surface: the one-tile root triangles are counted by a kernel of their own, k_expand_roots only walks the
        // blocks that hold something else (k_count_roots)
        O2V_LAUNCH("k_count_roots", s, k_count_roots, dim3((uint32_t) std::min<uint64_t>((uint64_t) ctx->num_cus * kCountRootsWgsPerCu, std::max<uint64_t>((walked_blocks + 3u) / 4u, 1))),
                           dim3(kBlock), 0, s, ctx->d_verts.ptr, ctr, block_list, ctx->d_block_count, ctx->d_need_list.ptr, &ctr->n_need_blocks, p);
        k1_list = ctx->d_need_list.ptr;
        k1_count = &ctr->n_need_blocks;
        root_wgs = (uint64_t) ctx->num_cus;  // (the list is short or empty)
    }
    if (!p.solo_roots)
        O2V_LAUNCH("k_expand_roots", s, k_expand_roots, dim3(std::min<uint64_t>(persistent, std::max<uint64_t>(root_wgs, 1))),
                           dim3(kBlock), 0, s, ctx->d_verts.ptr, ctx->d_uvs.ptr, ctr, ctx->d_leaves.ptr, ctx->d_tiles.ptr,
                           ctx->d_big.ptr, ctx->d_nodes[0].ptr, have_zrange ? ctx->d_zrange.ptr : nullptr,
                           ctx->d_zrange_xform.ptr, k1_list, k1_count, p);
    for (uint32_t round = 0; round < (p.solo_roots ? 0u : n_rounds); ++round) {
        // most rounds are empty or small: a narrow grid keeps an empty launch short (the kernel strides over its input)
        O2V_LAUNCH("k_expand_nodes", s, k_expand_nodes, dim3((uint32_t) ctx->num_cus * 2u), dim3(kBlock), 0, s, ctx->d_nodes[round & 1].ptr, round,
                           ctr, ctx->d_leaves.ptr, ctx->d_tiles.ptr, ctx->d_big.ptr, ctx->d_nodes[(round + 1) & 1].ptr, p);
    }
    // (left out if no leaf of this mesh can have more than four tiles, plan_rounds; should one turn up, the pass is repeated)
    if (!ctx->skip_big && !p.solo_roots)
        O2V_LAUNCH("k_expand_big", s, k_expand_big, dim3((uint32_t) ctx->num_cus * 2u), dim3(kBlock), 0, s, ctx->d_big.ptr, ctr, ctx->d_tiles.ptr, p);
    return O2V_HIP_OK;
}

// K2: k_voxelize in the variant of the pass, on persistent workgroups - four wavefronts per SIMD, in workgroups of
// VoxShape<UV>::block threads.
void launch_voxelize(o2v_hip_ctx *ctx, const Params &p, bool use_uv, const uint32_t *block_list)
{
    hipStream_t s = ctx->stream;
    Counters *const ctr = ctx->d_ctr.ptr;
    const uint32_t block = use_uv ? VoxShape<true>::block : VoxShape<false>::block;
    const dim3 blocks((uint32_t) ctx->num_cus * (uint32_t) (use_uv ? O2V_K2_WAVES_UV : O2V_K2_WAVES) * (kBlock / block));
    if (use_uv)
        O2V_LAUNCH_K2("k_voxelize<true>", k_voxelize<true>, blocks, dim3(block), ctx->d_leaves.ptr, ctx->d_tiles.ptr, ctr, ctx->d_grid.ptr,
                      ctx->d_brick_dirty.ptr, ctx->d_pool.ptr, ctx->d_jobq.ptr, p);
    else if (p.occupancy_only)
        O2V_LAUNCH_K2("k_voxelize_occ", k_voxelize_occ, blocks, dim3(block), ctx->d_leaves.ptr, ctx->d_tiles.ptr, ctr, ctx->d_grid.ptr,
                      ctx->d_brick_dirty.ptr, ctx->d_pool.ptr, ctx->d_jobq.ptr, ctx->d_verts.ptr, block_list, ctx->d_block_count, p);
    else
        O2V_LAUNCH_K2("k_voxelize<false>", k_voxelize<false>, blocks, dim3(block), ctx->d_leaves.ptr, ctx->d_tiles.ptr, ctr, ctx->d_grid.ptr,
                      ctx->d_brick_dirty.ptr, ctx->d_pool.ptr, ctx->d_jobq.ptr, p);
}

// The resolve stage of the general route (K5's scatter and K3), for hit records of 6 words (use_uv: with the uv mean) or 4.
// `resolve_wgs`: the workgroups of tier 1 on the inline cells.
int launch_resolve(o2v_hip_ctx *ctx, const Params &p, bool use_uv, uint32_t resolve_wgs)
{
    // the kernels that depend on the record size, and the names they are launched under (bench.py and the profile tools
    // match on them)
    const uint32_t R = use_uv ? 6u : 4u;
    const auto k_inline = use_uv ? k_resolve_inline_list<6> : k_resolve_inline_list<4>;
    const auto k_cells = use_uv ? k_resolve<6> : k_resolve<4>;
    const auto k_list16 = use_uv ? k_resolve_list16<6> : k_resolve_list16<4>;
    const char *inline_name = use_uv ? "k_resolve_inline_list<6>" : "k_resolve_inline_list<4>";
    const char *cells_name = use_uv ? "k_resolve<6>" : "k_resolve<4>";
    const char *list16_name = use_uv ? "k_resolve_list16<6>" : "k_resolve_list16<4>";
    hipStream_t s = ctx->stream;
    Counters *const ctr = ctx->d_ctr.ptr;
    const uint32_t persistent = (uint32_t) ctx->num_cus * 8u;
    const Materials &m = p.mat;
    const SortedView sorted_view{reinterpret_cast<const uint32_t *>(ctx->d_sorted.ptr), R};
    const SortedView slab_view{ctx->d_slabs.ptr, R};
    // What follows k_scan_bricks runs side by side (the tiers work on disjoint cells, filed by k_scan_bricks):
    //   main stream   tier 1 on the inline cells - most cells; their hits are in the slabs, so it needs no sorted array -
    //                 then, once that exists, on the short cells of bricks without a slab (none as a rule)
    //   aux 0         the counting sort of what the slabs do not hold (k_scatter), then the 9..16-hit tier
    //   aux 1, 2      (behind the sort) the counter reset and the cooperative tiers
    const bool fork = debug_sync_level() != 1;
    hipStream_t sw = s, sm = s, sl = s;
    if (fork) {
        for (Stream &q : ctx->aux) O2V_CHECK(q.create());
        sw = ctx->aux[0];
        sm = ctx->aux[1];
        sl = ctx->aux[2];
        O2V_CHECK(hipEventRecord(ctx->ev_fork, s));
        O2V_CHECK(hipStreamWaitEvent(sw, ctx->ev_fork, 0));
    }
    // (the inline cells with 5 .. 8 hits: from the slabs like the main stream's launch, so it starts with it)
    if (fork) O2V_CHECK(hipStreamWaitEvent(sm, ctx->ev_fork, 0));
    O2V_LAUNCH(inline_name, sm, k_inline, dim3((uint32_t) ctx->num_cus * 2u),
               dim3(kBlock), 0, sm, ctx->d_list_lane8.ptr, &ctr->n_lane8, ctr, ctx->d_occ.ptr, slab_view, m, ctx->d_out.ptr, p.cap_vox, p);
    O2V_LAUNCH("k_scatter", sw, k_scatter, dim3(persistent), dim3(kBlock), 0, sw, ctx->d_pool.ptr, ctx->d_grid.ptr, ctr,
                       reinterpret_cast<uint32_t *>(ctx->d_sorted.ptr), R, p);
    if (fork) {
        O2V_CHECK(hipEventRecord(ctx->ev_sorted, sw));
        O2V_CHECK(hipStreamWaitEvent(sm, ctx->ev_sorted, 0));
        O2V_CHECK(hipStreamWaitEvent(sl, ctx->ev_sorted, 0));
    }
    O2V_LAUNCH(cells_name, s, k_cells, dim3(resolve_wgs), dim3(kBlock), 0, s, ctx->d_occ.ptr, sorted_view, slab_view, ctr, m,
               ctx->d_out.ptr, 0u, p);
    if (fork) O2V_CHECK(hipStreamWaitEvent(s, ctx->ev_sorted, 0));
    O2V_LAUNCH(cells_name, s, k_cells, dim3(persistent), dim3(kBlock), 0, s, ctx->d_occ.ptr, sorted_view, slab_view, ctr, m,
               ctx->d_out.ptr, 1u, p);
    O2V_LAUNCH(list16_name, sw, k_list16, dim3((uint32_t) ctx->num_cus * 4u), dim3(kBlock), 0,
               sw, ctx->d_list_lane16.ptr, &ctr->n_lane16, ctr, ctx->d_occ.ptr, sorted_view, m, ctx->d_out.ptr, p.cap_vox, p);
    // (behind the 9..16-hit tier: nothing waits for the counters' reset but the next pass)
    O2V_LAUNCH("k_reset_bricks", sw, k_reset_bricks, dim3((uint32_t) ctx->num_cus * 4u), dim3(kBlock), 0, sw, ctx->d_grid.ptr,
                       ctx->d_dirty_list.ptr, ctr, p);
    {
        // the cooperative tiers for 17 .. 256 hits: one launch of one-wavefront workgroups (k_resolve_tiers)
        const uint32_t g_mid = (uint32_t) ctx->num_cus * 8u, g_w = (uint32_t) ctx->num_cus * 16u;
        const TierLists tl{ctx->d_list_mid.ptr, ctx->d_list_w64.ptr, ctx->d_list_lane.ptr, &ctr->n_mid, &ctr->n_w64, &ctr->n_lane, &ctr->cursor_mid};
        O2V_LAUNCH("k_resolve_tiers", sm, k_resolve_tiers, dim3(g_mid + 2u * g_w), dim3(64), 0, sm, tl, g_mid, g_w, ctr, ctx->d_occ.ptr, sorted_view, m,
                           ctx->d_out.ptr, p.cap_vox, p);
    }
    O2V_LAUNCH("k_resolve_sorted<256,2048>", sl, (k_resolve_sorted<kBlock, kLongList>), dim3((uint32_t) ctx->num_cus * 2u), dim3(kBlock), 0, sl,
                       ctx->d_list_long.ptr, &ctr->n_long, &ctr->cursor_long, ctr, ctx->d_occ.ptr, sorted_view, m,
                       ctx->d_out.ptr, p.cap_vox, p);
    O2V_LAUNCH("k_resolve_big", sl, k_resolve_big, dim3((uint32_t) ctx->num_cus / 2u), dim3(kBigThreads), kBigList * 12u, sl, ctx->d_list_big.ptr,
                       ctr, ctx->d_occ.ptr, sorted_view, m, ctx->d_out.ptr, p.cap_vox, p);
    if (ctx->d_scratch_key.ptr) {
        O2V_LAUNCH("k_resolve_huge", sl, k_resolve_huge, dim3((uint32_t) ctx->num_cus / 2u), dim3(kBlock), 0, sl, ctx->d_list_huge.ptr,
                           ctr, ctx->d_occ.ptr, sorted_view, m, ctx->d_out.ptr, ctx->d_scratch_key.ptr,
                           ctx->d_scratch_idx.ptr, (uint32_t) std::min(ctx->d_scratch_key.cap, ctx->d_scratch_idx.cap), p.cap_vox, p);
    }
    if (fork)
        for (int j = 0; j < 3; ++j) {
            O2V_CHECK(hipEventRecord(ctx->ev_join[j], ctx->aux[j]));
            O2V_CHECK(hipStreamWaitEvent(s, ctx->ev_join[j], 0));
        }
    return O2V_HIP_OK;
}

// The per-kernel times of the launches bracketed since the pass began (O2V_HIP_FLAG_KERNEL_TIMES), once the stream has drained.
int collect_kernel_times(o2v_hip_ctx *ctx)
{
    ctx->kernel_times.clear();
    for (size_t i = 0; i < ctx->ktimes_used; ++i) {
        const o2v_hip_ctx::KernelBracket &b = ctx->ktimes[i];
        float ms = 0.f;
        O2V_CHECK(b.times.elapsed(0, 1, ms));
        auto it = std::find_if(ctx->kernel_times.begin(), ctx->kernel_times.end(),
                               [&](const o2v_hip_kernel_time &k) { return std::strcmp(k.name, b.name) == 0; });
        if (it == ctx->kernel_times.end()) {
            o2v_hip_kernel_time k{};
            std::snprintf(k.name, sizeof(k.name), "%s", b.name);
            ctx->kernel_times.push_back(k);
            it = ctx->kernel_times.end() - 1;
        }
        it->ms += ms;
        it->launches += 1;
    }
    return O2V_HIP_OK;
}

// The end of a pass: the counters to the host, the per-kernel times, and the next pass's counters zeroed behind this one.
int finish_pass(o2v_hip_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    // (a kernel that writes the counters into the page-locked copy instead of this copy command was measured: the same step time)
    O2V_CHECK(hipMemcpyAsync(ctx->h_ctr.ptr, ctx->d_ctr.ptr, kPassCounterWords * 4u, hipMemcpyDeviceToHost, s));
    // (polling the stream with hipStreamQuery instead was measured: the same step time - the runtime's wait spins already)
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(hipGetLastError());
    if (const int rc = collect_kernel_times(ctx)) return rc;
    // the next pass's counters: zeroed now, behind this pass (its results are on the host)
    hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, s, ctx->d_ctr.ptr, kPassCounterWords);
    O2V_CHECK(hipGetLastError());
    ctx->ctr_clean = true;
    return O2V_HIP_OK;
}

// One pass of the pipeline with the current capacities.  Fills h_ctr; the caller checks for overflow.
int run_pass(o2v_hip_ctx *ctx, const Params &p, const Switches &sw, bool use_uv, uint32_t n_rounds)
{
    hipStream_t s = ctx->stream;
    Counters *const ctr = ctx->d_ctr.ptr;
    ctx->ktimes_used = 0;
    uint32_t *block_list = nullptr;
    int rc;
    if ((rc = launch_expand(ctx, p, sw, n_rounds, block_list))) return rc;
    // (a mesh that pooled no hits in its last pass with these settings - every triangle whole and on the direct MAX path - will
    // not pool any now: the two launches are left out; should K1's counters say otherwise, the pass is repeated with them)
    const uint64_t mark_key = ctx->tri_generation * 1000003ull + p.blend * 7u + p.S * 131ull + p.zs0 * 31ull + p.zs1 + p.exact_clip * 3u;
    const bool skip_mark = !ctx->force_general && ctx->no_pool_key == mark_key + 1u;
    ctx->marked_bricks = !p.occupancy_only && !skip_mark;
    if (ctx->marked_bricks) {
        // The bricks that can receive pooled hits are listed before k_voxelize (every brick a leaf's clamped box touches: a
        // superset of the bricks that do), and every listed brick gets a hit slab: the first kInlineHits hits of a cell go
        // there directly.  Neither kernel has work if the pass pools no hits (decided on the device from K1's counters).
        O2V_LAUNCH("k_mark_bricks", s, k_mark_bricks, dim3((uint32_t) ctx->num_cus * 4u), dim3(kBlock), 0, s, ctx->d_leaves.ptr, ctr, ctx->d_brick_dirty.ptr,
                           ctx->force_general ? 1u : 0u, p);
        const uint32_t flag_groups = (p.n_bricks + 15u) / 16u;
        O2V_LAUNCH("k_scan_flags", s, k_scan_flags, dim3(std::min<uint32_t>((uint32_t) ctx->num_cus * kScanFlagsWgsPerCu, std::max<uint32_t>(1u, (flag_groups + kBlock * kFlagLoads - 1) / (kBlock * kFlagLoads)))),
                           dim3(kBlock), 0, s, ctx->d_brick_dirty.ptr, &ctr->n_dirty, ctx->d_dirty_list.ptr, ctr, ctx->d_brick_slab.ptr, ctx->force_general ? 1u : 0u, p);
    }
    if (ctx->stage_events) O2V_CHECK(ctx->pass_times.mark(2, s));
    // (occupancy only: every hit takes the direct path whatever K1 counted - nothing to decide)
    const bool decide_from_k1 = p.direct_max && !(p.occupancy_only && !ctx->force_general);
    if (decide_from_k1) {
        // K1's counters go to the host on an auxiliary stream while k_voxelize runs (see below)
        O2V_CHECK(ctx->aux[0].create());
        O2V_CHECK(hipEventRecord(ctx->ev_k1, s));
        O2V_CHECK(hipStreamWaitEvent(ctx->aux[0], ctx->ev_k1, 0));
        O2V_CHECK(hipMemcpyAsync(ctx->h_ctr.ptr, ctr, kPassCounterWords * 4u, hipMemcpyDeviceToHost, ctx->aux[0]));
    }

    launch_voxelize(ctx, p, use_uv, block_list);
    if (ctx->stage_events) O2V_CHECK(ctx->pass_times.mark(3, s));

    // With the direct MAX path the rest of the pass depends on the mesh: one whose triangles are all voxelized whole needs
    // neither the counting sort nor the replay (a dozen launches that would each find nothing), one whose triangles are
    // mostly subdivided does not use the 64-bit grid at all.  Both follow from K1's counters, which reached the host
    // while k_voxelize was running: the follow-up stages are enqueued behind it without the stream ever draining.
    bool run_general = true, run_emit = false;
    if (p.direct_max) {
        if (decide_from_k1) {
            O2V_CHECK(hipStreamSynchronize(ctx->aux[0]));
            const Counters &h = *ctx->h_ctr.ptr;
            run_emit = p.occupancy_only || h.n_nodes[0] <= h.n_root_leaves;  // direct_active() on the device
            // hits are pooled only for leaves of subdivided triangles: without any, every hit goes straight into the 64-bit grid
            // (occupancy-only mode: those too)
            run_general = !run_emit || (h.n_nodes[0] != 0 && !p.occupancy_only) || ctx->force_general;
        }
        else {
            run_emit = true;
            run_general = false;
        }
        if (run_emit) {
            const uint32_t groups = (p.n_bricks + 15u) / 16u;
            O2V_LAUNCH("k_scan_flags", s, k_scan_flags, dim3(std::min<uint32_t>((uint32_t) ctx->num_cus * kScanFlagsWgsPerCu, std::max<uint32_t>(1u, (groups + kBlock * kFlagLoads - 1) / (kBlock * kFlagLoads)))),
                               dim3(kBlock), 0, s, ctx->d_dirty_max.ptr, &ctr->n_dirty_max, ctx->d_dirty_list_max.ptr, ctr, (uint32_t *) nullptr, 0u, p);
        }
    }

    if (run_general && !ctx->marked_bricks && !p.occupancy_only) {
        // the guess above was wrong (it cannot be for the same triangles and settings): no brick has a slab number, the pass is void
        ctx->no_pool_key = 0;
        ctx->mark_missing = true;
        run_general = false;
    }
    else if (!p.occupancy_only) {
        ctx->no_pool_key = run_general ? 0 : mark_key + 1u;
    }
    if (run_general) {
        // (the brick list was made before k_voxelize: see k_mark_bricks)
        const ResolveLists lists{ctx->d_list_lane16.ptr, ctx->d_list_lane.ptr, ctx->d_list_w64.ptr, ctx->d_list_mid.ptr, ctx->d_list_long.ptr,
                                 ctx->d_list_big.ptr, ctx->d_list_huge.ptr, ctx->d_list_lane8.ptr, p.cap_vox};
        O2V_LAUNCH("k_scan_bricks", s, k_scan_bricks, dim3((uint32_t) ctx->num_cus * 2u), dim3(kBlock), 0, s, ctx->d_grid.ptr,
                           ctx->d_dirty_list.ptr, ctr, ctx->d_occ.ptr, lists, p);
    }
    ctx->last_ran_general = run_general;
    if (ctx->stage_events) O2V_CHECK(ctx->pass_times.mark(4, s));

    if (run_general) {
        // (tier 1 on the inline cells runs as fast with two workgroups per CU as with eight - it is not bound by the wavefronts in
        // flight - and leaves the counting sort and the cooperative tiers beside it room: bench mesh with BLEND -0.1 ms)
        const uint32_t resolve_wgs = (uint32_t) ctx->num_cus * (sw.resolve_wgs_per_cu > 0 ? (uint32_t) sw.resolve_wgs_per_cu : 2u);
        if ((rc = launch_resolve(ctx, p, use_uv, resolve_wgs))) return rc;
    }
    if (run_emit && p.pick_max)
        O2V_LAUNCH("k_pick", s, k_pick, dim3((uint32_t) ctx->num_cus * 8u), dim3(kBlock), 0, s, ctx->d_pool.ptr, ctr, p);
    if (run_emit && p.occupancy_only) {
        O2V_LAUNCH("k_emit_occ", s, k_emit_occ, dim3((uint32_t) ctx->num_cus * kOccWgsPerCu), dim3(kBlock), 0, s, ctx->d_dirty_list_max.ptr, ctr,
                   ctx->d_out.ptr, p);
    }
    else if (run_emit) {
        // every voxel's winner is in the 64-bit grid now (k_voxelize: unsplit triangles, resolve: the rest)
        O2V_LAUNCH("k_emit_max", s, k_emit_max, dim3((uint32_t) ctx->num_cus * 3u), dim3(kBlock), 0, s, ctx->d_dirty_list_max.ptr, ctr, p.mat,
                           ctx->d_out.ptr, p);
    }
    if (ctx->stage_events) O2V_CHECK(ctx->pass_times.mark(5, s));
    if ((rc = finish_pass(ctx))) return rc;
    // (a pass that got its transform as an argument: the counters' copy has arrived, the host puts the transform where k_setup's
    // would be - publish and the fill stage read it there)
    if (p.xform_known) std::memcpy(ctx->h_ctr.ptr->xform, p.xform, sizeof(p.xform));
    return O2V_HIP_OK;
}

// One o2v_hip_voxelize call: its pass geometry and routes (Params), and what its passes ask of the buffers.
struct Run {
    Params p{};
    GridBox box{};             // the pass box (output space)
    HostTransform xf{};        // the bounds in effect and the transform from them, where the host knows them
    bool use_uv = false;
    uint64_t n_bricks = 0;
    uint32_t n_rounds = 0;     // subdivision rounds launched
    uint64_t solo_key = 0;     // the mesh and settings, for ctx->solo_refused_key
    // the capacities the next pass asks for; every counter keeps counting past its capacity, so one re-run sizes it exactly
    uint64_t want_leaves = 0, want_tiles = 0, want_big = 0, want_nodes = 0, want_hits = 0, want_vox = 0, want_slabs = 0, want_scratch = 0;
};

// Checks the call, starts it (the results of the last one are gone) and makes the pass' box and the geometry part of Params.
// `empty`: the mesh does not reach the slab (no voxels).
int pass_geometry(o2v_hip_ctx *ctx, const o2v_hip_params *params, const Switches &sw, Run &r, bool &empty)
{
    const uint32_t ss = params->supersampling ? params->supersampling : 1u;
    const uint64_t S64 = (uint64_t) params->resolution * ss;
    if (params->resolution == 0 || ss > 2 || params->strategy > 1) {
        ctx->err = "resolution must be non-zero, supersampling 1 or 2, strategy 0 or 1";
        return O2V_HIP_ERR_BAD_ARGUMENT;
    }
    if (S64 > 0x7fffffffull) {
        ctx->err = "sample resolution must be below 2^31";
        return O2V_HIP_ERR_LIMIT;
    }
    uint32_t z0 = params->z_begin, z1 = params->z_end;
    if (z0 == 0 && z1 == 0) z1 = params->resolution;
    if (z1 > params->resolution || z0 >= z1) {
        ctx->err = "z slab must satisfy z_begin < z_end <= resolution";
        return O2V_HIP_ERR_BAD_ARGUMENT;
    }
    // an x / y tile of the grid (0, 0: the whole axis), see o2v_hip_params::x_begin
    uint32_t xy0[2] = {params->x_begin, params->y_begin}, xy1[2] = {params->x_end, params->y_end};
    for (int k = 0; k < 2; ++k) {
        if (xy0[k] == 0 && xy1[k] == 0) xy1[k] = params->resolution;
        if (xy1[k] > params->resolution || xy0[k] >= xy1[k] || (xy0[k] & (kBrickX - 1u))) {
            ctx->err = "x / y tile must satisfy begin < end <= resolution, begin a multiple of 4";
            return O2V_HIP_ERR_BAD_ARGUMENT;
        }
    }
    O2V_CHECK(hipSetDevice(ctx->device));
    ctx->n_vox = 0;
    ctx->timings = {};
    ctx->stats = {};
    ctx->stats.triangles = ctx->n_tris;
    Params &p = r.p;
    p.n_tris = ctx->n_tris;
    p.S = (uint32_t) S64;
    p.G = params->resolution;
    // the dense grids cover the mesh's voxel bounding box within the slab (grid_box)
    r.xf = host_transform(ctx, params, p.S);  // (once per call: for the grids' box here, for the kernels in host_k0)
    const GridBox box = grid_box(ctx, params, sw, r.xf, ss, z0, z1);   // (within the x / y tile, if the call names one)
    r.box = box;
    empty = box.empty;
    if (empty) return O2V_HIP_OK;
    // Voxel coordinates travel in 16-bit fields relative to the grid's origin (Params::so): what is limited is the box of one
    // pass, not the resolution.  (The reference carries u32 coordinates and 64-bit Morton keys, src/util.hpp:185-196; a box wider
    // than this is cut into x / y tiles by the caller - obj2voxel_voxelize() does - as a slab too thick for memory is cut in z.)
    for (int k = 0; k < 3; ++k)
        if ((uint64_t) (box.hi[k] - box.lo[k]) * ss > 65535u) {
            ctx->err = "the pass' box (the mesh's voxel bounding box within the slab / tile) must be at most 65535 samples wide; use x / y tiles (o2v_hip_params::x_begin ..) or z-slabs";
            return O2V_HIP_ERR_LIMIT;
        }
    p.xo0 = box.lo[0];
    p.yo0 = box.lo[1];
    p.NBx = (box.hi[0] - box.lo[0] + kBrickX - 1) / kBrickX;
    p.NBy = (box.hi[1] - box.lo[1] + kBrickY - 1) / kBrickY;
    const uint32_t NBz = (box.hi[2] - box.lo[2] + kBrickZ - 1) / kBrickZ;
    r.n_bricks = (uint64_t) p.NBx * p.NBy * NBz;
    if (r.n_bricks >= (1ull << 32) / 2) {
        ctx->err = "slab has too many bricks for 32-bit brick ids; use more z-slabs";
        return O2V_HIP_ERR_LIMIT;
    }
    p.n_bricks = (uint32_t) r.n_bricks;
    p.cap_dirty = (uint32_t) std::min<uint64_t>((r.n_bricks + 15u) & ~15ull, kDirtyListMax);
    p.ss_shift = ss == 2 ? 1u : 0u;
    p.zs0 = z0 * ss;
    p.zs1 = z1 * ss;
    p.zo0 = box.lo[2];
    for (int k = 0; k < 3; ++k) {
        // the same box in sample space, z cut to the slab: what a leaf's box is clamped to (plan_leaf)
        p.cs_lo[k] = box.lo[k] * ss;
        p.cs_hi[k] = (uint32_t) std::min<uint64_t>((uint64_t) box.hi[k] * ss, S64);
    }
    p.cs_lo[2] = std::max(p.cs_lo[2], p.zs0);
    p.cs_hi[2] = std::min(p.cs_hi[2], p.zs1);
    p.so[0] = p.xo0 * ss;
    p.so[1] = p.yo0 * ss;
    p.so[2] = p.zo0 * ss;
    p.blend = params->strategy;
    p.bounds_known = params->bounds_known;
    for (int i = 0; i < 6; ++i) p.bounds[i] = params->bounds[i];
    for (int i = 0; i < 9; ++i) p.unit[i] = params->unit_transform[i];
    p.has_uv = ctx->d_uvs.ptr ? 1u : 0u;
    return O2V_HIP_OK;
}

// The routes of the call: occupancy only, the direct MAX path, the root bypass and lean roots (ctx->lean_roots).
void choose_routes(o2v_hip_ctx *ctx, const o2v_hip_params *params, const Switches &sw, Run &r)
{
    Params &p = r.p;
    const GridModes modes = grid_modes(ctx, params, sw);
    r.use_uv = modes.use_uv;
    ctx->sorted_stride = r.use_uv ? 6u : 4u;
    p.exact_clip = modes.exact_clip ? 1u : 0u;
    // Which dense grids a run needs depends on the mesh and the strategy:
    //   occupancy-only (no triangle has a material: every STL, an OBJ without materials)   1 byte per cell
    //   MAX strategy                       64-bit max grid (direct path) + 32-bit counter grid (subdivided triangles)
    //   BLEND strategy                     32-bit counter grid
    p.occupancy_only = modes.occupancy_only ? 1u : 0u;
    p.root_bypass = (modes.occupancy_only && !sw.no_root_bypass) ? 1u : 0u;  // (A/B: every leaf through its Leaf / Tile records)
    // ... and on a tessellated surface - fewer than one triangle in 512 is 4 voxels or more across (the histogram of the triangles'
    // extents, made at upload): practically every block of 256 holds nothing but one-tile leaves - a z-slab run lets k_count_roots
    // run ahead of k_expand_roots (run_pass).  Measured: the expand stage of a slab of the 8-GPU weak job 0.054 -> 0.034 ms; on the
    // whole grid (the bench headline) the two kernels take what k_expand_roots alone takes (0.028 against 0.026 ms), so not there.
    // Either way the same leaves are made; O2V_NO_COUNT_ROOTS=1: never, O2V_COUNT_ROOTS=1: also on the whole grid (A/B).
    ctx->lean_roots = false;
    if (p.root_bypass && ctx->max_tri_extent >= 0.f && ctx->n_tris && (p.zs0 != 0 || p.zs1 < p.S || sw.count_roots)) {
        const MeshScale m = mesh_scale(ctx, params);
        const float voxels_per_unit = m.unit_norm * (float) p.S / m.max_axis;
        if (m.max_axis > 0.f && std::isfinite(voxels_per_unit) && voxels_per_unit > 0.f && !sw.no_count_roots) {
            uint64_t large = ctx->ext_hist[255];
            for (uint32_t e = 1; e < 255; ++e)   // bin e: extents in [2^(e-127), 2^(e-126))
                if (std::ldexp(1.0f, (int) e - 127) * voxels_per_unit >= 4.0f) large += ctx->ext_hist[e];
            ctx->lean_roots = large * 512u <= ctx->n_tris;
        }
    }
    p.direct_max = modes.direct_max ? 1u : 0u;
    p.pick_max = (p.direct_max && r.use_uv) ? 1u : 0u;  // textured: the winner's colour is picked afterwards (k_pick)
    p.mat = Materials{ctx->d_types.ptr, ctx->d_colors.ptr, ctx->d_texids.ptr, ctx->d_textures.ptr, ctx->n_textures};
}

// zeroes the counter grid and / or the max grid, with their dirty flags
int clear_grids(o2v_hip_ctx *ctx, bool count_grid, bool max_grid)
{
    if (count_grid) O2V_CHECK(hipMemsetAsync(ctx->d_grid.ptr, 0, ctx->d_grid.cap * sizeof(uint32_t), ctx->stream));
    if (count_grid) O2V_CHECK(hipMemsetAsync(ctx->d_brick_dirty.ptr, 0, ctx->d_brick_dirty.cap, ctx->stream));
    if (max_grid) O2V_CHECK(hipMemsetAsync(ctx->d_maxgrid.ptr, 0, ctx->d_maxgrid.cap, ctx->stream));
    if (max_grid) O2V_CHECK(hipMemsetAsync(ctx->d_dirty_max.ptr, 0, ctx->d_dirty_max.cap, ctx->stream));
    return O2V_HIP_OK;
}

// The 32-bit counter grid for n_bricks bricks with its dirty flags (one per brick, padded to 16), dirty-brick list and slab
// numbers, zeroed (and kept clean by the scan / reset kernels).
int ensure_count_grid(o2v_hip_ctx *ctx, uint64_t n_bricks)
{
    const GridBytes b = grid_bytes(Grid::counter);
    const uint64_t bricks = (n_bricks + 15u) & ~15ull, listed = std::min<uint64_t>(bricks, kDirtyListMax);
    if (n_bricks * kBrickCells > ctx->d_grid.cap || bricks > ctx->d_brick_dirty.cap || listed > ctx->d_dirty_list.cap ||
        bricks > ctx->d_brick_slab.cap) {
        O2V_CHECK(ctx->d_grid.alloc(n_bricks * b.cells / sizeof(uint32_t)));
        O2V_CHECK(ctx->d_brick_dirty.alloc(bricks * b.flag));
        O2V_CHECK(ctx->d_dirty_list.alloc(listed * b.list / sizeof(uint32_t)));
        O2V_CHECK(ctx->d_brick_slab.alloc(bricks * b.slab / sizeof(uint32_t)));
        ctx->grid_dirty = true;
    }
    if (const int rc = clear_grids(ctx, ctx->grid_dirty, false)) return rc;
    ctx->grid_dirty = false;
    return O2V_HIP_OK;
}

// The direct MAX path's 64-bit max grid (occupancy only: one byte per cell) with its dirty flags and list, zeroed.  If it does
// not fit (8 bytes per cell at 4096^3 on one GPU) none of the three is kept - a context cached by the C API must not look ready
// after an allocation failed half-way - and `fits` is false: every hit then takes the sort-and-replay route.
int ensure_max_grid(o2v_hip_ctx *ctx, uint64_t n_bricks, bool occupancy_only, bool &fits)
{
    const GridBytes b = grid_bytes(occupancy_only ? Grid::occupancy : Grid::max64);
    const uint64_t bricks = (n_bricks + 15u) & ~15ull;
    fits = ctx->d_maxgrid.ptr && n_bricks * b.cells <= ctx->d_maxgrid.cap && n_bricks <= ctx->d_dirty_max.cap;
    if (!fits) {
        ctx->maxgrid_dirty = true;
        fits = ctx->d_maxgrid.alloc(n_bricks * b.cells) == hipSuccess && ctx->d_dirty_max.alloc(bricks * b.flag) == hipSuccess &&
               ctx->d_dirty_list_max.alloc(std::min<uint64_t>(bricks, kDirtyListMax) * b.list / sizeof(uint32_t)) == hipSuccess;
    }
    if (!fits) {
        (void) hipGetLastError();
        (void) ctx->d_maxgrid.release();
        (void) ctx->d_dirty_max.release();
        (void) ctx->d_dirty_list_max.release();
        return O2V_HIP_OK;
    }
    if (const int rc = clear_grids(ctx, false, ctx->maxgrid_dirty)) return rc;
    ctx->maxgrid_dirty = false;
    return O2V_HIP_OK;
}

// The dense grids of the call's routes; the direct MAX path gives way to the general route if its grid does not fit.
int ensure_grids(o2v_hip_ctx *ctx, Run &r)
{
    Params &p = r.p;
    int rc;
    ctx->stats.grid_cells = r.n_bricks * kBrickCells;
    ctx->stats.grid_bytes = 0;
    bool fits = false;
    if (p.direct_max && (rc = ensure_max_grid(ctx, r.n_bricks, p.occupancy_only, fits))) return rc;
    if (p.direct_max && !fits) p.direct_max = p.pick_max = p.occupancy_only = p.root_bypass = 0;
    if (p.direct_max) {
        p.maxgrid = reinterpret_cast<unsigned long long *>(ctx->d_maxgrid.ptr);
        p.occgrid = ctx->d_maxgrid.ptr;
        p.dirty_max = ctx->d_dirty_max.ptr;
        const GridBytes b = grid_bytes(p.occupancy_only ? Grid::occupancy : Grid::max64);
        ctx->stats.grid_bytes += r.n_bricks * (b.cells + b.flag);
    }
    if (!p.occupancy_only) {
        // the counter grid (no pooled hits exist in occupancy-only mode)
        const GridBytes b = grid_bytes(Grid::counter);
        ctx->stats.grid_bytes += r.n_bricks * (b.cells + b.flag);
        if ((rc = ensure_count_grid(ctx, r.n_bricks))) return rc;
    }
    return O2V_HIP_OK;
}

// K0 on the host, decided once per call (every pass of the call launches the same kernels): on the occupancy-only route, with
// the bounds in effect on the host and finite - the caller's, the sharded step's reduced ones (they arrive as the caller's), or
// the upload's, which k_bounds itself made from these triangles (min and max are exact and order-free: the same six floats) -
// the pass gets the bounds and the transform as arguments and launches neither k_bounds nor k_setup.  Bounds that are unknown or
// not finite, an empty mesh and the weighted routes keep both launches; so does O2V_ALL_LAUNCHES=1 (A/B).
void host_k0(const Switches &sw, Run &r)
{
    Params &p = r.p;
    if (!p.occupancy_only || !r.xf.have || !r.xf.finite || sw.all_launches) return;
    p.bounds_known = 1;
    for (int i = 0; i < 6; ++i) p.bounds[i] = r.xf.bounds[i];
    p.xform_known = 1;
    for (int i = 0; i < 3; ++i) {
        p.xform[i * 3 + 0] = r.xf.a.m[i].x;
        p.xform[i * 3 + 1] = r.xf.a.m[i].y;
        p.xform[i * 3 + 2] = r.xf.a.m[i].z;
    }
    p.xform[9] = r.xf.a.t.x;
    p.xform[10] = r.xf.a.t.y;
    p.xform[11] = r.xf.a.t.z;
}

// The capacities the first pass asks for.
int initial_wants(o2v_hip_ctx *ctx, const Switches &sw, Run &r)
{
    const uint64_t T = ctx->n_tris;
    const bool tiny = sw.tiny_buffers;  // (test hook: minimal buffers, so that every overflow -> grow -> re-run path is exercised)
    r.want_leaves = std::max<uint64_t>(ctx->d_leaves.cap, tiny ? 64 : T + T / 4 + (1u << 16));
    r.want_tiles = std::max<uint64_t>(ctx->d_tiles.cap, tiny ? 64 : T + T / 2 + (1u << 16));
    r.want_big = std::max<uint64_t>(ctx->d_big.cap, tiny ? 4 : 1u << 16);
    r.want_nodes = std::max<uint64_t>(ctx->d_nodes[0].cap, tiny ? 16 : 1u << 18);
    r.want_hits = std::max<uint64_t>(ctx->d_pool.cap, tiny ? 512 : std::min<uint64_t>(16 * T + (4u << 20), 1ull << 31));
    r.want_vox = std::max<uint64_t>(ctx->d_occ.cap, tiny ? 256 : std::min<uint64_t>(8 * T + (2u << 20), 1ull << 31));
    r.want_scratch = std::min(ctx->d_scratch_key.cap, ctx->d_scratch_idx.cap);
    // Hit slabs: one per listed brick (about 1.3 x the bricks that end up holding voxels on a tessellated surface).  They are a
    // budget, not a requirement - a listed brick beyond cap_slabs pools all its hits - so a pass is never repeated for them:
    // the capacity follows the last pass's list (ctx->want_slabs_next) up to a sixth of the device memory.
    if (ctx->slabs_stride != ctx->sorted_stride) {
        O2V_CHECK(ctx->d_slabs.release());  // (the records' size changed: the allocation is counted in slabs of the new size)
        ctx->slabs_stride = ctx->sorted_stride;
        ctx->slabs_wanted_at_grant = 0;
    }
    r.want_slabs = 0;
    if (!r.p.occupancy_only) {
        size_t free_b = 0, total_b = 0;
        O2V_CHECK(hipMemGetInfo(&free_b, &total_b));
        const uint64_t slab_bytes = (uint64_t) kInlineHits * kBrickCells * ctx->slabs_stride * sizeof(uint32_t);
        const uint64_t budget = std::max<uint64_t>(total_b / 6 / slab_bytes, 1);
        const uint64_t cap_slabs = ctx->cap_slabs();
        r.want_slabs = std::max<uint64_t>(ctx->want_slabs_next, T / 2 + (1u << 14));
        r.want_slabs = std::min<uint64_t>(std::min<uint64_t>(r.want_slabs, r.n_bricks), budget);
        r.want_slabs = std::max<uint64_t>(r.want_slabs, cap_slabs);
        if (tiny) r.want_slabs = std::max<uint64_t>(cap_slabs, 4);
        if (sw.no_slabs) r.want_slabs = cap_slabs;  // (A/B: every hit pooled)
    }
    return O2V_HIP_OK;
}

// The launches the hints let a pass leave out: subdivision rounds, k_expand_big (ctx->skip_big) and k_expand_roots (solo roots).
void plan_rounds(o2v_hip_ctx *ctx, const o2v_hip_params *params, const Switches &sw, Run &r)
{
    Params &p = r.p;
    // Subdivision rounds to launch: every round halves a node's extents and a node becomes a leaf once its voxel
    // AABB volume is below 512, so ceil(log2(S)) rounds cover the usual case; if a node is still waiting after the
    // last round the pass is repeated with the full kMaxRounds (nothing is lost, only re-run).
    r.n_rounds = 4;
    while ((1u << r.n_rounds) < p.S && r.n_rounds < kMaxRounds) ++r.n_rounds;
    ctx->skip_big = false;
    bool solo_ok = false;
    if (ctx->max_tri_extent >= 0.f) {
        // tighter: a (sub-)triangle whose extent is at most 5 voxels has a voxel AABB of at most 7^3 < 512 cells and is
        // a leaf; every round halves the extents.  Scale = the mesh transform's (obj2voxel.cpp:370-402).
        const MeshScale m = mesh_scale(ctx, params);
        // (the largest triangle's extent in voxels, rounded up a little; its voxel box has at most extent + 2 cells per axis)
        const float ext_vox = ctx->max_tri_extent * m.unit_norm * ((float) p.S / m.max_axis) * 1.0001f + 1e-3f;
        if (m.max_axis > 0.f && ext_vox == ext_vox && ext_vox < 3.0e9f) {
            // a (sub-)triangle less than 6 voxels across has a box of fewer than 8^3 = 512 cells and is a leaf: a mesh of such
            // triangles needs no subdivision round at all (most tessellated surfaces at their resolution), one `depth` halvings
            // larger needs `depth` rounds
            uint32_t depth = 0;
            for (float e = ext_vox; e > 5.9f; e *= 0.5f) ++depth;
            r.n_rounds = std::min<uint32_t>(r.n_rounds, depth);
            // ... and a leaf less than 7.9 voxels across has fewer than 10^3 cells = four tiles: none for k_expand_big (a larger
            // one can only be an axis-aligned triangle, voxelization.cpp:335-347)
            ctx->skip_big = ext_vox < 7.9f;
            solo_ok = ext_vox < 4.99f;
        }
    }
    if (sw.all_launches) {  // (A/B: no launch left out on the strength of the hints)
        r.n_rounds = std::max<uint32_t>(r.n_rounds, 1u);
        ctx->skip_big = false;
        solo_ok = false;
    }
    // Occupancy only, every triangle less than 5 voxels across (the largest extent, known since the upload, at this call's scale):
    // its voxel box has at most 6 cells per axis - 216: below the subdivision limit of 512 (voxelization.cpp:488-511) and one tile -
    // so every root triangle is a leaf of one tile or misses the slab, and k_expand_roots (K1) would write nothing: it is not
    // launched, k_voxelize_occ makes the leaves (as with root_bypass) and counts them.  The kernel checks the premise per triangle
    // (kErrSoloRoots); should it ever fail, the pass is repeated with K1 and this mesh keeps it.
    r.solo_key = ctx->tri_generation * 1000003ull + p.S * 131ull + p.zs0 * 31ull + p.zs1 + 1u;
    // (O2V_TEST_FORCE_SOLO_ROOTS: whatever the hint says)
    ctx->solo_roots = p.root_bypass && (solo_ok || sw.force_solo_roots) && ctx->solo_refused_key != r.solo_key && !sw.no_solo_roots;
    p.solo_roots = ctx->solo_roots ? 1u : 0u;
}

// Sizes the work buffers for the next pass and puts their capacities into Params.  The buffers a pass cannot do without come
// first; the hit slabs - a budget, the pass runs without them - take what is left afterwards, and give way (are freed, then
// the allocation is tried again) if one of the others does not fit.
int size_buffers(o2v_hip_ctx *ctx, Run &r)
{
    Params &p = r.p;
    auto required = [&](auto &a, uint64_t want) -> int {
        int rc_g = grow(ctx, a, want);
        if (rc_g == O2V_HIP_ERR_OUT_OF_MEMORY && ctx->d_slabs.ptr) {
            (void) hipGetLastError();
            (void) ctx->d_slabs.release();
            r.want_slabs = 0;  // (this call goes on without slabs: every hit is pooled)
            rc_g = grow(ctx, a, want);
        }
        return rc_g;
    };
    int rc;
    if ((rc = required(ctx->d_leaves, r.want_leaves))) return rc;
    if ((rc = required(ctx->d_tiles, r.want_tiles))) return rc;
    if ((rc = required(ctx->d_big, r.want_big))) return rc;
    if (ctx->lean_roots && (rc = required(ctx->d_need_list, (ctx->n_tris + kBlock - 1) / kBlock))) return rc;
    if ((rc = required(ctx->d_nodes[0], r.want_nodes)) || (rc = required(ctx->d_nodes[1], r.want_nodes))) return rc;
    if ((rc = required(ctx->d_pool, r.want_hits)) || (rc = required(ctx->d_sorted, r.want_hits))) return rc;
    if ((rc = required(ctx->d_occ, r.want_vox)) || (rc = required(ctx->d_out, r.want_vox))) return rc;
    if (p.pick_max) {
        if ((rc = required(ctx->d_pick_extra, r.want_vox))) return rc;
        p.pick_extra = reinterpret_cast<uint32_t *>(ctx->d_pick_extra.ptr);
    }
    uint64_t cap_vox = std::min(ctx->d_occ.cap, ctx->d_out.cap);
    for (DevArray<uint32_t> *list : {&ctx->d_list_lane8, &ctx->d_list_lane16, &ctx->d_list_w64, &ctx->d_list_lane, &ctx->d_list_mid,
                                     &ctx->d_list_long, &ctx->d_list_big, &ctx->d_list_huge}) {
        if ((rc = required(*list, r.want_vox))) return rc;
        cap_vox = std::min(cap_vox, list->cap);
    }
    if (r.want_scratch && ((rc = required(ctx->d_scratch_key, r.want_scratch)) || (rc = required(ctx->d_scratch_idx, r.want_scratch)))) return rc;
    // (a grant below what was asked for - the memory was short - is kept until more is asked for than then: asking again
    // with every call would free and allocate the slabs every time)
    const uint64_t slab_words = (uint64_t) kInlineHits * kBrickCells * ctx->slabs_stride;
    if (r.want_slabs > ctx->cap_slabs() && !(ctx->cap_slabs() && r.want_slabs <= ctx->slabs_wanted_at_grant)) {
        ctx->slabs_wanted_at_grant = r.want_slabs;
        O2V_CHECK(ctx->d_slabs.release());
        // (what is free now, every required buffer being in place, less 1 GiB for what a later pass may have to grow)
        size_t free_now = 0, total_now = 0;
        O2V_CHECK(hipMemGetInfo(&free_now, &total_now));
        const uint64_t slab_bytes = slab_words * sizeof(uint32_t);
        const uint64_t room = free_now > (1ull << 30) ? ((uint64_t) free_now - (1ull << 30)) / slab_bytes : 0ull;
        const uint64_t n_slabs_now = std::min<uint64_t>(std::min<uint64_t>(r.want_slabs, room), kMaxRecords);
        if (!n_slabs_now || ctx->d_slabs.alloc(n_slabs_now * slab_words) != hipSuccess) (void) hipGetLastError();  // (no slabs: every hit is pooled)
        r.want_slabs = ctx->cap_slabs();
    }
    p.cap_leaves = (uint32_t) ctx->d_leaves.cap;
    p.cap_tiles = (uint32_t) ctx->d_tiles.cap;
    p.cap_big = (uint32_t) ctx->d_big.cap;
    p.cap_nodes = (uint32_t) std::min(ctx->d_nodes[0].cap, ctx->d_nodes[1].cap);
    p.cap_hits = (uint32_t) std::min(ctx->d_pool.cap, ctx->d_sorted.cap);
    p.cap_vox = (uint32_t) cap_vox;
    p.cap_slabs = ctx->cap_slabs();
    p.slab_stride = ctx->slabs_stride;
    p.slabs = ctx->d_slabs.ptr;
    p.brick_slab = ctx->d_brick_slab.ptr;
    return O2V_HIP_OK;
}

// After a pass: whether it stands, or has to be repeated (`again`: larger buffers, more rounds, or without a shortcut whose
// premise did not hold) - or the call fails.  The rules are checked in this order.
int check_pass(o2v_hip_ctx *ctx, Run &r, bool &again)
{
    Params &p = r.p;
    const Counters &h = *ctx->h_ctr.ptr;
    again = false;
    if (p.solo_roots && (h.err_flags & kErrSoloRoots)) {
        // a root triangle that is k_expand_roots' business although the hint ruled that out: the pass again, with K1
        ctx->solo_refused_key = r.solo_key;
        ctx->solo_roots = false;
        p.solo_roots = 0;
        again = true;
        return O2V_HIP_OK;
    }
    if (h.err_flags) {
        // (a dirty-list overflow leaves bricks behind that no list names: the grids stay marked for a full clear)
        // (nor does a pass that ran without a brick list - mark_missing - clean up behind itself)
        if (!(h.err_flags & kErrDirtyList) && !p.occupancy_only && ctx->last_ran_general && ctx->marked_bricks) ctx->grid_dirty = false;
        ctx->mark_missing = false;
        ctx->err = (h.err_flags & kErrLeafTooLarge) ? "a leaf's voxel AABB has 2^32 or more candidate voxels"
                   : (h.err_flags & kErrDepth)      ? "subdivision deeper than 15 levels"
                   : (h.err_flags & kErrDirtyList)  ? "more than 2^27 bricks of the slab hold voxels; use more z-slabs"
                   : (h.err_flags & kErrCounterWrap) ? "2^32 or more leaves or tiles in one slab; use more z-slabs"
                                                    : "a voxel received 2^24 or more hits";
        return O2V_HIP_ERR_LIMIT;
    }
    const uint32_t max_nodes = *std::max_element(h.n_nodes, h.n_nodes + kMaxRounds + 1);
    auto need = [&](uint64_t used, uint32_t cap, uint64_t &want) {
        if (used > cap) {
            want = used + used / 4 + 1024;
            again = true;
        }
    };
    need(h.n_leaves, p.cap_leaves, r.want_leaves);
    need(h.n_tiles, p.cap_tiles, r.want_tiles);
    need(h.n_big, p.cap_big, r.want_big);
    need(max_nodes, p.cap_nodes, r.want_nodes);
    need(h.n_hits_reserved, p.cap_hits, r.want_hits);
    need(h.n_sorted, p.cap_hits, r.want_hits);  // (the sorted array also holds what the slabs held of the crowded cells)
    if (!p.occupancy_only) ctx->want_slabs_next = std::max<uint64_t>(ctx->want_slabs_next, (uint64_t) h.n_dirty + h.n_dirty / 8 + 64);
    need(h.n_vox, p.cap_vox, r.want_vox);
    if (p.direct_max) need(h.n_out, p.cap_vox, r.want_vox);
    if (r.n_rounds < kMaxRounds && h.n_nodes[r.n_rounds] != 0) {
        r.n_rounds = kMaxRounds;  // unusually deep subdivision (or the hint about the largest triangle did not hold)
        again = true;
    }
    if (ctx->skip_big && h.n_big != 0) {
        ctx->skip_big = false;  // a leaf of more than four tiles although the hint ruled that out: with k_expand_big, then
        again = true;
    }
    if (ctx->mark_missing) {
        // (run_pass left k_mark_bricks out on the strength of the last pass and K1's counters then asked for the general route)
        ctx->mark_missing = false;
        again = true;
    }
    if (!again && !ctx->last_ran_general && h.n_hits != h.n_direct) {
        // The stages behind k_voxelize were chosen from K1's counters alone, on the premise that only leaves of subdivided
        // triangles are pooled (order key 0 <=> unsplit triangle, a convention of k_expand_*).  Pooled hits exist although
        // the sort + replay stages were skipped: run the pass again with them.
        ctx->force_general = true;
        again = true;
    }
    const uint64_t cap_scratch = std::min(ctx->d_scratch_key.cap, ctx->d_scratch_idx.cap);
    if (!again && h.n_huge && (!ctx->d_scratch_key.ptr || h.scratch_used > cap_scratch)) {
        // some cell holds more than kLongList hits: the global-memory sort tier needs its scratch area
        r.want_scratch = std::max<uint64_t>(2ull * p.cap_hits, (uint64_t) h.scratch_used + 1024);
        again = true;
    }
    if (!again && ctx->last_ran_general && (uint32_t) (h.n_hits - h.n_direct) != h.n_listed_hits) {
        // k_voxelize counted a hit into a cell of a brick that k_mark_bricks did not list (the two must agree on the leaf's
        // clamped box, supersampling shift and slab origin): its voxel would be missing and its counter would stay behind
        // for the next run.  Never seen; checked because nothing else would notice.  The grids are cleared before the next call.
        ctx->grid_dirty = true;
        ctx->maxgrid_dirty = true;
        ctx->err = "internal error: hits outside the listed bricks (" + std::to_string(h.n_hits - h.n_direct) + " counted, " +
                   std::to_string(h.n_listed_hits) + " listed)";
        return O2V_HIP_ERR_HIP;
    }
    return O2V_HIP_OK;
}

// Whether the pass that stood emitted its records from the 64-bit max grid (direct_active() on the device): h.n_out records, else h.n_vox.
bool pass_direct(const Params &p, const Counters &h) { return p.direct_max && (p.occupancy_only || h.n_nodes[0] <= h.n_root_leaves); }

// K6's box of extent n from lo (output voxels) at supersampling ss; argb: the colour of its interior records.
FillBox fill_box(const uint32_t lo[3], const uint32_t n[3], uint32_t ss, uint32_t argb)
{
    const uint32_t nzw = (n[2] + 31u) / 32u;
    const uint64_t n_cols = (uint64_t) n[0] * n[1];
    return FillBox{lo[0], lo[1], lo[2], n[0], n[1], n[2], nzw, ss, argb, n_cols, (uint64_t) nzw * n_cols};
}

// K6's parity set of box b as a bitmap in ctx->d_fill_bits ([z-word][y][x]): the crossings of the context's triangles (sample
// space by xf) toggled and prefix-XORed along z, cut at the mesh's top layer.  Enqueued on the context's stream; the fill stage
// and o2v_hip_mesh_distance_dense (K9) share it.
int parity_bits(o2v_hip_ctx *ctx, const Affine &xf, const FillBox &b)
{
    hipStream_t s = ctx->stream;
    const uint64_t T = ctx->n_tris, n_blocks = (T + kBlock - 1) / kBlock;
    int rc;
    if ((rc = grow(ctx, ctx->d_fill_bits, b.n_words, kNoLimit)) || (rc = grow(ctx, ctx->d_fill_ends, T, kNoLimit)) ||
        (rc = grow(ctx, ctx->d_fill_blocks, n_blocks, kNoLimit)) || (rc = grow(ctx, ctx->d_fill_ctr, 3)))
        return rc;
    O2V_CHECK(hipMemsetAsync(ctx->d_fill_bits.ptr, 0, b.n_words * sizeof(uint32_t), s));
    O2V_CHECK(hipMemsetAsync(ctx->d_fill_ctr.ptr, 0, 3 * sizeof(unsigned long long), s));
    const uint32_t persistent = (uint32_t) ctx->num_cus * 8u;
    if (T) {
        O2V_LAUNCH("k_fill_count", s, k_fill_count, dim3((uint32_t) n_blocks), dim3(kBlock), 0, s, ctx->d_verts.ptr, T, xf, b,
                   ctx->d_fill_ends.ptr, ctx->d_fill_blocks.ptr, ctx->d_fill_ctr.ptr + 2);
        O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, ctx->d_fill_blocks.ptr, n_blocks, ctx->d_fill_ctr.ptr);
        O2V_LAUNCH("k_fill_offsets", s, k_fill_offsets, dim3((uint32_t) n_blocks), dim3(kBlock), 0, s, ctx->d_fill_ends.ptr, T, ctx->d_fill_blocks.ptr);
        O2V_LAUNCH("k_fill_cross", s, k_fill_cross, dim3(persistent), dim3(kBlock), 0, s, ctx->d_verts.ptr, T, xf, b, ctx->d_fill_ends.ptr,
                   ctx->d_fill_ctr.ptr, ctx->d_fill_bits.ptr);
    }
    O2V_LAUNCH("k_fill_prefix", s, k_fill_prefix, dim3((uint32_t) ((b.n_cols + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ctx->d_fill_bits.ptr, b,
               ctx->d_fill_ctr.ptr + 2);
    return O2V_HIP_OK;
}

// K6, the solid fill (O2V_HIP_FLAG_FILL_INTERIOR), behind the n_surf surface records of the pass that stood: appends the
// interior records of the pass box to d_out (o2v_dev_k6_fill.hpp) and returns their number in n_interior.
int fill_stage(o2v_hip_ctx *ctx, const o2v_hip_params *params, const Run &r, uint64_t n_surf, uint64_t &n_interior)
{
    hipStream_t s = ctx->stream;
    n_interior = 0;
    const uint32_t n[3] = {r.box.hi[0] - r.box.lo[0], r.box.hi[1] - r.box.lo[1], r.box.hi[2] - r.box.lo[2]};
    const FillBox b = fill_box(r.box.lo, n, params->supersampling ? params->supersampling : 1u, params->fill_argb);
    const uint64_t T = ctx->n_tris, n_blocks = (T + kBlock - 1) / kBlock;
    const uint64_t n_chunks = (b.n_words + kFillChunk - 1) / kFillChunk;
    // (kMaxRecords: the grids' arrays of 32-bit capacity; the bitmap is indexed in 64 bits, its limit is the memory)
    int rc;
    if ((rc = grow(ctx, ctx->d_fill_bits, b.n_words, kNoLimit)) || (rc = grow(ctx, ctx->d_fill_ends, T, kNoLimit)) ||
        (rc = grow(ctx, ctx->d_fill_blocks, n_blocks, kNoLimit)) || (rc = grow(ctx, ctx->d_fill_chunks, n_chunks, kNoLimit)) ||
        (rc = grow(ctx, ctx->d_fill_ctr, 3)) || (rc = grow(ctx, ctx->h_fill_ctr, 2)))
        return rc;
    if (ctx->stage_events) O2V_CHECK(ctx->fill_times.mark(0, s));
    Affine xf;
    const float *x = ctx->h_ctr.ptr->xform;  // (k_setup's transform of this pass)
    for (int i = 0; i < 3; ++i) xf.m[i] = {x[i * 3], x[i * 3 + 1], x[i * 3 + 2]};
    xf.t = {x[9], x[10], x[11]};
    if ((rc = parity_bits(ctx, xf, b))) return rc;
    const uint32_t persistent = (uint32_t) ctx->num_cus * 8u;
    if (n_surf)
        O2V_LAUNCH("k_fill_unmark", s, k_fill_unmark, dim3((uint32_t) std::min<uint64_t>(persistent, (n_surf + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                   ctx->d_out.ptr, n_surf, b, ctx->d_fill_bits.ptr);
    const uint32_t chunk_wgs = (uint32_t) std::min<uint64_t>(persistent, (n_chunks + kBlock / 64u - 1) / (kBlock / 64u));
    O2V_LAUNCH("k_fill_count_words", s, k_fill_count_words, dim3(chunk_wgs), dim3(kBlock), 0, s, ctx->d_fill_bits.ptr, b, ctx->d_fill_chunks.ptr,
               ctx->d_fill_ctr.ptr + 1);
    O2V_CHECK(hipMemcpyAsync(ctx->h_fill_ctr.ptr, ctx->d_fill_ctr.ptr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    n_interior = ctx->h_fill_ctr.ptr[1];
    const uint64_t need = n_surf + n_interior;
    if (need > kMaxRecords) {
        ctx->err = "the pass has 2^32 or more records with its interior voxels; use more z-slabs or x / y tiles";
        return O2V_HIP_ERR_LIMIT;
    }
    if (n_interior) {
        if (need > ctx->d_out.cap) {
            // (exactly what is needed, the surface records moved over: the interior can be most of the device's memory)
            DevArray<uint4> bigger;
            O2V_CHECK(bigger.alloc(need));
            if (n_surf) O2V_CHECK(hipMemcpyAsync(bigger.ptr, ctx->d_out.ptr, n_surf * sizeof(uint4), hipMemcpyDeviceToDevice, s));
            O2V_CHECK(hipStreamSynchronize(s));
            ctx->d_out = std::move(bigger);  // (the old array goes with `bigger`)
        }
        O2V_LAUNCH("k_fill_emit", s, k_fill_emit, dim3(chunk_wgs), dim3(kBlock), 0, s, ctx->d_fill_bits.ptr, b, ctx->d_fill_chunks.ptr, n_surf,
                   ctx->d_out.ptr);
    }
    if (ctx->stage_events) O2V_CHECK(ctx->fill_times.mark(1, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(hipGetLastError());
    if (ctx->stage_events) O2V_CHECK(ctx->fill_times.elapsed(0, 1, ctx->timings.fill_ms));
    return collect_kernel_times(ctx);
}

// The results of the pass that stood: counts, stats, stage times and the transform.  n_interior: records of the solid fill behind
// the surface records (0 without O2V_HIP_FLAG_FILL_INTERIOR).
int publish(o2v_hip_ctx *ctx, const Run &r, uint64_t n_interior, uint64_t *out_voxel_count)
{
    const Params &p = r.p;
    const Counters &h = *ctx->h_ctr.ptr;
    if (!p.occupancy_only) ctx->grid_dirty = false;
    ctx->maxgrid_dirty = false;
    const bool direct = pass_direct(p, h);
    const uint64_t n_final = (direct ? h.n_out : h.n_vox) + n_interior;
    ctx->last_direct = direct;
    ctx->n_vox = n_final;
    o2v_hip_stats &st = ctx->stats;
    st.interior_voxels = n_interior;
    st.leaves = h.n_leaves + h.n_bypass;  // (root_bypass: leaves of one tile that k_voxelize_occ made itself)
    st.tiles = h.n_tiles + h.n_bypass;
    st.candidates = h.n_candidates;
    st.hits = h.n_hits;
    st.voxels = n_final;
    st.direct_hits = h.n_direct;
    st.jobs = h.n_jobs;
    st.certain_hits = h.n_certain;
    st.skipped_jobs = h.n_jobs_skipped;
    st.bypassed_leaves = h.n_bypass;
    st.bricks = p.n_bricks;
    st.dirty_bricks = direct ? h.n_dirty_max : h.n_dirty;
    st.pool_slots = h.n_hits_reserved;
    std::memcpy(ctx->xform, h.xform, sizeof(ctx->xform));
    for (int i = 0; i < 16; ++i) ctx->dbg[i] = h.dbg[i];
    o2v_hip_timings &t = ctx->timings;
    float *const stage_ms[5] = {&t.bounds_ms, &t.expand_ms, &t.voxelize_ms, &t.scan_ms, &t.resolve_ms};  // (between marks i and i + 1)
    if (ctx->stage_events) {
        for (int i = 0; i < 5; ++i) O2V_CHECK(ctx->pass_times.elapsed(i, i + 1, *stage_ms[i]));
        O2V_CHECK(ctx->pass_times.elapsed(0, 5, t.total_ms));
    }
    else O2V_CHECK(ctx->pass_times.elapsed(2, 3, t.voxelize_ms));  // (k_voxelize's own dispatch: O2V_LAUNCH_K2)
    if (out_voxel_count) *out_voxel_count = ctx->n_vox;
    return O2V_HIP_OK;
}

// O2V_HIP_FLAG_KERNEL_TIMES holds while voxelize() runs and no longer: the launches of every other call go unbracketed.
struct KernelTimesScope {
    o2v_hip_ctx *ctx;
    KernelTimesScope(o2v_hip_ctx *c, bool on) : ctx(c) { ctx->ktimes_on = on; }
    ~KernelTimesScope() { ctx->ktimes_on = false; }
    KernelTimesScope(const KernelTimesScope &) = delete;
    KernelTimesScope &operator=(const KernelTimesScope &) = delete;
};

// o2v_hip_voxelize with the switches read by the caller (o2v_hip_voxelize_sharded reads them once for the whole call).
int voxelize(o2v_hip_ctx *ctx, const o2v_hip_params *params, const Switches &sw, uint64_t *out_voxel_count)
{
    if (out_voxel_count) *out_voxel_count = 0;
    const KernelTimesScope kernel_times(ctx, (params->flags & O2V_HIP_FLAG_KERNEL_TIMES) != 0);
    Run r;
    bool empty = false;
    int rc;
    if ((rc = pass_geometry(ctx, params, sw, r, empty)) || empty) return rc;
    ctx->stage_events = (params->flags & (O2V_HIP_FLAG_STAGE_TIMES | O2V_HIP_FLAG_KERNEL_TIMES)) != 0;
    ctx->kernel_times.clear();
    choose_routes(ctx, params, sw, r);
    if ((rc = ensure_grids(ctx, r))) return rc;
    if (ctx->n_tris == 0) return O2V_HIP_OK;  // empty mesh: empty model (obj2voxel.cpp:590-594)
    host_k0(sw, r);  // (behind ensure_grids: the route is final)
    // (= workgroups x VoxShape::queue for every shape; twice that for k_voxelize_occ)
    const uint64_t jobq = (uint64_t) ctx->num_cus * (O2V_K2_WAVES > O2V_K2_WAVES_UV ? O2V_K2_WAVES : O2V_K2_WAVES_UV) * (kBlock / 64u) * (64u * 64u) * 2u;
    if ((rc = grow(ctx, ctx->d_jobq, jobq))) return rc;
    if ((rc = initial_wants(ctx, sw, r))) return rc;
    plan_rounds(ctx, params, sw, r);
    ctx->force_general = false;
    ctx->mark_missing = false;  // (a call that ended early - an error, a failed allocation - must not leave it to the next one)
    if (!r.p.occupancy_only) ctx->grid_dirty = true;  // until a pass completes (the scan / reset kernels leave it clean)
    if (r.p.direct_max) ctx->maxgrid_dirty = true;
    for (uint32_t pass = 1; pass <= 12; ++pass) {
        // (a pass that overflowed a buffer may have left counters / offsets in cells it could not list)
        if (pass > 1 && (rc = clear_grids(ctx, !r.p.occupancy_only, r.p.direct_max))) return rc;
        if ((rc = size_buffers(ctx, r))) return rc;
        if ((rc = run_pass(ctx, r.p, sw, r.use_uv, r.n_rounds))) return rc;
        ctx->timings.passes = pass;
        bool again = false;
        if ((rc = check_pass(ctx, r, again))) return rc;
        if (again) continue;
        uint64_t n_interior = 0;
        if (params->flags & O2V_HIP_FLAG_FILL_INTERIOR) {
            const Counters &h = *ctx->h_ctr.ptr;
            if ((rc = fill_stage(ctx, params, r, pass_direct(r.p, h) ? h.n_out : h.n_vox, n_interior))) return rc;
        }
        return publish(ctx, r, n_interior, out_voxel_count);
    }
    ctx->err = "device buffers did not converge after 12 passes";
    return O2V_HIP_ERR_LIMIT;
}

}  // namespace

namespace o2v {

hipStream_t ctx_stream(o2v_hip_ctx *ctx) { return ctx->stream; }
int ctx_device(const o2v_hip_ctx *ctx) { return ctx->device; }

int ctx_alloc_triangles(o2v_hip_ctx *ctx, uint64_t count, bool uvs, bool types, bool colors, bool texids)
{
    if (count >= (1ull << 29)) {
        ctx->err = "triangle count must be below 2^29";
        return O2V_HIP_ERR_LIMIT;
    }
    O2V_CHECK(hipSetDevice(ctx->device));
    O2V_CHECK(hipStreamSynchronize(ctx->stream));  // nothing may still read the arrays that are about to be replaced
    // (an array grows only when it has to: repeated uploads of similar meshes reuse the allocation; an absent optional array is
    // released - it must read as null in the kernels: all MATERIALLESS / zero uvs / texture 0)
    auto size = [&](auto &a, uint64_t n, bool wanted) -> int {
        if (wanted && n) return grow(ctx, a, n, kNoLimit);
        O2V_CHECK(a.release());
        return O2V_HIP_OK;
    };
    int rc;
    if ((rc = size(ctx->d_verts, count * 9, true)) || (rc = size(ctx->d_uvs, count * 6, uvs)) || (rc = size(ctx->d_types, count, types)) ||
        (rc = size(ctx->d_colors, count * 3, colors)) || (rc = size(ctx->d_texids, count, texids)))
        return rc;
    ctx->n_tris = count;
    ctx->tri_generation += 1;
    ctx->bounds_generation = ~0ull;  // (the arrays are about to be replaced: ctx_finish_triangles brings the new bounds)
    ctx->max_tri_extent = -1.f;
    ctx->any_textured = false;
    return O2V_HIP_OK;
}

TriBuffers ctx_tri_buffers(o2v_hip_ctx *ctx)
{
    return TriBuffers{ctx->d_verts.ptr, ctx->d_uvs.ptr, ctx->d_types.ptr, ctx->d_colors.ptr, ctx->d_texids.ptr, ctx->n_tris};
}

TriHints ctx_tri_hints(const o2v_hip_ctx *ctx)
{
    TriHints h;
    h.any_textured = ctx->any_textured;
    for (int i = 0; i < 6; ++i) h.bounds[i] = ctx->mesh_bounds_hint[i];
    h.max_tri_extent = ctx->max_tri_extent;
    std::memcpy(h.ext_hist, ctx->ext_hist, sizeof(h.ext_hist));
    return h;
}

// After the arrays are filled (on ctx's stream): records whether any triangle is textured and the launch-configuration
// hints (mesh bounds and largest triangle extent, see k_tri_extent) - taken from `hints` if another rank already
// computed them for the same triangles, else computed here.  Waits for the stream.
int ctx_finish_triangles(o2v_hip_ctx *ctx, bool any_textured, const TriHints *hints)
{
    O2V_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t count = ctx->n_tris;
    ctx->any_textured = any_textured;
    if (hints) {
        for (int i = 0; i < 6; ++i) ctx->mesh_bounds_hint[i] = hints->bounds[i];
        ctx->bounds_generation = ctx->tri_generation;
        ctx->max_tri_extent = hints->max_tri_extent;
        std::memcpy(ctx->ext_hist, hints->ext_hist, sizeof(ctx->ext_hist));
        ctx->any_textured = hints->any_textured;
    }
    else if (count) {
        Counters *const ctr = ctx->d_ctr.ptr;
        ctx->ctr_clean = false;
        hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, s, ctr, (uint32_t) (sizeof(Counters) / 4));
        hipLaunchKernelGGL(k_bounds, dim3((uint32_t) std::min<uint64_t>((uint64_t) ctx->num_cus, (count * 9 / 12 + kBoundsBlock) / kBoundsBlock)),
                           dim3(kBoundsBlock), 0, s, ctx->d_verts.ptr, count * 9, ctr);
        hipLaunchKernelGGL(k_tri_extent, dim3((uint32_t) std::min<uint64_t>((uint64_t) ctx->num_cus * 4u, (count + kBlock - 1) / kBlock)),
                           dim3(kBlock), 0, s, ctx->d_verts.ptr, count, &ctr->pad2, ctr->ext_hist);
        O2V_CHECK(hipMemcpyAsync(ctx->h_ctr.ptr, ctr, sizeof(Counters), hipMemcpyDeviceToHost, s));
        O2V_CHECK(hipStreamSynchronize(s));
        for (int i = 0; i < 6; ++i) ctx->mesh_bounds_hint[i] = ord2f_host(ctx->h_ctr.ptr->bounds_enc[i]);
        ctx->bounds_generation = ctx->tri_generation;
        ctx->max_tri_extent = ord2f_host(ctx->h_ctr.ptr->pad2);
        std::memcpy(ctx->ext_hist, ctx->h_ctr.ptr->ext_hist, sizeof(ctx->ext_hist));
        return O2V_HIP_OK;
    }
    O2V_CHECK(hipStreamSynchronize(s));
    return O2V_HIP_OK;
}

}  // namespace o2v

extern "C" {

int o2v_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int o2v_hip_create(int device, o2v_hip_ctx **out_ctx)
{
    if (!out_ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    *out_ctx = nullptr;
    int n = 0;
    // (O2V_INIT_TIMES=1: where a new process' first session spends its time - the runtime's start is most of a CLI run)
    const char *init_times = std::getenv("O2V_INIT_TIMES");
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!(init_times && init_times[0] == '1')) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[o2v_hip_create] %s: %.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return O2V_HIP_ERR_NO_DEVICE;
    lap("hipGetDeviceCount (runtime start)");
    if (hipSetDevice(device) != hipSuccess) return O2V_HIP_ERR_NO_DEVICE;
    lap("hipSetDevice");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return O2V_HIP_ERR_NO_DEVICE;
    lap("hipGetDeviceProperties");
    o2v_hip_ctx *ctx = new o2v_hip_ctx;
    auto fail = [&](int rc) {
        delete ctx;
        return rc;
    };
    ctx->device = device;
    ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (ctx->stream.create() != hipSuccess) return fail(O2V_HIP_ERR_HIP);
    lap("the stream");
    bool ok = ctx->pass_times.create() == hipSuccess && ctx->ev_fork.create_sync() == hipSuccess &&
              ctx->ev_sorted.create_sync() == hipSuccess && ctx->ev_k1.create_sync() == hipSuccess;
    for (Event &e : ctx->ev_join) ok = ok && e.create_sync() == hipSuccess;
    lap("events");
    // (the auxiliary streams are made by the first pass that needs one - 0.3 ms each in a warm process, 7 - 8 ms in a new one -
    // and the occupancy-only route, every STL, never does)
    if (!ok) return fail(O2V_HIP_ERR_HIP);
    if (ctx->d_ctr.alloc(1) != hipSuccess) return fail(O2V_HIP_ERR_OUT_OF_MEMORY);
    lap("first hipMalloc");
    if (ctx->h_ctr.alloc(1) != hipSuccess) return fail(O2V_HIP_ERR_OUT_OF_MEMORY);
    lap("first hipHostMalloc");
    ctx->d_block_count = &ctx->d_ctr.ptr->n_listed_blocks;
    // k_resolve_big sorts in 96 KiB of dynamic LDS (above the default 64 KiB limit)
    (void) hipFuncSetAttribute(reinterpret_cast<const void *>(&k_resolve_big), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int) (kBigList * 12u));
    lap("hipFuncSetAttribute (code object)");
    // the first pass' counters, zeroed now: the launch also makes the runtime load the device code here - on the thread that
    // creates the session beside the input's parsing (obj2voxel_voxelize) - rather than in front of the first pass
    hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, ctx->stream, ctx->d_ctr.ptr, kPassCounterWords);
    if (hipStreamSynchronize(ctx->stream) == hipSuccess) ctx->ctr_clean = true;
    else (void) hipGetLastError();
    lap("first launch");
    *out_ctx = ctx;
    return O2V_HIP_OK;
}

void o2v_hip_destroy(o2v_hip_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->poisoned) {
        // a stuck collective is queued on the context's stream (o2v_hip_voxelize_sharded timed out): synchronising or freeing would
        // block for ever.  The device memory goes with the process, which the caller was told to end (include/o2v_hip.h) - and so
        // does the context object: it is left undeleted on purpose, because deleting it would free its arrays.
        return;
    }
    (void) hipSetDevice(ctx->device);
    (void) hipStreamSynchronize(ctx->stream);
    delete ctx;  // (the arrays, events and streams free themselves)
}

const char *o2v_hip_last_error(const o2v_hip_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int o2v_hip_set_triangles(o2v_hip_ctx *ctx, const float *verts, const float *uvs, const uint32_t *types,
                          const float *colors, const int32_t *texids, uint64_t count)
{
    if (!ctx || (count && !verts)) return O2V_HIP_ERR_BAD_ARGUMENT;
    int rc;
    if ((rc = o2v::ctx_alloc_triangles(ctx, count, uvs != nullptr, types != nullptr, colors != nullptr, texids != nullptr))) return rc;
    if (count) {
        hipStream_t s = ctx->stream;
        O2V_CHECK(hipMemcpyAsync(ctx->d_verts.ptr, verts, count * 9 * sizeof(float), hipMemcpyHostToDevice, s));
        if (uvs) O2V_CHECK(hipMemcpyAsync(ctx->d_uvs.ptr, uvs, count * 6 * sizeof(float), hipMemcpyHostToDevice, s));
        if (types) O2V_CHECK(hipMemcpyAsync(ctx->d_types.ptr, types, count * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        if (colors) O2V_CHECK(hipMemcpyAsync(ctx->d_colors.ptr, colors, count * 3 * sizeof(float), hipMemcpyHostToDevice, s));
        if (texids) O2V_CHECK(hipMemcpyAsync(ctx->d_texids.ptr, texids, count * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    // (the host scan overlaps the copies)
    const bool any_textured = types && std::find(types, types + count, (uint32_t) O2V_HIP_TRI_TEXTURED) != types + count;
    return o2v::ctx_finish_triangles(ctx, any_textured, nullptr);
}

int o2v_hip_begin_triangles(o2v_hip_ctx *ctx, o2v_hip_staging *out_block)
{
    if (!ctx || !out_block) return O2V_HIP_ERR_BAD_ARGUMENT;
    O2V_CHECK(hipSetDevice(ctx->device));
    O2V_CHECK(hipStreamSynchronize(ctx->stream));
    if (!ctx->stage[0].verts.ptr) {
        for (int b = 0; b < 2; ++b) {
            O2V_CHECK(ctx->stage[b].verts.alloc(kStageTriangles * 9));
            O2V_CHECK(ctx->ev_stage[b].create_sync());
        }
    }
    ctx->stage_cur = 0;
    ctx->stream_count = 0;
    ctx->stream_arrays = 0;
    ctx->n_tris = 0;
    ctx->bounds_generation = ~0ull;  // (the commits write over the arrays: the upload's bounds are nobody's until o2v_hip_end_triangles)
    *out_block = ctx->stage[0].view();
    return O2V_HIP_OK;
}

int o2v_hip_stage_arrays(o2v_hip_ctx *ctx, uint32_t arrays, o2v_hip_staging *inout_block)
{
    if (!ctx || !inout_block || !ctx->stage[0].verts.ptr) return O2V_HIP_ERR_BAD_ARGUMENT;
    O2V_CHECK(hipSetDevice(ctx->device));
    for (StageBlock &st : ctx->stage) {
        if ((arrays & O2V_HIP_ARRAY_UVS) && !st.uvs.ptr) O2V_CHECK(st.uvs.alloc(kStageTriangles * 6));
        if ((arrays & O2V_HIP_ARRAY_TYPES) && !st.types.ptr) O2V_CHECK(st.types.alloc(kStageTriangles));
        if ((arrays & O2V_HIP_ARRAY_COLORS) && !st.colors.ptr) O2V_CHECK(st.colors.alloc(kStageTriangles * 3));
        if ((arrays & O2V_HIP_ARRAY_TEXIDS) && !st.texids.ptr) O2V_CHECK(st.texids.alloc(kStageTriangles));
    }
    *inout_block = ctx->stage[ctx->stage_cur].view();
    return O2V_HIP_OK;
}

int o2v_hip_commit_triangles(o2v_hip_ctx *ctx, uint64_t count, uint32_t arrays, o2v_hip_staging *out_next_block)
{
    if (!ctx || !out_next_block || !ctx->stage[0].verts.ptr || count > kStageTriangles) return O2V_HIP_ERR_BAD_ARGUMENT;
    const StageBlock &st = ctx->stage[ctx->stage_cur];
    if (((arrays & O2V_HIP_ARRAY_UVS) && !st.uvs.ptr) || ((arrays & O2V_HIP_ARRAY_TYPES) && !st.types.ptr) ||
        ((arrays & O2V_HIP_ARRAY_COLORS) && !st.colors.ptr) || ((arrays & O2V_HIP_ARRAY_TEXIDS) && !st.texids.ptr)) {
        ctx->err = "an optional triangle array was committed without o2v_hip_stage_arrays";
        return O2V_HIP_ERR_BAD_ARGUMENT;
    }
    const uint64_t have = ctx->stream_count, need = have + count;
    if (need >= (1ull << 29)) {
        ctx->err = "triangle count must be below 2^29";
        return O2V_HIP_ERR_LIMIT;
    }
    O2V_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t fresh = arrays & ~ctx->stream_arrays;  // arrays that appear with this block
    ctx->stream_arrays |= arrays;
    // One array of `width` 4-byte words per triangle: made room for, its earlier triangles given the default if it appears
    // with this block (zero; types: MATERIALLESS), then the block's share copied in.
    auto append = [&](uint32_t bit, auto &a, const auto *staged, uint64_t width, uint32_t fill) -> int {
        static_assert(sizeof(*staged) == 4, "4-byte elements");
        if (bit && !(ctx->stream_arrays & bit)) return O2V_HIP_OK;
        const bool appears = (fresh & bit) != 0;
        if (const int rc_a = grow_keep(ctx, a, appears ? 0 : have * width, need * width, width << 20)) return rc_a;
        if (appears && have) O2V_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.ptr), (int) fill, have * width, s));
        if (count) O2V_CHECK(hipMemcpyAsync(a.ptr + have * width, staged, count * width * 4u, hipMemcpyHostToDevice, s));
        return O2V_HIP_OK;
    };
    int rc;
    if ((rc = append(0u, ctx->d_verts, st.verts.ptr, 9, 0u)) || (rc = append(O2V_HIP_ARRAY_UVS, ctx->d_uvs, st.uvs.ptr, 6, 0u)) ||
        (rc = append(O2V_HIP_ARRAY_TYPES, ctx->d_types, st.types.ptr, 1, O2V_HIP_TRI_MATERIALLESS)) ||
        (rc = append(O2V_HIP_ARRAY_COLORS, ctx->d_colors, st.colors.ptr, 3, 0u)) || (rc = append(O2V_HIP_ARRAY_TEXIDS, ctx->d_texids, st.texids.ptr, 1, 0u)))
        return rc;
    O2V_CHECK(hipEventRecord(ctx->ev_stage[ctx->stage_cur], s));
    ctx->stream_count = need;
    ctx->bounds_generation = ~0ull;  // (triangles appended)
    ctx->stage_cur ^= 1;
    O2V_CHECK(hipEventSynchronize(ctx->ev_stage[ctx->stage_cur]));  // the other block's copy (two commits ago) has landed
    *out_next_block = ctx->stage[ctx->stage_cur].view();
    return O2V_HIP_OK;
}

int o2v_hip_end_triangles(o2v_hip_ctx *ctx, uint32_t any_textured)
{
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    O2V_CHECK(hipSetDevice(ctx->device));
    // optional arrays the mesh never used read as null in the kernels
    if (!(ctx->stream_arrays & O2V_HIP_ARRAY_UVS)) retire(ctx, ctx->d_uvs);
    if (!(ctx->stream_arrays & O2V_HIP_ARRAY_TYPES)) retire(ctx, ctx->d_types);
    if (!(ctx->stream_arrays & O2V_HIP_ARRAY_COLORS)) retire(ctx, ctx->d_colors);
    if (!(ctx->stream_arrays & O2V_HIP_ARRAY_TEXIDS)) retire(ctx, ctx->d_texids);
    ctx->n_tris = ctx->stream_count;
    ctx->tri_generation += 1;
    ctx->bounds_generation = ~0ull;
    ctx->max_tri_extent = -1.f;
    const int rc = o2v::ctx_finish_triangles(ctx, any_textured != 0, nullptr);  // waits for the stream
    ctx->retired.clear();
    return rc;
}

int o2v_hip_set_textures(o2v_hip_ctx *ctx, const o2v_hip_texture *textures, uint32_t count)
{
    if (!ctx || (count && !textures)) return O2V_HIP_ERR_BAD_ARGUMENT;
    O2V_CHECK(hipSetDevice(ctx->device));
    ctx->d_texpix.clear();
    O2V_CHECK(ctx->d_textures.release());
    ctx->n_textures = 0;
    if (!count) return O2V_HIP_OK;
    std::vector<DevTexture> host(count);
    for (uint32_t i = 0; i < count; ++i) {
        const o2v_hip_texture &t = textures[i];
        if (!t.pixels || !t.width || !t.height || (t.channels != 3 && t.channels != 4)) {
            ctx->err = "texture must have pixels, a non-zero size and 3 or 4 channels";
            return O2V_HIP_ERR_BAD_ARGUMENT;
        }
        const size_t bytes = (size_t) t.width * t.height * t.channels;
        DevArray<uint8_t> &d = ctx->d_texpix.emplace_back();
        O2V_CHECK(d.alloc(bytes + 8));  // (+ 8: a texel is read as aligned 32-bit words, texel_ref)
        O2V_CHECK(hipMemset(d.ptr + bytes, 0, 8));
        O2V_CHECK(hipMemcpy(d.ptr, t.pixels, bytes, hipMemcpyHostToDevice));
        host[i] = DevTexture{d.ptr, t.width, t.height, t.channels, t.wrap};
    }
    O2V_CHECK(ctx->d_textures.alloc(count));
    O2V_CHECK(hipMemcpy(ctx->d_textures.ptr, host.data(), count * sizeof(DevTexture), hipMemcpyHostToDevice));
    ctx->n_textures = count;
    return O2V_HIP_OK;
}

int o2v_hip_voxelize(o2v_hip_ctx *ctx, const o2v_hip_params *params, uint64_t *out_voxel_count)
{
    if (!ctx || !params) return O2V_HIP_ERR_BAD_ARGUMENT;
    return voxelize(ctx, params, read_switches(), out_voxel_count);
}

}  // extern "C"

namespace {

// The buffers of the slab plan: the z histogram, the z extents of `zrange_blocks` blocks of 256 triangles and the transform
// they were computed with, the block list and - sharded runs - `gather_words` words for the all-gather of the ranks' records.
int size_plan_buffers(o2v_hip_ctx *ctx, uint64_t zrange_blocks, uint64_t gather_words)
{
    const uint64_t n_blocks = (ctx->n_tris + kBlock - 1) / kBlock;
    int rc;
    if ((rc = grow(ctx, ctx->d_zhist, kPlanBins)) || (rc = grow(ctx, ctx->h_zhist, kPlanBins)) || (rc = grow(ctx, ctx->d_zrange_xform, 12)) ||
        (rc = grow(ctx, ctx->d_zrange, std::max<uint64_t>(zrange_blocks, 1))) || (rc = grow(ctx, ctx->d_block_list, std::max<uint64_t>(n_blocks, 1))) ||
        (gather_words && (rc = grow(ctx, ctx->d_plan_gather, gather_words))))
        return rc;
    return O2V_HIP_OK;
}

// The triangle passes of the slab plan over the triangles [tri_begin, tri_end) - this rank's share; a single GPU takes the
// whole list: mesh bounds (unless given: reference findMeshBounds, src/obj2voxel.cpp:180-200), transform, the z
// histogram of predicted work and the z extent of every block of 256 triangles.  With a communicator the partial results
// are combined over the ranks: min / max of the bounds, sum of the histogram, all-gather of the block extents
// (`blocks_per_rank` blocks each).  Afterwards the histogram is in ctx->h_zhist and the counters in ctx->h_ctr.
// `bounds_reduced`: the counters already hold the bounds of the whole mesh (o2v_hip_voxelize_sharded reduces them together with
// the ranks' readiness word); else they are computed - and, with a communicator, reduced - here.
// The collectives are timed (collective_ms, parts_ms: two events and a wait for each) only in a call with
// O2V_HIP_FLAG_STAGE_TIMES: each wait is a round trip to the host that the step otherwise does not make.
int plan_passes(o2v_hip_ctx *ctx, const o2v_hip_params *params, const Switches &sw, uint64_t tri_begin, uint64_t tri_end, o2v_hip_comm *comm,
                uint64_t blocks_per_rank, uint32_t &n_bins, uint32_t &bin_out, float *collective_ms, float *parts_ms = nullptr,
                bool bounds_reduced = false)
{
    const uint32_t ss = params->supersampling ? params->supersampling : 1u;
    const uint32_t G = params->resolution;
    O2V_CHECK(hipSetDevice(ctx->device));
    const uint64_t world = comm ? (uint64_t) comm->world : 1u, n_blocks = (ctx->n_tris + kBlock - 1) / kBlock;
    int rc;
    if ((rc = size_plan_buffers(ctx, comm ? blocks_per_rank * world : n_blocks, comm ? (kPlanBins + blocks_per_rank) * world : 0))) return rc;
    Params p{};
    p.n_tris = ctx->n_tris;
    p.S = G * ss;
    p.G = G;
    for (int k = 0; k < 3; ++k) p.cs_hi[k] = p.S;   // (the planning passes see the whole grid: no crop, no tile)
    p.bounds_known = params->bounds_known;
    for (int i = 0; i < 6; ++i) p.bounds[i] = params->bounds[i];
    for (int i = 0; i < 9; ++i) p.unit[i] = params->unit_transform[i];
    // (what a leaf costs beside its hits, in hit equivalents: k_zhist)
    p.plan_leaf_cost = grid_modes(ctx, params, sw).occupancy_only ? kPlanLeafCostOccupancy : kPlanLeafCost;
    // sample layers per bin: a whole number of output layers, at most kPlanBins bins
    bin_out = (G + kPlanBins - 1) / kPlanBins;
    n_bins = (G + bin_out - 1) / bin_out;
    const uint64_t n_range = tri_end > tri_begin ? tri_end - tri_begin : 0;

    hipStream_t s = ctx->stream;
    float coll_ms = 0.f;
    const bool measure = (params->flags & (O2V_HIP_FLAG_STAGE_TIMES | O2V_HIP_FLAG_KERNEL_TIMES)) != 0;
    auto timed = [&](int part, auto &&collectives) -> int {
        if (!measure) return collectives();
        O2V_CHECK(ctx->coll_times.mark(0, s));
        const int rc = collectives();
        if (rc) return rc;
        O2V_CHECK(ctx->coll_times.mark(1, s));
        O2V_CHECK(hipEventSynchronize(ctx->coll_times.ev[1]));
        float ms = 0.f;
        O2V_CHECK(ctx->coll_times.elapsed(0, 1, ms));
        coll_ms += ms;
        if (parts_ms) parts_ms[part] += ms;
        return O2V_HIP_OK;
    };
    auto comm_failed = [&](int rc) {
        ctx->err = std::string("collective failed: ") + comm->err;
        return rc;
    };
    ctx->ctr_clean = false;
    if (!bounds_reduced) hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, s, ctx->d_ctr.ptr, kPassCounterWords);
    if (!p.bounds_known && !bounds_reduced) {
        if (n_range)
            hipLaunchKernelGGL(k_bounds, dim3((uint32_t) std::min<uint64_t>((uint64_t) ctx->num_cus, (n_range * 9 / 12 + kBoundsBlock) / kBoundsBlock)),
                               dim3(kBoundsBlock), 0, s, ctx->d_verts.ptr + tri_begin * 9, n_range * 9, ctx->d_ctr.ptr);
        O2V_STAGE("k_bounds");
        if (comm) {
            rc = timed(1, [&]() -> int {
                int r = comm->allreduce_min_u32(ctx->d_ctr.ptr->bounds_enc, 3, s);
                if (!r) r = comm->allreduce_max_u32(ctx->d_ctr.ptr->bounds_enc + 3, 3, s);
                return r;
            });
            if (rc) return comm_failed(rc);
        }
    }
    hipLaunchKernelGGL(k_setup, dim3(1), dim3(64), 0, s, ctx->d_ctr.ptr, p);
    O2V_CHECK(hipMemsetAsync(ctx->d_zhist.ptr, 0, kPlanBins * sizeof(unsigned long long), s));
    ctx->zrange_generation = ~0ull;
    hipLaunchKernelGGL(k_zhist, dim3((uint32_t) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) ctx->num_cus * 6u, (n_range + kBlock - 1) / kBlock))),
                       dim3(kBlock), 0, s, ctx->d_verts.ptr, ctx->d_ctr.ptr, ctx->d_zhist.ptr, ctx->d_zrange.ptr, ctx->d_zrange_xform.ptr, p,
                       bin_out * ss, tri_begin, tri_end);
    O2V_STAGE("k_zhist");
    if (comm) {
        // one all-gather for both: every rank's partial histogram and the extents of its blocks (k_pack_plan), summed / put in
        // place by every rank itself (an all-reduce and an all-gather, one after the other, cost a collective's latency more)
        const uint64_t rec_words = (uint64_t) kPlanBins + blocks_per_rank;
        const uint32_t wgs = (uint32_t) std::min<uint64_t>((uint64_t) ctx->num_cus * 2u, (rec_words * (uint64_t) comm->world + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_pack_plan, dim3(std::max(1u, std::min<uint32_t>(wgs, (uint32_t) ((rec_words + kBlock - 1) / kBlock)))), dim3(kBlock), 0, s,
                           ctx->d_zhist.ptr, ctx->d_zrange.ptr + (uint64_t) comm->rank * blocks_per_rank,
                           ctx->d_plan_gather.ptr + (uint64_t) comm->rank * rec_words, (uint32_t) blocks_per_rank);
        rc = timed(2, [&]() -> int { return comm->allgather(ctx->d_plan_gather.ptr, rec_words * sizeof(unsigned long long), s); });
        if (rc) return comm_failed(rc);
        hipLaunchKernelGGL(k_unpack_plan, dim3(std::max(1u, wgs)), dim3(kBlock), 0, s, ctx->d_plan_gather.ptr, (uint32_t) comm->world,
                           (uint32_t) blocks_per_rank, ctx->d_zhist.ptr, ctx->d_zrange.ptr);
    }
    O2V_CHECK(hipMemcpyAsync(ctx->h_zhist.ptr, ctx->d_zhist.ptr, n_bins * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipMemcpyAsync(ctx->h_ctr.ptr, ctx->d_ctr.ptr, kPassCounterWords * 4u, hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(hipGetLastError());
    ctx->zrange_generation = ctx->tri_generation;  // k_expand_roots may use the extents (it checks the transform)
    if (collective_ms) *collective_ms = coll_ms;
    return O2V_HIP_OK;
}

// Cuts the histogram into n_slabs parts of equal predicted work (whole bins; every slab keeps at least one layer).
void cuts_from_histogram(const unsigned long long *hist, uint32_t n_bins, uint32_t bin_out, uint32_t G, uint32_t n_slabs,
                         uint32_t *out_z)
{
    for (uint32_t k = 0; k <= n_slabs; ++k) out_z[k] = (uint32_t) ((uint64_t) G * k / n_slabs);  // equal heights
    unsigned __int128 total = 0;
    for (uint32_t b = 0; b < n_bins; ++b) total += hist[b];
    if (total == 0) return;
    unsigned __int128 before = 0;
    uint32_t k = 1;
    for (uint32_t b = 0; b < n_bins && k < n_slabs; ++b) {
        const unsigned __int128 after = before + hist[b];
        while (k < n_slabs && after * n_slabs >= total * k) {
            // the k-th cut falls inside bin b: take whichever end of the bin is closer to the target
            const unsigned __int128 target_n = total * k;  // compare in units of 1/n_slabs
            const bool take_start = (target_n - before * n_slabs) < (after * n_slabs - target_n);
            out_z[k] = std::min<uint32_t>(G, (take_start ? b : b + 1) * bin_out);
            ++k;
        }
        before = after;
    }
    for (; k < n_slabs; ++k) out_z[k] = G;
    // every slab keeps at least one layer
    for (uint32_t j = 1; j < n_slabs; ++j) out_z[j] = std::max(out_z[j], out_z[j - 1] + 1);
    for (uint32_t j = n_slabs - 1; j >= 1; --j) out_z[j] = std::min(out_z[j], out_z[j + 1] - 1);
}

bool plan_params_ok(o2v_hip_ctx *ctx, const o2v_hip_params *params, uint32_t n_slabs)
{
    const uint32_t ss = params->supersampling ? params->supersampling : 1u;
    const uint32_t G = params->resolution;
    if (G == 0 || ss > 2 || (uint64_t) G * ss > 65535u || n_slabs == 0 || n_slabs > G) {
        ctx->err = "slab plan: resolution must be non-zero and below 65536 samples, 1 <= n_slabs <= resolution";
        return false;
    }
    return true;
}

// The start of a sharded run: everything that can fail on one rank alone happens first, then the ranks agree on going ahead
// (o2v_hip_voxelize_sharded).  `bpr`: blocks of 256 triangles per rank, [tri_begin, tri_end) this rank's share;
// `ready_ms`: the time of the readiness all-reduce (timed calls only).
int agree_to_start(o2v_hip_ctx *ctx, o2v_hip_comm *comm, const o2v_hip_params *params, const Switches &sw, uint64_t bpr,
                   uint64_t tri_begin, uint64_t tri_end, float &ready_ms)
{
    // Everything that can fail on one rank alone - the device, the allocations of the planning passes - happens before the
    // first collective, and the ranks then agree on going ahead (one 4-byte max-reduce): a rank that returned early would
    // leave the others waiting for it in RCCL.  The only word that has to exist for that is allocated first.
    if (hipSetDevice(ctx->device) != hipSuccess) {
        ctx->err = "hipSetDevice failed";
        return O2V_HIP_ERR_HIP;  // (nothing can be communicated from a rank without its device)
    }
    if (!ctx->d_status.ptr || !ctx->h_status.ptr) {
        if (ctx->d_status.alloc(kReadyWords) != hipSuccess || ctx->h_status.alloc(1) != hipSuccess) {
            ctx->err = "allocating the status word failed";
            return O2V_HIP_ERR_OUT_OF_MEMORY;
        }
    }
    const uint32_t world = (uint32_t) comm->world, rank = (uint32_t) comm->rank;
    auto prepare = [&]() -> int {
        O2V_CHECK(ctx->coll_times.create());
        int rc_grow;
        if ((rc_grow = grow(ctx, ctx->d_counts, world)) || (rc_grow = grow(ctx, ctx->h_counts, world))) return rc_grow;
        return size_plan_buffers(ctx, bpr * world, ((uint64_t) kPlanBins + bpr) * world);
    };
    // (bad parameters are a failure of this rank like any other: reported through the status word, so that the other
    // ranks do not wait in the all-reduce for a rank that has already returned)
    int rc_prepare = plan_params_ok(ctx, params, world) ? prepare() : O2V_HIP_ERR_BAD_ARGUMENT;
    if (sw.fail_rank == (int) rank && rc_prepare == O2V_HIP_OK) {
        ctx->err = "O2V_TEST_FAIL_RANK: simulated failure of this rank before the collectives";  // test hook
        rc_prepare = O2V_HIP_ERR_OUT_OF_MEMORY;
    }
    // One max-reduce carries the ranks' "not ready" words and - unless the caller gave the bounds - the bounds of every rank's
    // share of the triangles (k_pack_ready): the first collective of the step, and the only one before the histogram.
    hipStream_t s0 = ctx->stream;
    const uint64_t n_share = tri_end > tri_begin ? tri_end - tri_begin : 0;
    ctx->ctr_clean = false;
    hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, s0, ctx->d_ctr.ptr, kPassCounterWords);
    if (!params->bounds_known && !rc_prepare && n_share)
        hipLaunchKernelGGL(k_bounds, dim3((uint32_t) std::min<uint64_t>((uint64_t) ctx->num_cus, (n_share * 9 / 12 + kBoundsBlock) / kBoundsBlock)),
                           dim3(kBoundsBlock), 0, s0, ctx->d_verts.ptr + tri_begin * 9, n_share * 9, ctx->d_ctr.ptr);
    hipLaunchKernelGGL(k_pack_ready, dim3(1), dim3(64), 0, s0, ctx->d_ctr.ptr, ctx->d_status.ptr, rc_prepare ? 1u : 0u);
    // (no local HIP error may keep this rank out of the collective: its peers would wait for the time limit instead of seeing
    // the error in the status word - a timing event that cannot be recorded only switches the timing off)
    bool time_it = (params->flags & (O2V_HIP_FLAG_STAGE_TIMES | O2V_HIP_FLAG_KERNEL_TIMES)) != 0;
    if (time_it && ctx->coll_times.mark(0, s0) != hipSuccess) {
        (void) hipGetLastError();
        time_it = false;
    }
    const std::string prepare_err = ctx->err;
    if (comm->allreduce_max_u32(ctx->d_status.ptr, 7, s0)) {
        ctx->err = std::string("collective failed: ") + comm->err;
        return O2V_HIP_ERR_HIP;
    }
    if (time_it && ctx->coll_times.mark(1, s0) != hipSuccess) {
        (void) hipGetLastError();
        time_it = false;
    }
    hipLaunchKernelGGL(k_unpack_ready, dim3(1), dim3(64), 0, s0, ctx->d_status.ptr, ctx->d_ctr.ptr);
    O2V_CHECK(hipMemcpyAsync(ctx->h_status.ptr, ctx->d_status.ptr + 6, sizeof(uint32_t), hipMemcpyDeviceToHost, s0));
    // (the first collective of the run: if a rank of the job never gets here - it died, or the node is set up wrongly - the
    // others say so after o2v::comm_timeout_seconds() instead of waiting for ever)
    if (!o2v::stream_wait_limited(s0, "the readiness all-reduce of the sharded run", ctx->err)) {
        // the collective stays queued on the stream: nothing may wait for this stream or this communicator again (a later
        // hipFree / hipStreamSynchronize / ncclCommDestroy would only move the hang to the teardown)
        ctx->poisoned = true;
        comm->poisoned = true;
        return O2V_HIP_ERR_HIP;
    }
    if (time_it) O2V_CHECK(ctx->coll_times.elapsed(0, 1, ready_ms));
    if (rc_prepare) {
        ctx->err = prepare_err;
        return rc_prepare;
    }
    if (*ctx->h_status.ptr) {
        ctx->err = "another rank could not prepare its sharded run";
        return O2V_HIP_ERR_HIP;
    }
    return O2V_HIP_OK;
}

}  // namespace

extern "C" {

int o2v_hip_plan_slabs(o2v_hip_ctx *ctx, const o2v_hip_params *params, uint32_t n_slabs, uint32_t *out_z,
                       float *out_bounds)
{
    if (!ctx || !params || !out_z || n_slabs == 0) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!plan_params_ok(ctx, params, n_slabs)) return O2V_HIP_ERR_BAD_ARGUMENT;
    const uint32_t G = params->resolution;
    for (uint32_t k = 0; k <= n_slabs; ++k) out_z[k] = (uint32_t) ((uint64_t) G * k / n_slabs);  // equal heights
    if (out_bounds)
        for (int i = 0; i < 6; ++i) out_bounds[i] = params->bounds_known ? params->bounds[i] : 0.f;
    if (ctx->n_tris == 0) return O2V_HIP_OK;
    uint32_t n_bins = 0, bin_out = 0;
    int rc;
    if ((rc = plan_passes(ctx, params, read_switches(), 0, ctx->n_tris, nullptr, 0, n_bins, bin_out, nullptr))) return rc;
    if (out_bounds && !params->bounds_known)
        for (int i = 0; i < 6; ++i) out_bounds[i] = ord2f_host(ctx->h_ctr.ptr->bounds_enc[i]);
    cuts_from_histogram(ctx->h_zhist.ptr, n_bins, bin_out, G, n_slabs, out_z);
    return O2V_HIP_OK;
}

void o2v_hip_cuts_from_histogram(const uint64_t *hist, uint32_t n_bins, uint32_t bin_layers, uint32_t resolution,
                                 uint32_t n_slabs, uint32_t *out_z)
{
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "histogram word");
    if (!hist || !out_z || !n_slabs || !bin_layers) return;
    cuts_from_histogram(reinterpret_cast<const unsigned long long *>(hist), n_bins, bin_layers, resolution, n_slabs, out_z);
}

int o2v_hip_voxelize_sharded(o2v_hip_ctx *ctx, o2v_hip_comm *comm, const o2v_hip_params *params, uint64_t *out_count,
                             uint64_t *out_counts_all, uint32_t *out_cuts)
{
    if (!ctx || !params) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (out_count) *out_count = 0;
    const uint32_t world = comm ? (uint32_t) comm->world : 1u, rank = comm ? (uint32_t) comm->rank : 0u;
    // test hook: a world of one normally needs no collective; O2V_TEST_FORCE_COLLECTIVES=1 runs them anyway (this is how
    // the RCCL code path is exercised on a single-GPU machine)
    const Switches sw = read_switches();
    if (world == 1 && !(comm && sw.force_collectives)) {
        o2v_hip_params whole = *params;
        whole.z_begin = whole.z_end = 0;
        uint64_t n = 0;
        const int rc = voxelize(ctx, &whole, sw, &n);
        if (rc) return rc;
        if (out_count) *out_count = n;
        if (out_counts_all) out_counts_all[0] = n;
        if (out_cuts) {
            out_cuts[0] = 0;
            out_cuts[1] = params->resolution;
        }
        return O2V_HIP_OK;
    }
    const uint64_t T = ctx->n_tris, n_blocks = (T + kBlock - 1) / kBlock;
    const uint64_t bpr = std::max<uint64_t>(1, (n_blocks + world - 1) / world);
    float parts_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    // this rank's share of the triangle list, in whole blocks of 256 (the unit of the block extents)
    const uint64_t b0 = std::min<uint64_t>(n_blocks, (uint64_t) rank * bpr), b1 = std::min<uint64_t>(n_blocks, (uint64_t) (rank + 1) * bpr);
    const uint64_t tri_begin = b0 * kBlock, tri_end = std::min<uint64_t>(T, b1 * kBlock);
    if (const int rc_ready = agree_to_start(ctx, comm, params, sw, bpr, tri_begin, tri_end, parts_ms[0])) return rc_ready;
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t n_bins = 0, bin_out = 0;
    float coll_ms = 0.f;
    int rc = plan_passes(ctx, params, sw, tri_begin, tri_end, comm, bpr, n_bins, bin_out, &coll_ms, parts_ms, /*bounds_reduced=*/true);
    if (rc) return rc;
    std::vector<uint32_t> cuts(world + 1);
    cuts_from_histogram(ctx->h_zhist.ptr, n_bins, bin_out, params->resolution, world, cuts.data());
    o2v_hip_params mine = *params;
    if (!params->bounds_known) {
        mine.bounds_known = 1;
        for (int i = 0; i < 6; ++i) mine.bounds[i] = ord2f_host(ctx->h_ctr.ptr->bounds_enc[i]);
    }
    mine.z_begin = cuts[rank];
    mine.z_end = cuts[rank + 1];
    const float plan_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();

    uint64_t n = 0;
    const int rc_vox = voxelize(ctx, &mine, sw, &n);
    // Every rank takes part in the exchange of the counts, also one whose voxelization failed (it reports ~0), so that no
    // rank is left waiting in a collective.
    hipStream_t s = ctx->stream;
    ctx->h_counts.ptr[rank] = rc_vox ? ~0ull : n;
    const std::string vox_err = ctx->err;
    O2V_CHECK(hipMemcpyAsync(ctx->d_counts.ptr + rank, ctx->h_counts.ptr + rank, sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    const bool time_counts = (params->flags & (O2V_HIP_FLAG_STAGE_TIMES | O2V_HIP_FLAG_KERNEL_TIMES)) != 0;
    if (time_counts) O2V_CHECK(ctx->coll_times.mark(0, s));
    rc = comm->allgather(ctx->d_counts.ptr, sizeof(unsigned long long), s);
    if (rc) {
        ctx->err = std::string("collective failed: ") + comm->err;
        return rc;
    }
    if (time_counts) O2V_CHECK(ctx->coll_times.mark(1, s));
    O2V_CHECK(hipMemcpyAsync(ctx->h_counts.ptr, ctx->d_counts.ptr, world * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    if (time_counts) O2V_CHECK(ctx->coll_times.elapsed(0, 1, parts_ms[4]));
    ctx->timings.plan_ms = plan_ms;
    ctx->timings.collective_ms = coll_ms + parts_ms[4] + parts_ms[0];
    for (int i = 0; i < 5; ++i) ctx->timings.collective_parts_ms[i] = parts_ms[i];
    if (rc_vox) {
        ctx->err = vox_err;
        return rc_vox;
    }
    for (uint32_t r = 0; r < world; ++r)
        if (ctx->h_counts.ptr[r] == ~0ull) {
            ctx->err = "the voxelization failed on rank " + std::to_string(r);
            return O2V_HIP_ERR_HIP;
        }
    if (out_count) *out_count = n;
    if (out_counts_all)
        for (uint32_t r = 0; r < world; ++r) out_counts_all[r] = ctx->h_counts.ptr[r];
    if (out_cuts)
        for (uint32_t r = 0; r <= world; ++r) out_cuts[r] = cuts[r];
    return O2V_HIP_OK;
}

int o2v_hip_max_slab_layers(o2v_hip_ctx *ctx, const o2v_hip_params *params, uint32_t *out_layers)
{
    if (!ctx || !params || !out_layers || !params->resolution) return O2V_HIP_ERR_BAD_ARGUMENT;
    *out_layers = 0;
    O2V_CHECK(hipSetDevice(ctx->device));
    size_t free_b = 0, total_b = 0;
    O2V_CHECK(hipMemGetInfo(&free_b, &total_b));
    const uint64_t G = params->resolution;
    // (a layer of the grids is as wide as the mesh's voxel bounding box, grid_box)
    const uint32_t ss_l = params->supersampling ? params->supersampling : 1u;
    const Switches sw = read_switches();
    const GridBox box = grid_box(ctx, params, sw, host_transform(ctx, params, params->resolution * ss_l), ss_l, 0u, params->resolution);
    const uint64_t per_layer_bricks = box.empty ? 1ull
                                                : (uint64_t) ((box.hi[0] - box.lo[0] + kBrickX - 1) / kBrickX) * ((box.hi[1] - box.lo[1] + kBrickY - 1) / kBrickY);
    // per brick: occupancy only (no triangle of the uploaded mesh has a material) one byte per cell; else the 32-bit counter
    // grid and, for the MAX strategy, the 64-bit grid; each with its side arrays (grid_bytes)
    const GridModes modes = grid_modes(ctx, params, sw);  // (the same decision o2v_hip_voxelize takes, flags and environment included)
    const bool occupancy_only = modes.occupancy_only;
    const bool max_grid = modes.direct_max && !occupancy_only;
    const GridBytes counter = grid_bytes(Grid::counter), max64 = grid_bytes(Grid::max64);
    const uint64_t per_brick = occupancy_only ? grid_bytes(Grid::occupancy).total() : counter.total() + (max_grid ? max64.total() : 0ull);
    // what the context already holds of these grids is reusable
    const uint64_t held = (occupancy_only ? 0ull : ctx->d_grid.cap * sizeof(uint32_t) + ctx->d_brick_dirty.cap * counter.side()) +
                          ctx->d_maxgrid.cap + ctx->d_dirty_max.cap * max64.side();
    // the work buffers (leaves, tiles, hit pool, sorted records, output) scale with the mesh, not with the grid: a quarter of
    // the device, at least 8 GiB, stays free for them
    // (the hit slabs - at most a sixth of the device, o2v_hip_voxelize - are part of that reserve: what the context holds of
    // them already counts towards it, and they give way if a required buffer does not fit)
    const uint64_t reserve = std::max<uint64_t>(8ull << 30, total_b / 4);
    const uint64_t held_slabs = ctx->d_slabs.cap * sizeof(uint32_t);
    const uint64_t avail = (uint64_t) free_b + held + held_slabs > reserve ? (uint64_t) free_b + held + held_slabs - reserve : 0;
    // solid fill (O2V_HIP_FLAG_FILL_INTERIOR): per layer of the box also its bits of the toggle bitmap and, at worst, one 16-byte
    // interior record per cell; and a pass holds fewer than 2^32 records
    const bool fill = (params->flags & O2V_HIP_FLAG_FILL_INTERIOR) != 0;
    const uint64_t per_layer_cells = per_layer_bricks * kBrickX * kBrickY;
    const uint64_t fill_bytes = fill ? per_layer_cells * kBrickZ * sizeof(uint4) + (per_layer_cells * kBrickZ + 7u) / 8u : 0ull;
    uint64_t brick_layers = avail / (per_layer_bricks * per_brick + fill_bytes);
    brick_layers = std::min<uint64_t>(brick_layers, ((1ull << 31) - 1) / per_layer_bricks);  // 32-bit brick ids
    if (fill) brick_layers = std::min<uint64_t>(brick_layers, kMaxRecords / (per_layer_cells * kBrickZ));
    const uint64_t layers = brick_layers * kBrickZ;
    // (the grids only span the mesh's box in z as well: if that many layers fit, the whole resolution is one slab)
    const uint64_t box_layers = box.empty ? 0ull : (uint64_t) (box.hi[2] - box.lo[2]) + kBrickZ;
    uint64_t out = (layers >= G || layers >= box_layers) ? G : layers;
    // ... and a pass' box is at most 65 535 samples tall, as it is wide (o2v_hip_voxelize): a mesh box taller than that is cut
    // into slabs of at most this many layers, whatever the memory would hold (a multiple of 4, as the x / y tiles of
    // obj2voxel_voxelize() are)
    const uint64_t pass_layers = (65535u / ss_l) & ~3u;
    if (!box.empty && (uint64_t) (box.hi[2] - box.lo[2]) * ss_l > 65535u) out = std::min(out, pass_layers);
    *out_layers = (uint32_t) out;
    return O2V_HIP_OK;
}

}  // extern "C"

namespace {
// the voxel records [first, first + count) of the last run to `out`: on the context's stream (async) or waiting for the copy
int read_voxels(o2v_hip_ctx *ctx, uint32_t *out, uint64_t first, uint64_t count, bool async)
{
    if (!ctx || (!out && count)) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (first + count > ctx->n_vox) {
        ctx->err = "voxel range out of bounds";
        return O2V_HIP_ERR_BAD_ARGUMENT;
    }
    if (!count) return O2V_HIP_OK;
    O2V_CHECK(hipSetDevice(ctx->device));
    if (async) O2V_CHECK(hipMemcpyAsync(out, ctx->d_out.ptr + first, count * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
    else O2V_CHECK(hipMemcpy(out, ctx->d_out.ptr + first, count * sizeof(uint4), hipMemcpyDeviceToHost));
    return O2V_HIP_OK;
}
}  // namespace

extern "C" {

int o2v_hip_read_voxels(o2v_hip_ctx *ctx, uint32_t *out, uint64_t first, uint64_t count) { return read_voxels(ctx, out, first, count, false); }
int o2v_hip_read_voxels_async(o2v_hip_ctx *ctx, uint32_t *out, uint64_t first, uint64_t count) { return read_voxels(ctx, out, first, count, true); }

int o2v_hip_read_voxels_wait(o2v_hip_ctx *ctx)
{
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    O2V_CHECK(hipSetDevice(ctx->device));
    O2V_CHECK(hipStreamSynchronize(ctx->stream));
    return O2V_HIP_OK;
}

void *o2v_hip_alloc_pinned(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void o2v_hip_free_pinned(void *p)
{
    if (p) (void) hipHostFree(p);
}

int o2v_hip_voxels_device_ptr(o2v_hip_ctx *ctx, const uint32_t **out_ptr, uint64_t *out_count)
{
    if (!ctx || !out_ptr || !out_count) return O2V_HIP_ERR_BAD_ARGUMENT;
    *out_ptr = reinterpret_cast<const uint32_t *>(ctx->d_out.ptr);
    *out_count = ctx->n_vox;
    return O2V_HIP_OK;
}

}  // extern "C"

// ---- K7 - K21: the dense-grid entry points, a host header per family (what they share: o2v_dev_host_args.hpp) -----------

#include "o2v_dev_host_args.hpp"
#include "o2v_dev_host_k7_dense.hpp"
#include "o2v_dev_host_k8_distance.hpp"
#include "o2v_dev_host_k9_mesh.hpp"
#include "o2v_dev_host_k10_surface.hpp"
#include "o2v_dev_host_k11_raycast.hpp"
#include "o2v_dev_host_k12_components.hpp"
#include "o2v_dev_host_k13_gather.hpp"
#include "o2v_dev_host_k17_downsample.hpp"
#include "o2v_dev_host_k26_octree.hpp"
#include "o2v_dev_host_k30_dag.hpp"
#include "o2v_dev_host_k31_treeray.hpp"
#include "o2v_dev_host_k27_openness.hpp"
#include "o2v_dev_host_k19_label_stats.hpp"
#include "o2v_dev_host_k21_thickness.hpp"
#include "o2v_dev_host_k22_thinning.hpp"
#include "o2v_dev_host_k23_watershed.hpp"
#include "o2v_dev_host_k24_adjacency.hpp"
#include "o2v_dev_host_k25_euler.hpp"
#include "o2v_dev_host_k28_grow.hpp"
#include "o2v_dev_host_k29_label_surface.hpp"

extern "C" {

namespace {
// Where a cell's hit records are after a run of the general route (the host-side twin of CellRecords): the first n_slab in its
// brick's slab, the other n_sorted in the sorted array.
struct HostCellRecords {
    size_t slab_first, sorted_first;
    uint32_t n_slab, n_sorted;
};
bool hit_lists_kept(o2v_hip_ctx *ctx)
{
    if (ctx->last_direct) ctx->err = "hit lists are not kept on the direct MAX path: run with O2V_NO_DIRECT_MAX=1 to inspect them";
    return !ctx->last_direct;
}
HostCellRecords host_cell_records(const Occ &o, uint32_t cap_slabs)
{
    const uint32_t cnt = o.count & ~kOccInline;
    const bool inl = (o.count & kOccInline) != 0u;
    const uint32_t slab = inl ? o.offset : o.slab();
    const bool has_slab = inl || slab < cap_slabs;
    HostCellRecords w{};
    w.slab_first = ((size_t) slab * kBrickCells + (o.cell_lo & (kBrickCells - 1u))) * kInlineHits;
    w.n_slab = !has_slab ? 0u : (cnt < kInlineHits ? cnt : kInlineHits);
    w.n_sorted = cnt - w.n_slab;
    w.sorted_first = inl ? 0u : (size_t) o.offset;
    return w;
}
}  // namespace

// Debugging aid: the hit records of one output cell of the last run (the occupied-cell list and the hit pool
// stay valid after a run).  Each record is 6 words: keyhi, keylo, w, u, v (as float bits) and the pool index.
int o2v_hip_debug_cell_hits(o2v_hip_ctx *ctx, uint32_t x, uint32_t y, uint32_t z, uint32_t *out, uint32_t max_records,
                            uint32_t *out_count)
{
    if (!ctx || !out || !out_count) return O2V_HIP_ERR_BAD_ARGUMENT;
    *out_count = 0;
    if (!hit_lists_kept(ctx)) return O2V_HIP_ERR_BAD_ARGUMENT;
    O2V_CHECK(hipSetDevice(ctx->device));
    std::vector<Occ> occ(ctx->n_vox);
    std::vector<uint4> vox(ctx->n_vox);
    if (!ctx->n_vox) return O2V_HIP_OK;
    O2V_CHECK(hipMemcpy(occ.data(), ctx->d_occ.ptr, occ.size() * sizeof(Occ), hipMemcpyDeviceToHost));
    O2V_CHECK(hipMemcpy(vox.data(), ctx->d_out.ptr, vox.size() * sizeof(uint4), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < ctx->n_vox; ++i) {
        if (vox[i].x != x || vox[i].y != y || vox[i].z != z) continue;
        const HostCellRecords where = host_cell_records(occ[i], ctx->cap_slabs());
        const uint32_t cnt = occ[i].count & ~kOccInline;
        const uint32_t n = cnt < max_records ? cnt : max_records;
        const size_t first = where.n_slab ? where.slab_first : where.sorted_first;
        for (uint32_t k = 0; k < n; ++k) {
            const bool in_slab = k < where.n_slab;
            const size_t at = in_slab ? where.slab_first + k : where.sorted_first + (k - where.n_slab);
            uint32_t r[6] = {};
            O2V_CHECK(hipMemcpy(r, (in_slab ? ctx->d_slabs.ptr : reinterpret_cast<const uint32_t *>(ctx->d_sorted.ptr)) + at * ctx->sorted_stride,
                                ctx->sorted_stride * sizeof(uint32_t), hipMemcpyDeviceToHost));
            uint32_t *o = out + k * 6;
            o[0] = r[0];
            o[1] = r[1];
            o[2] = r[2];
            o[3] = ctx->sorted_stride == 6 ? r[3] : 0u;
            o[4] = ctx->sorted_stride == 6 ? r[4] : 0u;
            o[5] = (uint32_t) (first + (size_t) k);
        }
        *out_count = n;
        break;
    }
    return O2V_HIP_OK;
}

// Debugging aid for parity work: every hit record of the last run (general route), 8 words each: the cell's x, y, z, keyhi
// (sub-voxel << 29 | triangle), keylo (leaf order key), and the bits of w, u, v - what k_voxelize computed per (leaf, voxel)
// pair, before any fold.  Cells in emission order, a cell's hits in the (arbitrary) order of the sorted array.
int o2v_hip_debug_hits(o2v_hip_ctx *ctx, uint32_t *out8, uint64_t max_hits, uint64_t *n_hits)
{
    if (!ctx || !n_hits || (!out8 && max_hits)) return O2V_HIP_ERR_BAD_ARGUMENT;
    *n_hits = 0;
    if (!hit_lists_kept(ctx)) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!ctx->n_vox) return O2V_HIP_OK;
    O2V_CHECK(hipSetDevice(ctx->device));
    std::vector<Occ> occ(ctx->n_vox);
    std::vector<uint4> vox(ctx->n_vox);
    O2V_CHECK(hipMemcpy(occ.data(), ctx->d_occ.ptr, occ.size() * sizeof(Occ), hipMemcpyDeviceToHost));
    O2V_CHECK(hipMemcpy(vox.data(), ctx->d_out.ptr, vox.size() * sizeof(uint4), hipMemcpyDeviceToHost));
    uint64_t total = 0, end = 0;
    for (const Occ &o : occ) {
        total += o.count & ~kOccInline;
        const HostCellRecords where = host_cell_records(o, ctx->cap_slabs());
        if (where.n_sorted) end = std::max<uint64_t>(end, (uint64_t) where.sorted_first + where.n_sorted);
    }
    *n_hits = total;
    if (total > max_hits) return O2V_HIP_OK;  // (the caller sizes its buffer from *n_hits and calls again)
    std::vector<uint32_t> raw((size_t) end * ctx->sorted_stride);
    if (end) O2V_CHECK(hipMemcpy(raw.data(), ctx->d_sorted.ptr, raw.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    // (cells with up to kInlineHits hits keep them side by side in their bricks' slabs)
    std::vector<uint32_t> slabs((size_t) ctx->cap_slabs() * kInlineHits * kBrickCells * ctx->sorted_stride);
    if (!slabs.empty()) O2V_CHECK(hipMemcpy(slabs.data(), ctx->d_slabs.ptr, slabs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t k = 0;
    for (uint64_t i = 0; i < ctx->n_vox; ++i) {
        const HostCellRecords where = host_cell_records(occ[i], ctx->cap_slabs());
        const uint32_t cnt = occ[i].count & ~kOccInline;
        for (uint32_t h = 0; h < cnt; ++h, ++k) {
            const uint32_t *r = h < where.n_slab ? &slabs[(where.slab_first + h) * ctx->sorted_stride]
                                                 : &raw[(where.sorted_first + (h - where.n_slab)) * ctx->sorted_stride];
            uint32_t *o = out8 + k * 8;
            o[0] = vox[i].x;
            o[1] = vox[i].y;
            o[2] = vox[i].z;
            o[3] = r[0];
            o[4] = r[1];
            o[5] = r[2];
            o[6] = ctx->sorted_stride == 6 ? r[3] : 0u;
            o[7] = ctx->sorted_stride == 6 ? r[4] : 0u;
        }
    }
    return O2V_HIP_OK;
}

// Debugging aid: histogram of hits per occupied cell of the last run; bucket b counts cells with 2^(b-1) < hits <= 2^b
// (bucket 0: exactly one hit), 32 buckets.
int o2v_hip_debug_hits_histogram(o2v_hip_ctx *ctx, uint64_t *out32)
{
    if (!ctx || !out32) return O2V_HIP_ERR_BAD_ARGUMENT;
    for (int i = 0; i < 32; ++i) out32[i] = 0;
    if (!ctx->n_vox) return O2V_HIP_OK;
    if (!hit_lists_kept(ctx)) return O2V_HIP_ERR_BAD_ARGUMENT;
    O2V_CHECK(hipSetDevice(ctx->device));
    std::vector<Occ> occ(ctx->n_vox);
    O2V_CHECK(hipMemcpy(occ.data(), ctx->d_occ.ptr, occ.size() * sizeof(Occ), hipMemcpyDeviceToHost));
    for (const Occ &o : occ) {
        uint32_t b = 0;
        while ((1u << b) < (o.count & ~kOccInline) && b < 31) ++b;
        out32[b]++;
    }
    return O2V_HIP_OK;
}

int o2v_hip_debug_check_third(o2v_hip_ctx *ctx, uint64_t *out2)
{
    if (!ctx || !out2) return O2V_HIP_ERR_BAD_ARGUMENT;
    O2V_CHECK(hipSetDevice(ctx->device));
    DevArray<unsigned long long> d;
    O2V_CHECK(d.alloc(2));
    const unsigned long long init[2] = {0ull, ~0ull};
    O2V_CHECK(hipMemcpy(d.ptr, init, sizeof(init), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_check_third, dim3((uint32_t) ctx->num_cus * 8u), dim3(256), 0, ctx->stream, d.ptr);
    O2V_CHECK(hipStreamSynchronize(ctx->stream));
    unsigned long long got[2] = {0, 0};
    O2V_CHECK(hipMemcpy(got, d.ptr, sizeof(got), hipMemcpyDeviceToHost));
    out2[0] = got[0];
    out2[1] = got[0] ? got[1] : 0;
    return O2V_HIP_OK;
}

int o2v_hip_debug_check_div(o2v_hip_ctx *ctx, uint32_t samples, uint64_t seed, uint32_t *out65536)
{
    if (!ctx || !out65536 || !samples) return O2V_HIP_ERR_BAD_ARGUMENT;
    O2V_CHECK(hipSetDevice(ctx->device));
    DevArray<uint32_t> d;
    O2V_CHECK(d.alloc(65536));
    O2V_CHECK(hipMemsetAsync(d.ptr, 0, 65536 * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_check_div, dim3(65536), dim3(256), 0, ctx->stream, d.ptr, samples, seed);
    O2V_CHECK(hipStreamSynchronize(ctx->stream));
    O2V_CHECK(hipMemcpy(out65536, d.ptr, 65536 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return O2V_HIP_OK;
}

int o2v_hip_debug_counters(const o2v_hip_ctx *ctx, uint64_t *out16)
{
    if (!ctx || !out16) return O2V_HIP_ERR_BAD_ARGUMENT;
    for (int i = 0; i < 16; ++i) out16[i] = ctx->dbg[i];
    return O2V_HIP_OK;
}

int o2v_hip_get_timings(const o2v_hip_ctx *ctx, o2v_hip_timings *out)
{
    if (!ctx || !out) return O2V_HIP_ERR_BAD_ARGUMENT;
    *out = ctx->timings;
    return O2V_HIP_OK;
}

int o2v_hip_get_kernel_times(const o2v_hip_ctx *ctx, o2v_hip_kernel_time *out, uint32_t max_entries, uint32_t *out_count)
{
    if (!ctx || !out_count || (max_entries && !out)) return O2V_HIP_ERR_BAD_ARGUMENT;
    const uint32_t n = (uint32_t) std::min<size_t>(ctx->kernel_times.size(), max_entries);
    for (uint32_t i = 0; i < n; ++i) out[i] = ctx->kernel_times[i];
    *out_count = (uint32_t) ctx->kernel_times.size();
    return O2V_HIP_OK;
}

const char *o2v_hip_build_id(void) { return O2V_BUILD_ID; }

int o2v_hip_get_stats(const o2v_hip_ctx *ctx, o2v_hip_stats *out)
{
    if (!ctx || !out) return O2V_HIP_ERR_BAD_ARGUMENT;
    *out = ctx->stats;
    return O2V_HIP_OK;
}

int o2v_hip_get_transform(const o2v_hip_ctx *ctx, float out12[12])
{
    if (!ctx || !out12) return O2V_HIP_ERR_BAD_ARGUMENT;
    std::memcpy(out12, ctx->xform, sizeof(ctx->xform));
    return O2V_HIP_OK;
}

}  // extern "C"
