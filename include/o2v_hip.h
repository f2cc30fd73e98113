/*
 * o2v_hip.h -- thin C-ABI between the C++ host code and the gfx950 HIP pipeline.
 *
 * Plain pointers and sizes only; no C++ or torch types.  This is the layer the host side of
 * obj2voxel_voxelize() (include/obj2voxel.h) calls where the reference runs its chunk loop
 * (reference src/obj2voxel.cpp:467-520) and Voxelizer::voxelize (reference src/voxelization.cpp:480-526).
 * A maintainer of the reference binds these entry points from obj2voxel.cpp; see INTEGRATION.md.
 *
 * Call sequence:  create -> set_triangles[/set_textures] -> voxelize -> read_voxels -> destroy.
 * A context owns one GPU's z-slab of the dense voxel grid and may be reused for any number of voxelize
 * calls (the grid is left clean by every call).  One context per GPU; contexts are not thread-safe.
 */
#ifndef O2V_HIP_H
#define O2V_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct o2v_hip_ctx o2v_hip_ctx;

/* error codes returned by every int-returning function */
enum {
    O2V_HIP_OK = 0,
    O2V_HIP_ERR_NO_DEVICE = 1,     /* no usable gfx950 device / HIP runtime failure at create */
    O2V_HIP_ERR_HIP = 2,           /* a HIP call failed; see o2v_hip_last_error */
    O2V_HIP_ERR_BAD_ARGUMENT = 3,
    O2V_HIP_ERR_OUT_OF_MEMORY = 4,
    O2V_HIP_ERR_LIMIT = 5,         /* mesh exceeds an implementation limit (e.g. >= 2^29 triangles) */
    O2V_HIP_ERR_IO = 6             /* o2v_hip_gather_save: the file cannot be opened, is of no output type, or stopped taking voxels */
};

/* triangle material types: reference src/triangle.hpp:21-29 */
enum { O2V_HIP_TRI_MATERIALLESS = 1, O2V_HIP_TRI_UNTEXTURED = 2, O2V_HIP_TRI_TEXTURED = 3 };

/* Texture description; pixels are copied to the device by o2v_hip_set_textures.
 * channels: 3 = RGB, 4 = ARGB, 8 bits each (reference include/obj2voxel.h:317-320). wrap: 0 clamp, 1 repeat. */
typedef struct {
    const uint8_t *pixels;
    uint32_t width, height, channels, wrap;
} o2v_hip_texture;

/* Parameters of one voxelization: what the reference keeps in obj2voxel_instance (src/obj2voxel.cpp:142-173). */
typedef struct {
    uint32_t resolution;       /* output resolution (obj2voxel_set_resolution) */
    uint32_t supersampling;    /* 1 or 2 (obj2voxel_set_supersampling) */
    uint32_t strategy;         /* 0 = MAX, 1 = BLEND (obj2voxel_set_color_strategy) */
    int32_t unit_transform[9]; /* row-major (obj2voxel_set_unit_transform) */
    uint32_t bounds_known;     /* 1: use bounds[] (obj2voxel_set_mesh_boundaries), 0: reduce them on the device */
    float bounds[6];           /* min xyz, max xyz */
    uint32_t z_begin, z_end;   /* this GPU's slab of output z, [z_begin, z_end); 0,0 = the whole grid */
    uint32_t flags;            /* O2V_HIP_FLAG_*; 0 = the product's defaults */
    /* An x / y tile of the output grid, [x_begin, x_end) x [y_begin, y_end) (0, 0 = the whole axis; begin a multiple of 4): only
     * the voxels inside are produced, as with the z slab.  One pass handles a box - the mesh's voxel bounding box within slab and
     * tile - of at most 65 535 samples (resolution x supersampling) per axis: voxel coordinates travel in 16-bit fields relative
     * to the box (the reference carries u32, src/util.hpp:185-196).  A wider grid is voxelized tile by tile; every output voxel
     * belongs to exactly one tile, so the tiles' records concatenated are the whole grid's (obj2voxel_voxelize() does that). */
    uint32_t x_begin, x_end, y_begin, y_end;
    /* O2V_HIP_FLAG_FILL_INTERIOR: the colour (0xAARRGGBB) of the interior voxels' records.  Unused without the flag. */
    uint32_t fill_argb;
} o2v_hip_params;

/* o2v_hip_params::flags.
 * EXACT_CLIP: switches off every piece of work-removal logic in the clip kernel that is not the reference's own
 * arithmetic (the separating-axis row test, the bounding-box plane masks with their margins, the single-plane rule): every
 * candidate voxel of a leaf's clamped AABB is tested as reference src/voxelization.cpp:446-470 does (plane-distance cull,
 * then all six planes through the classification of splitTriangle, :190-232).  Slower, results must be identical: the
 * tests run both on the device and compare (tests/test_gpu_exact_ab.py).  Also forced by O2V_EXACT_CLIP=1 in the
 * environment.
 * KERNEL_TIMES: brackets every kernel launch of the pipeline with two HIP events on the stream it is launched on;
 * o2v_hip_get_kernel_times then returns the per-kernel device times of the call (summed over the launches of one kernel).
 * Implies STAGE_TIMES.
 * STAGE_TIMES: records a HIP event before, between and behind the stages of a pass, for o2v_hip_timings' stage times and
 * total_ms.  Not the default because an event between two kernels is a command of its own in the queue and costs about 4 us
 * of device time (six of them: 3 % of the bench headline's step, profiles/r05/NOTES.md).
 * FILL_INTERIOR: solid voxelization.  The call returns the surface records it returns without the flag (the same multiset,
 * first in the output), followed by one record (i, j, k, fill_argb) for every voxel of the pass box that is not a surface voxel
 * and whose centre is inside by z-parity:
 *   S = resolution x supersampling; each triangle's vertices are transformed to sample space as the pipeline does (affine_apply,
 *   float32); a triangle with a non-finite coordinate contributes nothing.  The column of output voxel (i, j) is the vertical line
 *   through P = (i ss + ss/2, j ss + ss/2).  A triangle covers the column if the exact signs of its edge functions
 *   e(U, V, P) = (V.x - U.x)(P.y - U.y) - (V.y - U.y)(P.x - U.x) over V0->V1, V1->V2, V2->V0 (float32 vertex values, the sign
 *   of the exact value) are all +1 or all -1; an exact zero takes the sign of the symbolic perturbation P + (eps, eps^2),
 *   -sgn(V.y - U.y), or sgn(V.x - U.x) when V.y = U.y; an edge whose projected ends coincide has sign 0.  With one predicate
 *   and one perturbation for all edges, a mesh whose every edge (pair of bit-identical sample-space vertices) is shared by an
 *   even number of triangles covers every column an even number of times; vertical faces cover nothing.  A covering triangle
 *   crosses the column at z = (w0 V0.z + w1 V1.z + w2 V2.z) / (w0 + w1 + w2) in double, op by op, left to right, without FMA,
 *   with w0 = e(V1, V2, P), w1 = e(V2, V0, P), w2 = e(V0, V1, P) in double as written (the smallest vertex z if the denominator
 *   is 0 or z is not finite), and toggles every voxel k >= k0 of the column, k0 the smallest k >= 0 with k ss + ss/2 > z.  A voxel
 *   toggled an odd number of times and at or below the mesh's top layer floor(zmax / ss) is in the parity set, zmax the largest
 *   sample-space z of a triangle with finite coordinates.
 * Interior voxels exist only within the pass box (the mesh's voxel bounding box within slab and tile); a crossing below a
 * slab's first layer toggles from that layer up, a triangle whose lowest vertex lies at or above the slab's top is not looked
 * at.  For a closed mesh that is its solid interior; for an open one, whatever the definition gives (voxels above an open sheet,
 * up to the mesh's top layer) - nothing is repaired.  Slabs and tiles split the set exactly as they split the surface.  The
 * stage needs a bitmap of one bit per cell of the pass box and 16 bytes per interior record, and one pass may hold at most
 * 2^32 - 16 records in all (o2v_hip_max_slab_layers counts both). */
enum { O2V_HIP_FLAG_EXACT_CLIP = 1u, O2V_HIP_FLAG_KERNEL_TIMES = 2u, O2V_HIP_FLAG_STAGE_TIMES = 4u, O2V_HIP_FLAG_FILL_INTERIOR = 8u };

/* Device times of the last o2v_hip_voxelize call.  voxelize_ms is measured in every call (two hipEvents that ride on the clip
 * kernel's own dispatch), passes and plan_ms likewise; the other stage times, total_ms and the collectives' times only in a call
 * made with O2V_HIP_FLAG_STAGE_TIMES (else 0) - then voxelize_ms, too, is the time between two events on the stream, and every
 * timed collective of a sharded run is followed by a wait on the host (three more round trips per call). */
typedef struct {
    float bounds_ms;     /* K0  mesh bounds reduce + transform setup */
    float expand_ms;     /* K1  transform, classify, exact subdivision into leaves and tiles */
    float voxelize_ms;   /* K2  AABB walk + plane cull + SAT pre-test + six-plane clip + hit append (dense-grid atomics) */
    float scan_ms;       /* K5  dirty-brick scan, occupied-cell compaction + offsets, hit scatter, brick reset (on the direct
                            MAX path: the flag scan of the 64-bit grid, plus these kernels only if the mesh has subdivided
                            triangles) */
    float resolve_ms;    /* K3  per-cell ordered replay (MAX / BLEND), colour lookup, ARGB pack; emission of the max grid */
    float total_ms;      /* first event to last event */
    uint32_t passes;     /* 1, or more if a device buffer had to grow and the pipeline was re-run */
    float plan_ms;       /* o2v_hip_voxelize_sharded only: sharded bounds + work histogram passes incl. their collectives
                            (host wall time; not part of total_ms) */
    float collective_ms; /* ... of which inside the collectives (all-reduce of bounds and histogram, all-gather of the
                            block extents and of the slab counts) */
    float collective_parts_ms[5]; /* the same by collective, device time on the context's stream: [0] the ranks' readiness words
                            and the mesh bounds in one all-reduce (max of 7 x u32: the minima travel as their complements),
                            [1] unused (0), [2] every rank's z histogram of predicted work (2048 x u64) and the z extents of
                            its blocks (8 bytes per 256 triangles) in one all-gather - each rank adds the histograms up itself -
                            [3] unused (0), [4] slab voxel counts (all-gather, 8 bytes per rank) */
    float fill_ms;       /* K6  solid fill (O2V_HIP_FLAG_FILL_INTERIOR): crossings, prefix XOR, surface removal, count, emission;
                            measured like the other stage times (not part of total_ms) */
} o2v_hip_timings;

/* Work counters of the last o2v_hip_voxelize call. */
typedef struct {
    uint64_t triangles;   /* input triangles */
    uint64_t leaves;      /* leaf sub-triangles overlapping the slab */
    uint64_t tiles;       /* work tiles of <= 256 candidate voxels */
    uint64_t candidates;  /* (leaf, voxel) pairs examined */
    uint64_t hits;        /* (leaf, voxel) pairs with non-zero weight */
    uint64_t voxels;      /* occupied output voxels: every record of the call, interior voxels included */
    uint64_t grid_cells;  /* dense grid cells owned by this context (bricks of 4x4x4, padded) */
    uint64_t grid_bytes;  /* bytes of the dense grid allocation incl. the per-brick dirty flags */
    uint64_t bricks;      /* bricks of the slab */
    uint64_t dirty_bricks;/* bricks that received at least one hit */
    uint64_t pool_slots;  /* hit-pool slots reserved (hits + chunk slack) */
    uint64_t direct_hits; /* hits that went straight into the 64-bit max grid (MAX strategy, unsplit triangles) */
    uint64_t jobs;        /* candidates that passed the plane cull and the separating-axis pre-test: voxel jobs of the clip loop */
    uint64_t certain_hits;/* occupancy-only mode: hits established without a voxel job (the voxel centre's column meets the leaf
                             well inside both), included in hits and direct_hits */
    uint64_t skipped_jobs;/* occupancy-only mode: those of `jobs` that were not run because their voxel was marked already when
                             phase 2 of their batch began (which ones depends on the order the workgroups happen to run in, so
                             this number and `hits` - only hits that were established are counted - vary from run to run;
                             the voxels do not) */
    uint64_t bypassed_leaves; /* occupancy-only mode: those of `leaves` (and `tiles`) that have no Leaf / Tile record - root triangles
                                 of one tile, which the clip kernel stages from the vertex array itself */
    uint64_t interior_voxels; /* O2V_HIP_FLAG_FILL_INTERIOR: the records behind the surface records (part of voxels); else 0 */
} o2v_hip_stats;

int o2v_hip_device_count(void);
int o2v_hip_create(int device, o2v_hip_ctx **out_ctx);
void o2v_hip_destroy(o2v_hip_ctx *ctx);
const char *o2v_hip_last_error(const o2v_hip_ctx *ctx);

/* Host arrays, copied to the device.  verts: [count][9] model-space xyz of the three vertices.
 * uvs: [count][6] or NULL (zeros).  types: [count] or NULL (all MATERIALLESS).  colors: [count][3] or NULL.
 * texids: [count] indices into the texture table, or NULL (all 0). */
int o2v_hip_set_triangles(o2v_hip_ctx *ctx, const float *verts, const float *uvs, const uint32_t *types,
                          const float *colors, const int32_t *texids, uint64_t count);
int o2v_hip_set_textures(o2v_hip_ctx *ctx, const o2v_hip_texture *textures, uint32_t count);

/* Streamed variant of o2v_hip_set_triangles for a triangle source that is drained one triangle at a time (the reference's
 * cache loop, src/obj2voxel.cpp:578-600): the caller fills a block of page-locked staging memory owned by the context,
 * commits it - the block is copied to the device asynchronously while the caller fills the other block - and finishes.
 * `arrays` says which optional arrays the mesh has so far (bit 0 uvs, 1 types, 2 colors, 3 texids; verts always); an
 * array may appear at any commit, the triangles before it get its default (zero uvs / MATERIALLESS / zero colour /
 * texture 0) on the device, and from then on the caller fills it for every triangle.  Only verts is there from the
 * start: before the caller writes an optional array for the first time it asks for it with o2v_hip_stage_arrays (page
 * locking memory costs ~0.1 ms per MiB, and most meshes are vertices only). */
typedef struct {
    float *verts;      /* [capacity][9] */
    float *uvs;        /* [capacity][6], NULL until asked for */
    uint32_t *types;   /* [capacity]    , NULL until asked for */
    float *colors;     /* [capacity][3], NULL until asked for */
    int32_t *texids;   /* [capacity]    , NULL until asked for */
    uint64_t capacity; /* triangles per block */
} o2v_hip_staging;
enum { O2V_HIP_ARRAY_UVS = 1, O2V_HIP_ARRAY_TYPES = 2, O2V_HIP_ARRAY_COLORS = 4, O2V_HIP_ARRAY_TEXIDS = 8 };
int o2v_hip_begin_triangles(o2v_hip_ctx *ctx, o2v_hip_staging *out_block);
/* Makes the optional arrays named by `arrays` part of both staging blocks; *inout_block (the block being filled) gets their
 * addresses.  What the block holds already stays. */
int o2v_hip_stage_arrays(o2v_hip_ctx *ctx, uint32_t arrays, o2v_hip_staging *inout_block);
int o2v_hip_commit_triangles(o2v_hip_ctx *ctx, uint64_t count, uint32_t arrays, o2v_hip_staging *out_next_block);
int o2v_hip_end_triangles(o2v_hip_ctx *ctx, uint32_t any_textured);

/* Runs the whole device pipeline and waits for it.  out_voxel_count receives the number of occupied voxels. */
int o2v_hip_voxelize(o2v_hip_ctx *ctx, const o2v_hip_params *params, uint64_t *out_voxel_count);

/* Work-balanced z-slabs for a multi-GPU job (one process per GPU, every process holding the same triangles):
 * writes n_slabs+1 ascending output-z cuts to out_z (out_z[0] = 0, out_z[n_slabs] = resolution); slab k is
 * [out_z[k], out_z[k+1]) and goes into o2v_hip_params::z_begin/z_end of rank k.  The cuts equalise the predicted
 * number of (triangle, voxel) hits per slab, which the pipeline's time is proportional to; they are a pure
 * function of the triangles and the parameters, so every rank computes the same ones without communicating.
 * The reference balances its worker pool dynamically over 64^3 chunks (src/obj2voxel.cpp:482-497); slabs are
 * static, hence the up-front plan.  out_bounds (optional, 6 floats: min xyz, max xyz) receives the mesh bounds
 * found on the way (reference findMeshBounds, src/obj2voxel.cpp:180-200): passing them back as
 * o2v_hip_params::bounds with bounds_known = 1 saves the voxelize call its own bounds pass.  z_begin/z_end of
 * `params` are ignored. */
int o2v_hip_plan_slabs(o2v_hip_ctx *ctx, const o2v_hip_params *params, uint32_t n_slabs, uint32_t *out_z,
                       float *out_bounds);

/* The thickest z-slab (in output layers, a multiple of 4 unless it is the whole grid) whose dense grids fit the device memory
 * that is free right now (plus what the context already holds), leaving room for the work buffers: a voxelization of
 * `params` can be run as ceil(resolution / layers) calls with consecutive slabs.  obj2voxel_voxelize() does that by itself
 * (the reference's sparse VoxelMap has no such limit: src/util.hpp:179-208); 0 layers = not even one brick layer fits.
 * A slab is also never taller than one pass' box may be (65 535 samples): when the mesh's voxel bounding box is taller than
 * that in z, the result is at most (65535 / supersampling) & ~3 layers (65 532, or 32 764 at 2x supersampling), however
 * much memory is free. */
int o2v_hip_max_slab_layers(o2v_hip_ctx *ctx, const o2v_hip_params *params, uint32_t *out_layers);

/* Copies voxels [first, first+count) of the last result to host memory as (x, y, z, argb) uint32 quadruples,
 * the layout of the reference's voxel callback (include/obj2voxel.h:35,200-209).  Order is unspecified. */
int o2v_hip_read_voxels(o2v_hip_ctx *ctx, uint32_t *out, uint64_t first, uint64_t count);
/* The same copy in two steps, for overlapping it with the consumer of the previous batch: _async starts the copy on the
 * context's stream (`out` should be pinned memory, see o2v_hip_alloc_pinned), _wait returns when it has landed. */
int o2v_hip_read_voxels_async(o2v_hip_ctx *ctx, uint32_t *out, uint64_t first, uint64_t count);
int o2v_hip_read_voxels_wait(o2v_hip_ctx *ctx);
/* Page-locked host memory (hipHostMalloc / hipHostFree): transfers from and to it run asynchronously at link rate. */
void *o2v_hip_alloc_pinned(size_t bytes);
/* The same on a thread that has not selected a device yet: `device` becomes the calling thread's current device first (a
 * thread's default is device 0, which need not be the one the caller works on - or one it may touch at all). */
void *o2v_hip_alloc_pinned_on(int device, size_t bytes);
void o2v_hip_free_pinned(void *p);
/* Releases the device session that obj2voxel_voxelize() keeps between calls (contexts, dense grids, staging memory). */
void o2v_release_cached_device_memory(void);
/* Solid voxelization through the public C API: with enabled != 0, obj2voxel_voxelize() fills the interior of the mesh with voxels
 * of colour argb (0xAARRGGBB), O2V_HIP_FLAG_FILL_INTERIOR in every pass; every output receives them like any other voxel.
 * Off by default. */
struct obj2voxel_instance; /* include/obj2voxel.h */
void o2v_set_fill(struct obj2voxel_instance *instance, int enabled, uint32_t argb);
/* Device pointer to the same records (valid until the next voxelize/destroy). */
int o2v_hip_voxels_device_ptr(o2v_hip_ctx *ctx, const uint32_t **out_ptr, uint64_t *out_count);

/* ---- device-resident input and dense output -------------------------------------------------
 *
 * The arrays of o2v_hip_set_triangles, in device memory of the context's device.  faces == NULL: positions is [count][9]
 * (the host call's verts) and n_positions is ignored.  Otherwise positions is [n_positions][3], faces is [count][3] of
 * index_bytes (4: int32, 8: int64) each, and triangle t is positions[faces[t][0..2]].  uvs [count][6], types [count],
 * colors [count][3] and texids [count] are per triangle and optional, as in the host call.
 * The context then holds exactly the arrays o2v_hip_set_triangles would hold for the host-gathered mesh, bit for bit; the
 * rules on count (below 2^29), absent arrays and non-finite values are the host call's.
 * Every pointer must be device (or managed) memory of the context's device, with the array's whole extent inside its
 * allocation; anything else - host memory, another device's memory, an unknown pointer, a short allocation - is refused with
 * O2V_HIP_ERR_BAD_ARGUMENT before anything is launched.  A face index that is negative, not below n_positions or (int64) not
 * below 2^32 is never read (every index is clamped before its load) but fails the call with O2V_HIP_ERR_BAD_ARGUMENT
 * ("face index out of range ..."); the context is then left with no triangles and stays usable.
 * The arrays are read on the context's own stream: the caller must have finished writing them (synchronised its stream)
 * before the call.  The call returns after the reads have landed; the caller may reuse the memory at once. */
int o2v_hip_set_triangles_device(o2v_hip_ctx *ctx, const float *positions, uint64_t n_positions, const void *faces,
                                 uint32_t index_bytes, const float *uvs, const uint32_t *types, const float *colors,
                                 const int32_t *texids, uint64_t count);

enum { O2V_HIP_DENSE_U8 = 0, O2V_HIP_DENSE_ARGB32 = 1, O2V_HIP_DENSE_BITS = 2 };
/* Scatters the records of the last o2v_hip_voxelize call into a caller-owned dense grid in device memory of the context's
 * device.  Voxel (x, y, z) with origin <= (x, y, z) < origin + dims goes to
 *   U8, ARGB32: dst[(x - ox) * strides[0] + (y - oy) * strides[1] + (z - oz) * strides[2]]  (strides in elements)
 *   BITS:       bit (x - ox) % 32 of 32-bit word ((x - ox) / 32) + (y - oy) * strides[1] + (z - oz) * strides[2]
 *               (strides[0] must be 1; strides in words)
 * U8 writes 1 for a surface record and 2 for an interior record (O2V_HIP_FLAG_FILL_INTERIOR), ARGB32 the record's argb,
 * BITS sets the bit (a device-scope atomicOr).  ARGB32 does not encode occupancy: a texel with alpha 0 gives argb 0x00000000,
 * which reads like an empty cell; take occupancy from U8 or BITS.  Nothing else in dst is written: the caller clears it.
 * Records outside the box are not written and are counted in *out_outside (may be NULL).  dst is checked like the arrays of
 * o2v_hip_set_triangles_device: the highest address the box and strides reach must lie inside its allocation; zero dims and
 * BITS with strides[0] != 1 are refused.  The grid is written on the context's stream; the call returns when the writes have
 * landed (the caller must have finished clearing dst before). */
int o2v_hip_write_dense(o2v_hip_ctx *ctx, void *dst, uint32_t format, const uint32_t origin[3], const uint32_t dims[3],
                        const uint64_t strides[3], uint64_t *out_outside);
/* The tight box [lo, hi) of the last call's records, reduced on the device; lo = hi = 0 when there are none. */
int o2v_hip_voxels_box(o2v_hip_ctx *ctx, uint32_t lo[3], uint32_t hi[3]);

/* ---- distance grids --------------------------------------------------------------------------
 *
 * The exact Euclidean distance transform of a U8 label grid L in device memory (0 empty, 1 surface, 2 interior: what
 * o2v_hip_write_dense U8 writes) over the box dims = (nx, ny, nz).  Voxel (x, y, z) is labels[x * label_strides[0] +
 * y * label_strides[1] + z * label_strides[2]] and dst[x * dst_strides[0] + ...] (strides in elements, any order).  With S the
 * surface voxels (L == 1),
 *   d2(v) = min over s in S of (vx - sx)^2 + (vy - sy)^2 + (vz - sz)^2,  exact integers in voxel units, over the box only;
 *   DIST2 (int32):  d2(v); 0 on the surface; 0x7FFFFFFF everywhere if S is empty;
 *   SDF (float32):  sgn(v) * (float) sqrt((double) d2(v)), sgn = -1 where L == 2 and +1 elsewhere; +-inf if S is empty.
 * The call is refused with O2V_HIP_ERR_LIMIT when (nx-1)^2 + (ny-1)^2 + (nz-1)^2 is above 2^31 - 2, and with
 * O2V_HIP_ERR_BAD_ARGUMENT for zero dims, an unknown format, overlapping labels and dst ranges, dst_strides that map two
 * voxels of the box to one element (e.g. a stride of 0 on an axis of more than one voxel), or a pointer that is not device
 * memory of the context's device with the box's highest address inside its allocation: all before anything is launched.
 * Every voxel of the box in dst is written (the intermediate passes use dst itself); labels is only read.  The envelope stacks
 * are scratch of the context, o2v_hip_distance_scratch_bytes(dims, format) bytes = 8 x the larger of min(nx * nz, 2^17) * ny
 * (the y pass) and min(nx * ny, 2^17) * nz (the z pass), grown on demand; if it cannot be allocated the call returns O2V_HIP_ERR_OUT_OF_MEMORY and the context stays usable.  The grid is read and written
 * on the context's stream; the call returns when the writes have landed (the caller must have finished writing labels). */
enum { O2V_HIP_DIST_SQ_I32 = 0, O2V_HIP_DIST_SDF_F32 = 1 };
int o2v_hip_distance_dense(o2v_hip_ctx *ctx, const void *labels, const uint64_t label_strides[3], void *dst, uint32_t format,
                           const uint64_t dst_strides[3], const uint32_t dims[3]);
uint64_t o2v_hip_distance_scratch_bytes(const uint32_t dims[3], uint32_t format);
/* The device times of the last o2v_hip_distance_dense call's three passes (x, y, z), from events around each, in ms. */
int o2v_hip_distance_times(const o2v_hip_ctx *ctx, float out_ms[3]);

/* ---- narrow-band distance to the triangles ----------------------------------------------------
 *
 * The distance from each voxel centre of a box to the context's triangles themselves (not to surface voxels), exact in a band
 * and truncated at it.  The mesh is the context's triangles in their order (o2v_hip_set_triangles, _device or the streamed
 * upload).  Of params, resolution, supersampling (1 or 2), unit_transform, bounds_known and bounds are read; strategy, flags and
 * fill_argb are ignored; z_begin .. y_end must be 0 (else O2V_HIP_ERR_BAD_ARGUMENT).  The mesh transform A is the one
 * o2v_hip_voxelize computes for the same params and reports through o2v_hip_get_transform, bit for bit.
 *   Vertices: sample space as K1 / K6 take them (affine_apply of A, float32); a triangle with a non-finite coordinate is ignored.
 *   Centres: with ss = supersampling, voxel (x, y, z) has P = (x ss + ss/2, y ss + ss/2, z ss + ss/2), in double.
 *   d2_t(P), in double, op by op, left to right, no FMA; A, B, C converted from float32; dot, cross and squared norms written
 *   out component by component, left to right:
 *     ab = B - A, ac = C - A, ap = P - A, n = cross(ab, ac), nn = n.n;
 *     if nn > 0: s0 = n.cross(B - A, P - A), s1 = n.cross(C - B, P - B), s2 = n.cross(A - C, P - C); if all three are >= 0,
 *       d2 = (h * h) / nn with h = n.ap;
 *     otherwise (always when nn == 0): d2 = min(seg(P, A, B), seg(P, B, C), seg(P, C, A)), where seg(P, U, V): e = V - U,
 *       w = P - U, ee = e.e, t = 0 if ee == 0 else (w.e) / ee clamped by t < 0 ? 0 : (t > 1 ? 1 : t), q = w - t * e per
 *       component, result q.q.
 *   D(P) = min over the triangles of d2_t(P).  A triangle takes part for P only if P lies in its sample-space AABB dilated by
 *   band ss + ss on every side (compared in double: (double) min - m <= P <= (double) max + m, m = (double) band * ss + ss);
 *   the extra sample is a margin above every rounding of d2, so this cut leaves D unchanged wherever D < Bs2 (below).
 *   band (voxels) must be finite with 0 < band <= 32 (else O2V_HIP_ERR_BAD_ARGUMENT); Bs2 = (double) band * band * ss * ss.
 *   UNSIGNED_F32: u = D < Bs2 ? (float) (sqrt(D) / ss) : band.
 *   SIGNED_F32:   -u (float negation: a centre exactly on a triangle inside gives -0.0) where the voxel is in the parity set
 *                 of O2V_HIP_FLAG_FILL_INTERIOR (the definition above, with the mesh's top-layer cut) - for every voxel,
 *                 surface voxels included - else u.  An empty mesh gives +band everywhere.
 *   closest (optional, int32): the smallest t with d2_t = D where D < Bs2, else -1.
 * The value of a voxel depends only on its centre and the whole mesh: a box cut into z ranges gives the bits of one call.
 * Box: origin and dims are output voxels, dims >= 1 and origin + dims <= resolution per axis (else BAD_ARGUMENT); a dim above
 * 65 535 is refused with O2V_HIP_ERR_LIMIT.  Voxel (x, y, z) of the box is dst[(x - ox) * dst_strides[0] + (y - oy) *
 * dst_strides[1] + (z - oz) * dst_strides[2]] (elements, any order), likewise closest with closest_strides; every voxel of the
 * box is written to both.  Refused with O2V_HIP_ERR_BAD_ARGUMENT before any launch: an unknown format, strides that map two
 * voxels to one element, dst and closest overlapping, a pointer that is not device memory of the context's device with the
 * box's highest address inside its allocation.  Scratch (binned triangle lists, the parity bitmap) belongs to the context and
 * grows on demand; a failed allocation returns O2V_HIP_ERR_OUT_OF_MEMORY and the context stays usable.  The call runs on the
 * context's stream and returns when the writes have landed. */
enum { O2V_HIP_MESH_DIST_UNSIGNED_F32 = 0, O2V_HIP_MESH_DIST_SIGNED_F32 = 1 };
int o2v_hip_mesh_distance_dense(o2v_hip_ctx *ctx, const o2v_hip_params *params, float band, uint32_t format,
                                const uint32_t origin[3], const uint32_t dims[3], float *dst, const uint64_t dst_strides[3],
                                int32_t *closest /* may be NULL */, const uint64_t closest_strides[3]);
/* The device times (ms) of the last o2v_hip_mesh_distance_dense call's stages: binning, parity (0 unsigned), distance. */
int o2v_hip_mesh_distance_times(const o2v_hip_ctx *ctx, float out_ms[3]);

/* ---- surface extraction ------------------------------------------------------------------------
 *
 * The level set of a dense float32 grid as an indexed triangle mesh, by surface nets: one vertex per cell the surface passes
 * through, one quad (two triangles) per grid edge it crosses.  The mesh comes out in the shape o2v_hip_set_triangles_device
 * takes (positions [V][3] float32, faces [T][3] int32), in device memory the caller owns.
 *
 * Input: a grid f of dims = (nx, ny, nz) float32 samples in device memory, sample (x, y, z) at field[x * strides[0] +
 * y * strides[1] + z * strides[2]] (elements, any order; the field is only read, so a stride may be 0 and samples may share
 * elements, as in an expanded tensor), a finite level, and origin = (ox, oy, oz) in voxels.  Sample (x, y, z)
 * stands for the voxel centre (ox + x + 0.5, oy + y + 0.5, oz + z + 0.5): the voxel space of the sections above with
 * supersampling 1.
 *   inside(x, y, z) = f(x, y, z) < level (a NaN is outside; -inf inside, +inf outside).
 *   Cells: (i, j, k) with 0 <= i < nx - 1, 0 <= j < ny - 1, 0 <= k < nz - 1; its corner (a, b, c), each 0 or 1, is sample
 *   (i + a, j + b, k + c).  A cell is active if its eight corners are not all inside and not all outside.  A grid with a dim
 *   of 1 has no cells.
 *   Vertices: one per active cell, numbered in ascending cell order (k * (ny - 1) + j) * (nx - 1) + i.  Its position, all in
 *   float32, op by op, no FMA:
 *     the cell's 12 edges in this order: the four x edges (0,b,c)-(1,b,c) for (b, c) = (0,0), (1,0), (0,1), (1,1); the four y
 *     edges (a,0,c)-(a,1,c) for (a, c) in the same order; the four z edges (a,b,0)-(a,b,1) for (a, b) in the same order; p is
 *     always the end with the lower coordinate, q the other;
 *     an edge crosses if inside(p) != inside(q); then t = (level - f(p)) / (f(q) - f(p)), and t = 0.5f unless t >= 0 && t <= 1
 *     (this takes care of infinities and NaN); its crossing point, local to the cell, is p's (a, b, c) as floats with the
 *     component along the edge replaced by t;
 *     s = (0, 0, 0), then the crossing points are added component by component in edge order; n = their number;
 *     local = s / (float) n; position = ((float) (o + cell index) + 0.5f) + local per axis, (x, y, z) order in memory.
 *     The divisions are the correctly rounded float32 ones.
 *   Faces: for every sample c = (x, y, z) and axis ax in 0, 1, 2 such that the edge from c to c + e_ax exists, crosses, and is
 *   interior across (with u = (ax + 1) % 3, v = (ax + 2) % 3: 1 <= c[u] <= n_u - 2 and 1 <= c[v] <= n_v - 2), one quad of the four
 *   cells around the edge: c0 = c - e_u - e_v, c1 = c - e_v, c2 = c, c3 = c - e_u (a cell is named by its lowest corner; all four
 *   are active because they contain the edge).  If inside(c) the quad is (c0, c1, c2, c3), else (c0, c3, c2, c1): the normal
 *   points from inside to outside.  It is written as the two triangles (q0, q1, q2), (q0, q2, q3) of int32 vertex numbers.  Quads
 *   come in ascending order of ((z * ny + y) * nx + x) * 3 + ax.
 *   A crossing edge on the border of the box has fewer than four cells and gives no quad: a surface that leaves the box is open
 *   there, and a vertex of a border cell may be used by no face.
 *
 * The caller cannot know the output's size beforehand, so there are two calls.  o2v_hip_surface_count classifies the grid
 * (its only pass over the field), keeps what the second call needs in scratch of the context - per 64 samples along x their
 * sign bits, their active cells and two 16-bit prefixes, per 256 such words two offsets: 20 bytes per 64 samples, not an index
 * per cell - and returns the two totals.  o2v_hip_surface_write must follow a count with the same field, strides, dims and level
 * (else O2V_HIP_ERR_BAD_ARGUMENT, "no matching o2v_hip_surface_count"; another count, refused or not, replaces the last one) and
 * fills positions and faces, contiguous; it may be repeated.  The field must not change between the two calls; if it does, the
 * positions may be meaningless, but every index written is below the counted vertices and nothing is written outside the two
 * arrays: the topology comes from the kept bits, only t and the corner values from the field.
 * Refused before any launch: null arguments (positions or faces may be null only where the count is 0), zero dims, a level
 * that is not finite, capacities below the counted totals, positions / faces overlapping each other or the field, a pointer
 * that is not device memory of the context's device with its whole extent inside its allocation (O2V_HIP_ERR_BAD_ARGUMENT); a
 * dim above 65 536, or origin[a] + dims[a] above 65 536 (positions stay exact to 2^-7 voxel), or more than 2^31 - 1 vertices
 * (O2V_HIP_ERR_LIMIT).  A failed scratch allocation returns O2V_HIP_ERR_OUT_OF_MEMORY and the context stays usable.  Both calls
 * run on the context's stream and return when their results have landed (the caller must have finished writing the field). */
int o2v_hip_surface_count(o2v_hip_ctx *ctx, const float *field, const uint64_t strides[3], const uint32_t dims[3], float level,
                          uint64_t *out_vertices, uint64_t *out_triangles);
int o2v_hip_surface_write(o2v_hip_ctx *ctx, const float *field, const uint64_t strides[3], const uint32_t dims[3], float level,
                          const uint32_t origin[3], float *positions, uint64_t vertex_capacity, int32_t *faces,
                          uint64_t triangle_capacity);
/* The device times (ms) of the stages: classify, count + scan (the last o2v_hip_surface_count), vertices, faces (the last
 * o2v_hip_surface_write; 0 after a count). */
int o2v_hip_surface_times(const o2v_hip_ctx *ctx, float out_ms[4]);

/* ---- ray casting --------------------------------------------------------------------------------
 *
 * First hits of rays in a dense voxel grid, defined bit for bit by a walk from cell to cell; the device may skip empty space
 * but returns what this walk returns, for every ray.
 *
 * Space: the voxel space of the sections above with supersampling 1.  Voxel (x, y, z) of the grid is the cube
 * [ox + x, ox + x + 1) x [oy + y, oy + y + 1) x [oz + z, oz + z + 1), origin = (ox, oy, oz) integers, dims = (nx, ny, nz);
 * everything outside the box is empty.  A voxel is solid, by format:
 *   O2V_HIP_RAY_GRID_U8         grid[x * strides[0] + y * strides[1] + z * strides[2]] != 0 (bytes: bool tensors, labels; any strides)
 *   O2V_HIP_RAY_GRID_BITS       bit x % 32 of the 32-bit word (x / 32) + y * strides[1] + z * strides[2]: what o2v_hip_write_dense
 *                               BITS writes (strides[0] must be 1; strides in words)
 *   O2V_HIP_RAY_GRID_F32_BELOW  f < level for the float32 f at the U8 address (elements); a NaN is empty, as `inside` above;
 *                               level must be finite
 * The grid is only read: a stride may be 0 and voxels may share elements.
 *
 * A ray has an origin o and a direction d, three float32 each, converted to double; d is not normalised, so t is in units of
 * |d|; t_max is a float32, >= 0 or +inf, converted to double.  All arithmetic is in double, op by op, no FMA.
 *   For an axis a with d_a != 0: inv_a = 1.0 / d_a, s_a = sgn d_a, and the parameter of plane i is
 *     T_a(i) = ((double) i - o_a) * inv_a,
 *   computed per plane index, never accumulated.  An axis with d_a == 0 (-0.0 too) never steps.
 *   The start cell is c = floor(o); the next plane of axis a is n_a = c_a + 1 if d_a > 0, else c_a.
 *   If c is in the box and solid, the ray hits with t = 0, face = -1, voxel c.  Otherwise repeat:
 *     1. a = the axis with the smallest T_a(n_a); of equal ones the lowest axis;
 *     2. if no axis can step, or that T > t_max, the ray misses;
 *     3. c_a += s_a and n_a += s_a;
 *     4. if c is in the box and solid, the ray hits: t = (float) T, face = 2 a + (s_a > 0 ? 0 : 1) - the face it entered
 *        through: 0 / 1 the voxel's low / high x face, 2 / 3 y, 4 / 5 z -, voxel c;
 *     5. the ray misses once it has left the box on an axis for good (it is past the box in its direction on that axis, or
 *        beside the box on an axis it does not step on).
 *   A ray that starts on a voxel face and points in the negative direction visits the cell floor(o) first, at t = 0, and the
 *   cell below it next, also at T = 0: floor(o) is the start cell whatever the direction.  That is the definition.
 *   t_max exactly equal to a plane's T still crosses it (the test is T > t_max).
 * Output per ray: hit int32[4] = (x, y, z, face) in global voxel coordinates, and t float32.
 *   A miss: hit = (-1, -1, -1, -1), t = +inf.
 *   An invalid ray - a component of o or d that is not finite, or |o_a| > 2^22 -: hit = (-1, -1, -1, -2), t = NaN.
 *   d = 0 is valid: only the start cell is tested.
 * Why empty space can be skipped exactly: per axis T_a rises along the stepping direction, so the walk is the merge of the
 * three plane sequences in order of (T, axis).  Leaving an empty aligned block, or entering the box from outside, is "advance
 * to event E" - the least exit event of the block, or the greatest entry event of the axes on which the ray is still outside -
 * after which every other axis b stands at its first plane j with (T_b(j), b) > E; that plane is found from the estimate
 * floor(o_b + T d_b) and corrected by comparing T_b(j) itself.
 *
 * o2v_hip_raycast_build makes the one pass over the grid and keeps a snapshot in scratch of the context: a 64-bit word per
 * 4^3 voxels (their solid bits), per 16^3 (its non-empty 4^3 bricks) and per 64^3 (its non-empty 16^3 blocks), aligned to the
 * box's origin:
 *   o2v_hip_raycast_scratch_bytes(dims) = 8 * (B(4) + B(16) + B(64)),  B(k) = ceil(nx / k) * ceil(ny / k) * ceil(nz / k)
 * (0 for zero dims) - 1/8 byte per voxel and 1/63 more.  The grid may change or be freed afterwards: casting never reads it.
 * A new build, refused or not, replaces the last one; o2v_hip_raycast_generation counts the builds of the context, refused ones
 * included, so a caller can tell whether the snapshot is still the one it built.
 * o2v_hip_raycast casts n rays (origins, directions [n][3] float32; hit [n][4] int32 and t [n] float32, contiguous, all in
 * device memory of the context's device) through the last build; without one it returns O2V_HIP_ERR_BAD_ARGUMENT, "no
 * o2v_hip_raycast_build".  It may be repeated; n = 0 launches nothing and reads no pointer.
 * Refused before any launch: null arguments, zero dims, an unknown format, BITS with strides[0] != 1, a level that is not finite
 * (F32_BELOW only; ignored otherwise), t_max NaN or negative, hit and t overlapping each other or the rays, a pointer that is not
 * device memory of the context's device with its whole extent inside its allocation (O2V_HIP_ERR_BAD_ARGUMENT); origin[a] +
 * dims[a] above 65 536, n above 2^31 - 1 (O2V_HIP_ERR_LIMIT).  A failed scratch allocation returns O2V_HIP_ERR_OUT_OF_MEMORY
 * and the context stays usable.  Both calls run on the context's stream and return when their results have landed (the caller
 * must have finished writing the grid and the rays).
 * O2V_RAY_NO_SKIP=1 in the environment (A/B): the cast walks every fine cell; same results. */
enum { O2V_HIP_RAY_GRID_U8 = 0, O2V_HIP_RAY_GRID_BITS = 1, O2V_HIP_RAY_GRID_F32_BELOW = 2 };
int o2v_hip_raycast_build(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3],
                          float level, const uint32_t origin[3]);
int o2v_hip_raycast(o2v_hip_ctx *ctx, const float *origins /* [n][3] */, const float *directions /* [n][3] */, uint64_t n, float t_max,
                    int32_t *hit /* [n][4] */, float *t /* [n] */);
uint64_t o2v_hip_raycast_scratch_bytes(const uint32_t dims[3]);
uint64_t o2v_hip_raycast_generation(const o2v_hip_ctx *ctx);
/* The device times (ms) of the last o2v_hip_raycast_build and of the last o2v_hip_raycast. */
int o2v_hip_raycast_times(const o2v_hip_ctx *ctx, float out_ms[2]);

/* ---- connected components and flood fill ------------------------------------------------------------
 *
 * What is connected to what in a dense voxel grid, defined so that a numpy restatement reproduces every bit.
 *
 * The set.  The grid, its three formats, the rules for its strides and the rule for BITS (strides[0] == 1) are those of
 * o2v_hip_raycast_build: O2V_HIP_GRID_U8 (element != 0), O2V_HIP_GRID_BITS, O2V_HIP_GRID_F32_BELOW (f < level with a finite
 * level; a NaN is not below it) - the values of O2V_HIP_RAY_GRID_*, which stay.  The grid is only read: a stride may be 0.
 * Those voxels are the solid ones.  Without a flag the set S is the solid voxels of the box; with O2V_HIP_CC_INVERT it is the
 * voxels of the box that are not solid.
 * Connectivity is 6, 18 or 26: two voxels of S are adjacent if they differ by at most 1 on every axis and on at most 1, 2 or 3
 * axes.  Nothing outside the box is adjacent to anything.  A component is a class of the transitive closure of adjacency.
 *
 * o2v_hip_components_dense writes labels(x, y, z) = labels[x * label_strides[0] + y * label_strides[1] + z * label_strides[2]]
 * (int32, strides in elements, no two voxels on one element) for every voxel of the box: 0 outside S; inside S, 1 + the rank of
 * the voxel's component, the components ranked by their smallest linear index (z * ny + y) * nx + x.  *out_count is the number
 * of components.  This is the numbering of scipy.ndimage.label on a [z, y, x] array.
 *
 * o2v_hip_flood_dense marks the components that hold a seed.  seeds: int32 [n_seeds][3], local (x, y, z), in device memory; a
 * seed outside the box or not in S is ignored; with n_seeds = 0 the pointer is not read.  O2V_HIP_CC_SEED_BORDER additionally
 * seeds every voxel of S on the six faces of the box.  Every voxel of the box is written, out(x, y, z) (uint8, strides as for
 * labels) = values[0] if it is in S and its component holds a seed, values[1] if it is in S and its component holds none,
 * values[2] if it is not in S.  *out_reached is the number of voxels that got values[0].
 *
 * flags: O2V_HIP_CC_INVERT, O2V_HIP_CC_SEED_BORDER (flood only), O2V_HIP_FLAG_STAGE_TIMES (o2v_hip_components_counters counts).
 * Refused before any launch, labels / out untouched: null arguments, zero dims, an unknown format, a connectivity other than 6,
 * 18, 26, unknown flag bits, BITS with strides[0] != 1, a level that is not finite (F32_BELOW only), labels / out overlapping the
 * grid or the seeds, label / out strides that map two voxels to one element, a pointer that is not device memory of the context's
 * device with its whole extent inside its allocation (O2V_HIP_ERR_BAD_ARGUMENT); a dim above 65 536, nx * ny * nz or n_seeds above
 * 2^31 - 1 - a linear index and a label are one int32 - (O2V_HIP_ERR_LIMIT).  A failed scratch allocation returns
 * O2V_HIP_ERR_OUT_OF_MEMORY and the context stays usable.  After a later error labels / out are unspecified.  Both calls run on
 * the context's stream and return when their results have landed (the caller must have finished writing the grid and the seeds).
 *
 * Scratch of the context, grown on demand, with words = ceil(nx / 64) * ny * nz and voxels = nx * ny * nz:
 *   O2V_HIP_CC_SCRATCH_LABELS          20 * words + 8 * (ceil(words / 256) + 1) + 32: the set's bits, the root flags, the per-word
 *                                      prefixes, the block offsets, counters.  No per-voxel scratch: the parents live in labels
 *                                      until the last pass.  This holds where labels are contiguous (strides 1, nx, nx * ny);
 *   O2V_HIP_CC_SCRATCH_LABELS_STRIDED  ... + 4 * voxels: labels of any other strides, the parents in the context;
 *   O2V_HIP_CC_SCRATCH_FLOOD           16 * words + 4 * voxels + 32: the set's bits, the seed flags, the parents, counters.
 * (0 for zero dims or an unknown `which`.)
 * O2V_CC_NO_TILES=1 in the environment (A/B): no tile pass, every adjacent pair is united in global memory; same results. */
enum { O2V_HIP_GRID_U8 = 0, O2V_HIP_GRID_BITS = 1, O2V_HIP_GRID_F32_BELOW = 2 };
enum { O2V_HIP_CC_INVERT = 16u, O2V_HIP_CC_SEED_BORDER = 32u };
enum { O2V_HIP_CC_SCRATCH_LABELS = 0, O2V_HIP_CC_SCRATCH_LABELS_STRIDED = 1, O2V_HIP_CC_SCRATCH_FLOOD = 2 };
int o2v_hip_components_dense(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3],
                             float level, uint32_t connectivity, uint32_t flags, int32_t *labels, const uint64_t label_strides[3],
                             uint64_t *out_count);
int o2v_hip_flood_dense(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                        uint32_t connectivity, uint32_t flags, const int32_t *seeds /* [n_seeds][3] */, uint64_t n_seeds,
                        const uint8_t values[3], uint8_t *out, const uint64_t out_strides[3], uint64_t *out_reached);
uint64_t o2v_hip_components_scratch_bytes(const uint32_t dims[3], uint32_t which);
/* The device times (ms) of the last of the two calls: classify, tile pass, seams, flatten (+ root count), write (+ seeds). */
int o2v_hip_components_times(const o2v_hip_ctx *ctx, float out_ms[5]);
/* Of the last call made with O2V_HIP_FLAG_STAGE_TIMES (else zeros): the pairs united across tile seams (every pair with
 * O2V_CC_NO_TILES=1) and the atomic mins that did not meet a root and went round again. */
int o2v_hip_components_counters(const o2v_hip_ctx *ctx, uint64_t out2[2]);

/* ---- dense grids as voxel lists and voxel files -------------------------------------------------------
 *
 * The way back from a dense grid to (x, y, z, argb) records - the layout of o2v_hip_read_voxels - and to the voxel files of
 * obj2voxel_voxelize(), defined so that a numpy restatement reproduces every bit.
 *
 * The set.  grid, format (O2V_HIP_GRID_U8 / _BITS / _F32_BELOW), strides, dims and level are those of o2v_hip_components_dense:
 * the grid is only read, a stride may be 0, BITS needs strides[0] == 1, a NaN is not below the level.  Voxel (x, y, z) of the
 * box is solid by those rules.
 *
 * Records.  The solid voxels are taken in ascending linear index (z * ny + y) * nx + x - the order of numpy.nonzero on a
 * [z, y, x] array.  Record i is four uint32: (origin[0] + x, origin[1] + y, origin[2] + z, argb).  The colour by color_mode:
 *   O2V_HIP_GATHER_COLOR_CONSTANT   the call's argb;
 *   O2V_HIP_GATHER_COLOR_GRID       colors[x * color_strides[0] + y * color_strides[1] + z * color_strides[2]]: a uint32 grid in
 *                                   device memory, strides in elements (what o2v_hip_write_dense ARGB32 writes); only read, a
 *                                   stride may be 0;
 *   O2V_HIP_GATHER_COLOR_PALETTE    (format U8 only) palette[v], v the voxel's byte, palette uint32[256] in HOST memory, copied
 *                                   by the call.
 *
 * o2v_hip_gather_count is the only pass over the grid.  It keeps the set's bits and the offsets of the records in scratch of the
 * context and returns the number of solid voxels - a uint64: the count has no 32-bit limit.
 *
 * o2v_hip_gather_write fills records [first, first + n) of that numbering into `records` ([n][4] uint32, device memory, 16-byte
 * aligned), contiguously; it may be repeated with any ranges in any order, so that no caller needs memory for all 16 bytes per
 * voxel at once.  n = 0 launches nothing and reads no pointer.  It must follow an o2v_hip_gather_count with the same grid
 * pointer, format, strides, dims and level (else O2V_HIP_ERR_BAD_ARGUMENT, "no matching o2v_hip_gather_count"; another count
 * or save, refused or not, replaces the last one).  Occupancy comes from the kept bits only: a grid that changes between the two
 * calls changes no coordinate and nothing is written outside `records`; with PALETTE the byte read then may give another colour
 * (with GRID the colours are read at the time of the write), and that is all.
 *
 * o2v_hip_gather_save is the count, then ranges of 2^20 records written to two device buffers of 16 MiB and copied into two
 * page-locked host buffers while the sink consumes the batch before - into the file sink of obj2voxel_voxelize() for `path`,
 * the format from `type` (an extension without dot) or, if type is NULL, from the path's extension; `resolution` is the grid
 * resolution the paletted formats record.  The file holds exactly what obj2voxel_voxelize() would have written for those
 * records in that order.  *out_count: the voxels written.  O2V_HIP_ERR_IO: the path cannot be opened, the type is not an output
 * format (VL32, PLY, XYZRGB, QEF, VOX), or the sink stopped accepting voxels; the message is in o2v_hip_last_error.
 *
 * Refused before any launch, records and file untouched: null arguments - except colors, color_strides and palette where the
 * mode does not read them, and those and records where n = 0 -, zero dims, an unknown format or colour mode, PALETTE with a
 * format other than U8, BITS with strides[0] != 1, a level that is not finite (F32_BELOW only), first + n above the counted
 * total, records not 16-byte aligned or overlapping the grid or colors, a pointer that is not device memory of the context's
 * device with its whole extent inside its allocation, for save origin[a] + dims[a] > resolution (O2V_HIP_ERR_BAD_ARGUMENT); a dim
 * above 65 536, origin[a] + dims[a] above 2^32, more than 2^31 - 1 words = ceil(nx / 64) * ny * nz (O2V_HIP_ERR_LIMIT).  A failed
 * scratch or staging allocation returns O2V_HIP_ERR_OUT_OF_MEMORY and leaves the context usable.  All calls run on the context's
 * stream and return when their results have landed (the caller must have finished writing the grid and the colours).
 *
 * Scratch of the context, grown on demand (o2v_hip_gather_scratch_bytes; 0 for zero dims): 12 * words + 8 * (ceil(words / 256)
 * + 1) + 1032 - a 64-bit word per 64 voxels along x, a 32-bit prefix per word, a 64-bit offset per block of 256 words and the
 * count, the palette and the block of a range's first record.  o2v_hip_gather_save adds 2 x 16 MiB of device and 2 x 16 MiB of
 * page-locked host memory, kept by the context. */
enum { O2V_HIP_GATHER_COLOR_CONSTANT = 0, O2V_HIP_GATHER_COLOR_GRID = 1, O2V_HIP_GATHER_COLOR_PALETTE = 2 };
int o2v_hip_gather_count(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                         uint64_t *out_count);
int o2v_hip_gather_write(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                         const uint32_t origin[3], uint32_t color_mode, uint32_t argb, const uint32_t *colors, const uint64_t color_strides[3],
                         const uint32_t *palette /* [256], host */, uint64_t first, uint64_t n, uint32_t *records /* [n][4], device */);
int o2v_hip_gather_save(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                        const uint32_t origin[3], uint32_t color_mode, uint32_t argb, const uint32_t *colors, const uint64_t color_strides[3],
                        const uint32_t *palette /* [256], host */, const char *path, const char *type, uint32_t resolution, uint64_t *out_count);
uint64_t o2v_hip_gather_scratch_bytes(const uint32_t dims[3]);
/* The device times (ms) of the last count's classify and count + scan stages and of the last write (0 after a count; after a
 * save: of its last batch). */
int o2v_hip_gather_times(const o2v_hip_ctx *ctx, float out_ms[3]);

/* ---- dense grids as blocky meshes: exposed voxel faces as coloured quads -----------------------------
 *
 * The mesh of a voxel model: one quad per exposed voxel face, coloured by its voxel, faces of equal colour merged into runs;
 * defined so that a numpy restatement (tests/faces_ref.py) reproduces every bit.
 *
 * The set.  grid, format, strides, dims and level are exactly those of o2v_hip_gather_count: the grid is only read, a stride
 * may be 0, BITS needs strides[0] == 1, a NaN is not below the level.  Everything outside the box is empty.
 *
 * Colour of a voxel.  color_mode, argb, colors, color_strides and palette are those of o2v_hip_gather_write
 * (O2V_HIP_GATHER_COLOR_CONSTANT / _GRID / _PALETTE), with the same meaning.
 *
 * Faces.  Direction d = 0 .. 5 is -x, +x, -y, +y, -z, +z.  Face (x, y, z, d) is exposed if voxel (x, y, z) is solid and its
 * neighbour in direction d is not.
 *
 * Merging.  O2V_HIP_FACES_MERGE_NONE: one quad per exposed face.  O2V_HIP_FACES_MERGE_RUNS: one quad per maximal run.
 * Directions 2 .. 5 run along x, directions 0 and 1 along y.  Two exposed faces of one direction belong to one run if they are
 * neighbours along that axis and their voxels' colours are equal as uint32 (colours, not labels: two palette entries with the
 * same word merge; with CONSTANT every pair is equal).  A run is cut nowhere else: not at a multiple of 64 and not at any
 * boundary of the implementation.
 *
 * Order.  Quads ascend by the key ((z * ny + y) * 6 + d) * nx + x of the run's first face - the one of the lowest x, or of the
 * lowest y for d < 2: row by row, direction by direction within a row, then x.
 *
 * Geometry.  Vertices are not shared: quad q owns vertices 4q .. 4q + 3 and triangles 2q, 2q + 1 = (4q, 4q + 1, 4q + 2),
 * (4q, 4q + 2, 4q + 3).  With axis a = d >> 1, side s = d & 1 and (u, v) the two axes after a in cyclic order (x -> (y, z),
 * y -> (z, x), z -> (x, y)) the quad lies in the plane a = origin[a] + voxel[a] + s and spans [u0, u1] x [v0, v1], the lattice
 * bounds of its faces (origin included); its corners in order are (u0, v0), (u1, v0), (u1, v1), (u0, v1) for s = 1 and
 * (u0, v0), (u0, v1), (u1, v1), (u1, v0) for s = 0, so that both triangles' normals point out of the solid voxel.  Coordinates
 * are (float) of integers at most 65 536: exact.
 *
 * o2v_hip_faces_count is the only pass over the grid, and with GRID or PALETTE and MERGE_RUNS the only pass that compares
 * colours: it keeps the solid bits, and for those a bit per voxel each for "the colour of the voxel at x - 1" and "... at
 * y - 1", in scratch of the context, and returns the number of quads Q - a uint64: no 32-bit limit.  With MERGE_NONE and
 * CONSTANT it is the model's surface area in voxel faces.
 *
 * o2v_hip_faces_write fills all Q quads: positions ([4Q][3] float32, 16-byte aligned), faces ([2Q][3] int32, 8-byte aligned,
 * may be NULL) and quad_argb ([Q] uint32, may be NULL), device memory with room for quad_capacity >= Q quads.  It must follow an
 * o2v_hip_faces_count with the same grid pointer, format, strides, dims, level, merge and colour arguments (argb for CONSTANT,
 * colors and color_strides for GRID, the palette's 256 words for PALETTE), else O2V_HIP_ERR_BAD_ARGUMENT, "no matching
 * o2v_hip_faces_count"; another count, refused or not, replaces the last one.  Q = 0 launches nothing and reads no output
 * pointer.  The topology comes from the kept bits only; a quad's colour is read at the time of the write from the run's first
 * voxel.  A grid or colour grid that changes between the two calls can give other colours - no other coordinate and no write
 * outside the arrays.
 *
 * Refused before any launch, outputs untouched: what o2v_hip_gather_count and the colour arguments of o2v_hip_gather_write are
 * refused for, an unknown merge, quad_capacity below Q, misaligned outputs, outputs that overlap each other, the grid or colors
 * or are not device memory of the context's device with their whole extent inside one allocation (O2V_HIP_ERR_BAD_ARGUMENT); a
 * dim above 65 536, more than 2^31 - 1 words, for write origin[a] + dims[a] above 65 536 - beyond it a coordinate is no longer
 * exact in float32 - and 4 Q above 2^31 - 1, the message naming Q (O2V_HIP_ERR_LIMIT).  A failed scratch allocation returns
 * O2V_HIP_ERR_OUT_OF_MEMORY and leaves the context usable.  Both calls run on the context's stream and return when their
 * results have landed.
 *
 * Scratch of the context, grown on demand (o2v_hip_faces_scratch_bytes, an upper bound; 0 for zero dims): 8 * words - 24 *
 * words with GRID or PALETTE, of which MERGE_NONE uses 8 - + 8 * (ceil(6 * words / 256) + 1) + 1024: a 64-bit word per 64
 * voxels along x for the set and the two comparisons, a 64-bit offset per block of 256 (row, direction, word) items and the
 * count, the palette.
 *
 * Rectangles.  O2V_HIP_FACES_MERGE_RECTS = 3: one quad per maximal chain of equal runs.  The merge value
 * is read as flags, bit 0 "runs" and bit 1 "stack the runs"; 2 alone - stacking without runs - means nothing and stays refused
 * ("unknown merge 2").  The set, the colours, the exposed faces, the runs, the order key, the corner order and every refusal are
 * those above.
 *   The stack axis of direction d is y for d = 4, 5 (the -z / +z faces, runs along x) and z for d = 0 .. 3 (-y / +y, runs along
 * x; -x / +x, runs along y).  The row before a run's row is the one at y - 1 for d = 4, 5 and at z - 1 otherwise, the other
 * coordinates and the plane the same.
 *   Two runs of one direction in neighbouring rows are equal if they begin at the same coordinate along the run axis, have the
 * same length and their voxels have the same colour as uint32 (a run has one colour, so the first voxels decide; colours, not
 * labels, and with CONSTANT every pair is equal).
 *   A rectangle is a maximal chain of equal runs in consecutive rows, emitted as one quad over the lattice bounds of all its
 * faces.  Its key is that of the chain's first run - the lowest row -, ((z * ny + y) * 6 + d) * nx + x of its lowest face; its
 * colour is read at the time of the write at that run's first voxel; its corners are (u0, v0), (u1, v0), (u1, v1), (u0, v1) or
 * the mirrored order by the rule above, on the larger bounds.
 *   This is not the sequential greedy mesher, which depends on its scan order and cannot run in parallel: a rectangle never
 * joins runs of different extent, so an L-shaped wall keeps a quad per row of its narrow part.  The rule is a function of the set
 * and the colours alone, so two calls agree bit for bit and a numpy restatement (tests/rects_ref.py) reproduces it.
 * Rectangles, like runs, leave T-junctions.  Nothing is cut at a word, a block of items, the row y = ny - 1 or any other
 * boundary of the implementation, and nothing is joined across one: row (y = 0, z + 1) is not the row after (y = ny - 1, z).
 *   The limits, the alignment of the outputs, "no matching o2v_hip_faces_count" (the merge value is part of what must match)
 * and quad_capacity hold as above.
 *   Scratch: o2v_hip_faces_scratch_bytes keeps its values and is the bound of MERGE_NONE and MERGE_RUNS;
 * o2v_hip_faces_scratch_bytes_merge(dims, color_mode, merge) returns it for those, and for MERGE_RECTS
 *     o2v_hip_faces_scratch_bytes(dims, color_mode) + 48 * words + (8 * words with GRID or PALETTE):
 * the kept rectangle-start masks, a 64-bit word per (row, direction, word) item, and a bit per voxel for "the colour of the
 * voxel at z - 1".  These arrays belong to MERGE_RECTS alone: a count with another merge mode between a MERGE_RECTS count and
 * its write replaces the count (the write is then refused), but no other call of the context touches them. */
enum { O2V_HIP_FACES_MERGE_NONE = 0, O2V_HIP_FACES_MERGE_RUNS = 1, O2V_HIP_FACES_MERGE_RECTS = 3 };
int o2v_hip_faces_count(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                        uint32_t merge, uint32_t color_mode, uint32_t argb, const uint32_t *colors, const uint64_t color_strides[3],
                        const uint32_t *palette /* [256], host */, uint64_t *out_quads);
int o2v_hip_faces_write(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                        uint32_t merge, uint32_t color_mode, uint32_t argb, const uint32_t *colors, const uint64_t color_strides[3],
                        const uint32_t *palette /* [256], host */, const uint32_t origin[3], float *positions /* [4Q][3], device */,
                        int32_t *faces /* [2Q][3], device, may be NULL */, uint32_t *quad_argb /* [Q], device, may be NULL */,
                        uint64_t quad_capacity);
uint64_t o2v_hip_faces_scratch_bytes(const uint32_t dims[3], uint32_t color_mode);
uint64_t o2v_hip_faces_scratch_bytes_merge(const uint32_t dims[3], uint32_t color_mode, uint32_t merge);
/* The device times (ms) of the last count's classify (+ colour comparison) and count + scan stages and of the last write (0
 * after a count). */
int o2v_hip_faces_times(const o2v_hip_ctx *ctx, float out_ms[3]);

/* ---- nearest-voxel transform -------------------------------------------------------------------
 *
 * For every voxel of a box, which voxel of a seed set is closest to it, and optionally that seed's value: the feature
 * transform that goes with o2v_hip_distance_dense.
 *
 * The seeds.  dims = (nx, ny, nz).  grid, format, strides, dims and level are those of o2v_hip_components_dense: a voxel is a
 * seed where a O2V_HIP_GRID_U8 element is non-zero, where its O2V_HIP_GRID_BITS bit is set, where a O2V_HIP_GRID_F32_BELOW
 * element is < level (finite).  With O2V_HIP_NEAREST_SEED_ONE in flags (U8 only) a seed is an element that is exactly 1: the
 * rule of o2v_hip_distance_dense for label grids (1 surface, 2 interior).  S is the set of seeds; grid is only read.
 *
 * For every voxel v of the box:
 *   d2(v)      = min over s in S of |v - s|^2, an exact integer, as o2v_hip_distance_dense defines it;
 *   nearest(v) = the linear index (sz * ny + sy) * nx + sx of the seed that attains d2(v); among several at that distance the
 *                one with the smallest linear index - the lexicographically smallest (z, y, x).  A seed is its own nearest.
 *                -1 everywhere when S is empty.
 *
 * Outputs, device memory, strides in elements per axis x, y, z, any order; none may map two voxels to one element:
 *   nearest  int32, required; every voxel of the box is written (the passes use it as their working buffer).
 *   dist2    int32, may be NULL: d2(v), or 0x7FFFFFFF without seeds - bit for bit what o2v_hip_distance_dense DIST_SQ_I32 gives
 *            for the same seed set.
 *   values   int32, may be NULL, updated in place: for every voxel v that is not a seed, has nearest(v) >= 0 and
 *            d2(v) <= max_dist2, values(v) = values(nearest(v)).  With O2V_HIP_NEAREST_VALUES_INSIDE (U8 only) also only
 *            where the grid's element at v is non-zero - with SEED_ONE the interior voxels (2) of a label grid and nothing
 *            else.  Every other element keeps its bits.  Seeds are only read and the others only written, so the update has
 *            no race and one run equals another bit for bit.  max_dist2 = 0x7FFFFFFF (or more): no limit.  It limits values
 *            only: nearest and dist2 are always complete.
 *
 * Refused before anything is launched, the outputs untouched.  O2V_HIP_ERR_LIMIT: nx * ny * nz above 2^31 - 1 (an index is one
 * int32), (nx-1)^2 + (ny-1)^2 + (nz-1)^2 above 2^31 - 2 (o2v_hip_distance_dense's limit; with it an axis has at most 46 341
 * voxels) - both before the pointers are looked at.  O2V_HIP_ERR_BAD_ARGUMENT: zero dims, a null argument, an unknown format or
 * flag, a level that is not finite, a BITS grid with strides[0] != 1, a flag on a grid that is not U8, output strides that map
 * two voxels to one element, any two of grid, nearest, dist2 and values overlapping, a pointer that is not device memory of the
 * context's device with the box's highest address inside its allocation.
 *
 * The envelope stacks are the context's scratch of o2v_hip_distance_dense, o2v_hip_nearest_scratch_bytes(dims) =
 * o2v_hip_distance_scratch_bytes(dims, ...) bytes, grown on demand; if it cannot be allocated the call returns
 * O2V_HIP_ERR_OUT_OF_MEMORY and the context stays usable.  The call runs on the context's stream and returns when the writes
 * have landed (the caller must have finished writing grid and values). */
enum { O2V_HIP_NEAREST_SEED_ONE = 1u, O2V_HIP_NEAREST_VALUES_INSIDE = 2u };
int o2v_hip_nearest_dense(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                          uint32_t flags, int32_t *nearest, const uint64_t nearest_strides[3], int32_t *dist2 /* may be NULL */,
                          const uint64_t dist2_strides[3], int32_t *values /* may be NULL */, const uint64_t value_strides[3],
                          uint32_t max_dist2);
uint64_t o2v_hip_nearest_scratch_bytes(const uint32_t dims[3]);
/* The device times of the last o2v_hip_nearest_dense call's three passes (x, y, z), from events around each, in ms. */
int o2v_hip_nearest_times(const o2v_hip_ctx *ctx, float out_ms[3]);

/* ---- downsampling: a dense grid merged into a coarser one ------------------------------------------
 *
 * Blocks of f x f x f fine voxels become one coarse voxel each: its coverage count, its occupancy by a threshold on that count,
 * the smallest or largest label of the block and the mean colour of the block's solid voxels.  Supersampling is this operation
 * behind a voxelization at f times the resolution.
 *
 * The set.  grid, format (O2V_HIP_GRID_U8 / _BITS / _F32_BELOW), strides, dims = (nx, ny, nz) and level are those of
 * o2v_hip_components_dense: a fine voxel is solid where a U8 element is non-zero, where its BITS bit is set (strides[0] == 1),
 * where an F32_BELOW element is < level (finite; a NaN is not below it).  A stride may be 0.  grid is only read.
 * origin[3] holds the global fine-lattice coordinates of the box's voxel (0, 0, 0).  factor f is 2 ... 8.
 *
 * The coarse box.  Per axis a: corigin[a] = floor(origin[a] / f), cdims[a] = ceil((origin[a] + dims[a]) / f) - corigin[a];
 * o2v_hip_downsample_box computes both (O2V_HIP_ERR_BAD_ARGUMENT for a null argument, zero dims or a factor outside 2 ... 8,
 * O2V_HIP_ERR_LIMIT for origin + dims above 2^32).  Coarse voxel X = (X0, X1, X2) of the coarse box covers the fine voxels with
 * global coordinates in [(corigin[a] + Xa) f, (corigin[a] + Xa + 1) f) on each axis: blocks are aligned to the global lattice,
 * not to the box, and the fine voxels of a block that lie outside the box count as empty.  So the downsampled box of a
 * voxelization at 2R lines up with the voxelization at R with supersampling 2.
 *
 *   c(X) = the number of solid fine voxels of the block of X, 0 ... f^3 <= 512.
 *
 * Outputs over the coarse box, device memory, strides in elements per axis x, y, z, any order; none may map two coarse voxels
 * to one element; each may be NULL, but not all of them; every element of every given output is written:
 *   count   int16: c(X).
 *   solid   uint8: 1 if c(X) >= min_count, else 0.  min_count is 1 ... f^3: 1 is "any", f^3 "all", ceil(f^3 / 2) "majority".
 *   values  uint8, U8 grids only: where solid(X) the smallest (value_mode O2V_HIP_DOWN_VALUE_MIN) or largest (_MAX) non-zero
 *           byte of the block's fine voxels inside the box, else 0.  With label grids (1 surface, 2 interior) MIN gives "surface
 *           if any sub-voxel is surface".  value_mode is looked at only when values is given.
 *   argb    uint32, needs colors: a uint32 grid over the fine box, strides in elements as in o2v_hip_gather_write (a stride may
 *           be 0).  Where solid(X), each of the four 8-bit channels is the mean of that channel over the block's solid fine
 *           voxels, rounded half up: (2 sum + c) / (2 c) in integers, c = c(X); elsewhere 0.  The colours of fine voxels that
 *           are not solid are never used (and not read).  Without argb the memory at colors is not looked at.
 * All sums are integers, so the result does not depend on any order and one run equals another bit for bit.  No scratch.
 *
 * Refused before anything is launched, the outputs untouched.  O2V_HIP_ERR_BAD_ARGUMENT: a null grid, strides, dims or origin, a
 * given output or colors without its strides, zero dims, an unknown format, a BITS grid with strides[0] != 1, a level that is
 * not finite, no output at all, a factor outside 2 ... 8, min_count outside 1 ... f^3, values with a format other than U8 or an
 * unknown value_mode, argb without colors, output strides that map two coarse voxels to one element, an output overlapping the
 * grid, the colours or another output, a pointer that is not device memory of the context's device with its whole reach inside
 * its allocation.  O2V_HIP_ERR_LIMIT: a dim above 65 536, origin[a] + dims[a] above 2^32 - both before the pointers are looked
 * at.  The call runs on the context's stream and returns when the writes have landed (the caller must have finished writing
 * grid and colors). */
enum { O2V_HIP_DOWN_VALUE_MIN = 0, O2V_HIP_DOWN_VALUE_MAX = 1 };
int o2v_hip_downsample_box(const uint32_t origin[3], const uint32_t dims[3], uint32_t factor, uint32_t out_origin[3], uint32_t out_dims[3]);
int o2v_hip_downsample(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                       const uint32_t origin[3], uint32_t factor, uint32_t min_count, uint32_t value_mode,
                       const uint32_t *colors /* may be NULL */, const uint64_t color_strides[3], int16_t *count /* may be NULL */,
                       const uint64_t count_strides[3], uint8_t *solid /* may be NULL */, const uint64_t solid_strides[3],
                       uint8_t *values /* may be NULL */, const uint64_t value_strides[3], uint32_t *argb /* may be NULL */,
                       const uint64_t argb_strides[3]);
/* The device time of the last o2v_hip_downsample call's one launch, from events around it, in ms. */
int o2v_hip_downsample_times(const o2v_hip_ctx *ctx, float out_ms[1]);

/* ---- signed crossing numbers ------------------------------------------------------------------------
 *
 * For each voxel of a box, the signed number of times the context's triangles cross the axis-parallel lines through its centre,
 * counted from both ends of each line: the sum over the axes asked for of (D_a + U_a) below.  It is what a robust inside test
 * votes on (Nooruddin & Turk's ray stabbing with the nonzero rule): an outward-wound closed mesh gives 2 popcount(axes) inside
 * and 0 outside, an inward-wound one the negative, parts pushed into each other add up, and a ray that slips through a hole is
 * one of six.  The mean over all directions is the generalized winding number; the six axis rays are a six-point quadrature.
 * The mesh, params, transform, box, strides and pointer checks are those of o2v_hip_mesh_distance_dense: of params, resolution,
 * supersampling (1 or 2), unit_transform, bounds_known and bounds are read; z_begin .. y_end must be 0.
 *   axes: bit 0 the x rays, bit 1 y, bit 2 z; 1 ... 7.
 *   For a ray axis a, (u, v, w) = (x, y, z) for a = z, (y, z, x) for a = x, (z, x, y) for a = y.  The sample-space vertices are
 *   those of O2V_HIP_FLAG_FILL_INTERIOR (affine_apply, float32; a triangle with a non-finite coordinate contributes nothing), each
 *   read as (u, v, w).  The column test of that flag's definition is applied on (u, v) at the centre P = (i ss + ss/2,
 *   j ss + ss/2) - the same exact signs, the same perturbation, the same degenerate-edge rule.  A triangle whose three signs all
 *   equal sigma (+1 or -1) crosses the line, at that definition's height formula with w in place of z (the same fallback for
 *   den == 0 or a non-finite height); k0 is the first k with k ss + ss/2 > that height.  For the voxel at k on that line the
 *   crossing lies below it if k0 <= k, else above.
 *     D_a = - sum of sigma over the crossings below,   U_a = + sum of sigma over the crossings above,
 *     dst(voxel) = sum over the axes asked for of (D_a + U_a).
 *   Crossings outside the box count: below the box's first layer for every voxel of the line, above its last layer for U of every
 *   voxel.  There is no top-layer cut.  A voxel's value depends only on its centre and the mesh: a box cut into ranges along any
 *   axis gives the bits of one call.  An empty mesh gives 0.
 * Box: origin and dims are output voxels, dims >= 1 and origin + dims <= resolution per axis; voxel (x, y, z) of the box is
 * dst[(x - ox) * dst_strides[0] + (y - oy) * dst_strides[1] + (z - oz) * dst_strides[2]] (int32 elements, any order); every
 * voxel of the box is written.  Refused with O2V_HIP_ERR_BAD_ARGUMENT before any launch, dst untouched: a null argument, axes 0
 * or above 7, resolution 0, supersampling above 2, a slab or tile field of params that is not 0, a zero dim, a box that reaches
 * past the grid, strides that map two voxels to one element, a pointer that is not device memory of the context's device with the
 * box's highest address inside its allocation.  O2V_HIP_ERR_LIMIT: a dim above 65 535; 2 * popcount(axes) * triangles above
 * 2^31 - 1 (a voxel's value is bounded by that product, so no sum can wrap).  Scratch (an int32 delta grid of the box, one int32
 * per line, the enumeration of (triangle, line) pairs) belongs to the context and grows on demand; a failed allocation returns
 * O2V_HIP_ERR_OUT_OF_MEMORY and the context stays usable.  The call runs on the context's stream and returns when the writes
 * have landed. */
int o2v_hip_crossings_dense(o2v_hip_ctx *ctx, const o2v_hip_params *params, uint32_t axes /* bit 0 x, 1 y, 2 z; 1 ... 7 */,
                            const uint32_t origin[3], const uint32_t dims[3], int32_t *dst, const uint64_t dst_strides[3]);
/* The device times (ms) of the last o2v_hip_crossings_dense call per axis x, y, z; 0 for an axis not asked for. */
int o2v_hip_crossings_times(const o2v_hip_ctx *ctx, float out_ms[3]);

/* ---- per-label statistics of a dense grid ---------------------------------------------------------------
 *
 * One read of a label grid gives, per value L = 0 ... n_labels, the number of voxels that hold L, their bounding box, the sums of
 * their coordinates and of the coordinates' products, and their exposed faces: what a crop, a centroid, a covariance, an inertia
 * tensor and a surface area per part are derived from.
 *
 * The grid.  labels is device memory of the context's device, only read; format O2V_HIP_LABELS_I32 (int32 elements: what
 * o2v_hip_components_dense writes) or O2V_HIP_LABELS_U8 (uint8: occupancy, the labels of O2V_HIP_FLAG_FILL_INTERIOR, of a flood);
 * voxel (x, y, z) of the box dims = (nx, ny, nz) is labels[x * strides[0] + y * strides[1] + z * strides[2]] (elements, any order;
 * a stride may be 0).  origin[3] holds the global coordinates of voxel (0, 0, 0): a voxel's coordinates are origin + index.
 * A voxel whose value is negative or above n_labels adds nothing to any row; *out_outside receives how many there are.
 *
 * The table.  int64 [n_labels + 1][O2V_HIP_STATS_COLUMNS], contiguous, device memory; row L is for the value L, and row 0 is
 * treated like every other row.  The call writes every element.  `which` is a set of O2V_HIP_STATS_* bits; the count is always
 * made, and the columns of a group that is not asked for hold 0:
 *    0        the number of voxels.
 *    1 - 3    BOX: the smallest x, y, z;  4 - 6: the largest x, y, z.  Both inclusive, in global coordinates.  A row without
 *             voxels holds min = 2^31 - 1 and max = -1.
 *    7 - 9    SUMS: the sums of x, y, z.
 *    10 - 15  MOMENTS: the sums of xx, yy, zz, xy, xz, yz.
 *    16       FACES: the sum, over the row's voxels, of the voxel's six neighbours whose value differs from its own (the values
 *             as they are, counted or not); a neighbour outside the box differs.  On a 0 / 1 grid table[1][16] is
 *             o2v_hip_faces_count with O2V_HIP_FACES_MERGE_NONE.
 * Coordinates are the integer voxel coordinates; the + 0.5 of the voxel's centre is added by whoever derives a centroid.
 * No overflow: with every coordinate below 2^16 and fewer than 2^31 voxels (the limits below), a product of two coordinates is at
 * most (2^16 - 1)^2 = 2^32 - 131 071, and a sum of at most 2^31 - 1 of them is at most (2^32 - 131 071) (2^31 - 1) < 2^63.
 * Every column is an integer sum, minimum or maximum: the table does not depend on any order, one run equals another bit for bit.
 *
 * Refused before anything is launched, table and *out_outside untouched.  O2V_HIP_ERR_BAD_ARGUMENT: a null argument, zero dims,
 * an unknown format, an unknown bit in which, n_labels above 255 with U8, a table that is not 8-byte aligned or an I32 grid that
 * is not 4-byte aligned, a table that overlaps the grid, a pointer that is not
 * device memory of the context's device with its whole reach inside its allocation.  O2V_HIP_ERR_LIMIT (before the pointers are
 * looked at): a dim above 65 536, origin[a] + dims[a] above 65 536, more than 2^31 - 1 voxels, n_labels above 2^31 - 2.
 * O2V_HIP_ERR_OUT_OF_MEMORY, with the context usable, if the context's scratch (one counter) cannot be allocated.  The call runs on
 * the context's stream and returns when the table is written (the caller must have finished writing labels). */
enum { O2V_HIP_LABELS_I32 = 0, O2V_HIP_LABELS_U8 = 1 };
enum { O2V_HIP_STATS_BOX = 1, O2V_HIP_STATS_SUMS = 2, O2V_HIP_STATS_MOMENTS = 4, O2V_HIP_STATS_FACES = 8 };
enum { O2V_HIP_STATS_COLUMNS = 17 };
int o2v_hip_label_stats(o2v_hip_ctx *ctx, const void *labels, uint32_t format, const uint64_t strides[3], const uint32_t dims[3],
                        const uint32_t origin[3], uint32_t n_labels, uint32_t which, int64_t *table, uint64_t *out_outside);
/* The device times (ms) of the last o2v_hip_label_stats call, from events around them: [0] the table's initialisation, [1] the
 * pass over the grid. */
int o2v_hip_label_stats_times(const o2v_hip_ctx *ctx, float out_ms[2]);

/* ---- geodesic distances and shortest paths through a dense grid -----------------------------------------
 *
 * How far it is from A to B without leaving the set: single- or multi-source shortest path lengths on the voxel adjacency graph
 * of a set, with small integer edge weights, and the walk back along them; defined so that a numpy restatement reproduces every bit.
 *
 * The set.  grid, format, strides, dims and level are those of o2v_hip_components_dense: the grid is only read, a stride may be 0,
 * BITS needs strides[0] == 1, a NaN is not below the level.  S is the solid voxels of the box, or with O2V_HIP_CC_INVERT the
 * voxels of the box that are not solid.
 * The steps.  weights[3] (uint32, each 0 ... 65 535 = O2V_HIP_GEO_MAX_WEIGHT, not all 0) are the costs of a step to a neighbour
 * that differs by at most 1 on every axis and on exactly 1, 2 or 3 axes (face, edge, corner); a weight of 0 means that kind of
 * step does not exist.  (1, 0, 0) counts hops at connectivity 6, (1, 1, 0) at 18, (1, 1, 1) at 26; (3, 4, 5) is the chamfer
 * metric, whose thirds approximate Euclidean length.  A diagonal step needs only its two end voxels in S (the adjacency of
 * o2v_hip_components_dense).  Nothing outside the box is adjacent to anything.
 * The seeds.  int32 [n_seeds][3], local (x, y, z), in device memory; a seed outside the box or not in S is ignored; with
 * n_seeds = 0 the pointer is not read.  O2V_HIP_CC_SEED_BORDER additionally seeds every voxel of S on the six faces of the box.
 * The distance.  d(v) is the smallest sum of weights over all paths inside S from any seed to v; 0 at a seed.  max_distance
 * (uint32, at most 2^31 - 2 = O2V_HIP_GEO_MAX_DISTANCE; pass that for "no cap"): a voxel whose d is above it counts as not
 * reached, and nothing is propagated through it - which changes no other voxel's d, every weight being positive.  With d at most
 * 2^31 - 2 (2^31 - 1 while a voxel is not reached) and a weight at most 65 535, every d + w of the relaxation fits a uint32.
 * d is the least fixed point of a monotone integer relaxation: unique, the same bits on every run and under every schedule.
 *
 * o2v_hip_geodesic_dense writes dist(x, y, z) = dist[x * dist_strides[0] + y * dist_strides[1] + z * dist_strides[2]] (int32,
 * strides in elements, no two voxels on one element) for every voxel of the box: d(v) where v is reached, -1 everywhere else -
 * outside S, and in S but not reached.  *out_reached is the number of voxels with dist >= 0.
 * flags: O2V_HIP_CC_INVERT, O2V_HIP_CC_SEED_BORDER, O2V_HIP_FLAG_STAGE_TIMES (o2v_hip_geodesic_counters counts).
 *
 * o2v_hip_geodesic_paths walks back through a grid that o2v_hip_geodesic_dense wrote (dist >= 0 says "in S and reached": it takes
 * no set grid).  targets: int32 [n_targets][3]; paths: int32 [n_targets][max_len][3]; lengths: int32 [n_targets]; all contiguous
 * device memory.  For target i: outside the box, or dist < 0 there: lengths[i] = -1.  Otherwise the path starts at the target and
 * goes, until dist = 0, from v to the first neighbour u in the box with dist[u] >= 0 and dist[u] + w(u, v) == dist[v], the
 * neighbours taken in ascending (dz, dy, dx) order of their offsets and only the step kinds with a weight tried.  lengths[i] is
 * the number of voxels of the whole path, both ends included; the first min(lengths[i], max_len) of them are written,
 * paths[i][k] = (x, y, z), the rest of the row is left alone.  If no such neighbour exists, the grid was not made with these
 * weights: lengths[i] = -2 and the walk ends (what it had written of the row stays).  Every walk ends: dist strictly decreases.
 *
 * Refused before any launch, the outputs untouched.  O2V_HIP_ERR_BAD_ARGUMENT: null arguments, zero dims, an unknown format,
 * unknown flag bits, BITS with strides[0] != 1, a level that is not finite (F32_BELOW only), a weight above 65 535 or all three 0,
 * max_distance above 2^31 - 2, a dist that is not 4-byte aligned, an output overlapping an input or another output, dist strides
 * that map two voxels to one element (o2v_hip_geodesic_dense; the paths call only reads dist), a pointer that is not device memory
 * of the context's device with its whole extent inside its allocation.  O2V_HIP_ERR_LIMIT: a dim above 65 536, nx * ny * nz,
 * n_seeds or n_targets above 2^31 - 1.  A failed scratch allocation returns O2V_HIP_ERR_OUT_OF_MEMORY and the context stays
 * usable.  After a later error the outputs are unspecified.  Both calls run on the context's stream and return when their results
 * have landed (the caller must have finished writing their inputs).
 *
 * Scratch of the context, grown on demand, with words = ceil(nx / 64) * ny * nz, tiles = ceil(nx / 64) * ceil(ny / 8) *
 * ceil(nz / 8) and voxels = nx * ny * nz:
 *   O2V_HIP_GEO_SCRATCH_CONTIGUOUS  8 * words + 16 * tiles + 64: the set's bits, per tile two flag words and two list places,
 *                                   counters.  No per-voxel scratch: the distances live in dist.  This holds where dist is
 *                                   contiguous (strides 1, nx, nx * ny);
 *   O2V_HIP_GEO_SCRATCH_STRIDED     ... + 4 * voxels: a dist of any other strides, the distances in the context.
 * (0 for zero dims or an unknown `which`.)  o2v_hip_geodesic_paths takes none.
 * O2V_GEO_NO_TILES=1 in the environment (A/B): no tile pass, whole-grid sweeps until one changes nothing; same results. */
enum { O2V_HIP_GEO_MAX_WEIGHT = 65535u, O2V_HIP_GEO_MAX_DISTANCE = 0x7ffffffeu };
enum { O2V_HIP_GEO_SCRATCH_CONTIGUOUS = 0, O2V_HIP_GEO_SCRATCH_STRIDED = 1 };
int o2v_hip_geodesic_dense(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                           const uint32_t weights[3], uint32_t flags, const int32_t *seeds /* [n_seeds][3] */, uint64_t n_seeds,
                           uint32_t max_distance, int32_t *dist, const uint64_t dist_strides[3], uint64_t *out_reached);
int o2v_hip_geodesic_paths(o2v_hip_ctx *ctx, const int32_t *dist, const uint64_t dist_strides[3], const uint32_t dims[3], const uint32_t weights[3],
                           const int32_t *targets /* [n_targets][3] */, uint64_t n_targets, uint32_t max_len, int32_t *paths, int32_t *lengths);
uint64_t o2v_hip_geodesic_scratch_bytes(const uint32_t dims[3], uint32_t which);
/* The device times (ms) of the last o2v_hip_geodesic_dense call: classify, initialisation + seeds, propagation (the host's reads
 * between the rounds included), write. */
int o2v_hip_geodesic_times(const o2v_hip_ctx *ctx, float out_ms[4]);
/* Of the last o2v_hip_geodesic_dense call made with O2V_HIP_FLAG_STAGE_TIMES (else zeros): the rounds (launches of the
 * propagation), the tile visits over all rounds, the sweeps inside the tiles over all visits, and the host's 4-byte reads during
 * the propagation.  With O2V_GEO_NO_TILES=1: the whole-grid sweeps, 0, 0, the reads. */
int o2v_hip_geodesic_counters(const o2v_hip_ctx *ctx, uint64_t out4[4]);

/* ---- local thickness and ball morphology of a dense grid ---------------------------------------------------
 *
 * How thick is the model here, and where is it thinner than t: for every voxel of a set the largest inscribed ball that holds it,
 * and the opening, erosion, dilation and closing by a ball that fall out of the same passes.  Exact integers (squared radii),
 * the same bits on every run, defined so that a numpy restatement reproduces every bit.
 *
 * The set.  grid, format, strides, dims and level are those of o2v_hip_components_dense (U8, BITS, F32_BELOW with a level); the
 * grid is only read.  S is the solid voxels of the box, or with O2V_HIP_THICK_BACKGROUND the voxels of the box that are not solid.
 * cap = max_radius2, 1 <= cap <= 2^14 = O2V_HIP_THICK_MAX_RADIUS2.
 *
 *   depth2(p)  for p in S: the smallest |p - e|^2 over the voxels e of the box that are not in S.  With O2V_HIP_THICK_BORDER the
 *              voxels outside the box count as not in S: a pointwise min with (x+1)^2, (nx-x)^2, (y+1)^2, (ny-y)^2, (z+1)^2,
 *              (nz-z)^2 (the nearest outside voxel lies along an axis).  0x7FFFFFFF where there is no such voxel; 0 for p not in S.
 *   R(c)       = min(depth2(c), cap).
 *   T(p)       = max { R(c) : c in S, |p - c|^2 < R(c) } for p in S; 0 otherwise.  So 1 <= T <= cap on S, and T(p) == cap exactly
 *              when p lies in the opening of S by the ball {q : |q|^2 < cap}: a value at the cap means "at least".  Without BORDER
 *              the balls are clipped to the box.
 *
 * Outputs, device memory, strides in elements per axis x, y, z, any order; neither may map two voxels to one element:
 *   dst     int32 T.  With O2V_HIP_THICK_F32: float32 (float) (2.0 * sqrt((double) T) - 1.0), 0 outside S - the diameter in voxels
 *           of the largest inscribed ball, bit-identical to the same expression in numpy float64 -> float32.  A wall w voxels
 *           wide reads w for odd w and w - 1 for even w: the centre of a digital ball is a voxel, so its diameter is odd.
 *           With O2V_HIP_THICK_OPEN_ONLY the ball stage is skipped: dst is cap inside the opening and R(p) elsewhere in S, a lower
 *           bound of T that costs two distance transforms.
 *   depth2  int32, may be NULL: the values above (with BORDER: after the min).
 *
 * Stages: depth2 (an x pass and o2v_hip_distance_dense's two envelope passes); the core {depth2 >= cap} and the squared distance to
 * it (the same three passes), which gives the opening; the ball centres - the voxels of S with depth2 < cap, less those whose ball
 * a 26-neighbour's ball covers (o2v_hip_thickness_cover_table) - counted and listed in ascending linear index; an atomic max of
 * R(c) over the ball of every listed centre; the float conversion.  The ball stage writes about half the local thickness squared
 * per voxel of the regions thinner than the cap: that is why the cap is mandatory and bounded.
 * flags: O2V_HIP_THICK_BACKGROUND, _BORDER, _F32, _OPEN_ONLY, O2V_HIP_FLAG_STAGE_TIMES (o2v_hip_thickness_counters counts the ball voxels).
 *
 * Refused before any launch, the outputs untouched, in this order: null arguments; the set grid's checks (zero dims, an unknown
 * format, BITS with strides[0] != 1, a level that is not finite, a grid that is not device memory of the context's device inside
 * one allocation); unknown flag bits; max_radius2 of 0 (O2V_HIP_ERR_BAD_ARGUMENT) or above 2^14 (O2V_HIP_ERR_LIMIT); nx * ny * nz
 * above 2^31 - 1 (O2V_HIP_ERR_LIMIT: a centre is one int32 index); (nx-1)^2 + (ny-1)^2 + (nz-1)^2 above 2^31 - 2
 * (o2v_hip_distance_dense's limit); dst or depth2 strides that map two voxels to one element, or memory that is not the device's;
 * any two of grid, dst and depth2 overlapping.  A failed scratch allocation returns O2V_HIP_ERR_OUT_OF_MEMORY and the context stays
 * usable; after such an error the outputs are unspecified.  The call runs on the context's stream and returns when the writes have
 * landed (the caller must have finished writing grid).
 *
 * Scratch of the context, grown on demand: o2v_hip_thickness_scratch_bytes(dims, max_radius2, have_depth2) =
 *   4 * nx * ny * nz if have_depth2 is 0 (the depth grid)  +  o2v_hip_distance_scratch_bytes(dims, ...) (the envelope stacks, shared
 *   with o2v_hip_distance_dense)  +  8 * (ceil(nx * ny * nz / 256) + 1) (block offsets)  +  12 * (max_radius2 + 1) (the cover table)
 *   +  64; on top of that 4 bytes per kept centre, known only once they are counted.  (0 for zero dims or a cap out of range.) */
enum { O2V_HIP_THICK_BACKGROUND = 16u, O2V_HIP_THICK_BORDER = 32u, O2V_HIP_THICK_F32 = 64u, O2V_HIP_THICK_OPEN_ONLY = 128u };
enum { O2V_HIP_THICK_MAX_RADIUS2 = 1u << 14 };
int o2v_hip_thickness_dense(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                            uint32_t flags, uint32_t max_radius2, void *dst, const uint64_t dst_strides[3], int32_t *depth2 /* may be NULL */,
                            const uint64_t depth2_strides[3]);
uint64_t o2v_hip_thickness_scratch_bytes(const uint32_t dims[3], uint32_t max_radius2, int have_depth2);
/* The device times (ms) of the last o2v_hip_thickness_dense call: depth, opening, initialisation + list (the host's read of the
 * count included), balls, conversion. */
int o2v_hip_thickness_times(const o2v_hip_ctx *ctx, float out_ms[5]);
/* Of the last o2v_hip_thickness_dense call: the candidate centres (the voxels of S with depth2 < cap), the centres kept, and the
 * ball voxels visited - the last only with O2V_HIP_FLAG_STAGE_TIMES, else 0.  With OPEN_ONLY all three are 0. */
int o2v_hip_thickness_counters(const o2v_hip_ctx *ctx, uint64_t out3[3]);
/* The cover table of max_radius2 (1 ... 2^14), on the host; needs no context and no device: out[(k - 1) * (max_radius2 + 1) + R] =
 * L_k[R] = 1 + max { |q - v|^2 : q in Z^3, |q|^2 < R } for v = (1, 0, 0), (1, 1, 0), (1, 1, 1) (k = |v|^2) and R = 1 ... max_radius2 -
 * the smallest radius^2 at which the discrete ball of a neighbour at offset v contains the ball of radius^2 R; L_k[0] = 0.
 * L_k[R] > R.  O2V_HIP_ERR_BAD_ARGUMENT for a null out or a max_radius2 out of range. */
int o2v_hip_thickness_cover_table(uint32_t max_radius2, uint32_t *out /* [3][max_radius2 + 1] */);

/* ---- skeletons of a dense grid: topological thinning -------------------------------------------------------
 *
 * Reduces a set to its skeleton - the one-voxel-wide centrelines of a solid, or of its pore and channel space - by removing
 * simple voxels from its border until none is left.  The numbers of object components, of cavities and of tunnels never change.
 *
 * The definition.  S is the set of a set grid, as in o2v_hip_components_dense: U8 non-zero, BITS, or F32_BELOW with a level.
 * O2V_HIP_CC_INVERT takes the complement inside the box.  Voxels outside the box are background.  Objects are 26-connected.  The
 * background is 6-connected.
 *   Neighbourhood mask of a voxel: bit k = 9 (dz + 1) + 3 (dy + 1) + (dx + 1) is set where the neighbour is in S.  k runs 0 ... 26
 *   without 13.  This is o2v_hip_geodesic_dense's offset order.
 *   C26(m) is the number of 26-connected components of the set bits of m.
 *   C6(m): take the clear bits of m among the 18 positions that differ from the centre on at most two axes.  Connect them by
 *   6-adjacency within these 18.  Count the components that hold a face neighbour.
 *   Simple: a voxel is simple iff C26 == 1 && C6 == 1.  Of the 2^26 masks, 25 985 144 are simple.
 *   Border: a voxel of S is a border voxel if one of its six face neighbours is background.
 *   Subfield: the subfield of a voxel is s = (x & 1) | (y & 1) << 1 | (z & 1) << 2, in box coordinates.  Two voxels of one subfield
 *   are never 26-neighbours.
 *   One iteration:
 *     1. B := the border voxels of S as it is now.
 *     2. For s = 0 ... 7 in turn, remove from S at once every voxel v that meets all of these in the current S: v is in subfield s;
 *        v is in B; v is not in `keep`; v is simple; in mode CURVE, v has other than exactly one 26-neighbour in S.
 *     3. Iterations repeat until one removes nothing.  That iteration counts.
 *     4. If max_iterations != 0, they also stop once max_iterations have run.
 * Because of the subfields, every sub-step equals some sequential removal of simple voxels.  Every sub-step is also a pure function
 * of the grid, so the result is the same bits on every run and under every schedule.
 *
 * Modes.  O2V_HIP_THIN_ULTIMATE (no end points): a ball becomes one voxel, a torus a closed loop, a hollow shell a closed
 * one-voxel surface.  O2V_HIP_THIN_CURVE: end points stay, so arms stay.
 * Documented limits of the method: the result depends on the parity of the box's origin; the end-point rule keeps spurs at corners
 * (a 9^3 box gives 25 voxels with 8 end points).
 * keep: an optional U8 grid with strides of its own (may be NULL); non-zero means never removed.
 *
 * dst is uint8 with any strides that map no two voxels to one element.  O2V_HIP_THIN_DST_MASK: 1 in the skeleton, 0 elsewhere.
 * O2V_HIP_THIN_DST_DEGREE: 0 outside the skeleton; inside it, 1 + the number of 26-neighbours in the skeleton - so 1 is isolated, 2 an
 * end, 3 a plain curve voxel and 4 or more a junction.  Every voxel of the box is written.  grid may equal dst exactly (same pointer
 * and strides, U8), to thin in place.  Any other overlap of dst with grid or keep is refused (grid and keep are only read).
 * flags: O2V_HIP_CC_INVERT, O2V_HIP_FLAG_STAGE_TIMES (o2v_hip_thin_counters counts).
 *
 * Refused before any launch, the outputs untouched.  O2V_HIP_ERR_BAD_ARGUMENT: null arguments, zero dims, an unknown format, mode,
 * dst_format or flag bit, a level that is not finite (F32_BELOW), BITS with strides[0] != 1, pointers that are not device memory of
 * the context's device or reach outside their allocation, dst strides that map two voxels to one element.  O2V_HIP_ERR_LIMIT: a dim
 * above 65 536, or nx * ny * nz above 2^31 - 1 (o2v_hip_components_dense's limits, whose classification is reused).  A failed
 * scratch allocation returns O2V_HIP_ERR_OUT_OF_MEMORY and the context stays usable.  The call runs on the context's stream and
 * returns when the writes are done (the caller must have finished writing grid and keep).  Nine launches per iteration - the
 * border, then the eight subfields, tile by tile (64 x 8 x 8 voxels; a tile runs only while a voxel in its view was removed during
 * this iteration or the last) - and one 8-byte read by the host.
 *
 * Scratch of the context, grown on demand: o2v_hip_thin_scratch_bytes(dims, have_keep) = (16, with keep 24) * ceil(nx / 64) * ny * nz
 * (the bits of the set, of its border and of keep)  +  8 * the tiles (two stamps each)  +  64.  (0 for zero dims.) */
enum { O2V_HIP_THIN_ULTIMATE = 0, O2V_HIP_THIN_CURVE = 1 };
enum { O2V_HIP_THIN_DST_MASK = 0, O2V_HIP_THIN_DST_DEGREE = 1 };
int o2v_hip_thin_dense(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                       uint32_t flags, uint32_t mode, uint32_t max_iterations, const uint8_t *keep /* may be NULL */, const uint64_t keep_strides[3],
                       uint8_t *dst, const uint64_t dst_strides[3], uint32_t dst_format);
uint64_t o2v_hip_thin_scratch_bytes(const uint32_t dims[3], int have_keep);
/* The device times (ms) of the last o2v_hip_thin_dense call: classify, iterate (the host's reads included), write. */
int o2v_hip_thin_times(const o2v_hip_ctx *ctx, float out_ms[3]);
/* Of the last o2v_hip_thin_dense call made with O2V_HIP_FLAG_STAGE_TIMES (else zeros): the iterations, the launches of the
 * iterations (nine each: the border and the eight sub-steps), the tile turns (the tiles that ran a sub-step with a candidate in
 * them - a tile stamped by a neighbour while a launch runs may or may not count in that launch) and the voxels removed. */
int o2v_hip_thin_counters(const o2v_hip_ctx *ctx, uint64_t out4[4]);

/* ---- parts of a dense grid: watershed basins of a relief, merged by persistence ---------------------------
 *
 * Where one part ends and the next begins: two rooms joined by a corridor, two grains sintered at a neck.  The relief is usually a
 * depth map (o2v_hip_thickness_dense's depth2, or a scaled square root of it); every top of the relief gets a part, and spurious
 * tops are merged into their neighbours by how deep the pass between them is.
 *
 * The definition.
 *   Relief.  H is an int32 grid, indexed [z, y, x], with any element strides.
 *   The set.  S = { v : H[v] > 0 }.  Voxels outside the box are not in S.
 *   Index.  i(v) = (z * ny + y) * nx + x.  It stays below 2^31 by o2v_hip_components_dense's limits: a dim of at most 65 536 and at
 *   most 2^31 - 1 voxels.
 *   Key.  K(v) = (H[v], i(v)), compared lexicographically.  It is a strict total order, so there are no plateaus left to argue about.
 *   Ascent.  For v in S, take the neighbour u of v in S with the greatest key.  Connectivity is 6, 18 or 26.  If K(u) > K(v) then
 *   parent(v) = u.  Otherwise v is a peak.  Keys rise strictly along parents, so the parents form a forest.  basin(v) is the peak
 *   that v reaches.  This is ascent by value, not by slope: a diagonal neighbour counts like a face neighbour.
 *   Saddle.  Two basins A != B are adjacent if some u in A and v in B are neighbours.  saddle(A, B) is the maximum over such pairs
 *   of min(H[u], H[v]).
 *   Persistence (elder rule).  Sort the adjacent pairs by (saddle descending, smaller peak index ascending, larger peak index
 *   ascending).  Walk them with a union-find over the peaks.  Each class is represented by its peak of greatest key.  A pair that
 *   joins two classes kills the class whose representative p has the smaller key.  Then pers(p) = H[p] - saddle and partner(p) is
 *   the other class's representative at that moment.  A class that is never killed has infinite persistence.
 *   Result for min_depth = h >= 0.  final(p) = p if pers(p) >= h, else final(partner(p)).  The chain ends because keys rise.  The
 *   label of v in S is 1 + rank(final(basin(v))), where rank is among the surviving peaks in ascending linear index.  The label is
 *   0 outside S.  *count is the number of survivors.  With h = 0 the labels are the ascent basins and no pair is looked at.
 * What follows: the partitions for rising h nest; the surviving peak of a part is its voxel of greatest key; pers(p) = H[p] - t*,
 * where t* is the highest level t at which the component of {H >= t} that holds p also holds a voxel of greater key.
 * Documented limits of the method.  On a plateau the flow runs to the voxel of greatest index: a flat convex region is one basin
 * with its peak at its last voxel.  Part borders are where ascent paths diverge; they are not smoothed.  A relief of squared depths
 * measures min_depth in squared units.
 *
 * labels is int32 with any strides that map no two voxels to one element; every voxel of the box is written.  relief is only
 * read.  flags: O2V_HIP_FLAG_STAGE_TIMES (o2v_hip_watershed_counters counts).  The result is integers, the same bits on every run,
 * schedule and table size.
 *
 * Refused before any launch, the outputs untouched.  O2V_HIP_ERR_BAD_ARGUMENT: null arguments, zero dims, a connectivity other
 * than 6, 18 or 26, unknown flag bits, pointers that are not 4-byte aligned, that are not device memory of the context's device or
 * that reach outside their allocation, labels strides that map two voxels to one element, any overlap of labels with relief.
 * O2V_HIP_ERR_LIMIT: a dim above 65 536, or nx * ny * nz above 2^31 - 1.  A failed allocation, the pair table's included, returns
 * O2V_HIP_ERR_OUT_OF_MEMORY and the context stays usable.  The call runs on the context's stream and returns when the writes are
 * done (the caller must have finished writing relief).  The host reads the number of peaks; with min_depth > 0 and two peaks or
 * more it also reads the peaks and the distinct adjacent pairs, merges them (plain C++) and sends a label per peak back.
 * O2V_WS_NO_TILES=1 in the environment (A/B): the ascent without its tile pass in LDS; same results.
 *
 * Scratch of the context, grown on demand.  o2v_hip_watershed_scratch_bytes(dims) = 4 * nx * ny * nz (a parent per voxel)  +  12 *
 * words (the peak bits and their prefixes; words = ceil(nx / 64) * ny * nz)  +  8 * (ceil(words / 256) + 1)  +  64 is the part fixed
 * by the box (0 for zero dims).  With a merge come 12 bytes per peak on the device and page-locked, the pair table - 12 bytes a
 * slot, 2^k slots, at first 16 per peak and 2^10 at least, doubled while a probe run finds no place - and 12 bytes per distinct
 * pair on the device and page-locked: the counters report them. */
int o2v_hip_watershed_dense(o2v_hip_ctx *ctx, const int32_t *relief, const uint64_t strides[3], const uint32_t dims[3], uint32_t connectivity,
                            uint32_t min_depth, uint32_t flags, int32_t *labels, const uint64_t labels_strides[3], uint32_t *count);
uint64_t o2v_hip_watershed_scratch_bytes(const uint32_t dims[3]);
/* The times (ms) of the last o2v_hip_watershed_dense call: ascent, flatten (with the peaks' ranks and list), pairs (every turn of
 * the table and the list's way to the host), merge (on the host), labels. */
int o2v_hip_watershed_times(const o2v_hip_ctx *ctx, float out_ms[5]);
/* Of the last o2v_hip_watershed_dense call made with O2V_HIP_FLAG_STAGE_TIMES (else zeros): the peaks, the boundary pairs seen
 * (neighbour pairs whose basins differ, in the table's last turn), the distinct adjacent basin pairs, the table's growths, the
 * table's bytes at the end, the survivors. */
int o2v_hip_watershed_counters(const o2v_hip_ctx *ctx, uint64_t out6[6]);

/* ---- seeded watershed: markers grown through a relief ------------------------------------------------------
 *
 * o2v_hip_watershed_dense finds its own peaks; here the caller says where the parts are.  The hierarchical-queue flood of Meyer,
 * with its accidental FIFO order replaced by a distance and a smallest-label rule, so that the result is a unique fixed point.
 *
 * The definition.
 *   Relief.  H is an int32 grid indexed [z, y, x] with any strides.  The set is S = { v : H[v] > 0 }.  Voxels outside the box are
 *   not in S.  This is o2v_hip_watershed_dense's contract and orientation: high is the middle of a part, and the flood runs
 *   downhill from the markers.
 *   Markers.  M is an int32 grid of the same dims with any strides.  A voxel v in S with M[v] > 0 is a seed of label M[v], which
 *   may be 1 .. 2^31 - 1.  Markers outside S and values <= 0 are ignored.
 *   Steps.  weights[3] are o2v_hip_geodesic_dense's.  Each is 0 .. 65 535, not all are 0, and 0 means "no such step".  A diagonal
 *   step needs only its two end voxels in S.
 *   Key.  Every v in S gets a key K(v) = (Q, T).  Q is the level and T the ticks.  (Q, T) is better than (Q', T') if Q > Q', or if
 *   Q == Q' and T < T'.
 *     A seed has K(s) = (H[s], 0).
 *     A step from u to v with weight w turns (Q, T) into (H[v], 0) if H[v] < Q.  The flood descends onto v and the clock restarts.
 *     Otherwise it turns it into (Q, min(T + w, 2^31 - 2)).  The flood spreads on a plateau, or spills uphill at the level of the
 *     pass it came over, and the clock runs and saturates.
 *   This step is monotone in the key, so K is the best fixed point of "seed key, or the best step from a neighbour", and it is
 *   unique.  Label comparison must not be part of this relaxation.  With the label in the key the step is no longer monotone and
 *   the result depends on the schedule.
 *   The three phases.  K decomposes into three 32-bit fixed points, each final before the next is computed.
 *   1. Level.  Q(v) = max(seed ? H[v] : 0, max_u min(Q(u), H[v])), starting from 0 and only rising.  This is the max-min
 *      (bottleneck) height over all paths from a seed.  Q(v) >= t exactly if the component of {H >= t} that holds v (connectivity
 *      by the weights) holds a seed s with H[s] >= t.  Q = 0 means not reached.
 *   2. Ticks.  T(v) = 0 if v is a seed or has a neighbour u with Q(u) > H[v].  Otherwise T(v) = min over neighbours u with Q(u) ==
 *      Q(v) of min(T(u) + w, 2^31 - 2), only falling.
 *   3. Label.  A seed keeps M[v].  Every other reached v takes the smallest L(u) over its tight neighbours u, those whose step
 *      gives exactly K(v).  A neighbour is tight if Q(u) > H[v], which implies T(v) == 0.  It is also tight if Q(u) == Q(v) and
 *      min(T(u) + w, cap) == T(v).  Labels only fall, and every reached voxel has a tight path to a seed.
 *   Outputs.  labels is int32: L, or 0 outside S and where not reached.  level (optional) is int32: Q, or 0.  ticks (optional) is
 *   int32: T, or -1 outside S and where not reached.  *reached is the number of voxels with Q > 0.
 * On a constant relief ticks is o2v_hip_geodesic_dense's distance to the nearest seed, and labels is the geodesic Voronoi diagram,
 * with the smallest label on a tie.
 *
 * level and ticks may be null; their strides are then not read.  The outputs take any strides that map no two voxels to one
 * element; every voxel of the box is written.  relief and markers are only read.  flags: O2V_HIP_FLAG_STAGE_TIMES
 * (o2v_hip_grow_counters counts).  The result is integers, the same bits on every run and schedule.
 *
 * Refused before any launch, the outputs untouched.  O2V_HIP_ERR_BAD_ARGUMENT: a null relief, markers, labels, reached, weights
 * or strides of a grid that is given, zero dims, a weight above 65 535 or all weights 0, unknown flag bits, pointers that are not
 * 4-byte aligned, that are not device memory of the context's device or that reach outside their allocation, output strides that
 * map two voxels to one element, any overlap between an output and an input or between two outputs.  O2V_HIP_ERR_LIMIT: a dim
 * above 65 536, or nx * ny * nz above 2^31 - 1.  A failed allocation returns O2V_HIP_ERR_OUT_OF_MEMORY and the context stays usable.
 * The call runs on the context's stream and returns when the writes are done (the caller must have finished writing relief and
 * markers).  The host reads 4 bytes between the rounds of a phase.  O2V_GROW_NO_TILES=1 in the environment (A/B): every phase by
 * whole-grid sweeps instead of tiles in LDS; same results.
 *
 * Scratch of the context, grown on demand.  Q, T and L live in level, ticks and labels themselves where those are given and
 * contiguous (linear index (z * ny + y) * nx + x is the element).  o2v_hip_grow_scratch_bytes(dims, which), `which` the OR of
 * O2V_HIP_GROW_SCRATCH_LABELS / _LEVEL / _TICKS for those of the three that are not: 4 * nx * ny * nz (the neighbour masks)  +  4 *
 * nx * ny * nz for each bit of `which`  +  16 * tiles (per tile two flag words and two list places; tiles of 64 x 8 x 8 voxels)  +
 * 128.  (0 for zero dims or unknown bits.) */
enum { O2V_HIP_GROW_MAX_TICKS = 0x7ffffffeu };
enum { O2V_HIP_GROW_SCRATCH_LABELS = 1u, O2V_HIP_GROW_SCRATCH_LEVEL = 2u, O2V_HIP_GROW_SCRATCH_TICKS = 4u };
int o2v_hip_grow_dense(o2v_hip_ctx *ctx, const int32_t *relief, const uint64_t relief_strides[3], const int32_t *markers,
                       const uint64_t marker_strides[3], const uint32_t dims[3], const uint32_t weights[3], uint32_t flags,
                       int32_t *labels, const uint64_t labels_strides[3], int32_t *level, const uint64_t level_strides[3],
                       int32_t *ticks, const uint64_t ticks_strides[3], uint64_t *reached);
uint64_t o2v_hip_grow_scratch_bytes(const uint32_t dims[3], uint32_t which);
/* The device times (ms) of the last o2v_hip_grow_dense call: init, level rounds, sources, tick rounds, tight, label rounds (the
 * host's reads between the rounds included), write. */
int o2v_hip_grow_times(const o2v_hip_ctx *ctx, float out_ms[7]);
/* Of the last o2v_hip_grow_dense call made with O2V_HIP_FLAG_STAGE_TIMES (else zeros), for the level, the ticks and the labels
 * in turn: the rounds (launches of the tile kernel, or whole-grid sweeps), the tile visits, the in-tile sweeps. */
int o2v_hip_grow_counters(const o2v_hip_ctx *ctx, uint64_t out9[9]);

/* ---- which labels touch: the region adjacency of a label grid ---------------------------------------------
 *
 * The grid.  labels, format (O2V_HIP_LABELS_I32 / O2V_HIP_LABELS_U8), strides (elements per axis x, y, z; any order, a stride may
 * be 0) and dims are what o2v_hip_label_stats takes; the grid is only read.
 *
 * Contacts.  A contact is an unordered pair of voxels {u, v} of the box, u != v, whose coordinates differ by at most 1 on every
 * axis.  Its class is the number of axes on which they differ: 1 a shared face, 2 a shared edge only, 3 a shared corner only.
 * connectivity 6 counts class 1, 18 classes 1 and 2, 26 all three.  A voxel outside the box makes no contact.
 *
 * Which labels take part: lo ... n_labels, lo = 1 - the value 0 is background and touches nothing - or, with O2V_HIP_ADJ_ZERO, lo =
 * 0: the background is a label like any other.  A voxel whose value is below lo, negative or above n_labels makes no contact;
 * *out_outside receives the number of voxels that are negative or above n_labels, as o2v_hip_label_stats counts them.
 *
 * What is listed.  For every pair of labels a < b with at least one counted contact between a voxel of a and a voxel of b, one
 * row of O2V_HIP_ADJ_COLUMNS int64:
 *   0  face contacts: the contact area in voxel faces
 *   1  edge-only contacts (0 where the connectivity does not count them)
 *   2  corner-only contacts (0 where the connectivity does not count them)
 *   3  with values: the maximum over the counted contacts of min(V[u], V[v]); else 0
 *   4  with values: the minimum over the counted contacts of max(V[u], V[v]); else 0
 * values is an int32 grid of the same dims with strides of its own (value_strides), or null.  Column 3 is the pass of an
 * ascending relief - with the depth map of a solid the depth of the neck between two parts, o2v_hip_watershed_dense's saddle -,
 * column 4 the pass of a descending one.  The pairs come sorted ascending by (a, b), as int32 [m][2].  Every column is a sum, a
 * maximum or a minimum and the list is sorted: one run equals another bit for bit.  There are at most 13 (2^31 - 1) contacts in
 * all, far below 2^63.
 *
 * o2v_hip_adjacency_count runs the pass and keeps the sorted list in the context: *out_pairs = m.  o2v_hip_adjacency_write copies
 * it into the caller's device arrays pairs [m][2] and table [m][5]; it is refused (O2V_HIP_ERR_BAD_ARGUMENT) when no count precedes
 * it on this context - a count that was refused is none -, when capacity < m, for null, misaligned or overlapping arrays or arrays
 * that are not device memory of the context's device with m rows inside their allocation; with m = 0 both may be null.
 *
 * count is refused before anything is launched, the outputs untouched.  O2V_HIP_ERR_BAD_ARGUMENT: a null argument (values may be
 * null; value_strides only without values), zero dims, an unknown format, a connectivity other than 6, 18 or 26, unknown flag bits
 * (known: O2V_HIP_ADJ_ZERO, O2V_HIP_FLAG_STAGE_TIMES), n_labels above 255 with U8, an I32 grid or values not 4-byte aligned, a
 * grid that is not device memory of the context's device or reaches outside its allocation.  O2V_HIP_ERR_LIMIT (before the
 * pointers are looked at): a dim above 65 536, more than 2^31 - 1 voxels, n_labels above 2^31 - 2.  Both calls run on the
 * context's stream and return when their writes have landed (the caller must have finished writing the grids).
 *
 * Scratch of the context, grown on demand: the pair table - 48 bytes a slot, 2^k slots, at first 16 per label that can occur
 * (min(n_labels + 1, voxels)), 2^10 at least and 2^24 at most, doubled and the pass run again while a probe run finds no place
 * (O2V_ADJ_TABLE_LOG2=k in the environment, a test hook, forces the first size) - and o2v_hip_adjacency_scratch_bytes(m) = 48 m +
 * 64 for the list (as much again page-locked, twice: the host sorts it).  A table or list that cannot be allocated returns
 * O2V_HIP_ERR_OUT_OF_MEMORY and leaves the context usable.  O2V_ADJ_NO_TABLE=1 in the environment (A/B): the pass without its
 * table in LDS, every pending pair straight to global memory; same results. */
enum { O2V_HIP_ADJ_ZERO = 16u };
enum { O2V_HIP_ADJ_COLUMNS = 5 };
int o2v_hip_adjacency_count(o2v_hip_ctx *ctx, const void *labels, uint32_t format, const uint64_t strides[3], const uint32_t dims[3],
                            uint32_t n_labels, uint32_t connectivity, uint32_t flags, const int32_t *values, const uint64_t value_strides[3],
                            uint64_t *out_pairs, uint64_t *out_outside);
int o2v_hip_adjacency_write(o2v_hip_ctx *ctx, int32_t *pairs /* [m][2] */, int64_t *table /* [m][5] */, uint64_t capacity);
/* The times (ms) of the last o2v_hip_adjacency_count call: the table's initialisation and the pass (of the table's last turn), the
 * list and its way to the host, the sort (on the host) and its way back. */
int o2v_hip_adjacency_times(const o2v_hip_ctx *ctx, float out_ms[4]);
/* Of the last o2v_hip_adjacency_count call made with O2V_HIP_FLAG_STAGE_TIMES (else zeros): the pending pairs flushed into a
 * workgroup's table in LDS and those flushed to global memory (in the table's last turn), the table's growths, the table's bytes
 * at the end. */
int o2v_hip_adjacency_counters(const o2v_hip_ctx *ctx, uint64_t out4[4]);
uint64_t o2v_hip_adjacency_scratch_bytes(uint64_t pairs);

/* ---- Euler numbers: the cell counts of a label grid -----------------------------------------------------
 *
 * What shape class a piece has - handles, through-holes, closed shells, loops - is read off its Euler characteristic, an exact
 * integer sum over the 2x2x2 neighbourhoods of the grid.  This call counts, per value of a label grid, the cells that the sums
 * are made of; defined so that a numpy restatement (tests/topology_ref.py) reproduces every bit.
 *
 * Input.  A label grid exactly as o2v_hip_label_stats takes it: O2V_HIP_LABELS_I32 or O2V_HIP_LABELS_U8, element strides per
 * axis in any order (a stride may be 0), dims (nx, ny, nz); the grid is only read.  Rows 0 ... n_labels take part, row 0 like
 * every other row.  A voxel whose value is negative or above n_labels belongs to no row and is counted in *out_outside.
 * Everything outside the box belongs to no row.
 *
 * Cells.  Take the unit lattice of the box: (nx + 1)(ny + 1)(nz + 1) vertices, with the edges, faces and cubes between them.  A
 * lattice cell is incident to 8 (vertex), 4 (edge), 2 (face) or 1 (cube) voxel positions; positions outside the box hold no
 * label.  For label L a cell is closed-in if at least one incident voxel has value L, and inner if every incident position lies
 * in the box and has value L.
 *
 * The table: int64 [n_labels + 1][O2V_HIP_EULER_COLUMNS], contiguous, every element written:
 *   [0] voxels (n3)                [1] closed-in faces (n2)     [2] closed-in edges (n1)     [3] closed-in vertices (n0)
 *   [4] inner faces: face-adjacent pairs both L   [5] inner edges: 2x2x1 blocks all L   [6] inner vertices: 2x2x2 blocks all L
 *
 * The same as 2x2x2 windows.  The window at lattice vertex v holds the voxels at v + {-1, 0}^3 and owns v, the three edges from v
 * towards +x, +y and +z, the three faces spanned by two of these directions and the cube at v.  All incident positions of these
 * eight cells lie inside the window, so a label's 8-bit configuration in the window gives its increment to all seven columns; a
 * window of one label adds (1, 3, 3, 1, 3, 3, 1).
 *
 * What follows from a row: chi_26 = n0 - n1 + n2 - n3 (the set as a union of closed cubes: 26-connectivity), chi_6 = n3 - [4] +
 * [5] - [6] (the dual complex: 6-connectivity), the intrinsic volumes of the closed model V0 = chi_26, V1 = n1 - 2 n2 + 3 n3,
 * V2 = n2 - 3 n3 (half the surface area), V3 = n3, and the exposed faces 6 n3 - 2 [4], o2v_hip_label_stats' faces column.
 *
 * Limits: dims at most 65 536 per axis and at most 2^31 - 1 voxels (every column then stays below 2^36), n_labels at most
 * 2^31 - 2 (O2V_HIP_ERR_LIMIT).  O2V_HIP_ERR_BAD_ARGUMENT: a null argument, zero dims, an unknown format, n_labels above 255 with
 * U8, a table that is not 8-byte aligned or an I32 grid that is not 4-byte aligned, a table that overlaps the grid, a pointer
 * outside its allocation.  A refusal comes before any launch and leaves the outputs untouched.  The scratch is one counter
 * (O2V_HIP_ERR_OUT_OF_MEMORY).  Every result is an integer sum: one run equals another bit for bit. */
enum { O2V_HIP_EULER_COLUMNS = 7 };
int o2v_hip_euler_stats(o2v_hip_ctx *ctx, const void *labels, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], uint32_t n_labels,
                        int64_t *table, uint64_t *out_outside);
/* The device times (ms) of the last o2v_hip_euler_stats call, from events around them: [0] the table's initialisation, [1] the
 * pass over the grid. */
int o2v_hip_euler_stats_times(const o2v_hip_ctx *ctx, float out_ms[2]);

/* ---- Sparse voxel octrees of dense grids ------------------------------------------------------------------
 *
 * The set of a dense grid as a tree that can be stored, shipped and queried by coordinate: the format renderers and collision
 * queries consume, the LOD chain of the grid (level l is its occupancy at 1 / 2^(D - l)), and for solids far smaller than the grid.
 * Defined so that a numpy restatement (tests/octree_ref.py) reproduces every bit.
 *
 * The set and the cube.  The set grid, its three formats (O2V_HIP_GRID_U8, _BITS, _F32_BELOW), strides and `level` are those of
 * o2v_hip_gather_count; the grid is only read.  origin[3] (global voxel coordinates of the box's low corner) and dims[3] give the
 * box; every voxel outside it is empty.  The root cube is [0, 2^D)^3 in global coordinates - low corner 0, the global lattice, as
 * o2v_hip_downsample has it -, so trees of different boxes of one model line up with each other and with the levels of
 * o2v_hip_downsample.  depth = D, 1 <= D <= 16, origin[a] + dims[a] <= 2^D on every axis; depth = 0 on entry asks for the
 * smallest such D.  A cell of level l (0 <= l <= D) is an aligned cube of side 2^(D - l); level D is the voxels.  A cell is
 * non-empty if it holds a solid voxel and full if all 8^(D - l) of its voxels are solid (it then lies wholly in the box).
 *
 * Nodes.  A node is a stored cell of level l < D; the root (level 0) is always stored.  Per node, bit o of `valid` (uint8) is set
 * iff child octant o = dx + 2 dy + 4 dz is non-empty, bit o of `full` (uint8) iff it is full; at level D - 1 the children are
 * voxels and full == valid.  The stored children of a node of level l < D - 1 are stored = valid, and stored = valid & ~full with
 * O2V_HIP_OCT_COLLAPSE: a full cell is then a leaf and nothing below it is stored.  Nodes of level D - 1 have no stored children.
 *
 * Order.  Nodes are stored level by level, within level l + 1 by (index of the parent, octant): the children of a node are
 * contiguous, and every level is in Morton order (z the high bit).  first_child[i] (int32): for a node of level < D - 1 the index
 * of its first stored child, -1 if stored == 0; for a node of level D - 1 the number of solid voxels under all earlier nodes of
 * level D - 1 - the index of its first voxel in a per-voxel attribute array in Morton order, a voxel's slot being first_child[i] +
 * popcount(valid & ((1 << o) - 1)).  voxels_listed is the total of these popcounts (voxels inside collapsed cells are not
 * listed).  coords[i] (int32 [3], optional) is the low corner (x, y, z) of the node's cell.  level_counts[l] is the number of nodes
 * of level l, 0 from l = D on.
 *
 * Descent.  For an int32 point (x, y, z) in global coordinates the result is int32 [4] = (solid, level, node, voxel_index).
 * Outside the root cube: (0, -1, -1, -1).  Start at node 0, level 0; at node i of level l take o, the octant of the point:
 * `valid` bit clear: (0, l, i, -1); l = D - 1: (1, l, i, first_child[i] + rank of o in valid); `full` bit set and the tree
 * collapsed: (1, l, i, -1); otherwise go to child first_child[i] + rank of o in stored.  At most D steps; a child index outside
 * [0, n_nodes), or a -1 where a child is needed, ends it with (0, -2, -1, -1): no array is read outside its n_nodes entries.
 *
 * o2v_hip_octree_build builds the tree into scratch of the context (flags: O2V_HIP_OCT_COLLAPSE, O2V_HIP_FLAG_STAGE_TIMES) and
 * returns its depth, level counts, node count and listed voxels; o2v_hip_octree_write copies it into the caller's contiguous device
 * arrays of *out_nodes entries (coords may be null).  o2v_hip_octree_lookup runs the descent per point on the caller's arrays (a
 * tree from anywhere works; flags say whether it is collapsed); o2v_hip_octree_to_dense writes out(x, y, z) = 1 where the descent
 * is solid and 0 elsewhere for every voxel of any box, also one that sticks out of the root cube.
 *
 * Limits (O2V_HIP_ERR_LIMIT): dims above 65 536 per axis or 2^31 - 1 voxels in all, origin + dims above 65 536 (build) or 2^32
 * (to_dense), n_nodes or n above 2^31 - 1.  O2V_HIP_ERR_BAD_ARGUMENT: what o2v_hip_gather_count refuses of a grid, depth above
 * 16 or origin + dims above 2^depth, unknown flag bits, a null argument, n_nodes = 0, arrays that are not 4-byte aligned where they
 * hold int32, output arrays that overlap each other or the inputs, out strides that map two voxels to one element, a pointer that is
 * not device memory of the context's device with its whole extent inside its allocation, o2v_hip_octree_write without a build
 * ("no o2v_hip_octree_build").  A refusal comes before any launch.  A failed scratch allocation is O2V_HIP_ERR_OUT_OF_MEMORY and
 * leaves the context usable.  Scratch: o2v_hip_octree_scratch_bytes is the most a build of the box takes - 1/8 byte per voxel of
 * bits, 2 bytes per touched cell of the pyramid (2/7 byte per voxel) and 18 bytes per node with a node per cell; a build sizes its
 * nodes by the cells that are nodes.  Integers throughout: one run equals another bit for bit. */
enum { O2V_HIP_OCT_COLLAPSE = 64u, O2V_HIP_OCT_MAX_DEPTH = 16 };
int o2v_hip_octree_build(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                         const uint32_t origin[3], uint32_t depth, uint32_t flags, uint32_t *out_depth, uint64_t level_counts[16], uint64_t *out_nodes,
                         uint64_t *out_voxels_listed);
int o2v_hip_octree_write(o2v_hip_ctx *ctx, uint8_t *valid, uint8_t *full, int32_t *first_child, int32_t *coords);
int o2v_hip_octree_lookup(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, uint64_t n_nodes, uint32_t depth,
                          uint32_t flags, const int32_t *points, uint64_t n, int32_t *out);
int o2v_hip_octree_to_dense(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, uint64_t n_nodes, uint32_t depth,
                            uint32_t flags, const uint32_t origin[3], const uint32_t dims[3], uint8_t *out, const uint64_t out_strides[3]);
/* The device times (ms) of the last build's classify, pyramid and order stages and of the last write, from events around them. */
int o2v_hip_octree_times(const o2v_hip_ctx *ctx, float out_ms[4]);
uint64_t o2v_hip_octree_scratch_bytes(const uint32_t dims[3], const uint32_t origin[3], uint32_t depth);
/* The smallest depth whose root cube holds origin + [0, dims); 0 if a dim is 0 or origin + dims is above 65 536.  Needs no device. */
uint32_t o2v_hip_octree_depth(const uint32_t origin[3], const uint32_t dims[3]);

/* ---- Sparse voxel DAGs: equal subtrees of an octree merged -------------------------------------------------
 *
 * An octree of a voxelized model repeats itself: at level D - 1 there are at most 255 different nodes, and flat walls, the inside
 * of shells and periodic structures repeat one level up and further.  Merging equal subtrees gives the sparse voxel DAG (Kaempe,
 * Sintorn, Assarsson 2013), which is what makes trees of fine grids cheap to keep and to ship.  Per child pointer it keeps the
 * number of listed voxels under the earlier siblings, so a descent through the DAG finds the same voxel slot as one through the
 * tree, and an attribute array made for the tree works unchanged with the DAG.  Integers only; defined so that a numpy restatement
 * (tests/dag_ref.py) reproduces every bit.
 *
 * Input.  A tree as o2v_hip_octree_build defines it, in the caller's device arrays valid, full, first_child of n_nodes entries,
 * its depth D, O2V_HIP_OCT_COLLAPSE in flags or not, and level_counts[16], the nodes per level (0 from level D on, 1 at level 0;
 * their sum is n_nodes): the merge works level by level.  stored(i) is `valid` at level D - 1 and, above it, `valid` for a plain
 * tree and valid & ~full for a collapsed one.  listed(i) is popcount(valid) at level D - 1 and the sum of `listed` over the stored
 * children above it, in uint32 arithmetic.
 *
 * Equality.  Two nodes of one level are equal if their `valid` masks are equal, their `full` masks are equal, and their stored
 * children are equal one by one, recursively; at level D - 1: equal `valid`.  Nodes of different levels are never merged.
 *
 * Numbering.  The classes of level l are numbered by the smallest tree index among their members, ascending: the first occurrence
 * in Morton order decides.  DAG node dag_offset[l] + rank is that class, dag_offset the exclusive scan of out_level_counts, the
 * classes per level; the root is DAG node 0; M is their sum.
 *
 * Arrays.  valid, full (uint8 [M]) are those of the class.  first_child (int32 [M]) is the node's first entry in the pointer
 * arrays, -1 at level D - 1 and where stored == 0.  child (int32 [P]) is the DAG node of each stored child, the entries in node
 * order and within a node in octant order, so first_child is the exclusive scan of popcount(stored) over the nodes above level
 * D - 1.  skip (int32 [P], uint32 bits) is the sum of `listed` over the node's stored children before this one - the same for every
 * member of a class, which is why it can live in the DAG.
 *
 * Descent.  For an int32 point (x, y, z) the result is int32 [4] = (solid, level, node, voxel_index); outside the root cube
 * (0, -1, -1, -1).  Start at node 0 with acc = 0 (uint32); at node i of level l take o, the octant of the point: `valid` bit
 * clear: (0, l, i, -1); l = D - 1: (1, l, i, acc + rank of o in valid), or (1, l, i, -1) without skip; `full` bit set and the DAG
 * collapsed: (1, l, i, -1); otherwise e = first_child[i] + rank of o in stored: first_child[i] < 0 or e outside [0, P) ends it
 * with (0, -2, -1, -1); else acc += skip[e], i = child[e], and an i outside [0, M) ends it with (0, -2, -1, -1).  At most D steps,
 * and nothing is read outside the arrays, whatever they hold.  On the DAG of a tree, columns 0, 1 and 3 equal
 * o2v_hip_octree_lookup's on that tree for every point, and column 2 is the class of the tree node it reports.
 *
 * o2v_hip_octree_dag_build merges into scratch of the context (flags: O2V_HIP_OCT_COLLAPSE, O2V_HIP_FLAG_STAGE_TIMES) and returns
 * the classes per level, M and P; o2v_hip_octree_dag_write copies the DAG into the caller's contiguous device arrays (skip may be
 * null; child too where P is 0).  o2v_hip_octree_dag_lookup runs the descent per point on the caller's arrays (skip may be null:
 * voxel_index is then -1, except where P is 0 - a root alone has nothing to skip), o2v_hip_octree_dag_to_dense writes out(x, y, z) = 1 where the descent is solid and 0 elsewhere for
 * every voxel of any box, as o2v_hip_octree_to_dense does.
 *
 * A tree that is not one.  A stored child index outside the next level, [offset[l + 1], offset[l + 2]), makes the build fail with
 * O2V_HIP_ERR_BAD_ARGUMENT ("... are not a tree of these level counts").  The index is checked before it is used; the failure is
 * found through a flag on the device that the host reads at the wait the build has anyway; nothing is written to caller memory.
 *
 * O2V_HIP_ERR_BAD_ARGUMENT, in this order: a null argument, unknown flag bits, depth outside 1 ... 16, level counts that do not
 * add up to n_nodes (n_nodes = 0 for the queries); O2V_HIP_ERR_LIMIT: n_nodes, P or n above 2^31 - 1, and what
 * o2v_hip_octree_to_dense limits of a box; then O2V_HIP_ERR_BAD_ARGUMENT again: int32 arrays that are not 4-byte aligned, output
 * arrays that overlap each other or the inputs, a pointer that is not device memory of the context's device with its whole extent
 * inside its allocation, o2v_hip_octree_dag_write without a build ("no o2v_hip_octree_dag_build").  All of these come before any
 * launch.  A failed scratch allocation is O2V_HIP_ERR_OUT_OF_MEMORY and leaves the context usable.  Scratch:
 * o2v_hip_octree_dag_scratch_bytes is the most a build takes (0 for level counts a build refuses) - 8 bytes per tree node, 4 per
 * node of the widest level, 4 per table entry (a power of two, at least twice the widest level above D - 1) and a DAG that merges
 * nothing, 6 bytes per node and 8 per pointer; a build sizes the DAG by what it merged. */
int o2v_hip_octree_dag_build(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, uint64_t n_nodes, uint32_t depth,
                             uint32_t flags, const uint64_t level_counts[16], uint64_t out_level_counts[16], uint64_t *out_nodes, uint64_t *out_pointers);
int o2v_hip_octree_dag_write(o2v_hip_ctx *ctx, uint8_t *valid, uint8_t *full, int32_t *first_child, int32_t *child, int32_t *skip);
int o2v_hip_octree_dag_lookup(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, const int32_t *child,
                              const int32_t *skip, uint64_t n_nodes, uint64_t n_pointers, uint32_t depth, uint32_t flags, const int32_t *points, uint64_t n,
                              int32_t *out);
int o2v_hip_octree_dag_to_dense(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, const int32_t *child, uint64_t n_nodes,
                                uint64_t n_pointers, uint32_t depth, uint32_t flags, const uint32_t origin[3], const uint32_t dims[3], uint8_t *out,
                                const uint64_t out_strides[3]);
/* The device times (ms) of the last build's merge of level D - 1, merge of the levels above and output (the pointers scanned, the
 * DAG filled) and of the last write, from events around them. */
int o2v_hip_octree_dag_times(const o2v_hip_ctx *ctx, float out_ms[4]);
uint64_t o2v_hip_octree_dag_scratch_bytes(const uint64_t level_counts[16], uint32_t depth);

/* ---- Rays through sparse voxel octrees and DAGs ------------------------------------------------------------
 *
 * The first solid voxel along each ray, found in the tree or the DAG itself: nothing is expanded, nothing is kept in the context.
 * Defined so that a numpy restatement (tests/treeray_ref.py) reproduces every bit, and so that for any arrays at all
 *   o2v_hip_octree_raycast(arrays) == o2v_hip_raycast_build(o2v_hip_octree_to_dense(arrays)) + o2v_hip_raycast.
 *
 * Space.  Voxel space and rays are those of o2v_hip_raycast: a ray is six float32 widened to double; the plane i of axis a is
 * crossed at T_a(i) = ((double) i - o_a) * (1.0 / d_a), computed per plane, without FMA; the walk starts in floor(o) with t = 0 and
 * face -1; of planes with equal T the lowest axis is crossed first; a ray misses when the next T > t_max.  An invalid ray (a
 * component that is not finite, |o_a| above 2^22) gives (-1, -1, -1, -2) and NaN, a miss (-1, -1, -1, -1) and +inf; d = 0 tests the
 * start cell only.
 *
 * Solid set.  The voxels for which the descent of o2v_hip_octree_lookup (tree) or o2v_hip_octree_dag_lookup (DAG) says solid.  The
 * root cube [0, 2^D)^3 sits on the global lattice and everything outside it is empty; there is no origin argument.
 *
 * Corrupt arrays.  A step that the descent calls corrupt - a child or pointer index outside the arrays, a -1 where a child is
 * needed - makes that octant empty, which is what o2v_hip_octree_to_dense and o2v_hip_octree_dag_to_dense do.  Nothing is read
 * outside the n_nodes / n_pointers entries; a descent takes at most D steps, cyclic pointers included; every event moves the ray
 * strictly forward in (T, axis), so the walk ends.
 *
 * Outputs.  hit int32 [n][4] = (x, y, z, face), t float32 [n] as o2v_hip_raycast writes them; voxel_index int32 [n] (may be null):
 * column 3 of o2v_hip_octree_lookup / o2v_hip_octree_dag_lookup at the hit cell, so -1 for a miss, an invalid ray, a hit inside a
 * full cell of a collapsed tree, or a DAG passed without skip.
 *
 * flags: O2V_HIP_OCT_COLLAPSE or 0.  No scratch and no snapshot: the caller's arrays are walked in place.  O2V_TREERAY_NO_STACK=1 in
 * the environment makes every event descend again from the root instead of from the deepest common ancestor of the old and the new
 * cell (an A/B switch: the results are the same).
 *
 * O2V_HIP_ERR_BAD_ARGUMENT: a null argument (voxel_index and skip may be null, child too where n_pointers is 0), unknown flag
 * bits, depth outside 1 ... 16, n_nodes = 0, t_max NaN or negative, int32 / float arrays that are not 4-byte aligned, outputs that
 * overlap each other, the rays or the tree, a pointer that is not device memory of the context's device with its whole extent
 * inside its allocation.  O2V_HIP_ERR_LIMIT: n_nodes, n_pointers or n above 2^31 - 1.  All of these come before any launch and
 * leave the outputs untouched.  n = 0 succeeds and writes nothing. */
int o2v_hip_octree_raycast(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, uint64_t n_nodes, uint32_t depth,
                           uint32_t flags, const float *origins, const float *directions, uint64_t n, float t_max, int32_t *hit, float *t,
                           int32_t *voxel_index);
int o2v_hip_octree_dag_raycast(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, const int32_t *child,
                               const int32_t *skip, uint64_t n_nodes, uint64_t n_pointers, uint32_t depth, uint32_t flags, const float *origins,
                               const float *directions, uint64_t n, float t_max, int32_t *hit, float *t, int32_t *voxel_index);
/* The device time (ms) of the last cast of either kind, from events around it. */
int o2v_hip_octree_raycast_times(const o2v_hip_ctx *ctx, float out_ms[1]);

/* ---- Sky visibility and ambient occlusion of dense grids --------------------------------------------------
 *
 * Per target voxel, in how many of D integer directions a ray from its centre gets out: the quantity ambient occlusion is baked
 * from, and which tells what a spray, a tool or a sun direction reaches.  Defined so that a numpy restatement
 * (tests/openness_ref.py) reproduces every bit; integers only, one run equals another bit for bit.
 *
 * The set grid, its three formats (O2V_HIP_RAY_GRID_U8, _BITS, _F32_BELOW), strides and `level` are those of
 * o2v_hip_raycast_build; the grid is only read, the box is [0, dims).  directions: D rows of int32 (dx, dy, dz) in host memory,
 * none all zero, |d_a| <= 127, 1 <= D <= 254.  max_distance2: uint32, 0 means unlimited.
 *
 * The walk.  For the target voxel c0 and the direction d let s_a = sgn d_a, m_a = |d_a| and k_a the crossings made so far on axis
 * a (0 at the start).  The next event of an axis with m_a != 0 is T_a = (2 k_a + 1) / (2 m_a): the ray c0 + 1/2 + t d meets the
 * next lattice plane of axis a there.  Events are compared by cross-multiplication in integers.  A step takes the least event and
 * crosses EVERY axis whose event equals it, together (k_a += 1 for each): a ray through a lattice edge or corner does not enter
 * the cells beside it, a voxel blocks a ray only if the ray passes through its open interior.  After a step the cell is
 * c0 + s * k, and the ray is, in this order,
 *   open     if the cell is outside the box (the box is convex: the ray never returns),
 *   open     if max_distance2 != 0 and k_x^2 + k_y^2 + k_z^2 > max_distance2 (the sum grows with every step),
 *   blocked  if the cell is solid;
 * otherwise the next step follows.  The start cell is never tested.  With dims <= 65 536 and m <= 127 every product
 * (2 k + 1) * m is below 2^25: int32 is enough everywhere.  The rule for ties makes the result commute with the 48 symmetries of
 * the lattice applied to the grid and the direction set together (the lowest-axis-first rule of o2v_hip_raycast does not: with it
 * the centre of a flat roof sees 1 of the 26 neighbour directions, not 9).
 *
 * Targets (target_mode): O2V_HIP_OPEN_SURFACE - solid voxels with at least one of the six neighbours empty, outside the box
 * counting as empty; _SOLID - all solid voxels; _EMPTY - all empty voxels; _GRID - the voxels where target_grid, a uint8 grid of
 * the same dims at target_strides (any strides), is nonzero.  target_grid and target_strides are read with _GRID only.
 *
 * Results.  dst (uint8, any strides that keep the voxels apart): the number of open directions of every target, 255 for every
 * voxel that is no target.  mask (int64, optional, D <= 64): bit i set iff direction i is open, 0 for voxels that are no targets.
 * *out_targets: the number of targets.  A sun shadow is one direction and dst == 0.
 *
 * The call builds the three mask levels of o2v_hip_raycast_build into scratch of its own: a snapshot of o2v_hip_raycast_build
 * and o2v_hip_raycast_generation are untouched by it.  flags: O2V_HIP_FLAG_STAGE_TIMES or 0.  O2V_OPEN_NO_SKIP=1 in the
 * environment makes the kernel walk every fine cell (an A/B switch: the results are the same).
 *
 * O2V_HIP_ERR_BAD_ARGUMENT: what o2v_hip_raycast_build refuses of a grid, a null argument (mask may be null; target_grid and
 * target_strides with _GRID only), an unknown target mode or flag bit, D = 0, a zero direction, a component above 127 in
 * magnitude, a mask with D > 64 or not 8-byte aligned, dst or mask strides that map two voxels to one element, dst or mask
 * overlapping each other, the grid or the target grid, a pointer that is not device memory of the context's device with its whole
 * extent inside its allocation.  O2V_HIP_ERR_LIMIT: D above 254, a dim above 65 536, more than 2^31 - 1 voxels.  A refusal comes
 * before any launch and leaves the outputs untouched.  A failed scratch allocation is O2V_HIP_ERR_OUT_OF_MEMORY and leaves the
 * context usable and the outputs untouched.  Scratch: o2v_hip_openness_scratch_bytes is the most a call over dims takes - the
 * masks of o2v_hip_raycast_scratch_bytes and 4 bytes per voxel for the list of targets if every voxel is one; a call sizes its
 * list by the targets it counted. */
enum { O2V_HIP_OPEN_SURFACE = 0, O2V_HIP_OPEN_SOLID = 1, O2V_HIP_OPEN_EMPTY = 2, O2V_HIP_OPEN_GRID = 3 };
enum { O2V_HIP_OPEN_MAX_DIRECTIONS = 254, O2V_HIP_OPEN_MAX_COMPONENT = 127 };
int o2v_hip_openness(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                     const int32_t *directions, uint32_t n_directions, uint32_t target_mode, const uint8_t *target_grid,
                     const uint64_t target_strides[3], uint32_t max_distance2, uint32_t flags, uint8_t *dst, const uint64_t dst_strides[3],
                     int64_t *mask, const uint64_t mask_strides[3], uint64_t *out_targets);
/* The device times (ms) of the last call's stages: build (the masks), targets (counted, the host's wait for their number, listed)
 * and walk, from events around them. */
int o2v_hip_openness_times(const o2v_hip_ctx *ctx, float out_ms[3]);
uint64_t o2v_hip_openness_scratch_bytes(const uint32_t dims[3]);

int o2v_hip_get_timings(const o2v_hip_ctx *ctx, o2v_hip_timings *out);
/* Per-kernel device times of the last o2v_hip_voxelize call made with O2V_HIP_FLAG_KERNEL_TIMES (else none): up to
 * max_entries entries are written, *out_count receives how many there are. */
typedef struct {
    char name[48];     /* kernel name as rocprofv3 prints it, e.g. "k_voxelize<false>" */
    float ms;          /* summed over the launches of the call's last pass */
    uint32_t launches;
} o2v_hip_kernel_time;
int o2v_hip_get_kernel_times(const o2v_hip_ctx *ctx, o2v_hip_kernel_time *out, uint32_t max_entries, uint32_t *out_count);
/* Hash of the device sources this library was built from: profiles record it, bench.py refuses counters of another build. */
const char *o2v_hip_build_id(void);
int o2v_hip_get_stats(const o2v_hip_ctx *ctx, o2v_hip_stats *out);
/* The mesh transform of the last run: row-major 3x3 then translation (reference obj2voxel.cpp:370-402). */
int o2v_hip_get_transform(const o2v_hip_ctx *ctx, float out12[12]);

/* Debugging aid for parity work: hit records of one output cell of the last run, 6 words each
 * (keyhi = sub-voxel<<29 | triangle, keylo = leaf order key, w, u, v as float bits, pool index).  The two debug calls
 * need the hit lists, which the direct MAX path does not keep: they return O2V_HIP_ERR_BAD_ARGUMENT after such a run
 * (set O2V_NO_DIRECT_MAX=1 in the environment to route every hit through the lists). */
int o2v_hip_debug_cell_hits(o2v_hip_ctx *ctx, uint32_t x, uint32_t y, uint32_t z, uint32_t *out, uint32_t max_records,
                            uint32_t *out_count);

/* Debugging aid for parity work: every hit record of the last run, 8 words each (cell x, y, z, keyhi, keylo, bits of w, u, v):
 * what the clip kernel computed per (leaf, voxel) pair, before any fold.  *n_hits receives the number of hits; records are
 * written only if max_hits >= *n_hits (call with max_hits = 0 first).  Same restriction as o2v_hip_debug_cell_hits. */
int o2v_hip_debug_hits(o2v_hip_ctx *ctx, uint32_t *out8, uint64_t max_hits, uint64_t *n_hits);

/* Debugging aid: log2 histogram of hits per occupied cell of the last run (32 buckets; bucket b: 2^(b-1) < hits <= 2^b). */
int o2v_hip_debug_hits_histogram(o2v_hip_ctx *ctx, uint64_t *out32);

/* ---- smooth meshes of label grids: shared-interface surface nets ------------------------------------------
 *
 * The interfaces between the parts of a label grid as ONE indexed mesh, by surface nets in Gibson's form on labels: one vertex per
 * cell of 2 x 2 x 2 samples that are not all equal, one quad per pair of face-adjacent samples with different labels - so the wall
 * between two parts is meshed once, and the meshes of two parts share its vertices - and a relaxation that moves every vertex
 * towards its neighbours in the net without leaving its cell.
 *
 * Grid.  labels is device memory of the context's device, only read: O2V_HIP_LABELS_I32 or O2V_HIP_LABELS_U8 exactly as
 * o2v_hip_label_stats takes them (a bool tensor is U8), sample (x, y, z) at labels[x * strides[0] + y * strides[1] + z * strides[2]]
 * (elements, any order, a stride may be 0), dims = (nx, ny, nz).  Labels are compared as signed int32; any value is allowed and no
 * n_labels is needed.  E = 1 if flags has O2V_HIP_LABEL_SURFACE_CLOSED, else 0.  The extended lattice has the samples (x, y, z) with
 * -E <= x < nx + E, -E <= y < ny + E, -E <= z < nz + E; a sample outside the box has label 0, L(c) is the label of sample c.  CLOSED
 * therefore caps every part at the sides of the box; without it a surface that leaves the box is open there, as
 * o2v_hip_surface_write's.
 *   Cells: (i, j, k) with -E <= i < nx - 1 + E, -E <= j < ny - 1 + E, -E <= k < nz - 1 + E, named by its lowest sample; it holds
 *   the samples (i + a, j + b, k + c), each of a, b, c 0 or 1.  A cell is active if its eight labels are not all equal.
 *   Vertices: one per active cell, numbered in ascending (k, j, i).  cells[v] = (i, j, k), int32 (a component is -1 at the lower
 *   sides of a CLOSED box).  Its centre is (float) (o + i + 1) per axis for an origin o: exact, and >= 0.  (Sample (x, y, z) stands
 *   for the voxel centre o + (x, y, z) + 0.5, so the cell's centre is the lattice point between its eight voxels.)
 *   Quads: for every extended sample c and axis ax in 0, 1, 2, with q = c + e_ax, u = (ax + 1) % 3, v = (ax + 2) % 3, one quad if q
 *   is in the extended lattice, L(c) != L(q), and the edge is interior across: -E + 1 <= c[u] <= n_u + E - 2 and the same for v.  Its
 *   cells are c0 = c - e_u - e_v, c1 = c - e_v, c2 = c, c3 = c - e_u, exactly o2v_hip_surface_write's (all four are active: they
 *   contain the edge).  If L(c) > L(q) the quad is (c0, c1, c2, c3), else (c0, c3, c2, c1): the normal points from the larger label
 *   to the smaller, against the background 0 outward for positive labels.  pairs[quad] = (hi, lo), the larger label first.  The quad
 *   is written as the two triangles (q0, q1, q2), (q0, q2, q3): faces [2 Q][3] int32, triangles 2 n and 2 n + 1 are quad n.  Quads
 *   come in ascending ((z * NY + y) * NX + x) * 3 + ax over the extended lattice (NX = nx + 2 E, x counted from -E).
 *   Links: links[v][d] for d = -x, +x, -y, +y, -z, +z is the vertex of the neighbouring cell in that direction if that cell exists
 *   and the four samples of the face the two cells share are not all equal (both cells are then active), else -1.  "The neighbour
 *   is active" is NOT the rule: two active cells may share a uniform face, and they are not linked.  The links are the edges of the
 *   quads.
 *
 * Relaxation (o2v_hip_label_surface_relax): a pure function of cells, links, origin and iterations, relaxation, reach; float32, op
 * by op, no FMA, the division correctly rounded.
 *   p_0[v] = centre(v).  For t < iterations every vertex is computed from p_t (Jacobi, two buffers, never in place):
 *     s = (0, 0, 0); for d = 0 .. 5 in turn, if links[v][d] is valid, s = s + p_t[links[v][d]] component by component; m = the
 *     number of valid links.  m == 0: p_{t+1}[v] = p_t[v].  Else avg = s / (float) m, r = p_t[v] + relaxation * (avg - p_t[v]),
 *     p_{t+1}[v] = fminf(fmaxf(r, centre - reach), centre + reach) per component.
 *   A link < 0 or >= n_vertices is no link and is never followed: arrays from anywhere cannot make the call read outside them.
 *   0 < relaxation <= 1, 0 <= reach <= 0.5, 0 <= iterations <= 1024.  With iterations 0, positions are the centres; with them the
 *   signed volume of the quads of a label is its number of voxels.
 *   With reach 0.5 a feature one voxel wide collapses as the iterations go on (a single voxel's eight vertices meet in its centre):
 *   Gibson's behaviour; reach 0.25 keeps such a feature at half its size.  The relaxation is Laplacian smoothing and shrinks noisy
 *   labels; neither is corrected.
 *
 * Two calls, as for o2v_hip_surface_*.  o2v_hip_label_surface_count classifies the grid (its only pass over the labels) and keeps in
 * scratch of the context, per 64 extended samples along x, three difference words (the label differs from the one at x + 1, y + 1,
 * z + 1), the word of active cells and two 16-bit prefixes - 36 bytes per 64 samples - and per 256 such words two offsets; it
 * returns the vertices V and the quads Q.  o2v_hip_label_surface_write must follow a count with the same labels, format, strides,
 * dims and flags (else O2V_HIP_ERR_BAD_ARGUMENT, "no matching o2v_hip_label_surface_count"; another count, refused or not, replaces
 * the last one) and fills cells [V][3], links [V][6], faces [2 Q][3], pairs [Q][2], all int32 and contiguous; it may be repeated.
 * Only the pairs and the winding are read from the labels again: if the grid changed between the calls they may be meaningless,
 * but every index written is below V and nothing is written outside the arrays.  o2v_hip_label_surface_relax needs no count: it
 * takes cells and links from anywhere and writes positions [n_vertices][3] float32; its second buffer is scratch of the context.
 * No atomics anywhere: one run equals another bit for bit.
 * Refused before any launch (O2V_HIP_ERR_BAD_ARGUMENT): null arguments (an output may be null only where its count is 0), zero
 * dims, an unknown format or flag bit, an I32 grid that is not 4-byte aligned, outputs that are not 4-byte aligned, capacities
 * below the counted totals, outputs overlapping each other or the grid (relax: positions overlapping cells or links), a pointer
 * that is not device memory of the context's device with its whole extent inside its allocation, a relaxation or reach outside
 * its range (a NaN included).  O2V_HIP_ERR_LIMIT: a dim above 65 536 - 2 E, more than 2^31 - 1 vertices or triangles (2 Q), more
 * than 1024 iterations, an origin component above 65 536 (the caller keeps origin[a] + dims[a] + E at or below 65 536: centres are
 * then exact and positions exact to 2^-7 voxel).  A failed scratch allocation returns O2V_HIP_ERR_OUT_OF_MEMORY and the context
 * stays usable.  The calls run on the context's stream and return when their results have landed. */
enum { O2V_HIP_LABEL_SURFACE_CLOSED = 1 };
int o2v_hip_label_surface_count(o2v_hip_ctx *ctx, const void *labels, uint32_t format, const uint64_t strides[3], const uint32_t dims[3],
                                uint32_t flags, uint64_t *out_vertices, uint64_t *out_quads);
int o2v_hip_label_surface_write(o2v_hip_ctx *ctx, const void *labels, uint32_t format, const uint64_t strides[3], const uint32_t dims[3],
                                uint32_t flags, int32_t *cells, int32_t *links, uint64_t vertex_capacity, int32_t *faces, int32_t *pairs,
                                uint64_t quad_capacity);
int o2v_hip_label_surface_relax(o2v_hip_ctx *ctx, const int32_t *cells, const int32_t *links, uint64_t n_vertices, const uint32_t origin[3],
                                uint32_t iterations, float relaxation, float reach, float *positions);
/* The device times (ms) of the stages: classify, count + scan (the last count), vertices (cells + links), faces (+ pairs) (the last
 * write; 0 after a count), relax (the last relax, all its iterations). */
int o2v_hip_label_surface_times(const o2v_hip_ctx *ctx, float out_ms[5]);

/* ---- multi-GPU: the grid sharded by z-slab over the GPUs of one node --------------------------
 *
 * Every rank (one per GPU) holds the whole triangle list, like every 64^3 chunk of the reference sees every triangle
 * that overlaps it (src/obj2voxel.cpp:226-243), and voxelizes only its own z-slab (walk clamped as in
 * src/voxelization.cpp:440-444).  Voxel data never crosses GPUs: each output voxel is owned by exactly one slab and the
 * union of the slabs is bit-identical to the single-GPU result.  What the ranks exchange is planning data, with RCCL over
 * xGMI: the passes over the triangle list that find the mesh bounds and the z histogram of predicted work are SHARDED
 * (rank r streams triangles [r, r+1) * T / N only).  Three collectives per run: an all-reduce (max of 7 words: the six bounds -
 * the minima as complements - and a "this rank cannot go ahead" word); an all-gather of every rank's partial histogram (2048 u64,
 * added up by every rank itself) together with the z extents of its blocks of 256 triangles (so that each rank can skip the
 * blocks that miss its slab without reading them); an all-gather of the per-slab voxel counts (output offsets for the sink).
 *
 * Two ways to use it:
 *   one process per GPU   o2v_hip_comm_unique_id on rank 0 -> ship the 128 bytes to every rank (MPI, torch.distributed,
 *                         a file) -> o2v_hip_comm_create_rccl on every rank -> o2v_hip_voxelize_sharded, collectively.
 *   one process, N GPUs   o2v_hip_group_*: one context and one host thread per GPU; obj2voxel_voxelize() uses this when
 *                         the environment names more than one device (O2V_DEVICES=0,1,2,3 or O2V_DEVICES=all).
 */
#define O2V_HIP_COMM_ID_BYTES 128
typedef struct o2v_hip_comm o2v_hip_comm;

/* Collectives supplied by the embedding program, on HOST memory, in place; every rank calls them in the same order.
 * Return 0 on success.  Used where RCCL cannot be (tests with a gloo group; two ranks sharing one GPU). */
typedef struct {
    void *user;
    int (*allreduce_min_u32)(void *user, uint32_t *buf, size_t n);
    int (*allreduce_max_u32)(void *user, uint32_t *buf, size_t n);
    int (*allreduce_sum_u64)(void *user, uint64_t *buf, size_t n);
    int (*allgather)(void *user, void *buf, size_t bytes_per_rank); /* rank r's part sits at buf + r * bytes_per_rank */
    int (*broadcast)(void *user, void *buf, size_t bytes, int root);
} o2v_hip_comm_callbacks;

int o2v_hip_comm_unique_id(uint8_t id[O2V_HIP_COMM_ID_BYTES]); /* ncclGetUniqueId; call on one rank */
int o2v_hip_comm_create_rccl(const uint8_t id[O2V_HIP_COMM_ID_BYTES], int rank, int world, int device, o2v_hip_comm **out);
int o2v_hip_comm_create_callbacks(const o2v_hip_comm_callbacks *callbacks, int rank, int world, o2v_hip_comm **out);
void o2v_hip_comm_destroy(o2v_hip_comm *comm);
const char *o2v_hip_comm_kind(const o2v_hip_comm *comm); /* "rccl" or "callbacks" */
const char *o2v_hip_comm_last_error(const o2v_hip_comm *comm);

/* Collective over `comm`: every rank calls it with the same triangles (o2v_hip_set_triangles) and the same params
 * (z_begin / z_end are ignored).  Plans work-balanced slabs from the sharded passes, voxelizes this rank's slab and
 * gathers the slab counts.  out_count: this rank's voxels (read them with o2v_hip_read_voxels); out_counts_all (optional):
 * world entries; out_cuts (optional): world + 1 ascending z cuts, rank r owns [out_cuts[r], out_cuts[r + 1]).
 * With a world of 1 this is o2v_hip_voxelize.
 * Time limits: ncclCommInitRank and the run's first collective are given O2V_COMM_TIMEOUT_S seconds (120) for the other ranks to
 * arrive; after that the call fails with a message naming the rank.  A collective that timed out stays queued on the device:
 * the context and the communicator are then unusable (every later call on them fails or would wait for ever), o2v_hip_destroy
 * and o2v_hip_comm_destroy return without waiting for the device (the communicator is aborted, the context's device memory is
 * left to the process' end) - the process should report the error and exit.
 */
int o2v_hip_voxelize_sharded(o2v_hip_ctx *ctx, o2v_hip_comm *comm, const o2v_hip_params *params, uint64_t *out_count,
                             uint64_t *out_counts_all, uint32_t *out_cuts);

/* In-process group: N contexts (one per listed device; a device may be listed more than once, which only makes sense
 * for tests on a single-GPU machine) driven by N host threads.  The ranks talk through RCCL when every device is listed
 * once and librccl can be loaded, otherwise through shared host memory. */
typedef struct o2v_hip_group o2v_hip_group;
enum {
    O2V_HIP_UPLOAD_H2D = 0,       /* every GPU copies the triangles from host memory over its own PCIe link, in parallel */
    O2V_HIP_UPLOAD_BROADCAST = 1, /* one H2D copy to the first GPU, then an RCCL broadcast over xGMI */
    O2V_HIP_UPLOAD_PEER = 2       /* one H2D copy to the first GPU, then hipMemcpyPeerAsync to each of the others */
};
int o2v_hip_group_create(const int *devices, uint32_t n_devices, o2v_hip_group **out);
void o2v_hip_group_destroy(o2v_hip_group *group);
uint32_t o2v_hip_group_size(const o2v_hip_group *group);
o2v_hip_ctx *o2v_hip_group_ctx(o2v_hip_group *group, uint32_t rank); /* for read_voxels / timings / stats of one rank */
const char *o2v_hip_group_comm_kind(const o2v_hip_group *group);      /* "rccl" or "callbacks" */
const char *o2v_hip_group_last_error(const o2v_hip_group *group);
int o2v_hip_group_set_triangles(o2v_hip_group *group, const float *verts, const float *uvs, const uint32_t *types,
                                const float *colors, const int32_t *texids, uint64_t count, int upload_mode);
int o2v_hip_group_set_textures(o2v_hip_group *group, const o2v_hip_texture *textures, uint32_t count);
/* out_counts: n_devices entries; out_cuts (optional): n_devices + 1 entries */
int o2v_hip_group_voxelize(o2v_hip_group *group, const o2v_hip_params *params, uint64_t *out_counts, uint32_t *out_cuts);

/* Host-only pieces of the above, exported so that they can be tested without a GPU:
 * the cuts for n_slabs slabs of equal predicted work from a z histogram of n_bins bins of bin_layers output layers each
 * (out_z: n_slabs + 1 entries); a self-test that drives every callback of a callbacks table with known patterns from
 * this rank and checks what comes back (0 = all collectives behave as specified); and the same for the shared-memory
 * exchange between the threads of an in-process group. */
void o2v_hip_cuts_from_histogram(const uint64_t *hist, uint32_t n_bins, uint32_t bin_layers, uint32_t resolution,
                                 uint32_t n_slabs, uint32_t *out_z);
int o2v_hip_comm_callbacks_selftest(const o2v_hip_comm_callbacks *callbacks, int rank, int world);
int o2v_hip_group_exchange_selftest(uint32_t n_threads);
/* The RCCL code path of an n-rank in-process group (unique id, ncclCommInitRank on one thread per rank, all five collectives,
 * teardown) on host memory, without selecting a device: only meaningful with a librccl that works on host memory (the tests'
 * stand-in, loaded through O2V_RCCL_LIB).  0 = everything behaved as specified. */
int o2v_hip_group_rccl_selftest(uint32_t n_ranks);

/* A triangle file (OBJ with MTL + PNG textures, binary STL; `type` = extension or NULL to take the path's) read by the
 * library's own readers into the flat host arrays o2v_hip_set_triangles takes - what obj2voxel_voxelize() does with
 * obj2voxel_set_input_file (reference src/io.cpp:244-312,395-435), without the voxelization.  bench.py uses it to run the
 * real Spot / Dragon / Sponza assets when $O2V_ASSETS holds them.  Arrays a mesh does not need are NULL; the pointers and
 * the texture pixels stay valid until o2v_mesh_free. */
typedef struct o2v_mesh o2v_mesh;
int o2v_mesh_load_file(const char *path, const char *type, o2v_mesh **out);
uint64_t o2v_mesh_arrays(const o2v_mesh *mesh, const float **verts, const float **uvs, const uint32_t **types,
                         const float **colors, const int32_t **texids, uint32_t *n_textures); /* returns the triangle count */
int o2v_mesh_texture(const o2v_mesh *mesh, uint32_t index, o2v_hip_texture *out);
void o2v_mesh_free(o2v_mesh *mesh);

/* Debugging aid for kernel work: 16 event counters of the clip loop of the last run.  All zero unless the library was
 * built with -DO2V_INSTRUMENT (make INSTR=1, tools/instrument.sh); the meaning of each slot is documented there. */
int o2v_hip_debug_counters(const o2v_hip_ctx *ctx, uint64_t *out16);

/* Self checks of the clip loop's short division forms on the device (obj2voxel_amd/csrc/o2v_dev_arith.hpp).
 * _check_third: x / 3 against its three-instruction form for all 2^32 float32 bit patterns; out2[0] = differing inputs,
 * out2[1] = the first of them + 1 (0 if none).
 * _check_div: n / d against the lean form for `samples` pairs per pair of biased exponents (numerator, divisor);
 * out65536[en * 256 + ed] = differing pairs.  The kernels only use the lean form inside the region that is all zero. */
int o2v_hip_debug_check_third(o2v_hip_ctx *ctx, uint64_t *out2);
int o2v_hip_debug_check_div(o2v_hip_ctx *ctx, uint32_t samples, uint64_t seed, uint32_t *out65536);

#ifdef __cplusplus
}
#endif
#endif
