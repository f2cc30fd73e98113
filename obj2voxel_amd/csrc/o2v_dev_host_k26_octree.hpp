// Host side of K26 (o2v_dev_k26_octree.hpp): the sparse voxel octree of a set grid.  It classifies with K12's launch_classify and
// takes K12's limits, so it comes after o2v_dev_host_k12_components.hpp (bit_grid, launch_classify, index_limits).

namespace {

static_assert(kOctMaxDepth == O2V_HIP_OCT_MAX_DEPTH, "one depth limit for the callers and the kernels");
constexpr uint32_t kOctCollapse = O2V_HIP_OCT_COLLAPSE;
constexpr uint32_t kOctFlagsKnown = O2V_HIP_OCT_COLLAPSE | O2V_HIP_FLAG_STAGE_TIMES;
constexpr uint64_t kOctMaxExtent = 1ull << kOctMaxDepth;   // origin + dims per axis: the root cube of the deepest tree
constexpr uint32_t kOctNodeBytes = 1u + 1u + 4u + 12u;     // valid, full, first_child, coords

// The levels 0 ... depth - 1 of the tree of the box: the cells each touches and where its entries begin in the pyramid.
struct OctPlan {
    uint32_t depth = 0;
    OctLevel lv[kOctMaxDepth] = {};
    uint64_t cells = 0;   // of all levels
};

// the smallest depth whose root cube holds the box (origin + dims at most 2^16 per axis)
uint32_t oct_min_depth(const uint32_t origin[3], const uint32_t dims[3])
{
    uint32_t d = 1;
    for (int a = 0; a < 3; ++a)
        while ((uint64_t) origin[a] + dims[a] > (1ull << d)) ++d;
    return d;
}

OctPlan oct_plan(const uint32_t origin[3], const uint32_t dims[3], uint32_t depth)
{
    OctPlan p;
    p.depth = depth;
    for (uint32_t l = 0; l < depth; ++l) {
        OctLevel &L = p.lv[l];
        L.cells = 1;
        for (int a = 0; a < 3; ++a) {
            L.c0[a] = oct_cell_lo(origin[a], depth - l);
            L.n[a] = oct_cell_n(origin[a], dims[a], depth - l);
            L.cells *= L.n[a];
        }
        L.first = p.cells;
        p.cells += L.cells;
    }
    return p;
}

// origin and depth of a build or a scratch question: *depth is the depth in effect
int oct_depth(o2v_hip_ctx *ctx, const char *fn, const uint32_t origin[3], const uint32_t dims[3], uint32_t *depth)
{
    if (*depth > kOctMaxDepth) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "depth must be 0 ... 16, not " + std::to_string(*depth));
    if (int rc = extent_limit(ctx, fn, origin, dims, kOctMaxExtent, "origin + dims is above 65 536 along an axis: the deepest root cube is 2^16 wide")) return rc;
    if (*depth == 0) *depth = oct_min_depth(origin, dims);
    for (int a = 0; a < 3; ++a)
        if ((uint64_t) origin[a] + dims[a] > (1ull << *depth))
            return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "origin + dims is above 2^depth = " + std::to_string(1u << *depth) + " along an axis");
    return O2V_HIP_OK;
}

// The tree arguments of the two queries, checked: *t as the kernels take it, spans[0, 3) its arrays.
int oct_tree(o2v_hip_ctx *ctx, const char *fn, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, uint64_t n_nodes, uint32_t depth,
             uint32_t flags, OctTree *t, Span *spans)
{
    if (!valid || !full || !first_child) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if (depth < 1u || depth > kOctMaxDepth) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "depth must be 1 ... 16, not " + std::to_string(depth));
    if (flags & ~kOctFlagsKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if (n_nodes == 0) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "n_nodes is 0: a tree has its root");
    if (n_nodes > kMaxInt32) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 2^31 - 1 nodes");
    if ((uintptr_t) first_child % sizeof(int32_t)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "first_child must be 4-byte aligned");
    O2V_CHECK(hipSetDevice(ctx->device));
    spans[0] = Span{"valid", valid, n_nodes}, spans[1] = Span{"full", full, n_nodes}, spans[2] = Span{"first_child", first_child, n_nodes * 4u};
    for (int i = 0; i < 3; ++i)
        if (int rc = check_device_range(ctx, fn, spans[i].p, spans[i].bytes, spans[i].what)) return rc;
    *t = OctTree{valid, full, first_child, (uint32_t) n_nodes, depth, (flags & kOctCollapse) ? 1u : 0u};
    return O2V_HIP_OK;
}

}  // namespace

extern "C" {

uint32_t o2v_hip_octree_depth(const uint32_t origin[3], const uint32_t dims[3])
{
    if (!origin || !dims || !dims[0] || !dims[1] || !dims[2]) return 0;
    for (int a = 0; a < 3; ++a)
        if ((uint64_t) origin[a] + dims[a] > kOctMaxExtent) return 0;
    return oct_min_depth(origin, dims);
}

uint64_t o2v_hip_octree_scratch_bytes(const uint32_t dims[3], const uint32_t origin[3], uint32_t depth)
{
    const uint32_t min_depth = o2v_hip_octree_depth(origin, dims);
    if (!min_depth || depth > kOctMaxDepth || (depth && depth < min_depth)) return 0;
    const OctPlan p = oct_plan(origin, dims, depth ? depth : min_depth);
    // the bits, the pyramid, the counters; at most a node per cell of the pyramid, and the block offsets of the widest level
    return 8u * cc_words(dims) + 2u * p.cells + 8u * kOctMeta + (uint64_t) kOctNodeBytes * p.cells + 8u * (p.lv[p.depth - 1u].cells / kBlock + 2u);
}

int o2v_hip_octree_build(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                         const uint32_t origin[3], uint32_t depth, uint32_t flags, uint32_t *out_depth, uint64_t level_counts[16], uint64_t *out_nodes,
                         uint64_t *out_voxels_listed)
{
    static const char fn[] = "o2v_hip_octree_build";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    ctx->oct.valid = false;
    SetGrid sg;
    int rc;
    if ((rc = set_grid(ctx, fn, grid, format, strides, dims, level, &sg)) || (rc = index_limits(ctx, fn, dims, 0u, "nodes"))) return rc;
    if (!origin) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((rc = oct_depth(ctx, fn, origin, dims, &depth))) return rc;
    if (flags & ~kOctFlagsKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if (!out_depth || !level_counts || !out_nodes || !out_voxels_listed) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    const uint32_t collapsed = (flags & kOctCollapse) ? 1u : 0u, D = depth;
    const BitGrid bg = bit_grid(dims);
    const OctPlan plan = oct_plan(origin, dims, D);
    if ((rc = grow_scratch(ctx, ctx->d_oct_bits, bg.words, fn, "set bits")) || (rc = grow_scratch(ctx, ctx->d_oct_pyr, plan.cells, fn, "pyramid")) ||
        (rc = grow_scratch(ctx, ctx->d_oct_meta, kOctMeta, fn, "counters")) || (rc = grow_scratch(ctx, ctx->h_oct_meta, 2u * kOctMeta, fn, "counters")))
        return rc;
    unsigned long long *const bits = ctx->d_oct_bits.ptr, *const meta = ctx->d_oct_meta.ptr, *const h_meta = ctx->h_oct_meta.ptr;
    uint16_t *const pyr = ctx->d_oct_pyr.ptr;
    hipStream_t s = ctx->stream;

    // the bit grid and, bottom up, the pyramid; the host waits for the number of cells per level that are nodes
    O2V_CHECK(hipMemsetAsync(meta, 0, kOctMeta * sizeof(unsigned long long), s));
    O2V_CHECK(ctx->oct_times.mark(0, s));
    launch_classify(ctx, sg, 0u, bits);
    O2V_CHECK(ctx->oct_times.mark(1, s));
    {
        const OctLevel &L = plan.lv[D - 1u];
        O2V_LAUNCH("k_oct_leaves", s, k_oct_leaves, dim3(stream_grid(ctx, L.cells, 8u)), dim3(kBlock), 0, s, bits, bg, origin[0], origin[1], origin[2], L,
                   collapsed, pyr, meta + kOctBound + (D - 1u));
    }
    for (uint32_t l = D - 1u; l-- > 0u;) {
        const OctLevel &L = plan.lv[l];
        O2V_LAUNCH("k_oct_up", s, k_oct_up, dim3(stream_grid(ctx, L.cells, 8u)), dim3(kBlock), 0, s, pyr, plan.lv[l + 1u], L, collapsed, meta + kOctBound + l);
    }
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(ctx->oct_times.mark(2, s));
    O2V_CHECK(hipMemcpyAsync(h_meta, meta, kOctMeta * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    uint64_t bound[kOctMaxDepth] = {}, cap = 0, widest = 1;
    for (uint32_t l = 0; l < D; ++l) {
        bound[l] = l ? h_meta[kOctBound + l] : 1u;   // (the root is stored whatever it holds)
        cap += bound[l];
        widest = std::max(widest, bound[l]);
    }
    if (cap > kMaxInt32) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 2^31 - 1 nodes");   // (never, by the limits above: a level's cells are no more than the voxels)
    if ((rc = grow_scratch(ctx, ctx->d_oct_valid, cap, fn, "nodes")) || (rc = grow_scratch(ctx, ctx->d_oct_full, cap, fn, "nodes")) ||
        (rc = grow_scratch(ctx, ctx->d_oct_first, cap, fn, "nodes")) || (rc = grow_scratch(ctx, ctx->d_oct_coords, 3u * cap, fn, "nodes")) ||
        (rc = grow_scratch(ctx, ctx->d_oct_boff, (widest + kBlock - 1u) / kBlock + 1u, fn, "block offsets")))
        return rc;
    const OctNodes nd{ctx->d_oct_valid.ptr, ctx->d_oct_full.ptr, ctx->d_oct_first.ptr, ctx->d_oct_coords.ptr, cap};
    unsigned long long *const boff = ctx->d_oct_boff.ptr;

    // top down, level by level: the launches are sized by the pyramid's counts, the scans' counts stay on the device
    O2V_CHECK(hipEventRecord(ctx->oct_times.ev[3], s));
    O2V_LAUNCH("k_oct_root", s, k_oct_root, dim3(1), dim3(64), 0, s, pyr, plan.lv[0].first, nd, meta);
    for (uint32_t l = 0; l < D; ++l) {
        const uint32_t leaf = l + 1u == D ? 1u : 0u;
        const uint64_t n_blocks = std::max<uint64_t>(1u, (bound[l] + kBlock - 1u) / kBlock);
        const dim3 blocks((uint32_t) std::min<uint64_t>(n_blocks, (uint64_t) ctx->num_cus * 8u));
        O2V_LAUNCH("k_oct_count", s, k_oct_count, blocks, dim3(kBlock), 0, s, nd, meta, l, leaf, collapsed, n_blocks, boff);
        O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, boff, n_blocks, leaf ? meta + kOctVoxels : meta + kOctCount + l + 1u);
        O2V_LAUNCH("k_oct_children", s, k_oct_children, blocks, dim3(kBlock), 0, s, nd, meta, l, leaf, collapsed, n_blocks, boff, pyr, plan.lv[leaf ? l : l + 1u],
                   D - l - 1u);
    }
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipEventRecord(ctx->oct_times.ev[4], s));
    O2V_CHECK(hipMemcpyAsync(h_meta + kOctMeta, meta, kOctMeta * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(ctx->oct_times.elapsed(0, 1, ctx->oct_times.ms[0]));
    O2V_CHECK(ctx->oct_times.elapsed(1, 2, ctx->oct_times.ms[1]));
    O2V_CHECK(ctx->oct_times.elapsed(3, 4, ctx->oct_times.ms[2]));
    ctx->oct_times.ms[3] = 0.f;
    const unsigned long long *const got = h_meta + kOctMeta;
    for (uint32_t l = 1; l < D; ++l)
        if (got[kOctCount + l] != bound[l])
            return refuse(ctx, O2V_HIP_ERR_HIP, fn, "level " + std::to_string(l) + ": the scans found " + std::to_string(got[kOctCount + l]) +
                                                        " nodes, the pyramid " + std::to_string(bound[l]));
    o2v_hip_ctx::OctreeBuild &b = ctx->oct;
    b.key = sg.key;
    std::copy(origin, origin + 3, b.origin);
    b.depth = D, b.flags = flags & kOctCollapse;
    b.nodes = got[kOctFirst + D], b.voxels = got[kOctVoxels];
    b.valid = true;
    *out_depth = D;
    for (uint32_t l = 0; l < kOctMaxDepth; ++l) level_counts[l] = l < D ? got[kOctCount + l] : 0u;
    *out_nodes = b.nodes;
    *out_voxels_listed = b.voxels;
    return O2V_HIP_OK;
}

int o2v_hip_octree_write(o2v_hip_ctx *ctx, uint8_t *valid, uint8_t *full, int32_t *first_child, int32_t *coords)
{
    static const char fn[] = "o2v_hip_octree_write";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!ctx->oct.valid) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "no o2v_hip_octree_build");
    if (!valid || !full || !first_child) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((uintptr_t) first_child % sizeof(int32_t) || (uintptr_t) coords % sizeof(int32_t))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "first_child and coords must be 4-byte aligned");
    const uint64_t n = ctx->oct.nodes;
    O2V_CHECK(hipSetDevice(ctx->device));
    const Span spans[] = {{"valid", valid, n}, {"full", full, n}, {"first_child", first_child, n * 4u}, {"coords", coords, n * 12u}};
    int rc;
    for (const Span &sp : spans)
        if (sp.p && (rc = check_device_range(ctx, fn, sp.p, sp.bytes, sp.what))) return rc;
    if ((rc = refuse_overlap(ctx, fn, spans, 4))) return rc;
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->oct_write_times.mark(0, s));
    O2V_CHECK(hipMemcpyAsync(valid, ctx->d_oct_valid.ptr, n, hipMemcpyDeviceToDevice, s));
    O2V_CHECK(hipMemcpyAsync(full, ctx->d_oct_full.ptr, n, hipMemcpyDeviceToDevice, s));
    O2V_CHECK(hipMemcpyAsync(first_child, ctx->d_oct_first.ptr, n * 4u, hipMemcpyDeviceToDevice, s));
    if (coords) O2V_CHECK(hipMemcpyAsync(coords, ctx->d_oct_coords.ptr, n * 12u, hipMemcpyDeviceToDevice, s));
    if ((rc = finish_stages(ctx, ctx->oct_write_times))) return rc;
    ctx->oct_times.ms[3] = ctx->oct_write_times.ms[0];
    return O2V_HIP_OK;
}

int o2v_hip_octree_lookup(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, uint64_t n_nodes, uint32_t depth,
                          uint32_t flags, const int32_t *points, uint64_t n, int32_t *out)
{
    static const char fn[] = "o2v_hip_octree_lookup";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    OctTree t{};
    Span spans[5] = {};
    int rc;
    if ((rc = oct_tree(ctx, fn, valid, full, first_child, n_nodes, depth, flags, &t, spans + 1))) return rc;
    if (n > kMaxInt32) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 2^31 - 1 points");
    if (n == 0) return O2V_HIP_OK;
    if (!points || !out) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((uintptr_t) points % sizeof(int32_t) || (uintptr_t) out % sizeof(int32_t)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "points and out must be 4-byte aligned");
    spans[0] = Span{"out", out, n * 16u}, spans[4] = Span{"points", points, n * 12u};
    if ((rc = check_device_range(ctx, fn, points, n * 12u, "points")) || (rc = check_device_range(ctx, fn, out, n * 16u, "out")) ||
        (rc = refuse_overlap(ctx, fn, spans, 1)))
        return rc;
    hipStream_t s = ctx->stream;
    O2V_LAUNCH("k_oct_lookup", s, k_oct_lookup, dim3(stream_grid(ctx, n, 8u)), dim3(kBlock), 0, s, t, points, n, out);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipStreamSynchronize(s));
    return O2V_HIP_OK;
}

int o2v_hip_octree_to_dense(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, uint64_t n_nodes, uint32_t depth,
                            uint32_t flags, const uint32_t origin[3], const uint32_t dims[3], uint8_t *out, const uint64_t out_strides[3])
{
    static const char fn[] = "o2v_hip_octree_to_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    OctTree t{};
    Span spans[4] = {};
    int rc;
    if ((rc = oct_tree(ctx, fn, valid, full, first_child, n_nodes, depth, flags, &t, spans + 1))) return rc;
    if (!origin) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((rc = grid_given(ctx, fn, out, out_strides, dims))) return rc;
    if ((rc = axis_limit(ctx, fn, dims, origin, 1ull << 32, "origin + dims is above 2^32 along an axis"))) return rc;
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2];
    if (voxels > kMaxInt32) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, std::to_string(voxels) + " voxels: a box holds at most 2^31 - 1");
    const OutGrid outs[] = {{"out", out, out_strides, 1u}};
    if ((rc = check_outputs(ctx, fn, outs, dims, spans)) || (rc = refuse_overlap(ctx, fn, spans, 1))) return rc;
    OctDense d{};
    d.blocks = 1;
    for (int a = 0; a < 3; ++a) {
        d.o[a] = origin[a], d.n[a] = dims[a], d.b0[a] = origin[a] >> 1;
        d.nb[a] = (uint32_t) ((((uint64_t) origin[a] + dims[a] - 1u) >> 1) - d.b0[a] + 1u);
        d.blocks *= d.nb[a];
    }
    d.s0 = out_strides[0], d.s1 = out_strides[1], d.s2 = out_strides[2];
    hipStream_t s = ctx->stream;
    O2V_LAUNCH("k_oct_dense", s, k_oct_dense, dim3(stream_grid(ctx, d.blocks, 8u)), dim3(kBlock), 0, s, t, d, out);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipStreamSynchronize(s));
    return O2V_HIP_OK;
}

int o2v_hip_octree_times(const o2v_hip_ctx *ctx, float out_ms[4]) { return ctx ? ctx->oct_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"
