// Host side of K30 (o2v_dev_k30_dag.hpp): the sparse voxel DAG of an octree.  Its refusals, their order and their wording follow
// K26's, so it comes after o2v_dev_host_k26_octree.hpp (kOctFlagsKnown, kOctCollapse, the box of 2^3 blocks of o2v_hip_octree_to_dense).

namespace {

constexpr uint32_t kDagNodeBytes = 1u + 1u + 4u;   // valid, full, first_child
constexpr uint32_t kDagPointerBytes = 4u + 4u;     // child, skip
constexpr uint64_t kDagLeafTable = 256u;           // the entries of level D - 1's table: a smallest index per value of `valid`

// the entries of the table of a level of n nodes: a power of two, at least twice the nodes
uint64_t dag_slots(uint64_t n)
{
    uint64_t slots = kDagLeafTable;
    while (slots < 2u * n) slots *= 2u;
    return slots;
}

// The levels of a tree as its caller gives them: where each begins, the widest, the widest above level D - 1.
struct DagPlan {
    uint64_t first[kOctMaxDepth + 2u] = {};
    uint64_t nodes = 0, widest = 1, widest_above = 0;
};

DagPlan dag_plan(const uint64_t level_counts[16], uint32_t depth)
{
    DagPlan p;
    for (uint32_t l = 0; l < depth; ++l) {
        p.first[l + 1u] = p.first[l] + level_counts[l];
        p.widest = std::max(p.widest, level_counts[l]);
        if (l + 1u < depth) p.widest_above = std::max(p.widest_above, level_counts[l]);
    }
    p.first[depth + 1u] = p.nodes = p.first[depth];
    return p;
}

// the level counts of a tree of n_nodes nodes and this depth: below 2^31 each, the root alone at level 0, nothing from level depth on
bool dag_counts_fit(const uint64_t level_counts[16], uint32_t depth, uint64_t n_nodes)
{
    uint64_t sum = 0;
    for (uint32_t l = 0; l < kOctMaxDepth; ++l) {
        if (level_counts[l] > (1ull << 32) || (l >= depth && level_counts[l])) return false;
        sum += level_counts[l];
    }
    return sum == n_nodes && level_counts[0] == 1u;
}

// The DAG arguments of the two queries, checked: *d as the kernels take it, spans[0, 5) its arrays (skip: not there if null).
int dag_args(o2v_hip_ctx *ctx, const char *fn, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, const int32_t *child,
             const int32_t *skip, uint64_t n_nodes, uint64_t n_pointers, uint32_t depth, uint32_t flags, OctDag *d, Span *spans)
{
    if (!valid || !full || !first_child || (!child && n_pointers)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if (flags & ~kOctFlagsKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if (depth < 1u || depth > kOctMaxDepth) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "depth must be 1 ... 16, not " + std::to_string(depth));
    if (n_nodes == 0) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "n_nodes is 0: a DAG has its root");
    if (n_nodes > kMaxInt32) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 2^31 - 1 nodes");
    if (n_pointers > kMaxInt32) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 2^31 - 1 pointers");
    if ((uintptr_t) first_child % sizeof(int32_t) || (uintptr_t) child % sizeof(int32_t) || (uintptr_t) skip % sizeof(int32_t))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "first_child, child and skip must be 4-byte aligned");
    spans[0] = Span{"valid", valid, n_nodes}, spans[1] = Span{"full", full, n_nodes}, spans[2] = Span{"first_child", first_child, n_nodes * 4u};
    spans[3] = Span{"child", child, n_pointers * 4u}, spans[4] = Span{"skip", skip, n_pointers * 4u};
    *d = OctDag{valid, full, first_child, child, skip, (uint32_t) n_nodes, (uint32_t) n_pointers, depth, (flags & kOctCollapse) ? 1u : 0u, dag_skips(skip, n_pointers)};
    return O2V_HIP_OK;
}

// ... and their memory, behind the call's own argument and overlap checks
int dag_memory(o2v_hip_ctx *ctx, const char *fn, const Span *spans)
{
    O2V_CHECK(hipSetDevice(ctx->device));
    for (int i = 0; i < 5; ++i)
        if (spans[i].p && spans[i].bytes)
            if (int rc = check_device_range(ctx, fn, spans[i].p, spans[i].bytes, spans[i].what)) return rc;
    return O2V_HIP_OK;
}

}  // namespace

extern "C" {

uint64_t o2v_hip_octree_dag_scratch_bytes(const uint64_t level_counts[16], uint32_t depth)
{
    if (!level_counts || depth < 1u || depth > kOctMaxDepth) return 0;
    uint64_t n = 0;
    for (uint32_t l = 0; l < depth; ++l) n += level_counts[l];
    if (!dag_counts_fit(level_counts, depth, n) || n > kMaxInt32) return 0;
    const DagPlan p = dag_plan(level_counts, depth);
    // per tree node its class and its listed voxels, the widest level's scans and block offsets, the table, the counters; and the
    // most a DAG takes: a node per tree node, a pointer per tree node but the root
    return 8u * p.nodes + 4u * p.widest + 8u * (p.widest / kBlock + 2u) + 4u * dag_slots(p.widest_above) + 8u * kDagMeta + (uint64_t) kDagNodeBytes * p.nodes +
           (uint64_t) kDagPointerBytes * (p.nodes - 1u);
}

int o2v_hip_octree_dag_build(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, uint64_t n_nodes, uint32_t depth,
                             uint32_t flags, const uint64_t level_counts[16], uint64_t out_level_counts[16], uint64_t *out_nodes, uint64_t *out_pointers)
{
    static const char fn[] = "o2v_hip_octree_dag_build";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    ctx->dag.valid = false;
    if (!valid || !full || !first_child || !level_counts || !out_level_counts || !out_nodes || !out_pointers)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if (flags & ~kOctFlagsKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if (depth < 1u || depth > kOctMaxDepth) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "depth must be 1 ... 16, not " + std::to_string(depth));
    if (!dag_counts_fit(level_counts, depth, n_nodes))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "level_counts must hold 1 for the root, 0 from level " + std::to_string(depth) + " on and add up to n_nodes = " +
                                                            std::to_string(n_nodes));
    if (n_nodes > kMaxInt32) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 2^31 - 1 nodes");
    if ((uintptr_t) first_child % sizeof(int32_t)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "first_child must be 4-byte aligned");
    O2V_CHECK(hipSetDevice(ctx->device));
    int rc;
    if ((rc = check_device_range(ctx, fn, valid, n_nodes, "valid")) || (rc = check_device_range(ctx, fn, full, n_nodes, "full")) ||
        (rc = check_device_range(ctx, fn, first_child, n_nodes * 4u, "first_child")))
        return rc;
    const uint32_t collapsed = (flags & kOctCollapse) ? 1u : 0u, D = depth;
    const DagPlan plan = dag_plan(level_counts, D);
    const uint64_t slots = dag_slots(plan.widest_above);
    if ((rc = grow_scratch(ctx, ctx->d_dag_cls, plan.nodes, fn, "classes")) || (rc = grow_scratch(ctx, ctx->d_dag_listed, plan.nodes, fn, "listed voxels")) ||
        (rc = grow_scratch(ctx, ctx->d_dag_num, plan.widest, fn, "scans")) || (rc = grow_scratch(ctx, ctx->d_dag_tab, slots, fn, "table")) ||
        (rc = grow_scratch(ctx, ctx->d_dag_boff, (plan.widest + kBlock - 1u) / kBlock + 1u, fn, "block offsets")) ||
        (rc = grow_scratch(ctx, ctx->d_dag_meta, kDagMeta, fn, "counters")) || (rc = grow_scratch(ctx, ctx->h_dag_meta, kDagMeta, fn, "counters")))
        return rc;
    const DagWork w{ctx->d_dag_cls.ptr, ctx->d_dag_listed.ptr, ctx->d_dag_num.ptr};
    uint32_t *const tab = ctx->d_dag_tab.ptr;
    unsigned long long *const boff = ctx->d_dag_boff.ptr, *const meta = ctx->d_dag_meta.ptr, *const h_meta = ctx->h_dag_meta.ptr;
    hipStream_t s = ctx->stream;
    const auto level = [&](uint32_t l) { return DagLevel{valid, full, first_child, w.cls, plan.first[l], plan.first[l + 1u], plan.first[l + 2u], collapsed}; };
    const auto scan_blocks = [&](uint64_t n) { return std::max<uint64_t>(1u, (n + kBlock - 1u) / kBlock); };
    const auto scan_grid = [&](uint64_t n_blocks) { return dim3((uint32_t) std::min<uint64_t>(n_blocks, (uint64_t) ctx->num_cus * 8u)); };

    // bottom up, level by level: the representative of every node, the rank of its class, its listed voxels.  No host wait between.
    O2V_CHECK(hipMemsetAsync(meta, 0, kDagMeta * sizeof(unsigned long long), s));
    O2V_CHECK(ctx->dag_times.mark(0, s));
    for (uint32_t l = D; l-- > 0u;) {
        const uint32_t n = (uint32_t) level_counts[l], leaf = l + 1u == D ? 1u : 0u;
        if (n) {
            const DagLevel L = level(l);
            const dim3 per_node(stream_grid(ctx, n, 8u));
            if (leaf) {
                O2V_CHECK(hipMemsetAsync(tab, 0xff, kDagLeafTable * sizeof(uint32_t), s));
                O2V_LAUNCH("k_dag_leaf_min", s, k_dag_leaf_min, dim3(stream_grid(ctx, (n + 7u) / 8u, 8u)), dim3(kBlock), 0, s, valid, L.first, n, tab);
                O2V_LAUNCH("k_dag_leaf_rep", s, k_dag_leaf_rep, per_node, dim3(kBlock), 0, s, valid, L.first, n, tab, w.cls);
            } else {
                const uint32_t mask = (uint32_t) (dag_slots(n) - 1u);
                O2V_CHECK(hipMemsetAsync(tab, 0xff, ((uint64_t) mask + 1u) * sizeof(uint32_t), s));
                O2V_LAUNCH("k_dag_insert", s, k_dag_insert, per_node, dim3(kBlock), 0, s, L, n, tab, mask, meta + kDagFlag);
                O2V_LAUNCH("k_dag_find", s, k_dag_find, per_node, dim3(kBlock), 0, s, L, n, tab, mask, w.cls, meta + kDagFlag);
            }
            const uint64_t n_blocks = scan_blocks(n);
            O2V_LAUNCH("k_dag_flags", s, k_dag_flags, scan_grid(n_blocks), dim3(kBlock), 0, s, w.cls, L.first, n, n_blocks, w.num, boff);
            O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, boff, n_blocks, meta + kDagCount + l);
            O2V_LAUNCH("k_dag_ids", s, k_dag_ids, per_node, dim3(kBlock), 0, s, L, n, leaf, w.num, boff, w, meta + kDagPtr + l);
        }
        if (leaf) O2V_CHECK(ctx->dag_times.mark(1, s));
    }
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(ctx->dag_times.mark(2, s));
    // the wait of the build: the classes and pointers per level, which size the DAG, and with them the flag
    O2V_CHECK(hipMemcpyAsync(h_meta, meta, kDagMeta * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    if (h_meta[kDagFlag] & kDagBadTree)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "valid, full and first_child are not a tree of these level counts: a stored child lies outside the next level");
    if (h_meta[kDagFlag]) return refuse(ctx, O2V_HIP_ERR_HIP, fn, "a level's table took no more keys");   // (never: it has twice the level's nodes)
    uint64_t node0[kOctMaxDepth + 1u] = {}, ptr0[kOctMaxDepth + 1u] = {};
    for (uint32_t l = 0; l < D; ++l) node0[l + 1u] = node0[l] + h_meta[kDagCount + l], ptr0[l + 1u] = ptr0[l] + h_meta[kDagPtr + l];
    const uint64_t M = node0[D], P = ptr0[D];
    if (M > plan.nodes || P > plan.nodes) return refuse(ctx, O2V_HIP_ERR_HIP, fn, "more classes or pointers than nodes");   // (never)
    if ((rc = grow_scratch(ctx, ctx->d_dag_valid, M, fn, "nodes")) || (rc = grow_scratch(ctx, ctx->d_dag_full, M, fn, "nodes")) ||
        (rc = grow_scratch(ctx, ctx->d_dag_first, M, fn, "nodes")) || (rc = grow_scratch(ctx, ctx->d_dag_child, P, fn, "pointers")) ||
        (rc = grow_scratch(ctx, ctx->d_dag_skip, P, fn, "pointers")))
        return rc;
    const DagOut out{ctx->d_dag_valid.ptr, ctx->d_dag_full.ptr, ctx->d_dag_first.ptr, ctx->d_dag_child.ptr, ctx->d_dag_skip.ptr, M, P};

    // the output: per level the representatives' pointers scanned, then their nodes and pointers written
    O2V_CHECK(hipEventRecord(ctx->dag_times.ev[3], s));
    for (uint32_t l = 0; l < D; ++l) {
        const uint32_t n = (uint32_t) level_counts[l], leaf = l + 1u == D ? 1u : 0u;
        if (!n) continue;
        const DagLevel L = level(l);
        const uint64_t n_blocks = scan_blocks(n);
        if (!leaf) {
            O2V_LAUNCH("k_dag_ptr_count", s, k_dag_ptr_count, scan_grid(n_blocks), dim3(kBlock), 0, s, L, n, n_blocks, w.num, boff);
            O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, boff, n_blocks, meta + kDagPtrScan + l);
        }
        O2V_LAUNCH("k_dag_emit", s, k_dag_emit, dim3(stream_grid(ctx, n, 8u)), dim3(kBlock), 0, s, L, n, leaf, w.num, boff, w.listed, node0[l], node0[l + 1u],
                   ptr0[l], out);
    }
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipEventRecord(ctx->dag_times.ev[4], s));
    O2V_CHECK(hipMemcpyAsync(h_meta, meta, kDagMeta * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(ctx->dag_times.elapsed(0, 1, ctx->dag_times.ms[0]));
    O2V_CHECK(ctx->dag_times.elapsed(1, 2, ctx->dag_times.ms[1]));
    O2V_CHECK(ctx->dag_times.elapsed(3, 4, ctx->dag_times.ms[2]));
    ctx->dag_times.ms[3] = 0.f;
    for (uint32_t l = 0; l + 1u < D; ++l)
        if (h_meta[kDagPtrScan + l] != h_meta[kDagPtr + l])
            return refuse(ctx, O2V_HIP_ERR_HIP, fn, "level " + std::to_string(l) + ": the scan found " + std::to_string(h_meta[kDagPtrScan + l]) +
                                                        " pointers, the sum " + std::to_string(h_meta[kDagPtr + l]));
    ctx->dag.nodes = M, ctx->dag.pointers = P;
    ctx->dag.valid = true;
    for (uint32_t l = 0; l < kOctMaxDepth; ++l) out_level_counts[l] = l < D ? h_meta[kDagCount + l] : 0u;
    *out_nodes = M;
    *out_pointers = P;
    return O2V_HIP_OK;
}

int o2v_hip_octree_dag_write(o2v_hip_ctx *ctx, uint8_t *valid, uint8_t *full, int32_t *first_child, int32_t *child, int32_t *skip)
{
    static const char fn[] = "o2v_hip_octree_dag_write";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!ctx->dag.valid) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "no o2v_hip_octree_dag_build");
    const uint64_t M = ctx->dag.nodes, P = ctx->dag.pointers;
    if (!valid || !full || !first_child || (!child && P)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((uintptr_t) first_child % sizeof(int32_t) || (uintptr_t) child % sizeof(int32_t) || (uintptr_t) skip % sizeof(int32_t))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "first_child, child and skip must be 4-byte aligned");
    const Span spans[] = {{"valid", valid, M}, {"full", full, M}, {"first_child", first_child, M * 4u}, {"child", child, P * 4u}, {"skip", skip, P * 4u}};
    int rc;
    if ((rc = refuse_overlap(ctx, fn, spans, 5)) || (rc = dag_memory(ctx, fn, spans))) return rc;
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->dag_write_times.mark(0, s));
    O2V_CHECK(hipMemcpyAsync(valid, ctx->d_dag_valid.ptr, M, hipMemcpyDeviceToDevice, s));
    O2V_CHECK(hipMemcpyAsync(full, ctx->d_dag_full.ptr, M, hipMemcpyDeviceToDevice, s));
    O2V_CHECK(hipMemcpyAsync(first_child, ctx->d_dag_first.ptr, M * 4u, hipMemcpyDeviceToDevice, s));
    if (P) O2V_CHECK(hipMemcpyAsync(child, ctx->d_dag_child.ptr, P * 4u, hipMemcpyDeviceToDevice, s));
    if (P && skip) O2V_CHECK(hipMemcpyAsync(skip, ctx->d_dag_skip.ptr, P * 4u, hipMemcpyDeviceToDevice, s));
    if ((rc = finish_stages(ctx, ctx->dag_write_times))) return rc;
    ctx->dag_times.ms[3] = ctx->dag_write_times.ms[0];
    return O2V_HIP_OK;
}

int o2v_hip_octree_dag_lookup(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, const int32_t *child,
                              const int32_t *skip, uint64_t n_nodes, uint64_t n_pointers, uint32_t depth, uint32_t flags, const int32_t *points, uint64_t n,
                              int32_t *out)
{
    static const char fn[] = "o2v_hip_octree_dag_lookup";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    OctDag d{};
    Span spans[7] = {};
    int rc;
    if ((rc = dag_args(ctx, fn, valid, full, first_child, child, skip, n_nodes, n_pointers, depth, flags, &d, spans + 1))) return rc;
    if (n > kMaxInt32) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 2^31 - 1 points");
    if (n && (!points || !out)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((uintptr_t) points % sizeof(int32_t) || (uintptr_t) out % sizeof(int32_t)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "points and out must be 4-byte aligned");
    spans[0] = Span{"out", out, n * 16u}, spans[6] = Span{"points", points, n * 12u};
    if ((rc = refuse_overlap(ctx, fn, spans, 1)) || (rc = dag_memory(ctx, fn, spans + 1))) return rc;
    if (n == 0) return O2V_HIP_OK;
    if ((rc = check_device_range(ctx, fn, points, n * 12u, "points")) || (rc = check_device_range(ctx, fn, out, n * 16u, "out"))) return rc;
    hipStream_t s = ctx->stream;
    O2V_LAUNCH("k_dag_lookup", s, k_dag_lookup, dim3(stream_grid(ctx, n, 8u)), dim3(kBlock), 0, s, d, points, n, out);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipStreamSynchronize(s));
    return O2V_HIP_OK;
}

int o2v_hip_octree_dag_to_dense(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, const int32_t *child, uint64_t n_nodes,
                                uint64_t n_pointers, uint32_t depth, uint32_t flags, const uint32_t origin[3], const uint32_t dims[3], uint8_t *out,
                                const uint64_t out_strides[3])
{
    static const char fn[] = "o2v_hip_octree_dag_to_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    OctDag d{};
    Span spans[6] = {};
    int rc;
    if ((rc = dag_args(ctx, fn, valid, full, first_child, child, nullptr, n_nodes, n_pointers, depth, flags, &d, spans + 1))) return rc;
    if (!origin) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((rc = grid_given(ctx, fn, out, out_strides, dims))) return rc;
    if ((rc = axis_limit(ctx, fn, dims, origin, 1ull << 32, "origin + dims is above 2^32 along an axis"))) return rc;
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2];
    if (voxels > kMaxInt32) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, std::to_string(voxels) + " voxels: a box holds at most 2^31 - 1");
    if ((rc = dag_memory(ctx, fn, spans + 1))) return rc;
    const OutGrid outs[] = {{"out", out, out_strides, 1u}};
    if ((rc = check_outputs(ctx, fn, outs, dims, spans)) || (rc = refuse_overlap(ctx, fn, spans, 1))) return rc;
    OctDense b{};
    b.blocks = 1;
    for (int a = 0; a < 3; ++a) {
        b.o[a] = origin[a], b.n[a] = dims[a], b.b0[a] = origin[a] >> 1;
        b.nb[a] = (uint32_t) ((((uint64_t) origin[a] + dims[a] - 1u) >> 1) - b.b0[a] + 1u);
        b.blocks *= b.nb[a];
    }
    b.s0 = out_strides[0], b.s1 = out_strides[1], b.s2 = out_strides[2];
    hipStream_t s = ctx->stream;
    O2V_LAUNCH("k_dag_dense", s, k_dag_dense, dim3(stream_grid(ctx, b.blocks, 8u)), dim3(kBlock), 0, s, d, b, out);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipStreamSynchronize(s));
    return O2V_HIP_OK;
}

int o2v_hip_octree_dag_times(const o2v_hip_ctx *ctx, float out_ms[4]) { return ctx ? ctx->dag_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"
