// Host side of K31 (o2v_dev_k31_treeray.hpp): rays through a sparse voxel octree or DAG.  The tree and DAG arguments are checked by
// K26's oct_tree and K30's dag_args / dag_memory, the rays and outputs as o2v_hip_raycast checks them, so it comes after
// o2v_dev_host_k11_raycast.hpp (kRayMaxRays), o2v_dev_host_k26_octree.hpp and o2v_dev_host_k30_dag.hpp.

namespace {

// The rays and outputs of a cast, behind the source's own checks: t_max, the number of rays, then (for n != 0) null arguments,
// alignment, memory and overlaps.  spans[0, 3) are filled here (hit, t, voxel_index), the source's arrays lie behind them, the rays
// in the last two.  *go: there is something to launch.
template <size_t N>
int treeray_args(o2v_hip_ctx *ctx, const char *fn, const float *origins, const float *directions, uint64_t n, float t_max, int32_t *hit, float *t,
                 int32_t *voxel_index, Span (&spans)[N], bool *go)
{
    *go = false;
    if (!(t_max >= 0.f)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "t_max must be >= 0 or +inf");
    if (n > kRayMaxRays) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 2^31 - 1 rays");
    if (n == 0) return O2V_HIP_OK;
    if (!origins || !directions || !hit || !t) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((uintptr_t) origins % sizeof(float) || (uintptr_t) directions % sizeof(float) || (uintptr_t) hit % sizeof(int32_t) || (uintptr_t) t % sizeof(float) ||
        (uintptr_t) voxel_index % sizeof(int32_t))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "origins, directions, hit, t and voxel_index must be 4-byte aligned");
    spans[0] = Span{"hit", hit, n * 16u}, spans[1] = Span{"t", t, n * 4u}, spans[2] = Span{"voxel_index", voxel_index, n * 4u};
    spans[N - 2] = Span{"origins", origins, n * 12u}, spans[N - 1] = Span{"directions", directions, n * 12u};
    O2V_CHECK(hipSetDevice(ctx->device));
    for (const size_t k : {N - 2, N - 1, (size_t) 0, (size_t) 1, (size_t) 2})
        if (spans[k].p)
            if (int rc = check_device_range(ctx, fn, spans[k].p, spans[k].bytes, spans[k].what)) return rc;
    if (int rc = refuse_overlap(ctx, fn, spans, 3)) return rc;
    *go = true;
    return O2V_HIP_OK;
}

// the launch: a ray per lane; with the stack, (D - 1) entries of LDS per lane
template <class Src>
int treeray_launch(o2v_hip_ctx *ctx, const Src &src, uint32_t depth, bool stack, const float *origins, const float *directions, uint64_t n, float t_max,
                   int32_t *hit, float *t, int32_t *voxel_index)
{
    const dim3 blocks((uint32_t) ((n + kBlock - 1) / kBlock));
    const uint32_t lds = stack ? (depth - 1u) * kTreeRayEntryBytes * kBlock : 0u;
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->treeray_times.mark(0, s));
    with_flag(stack && depth > 1u, [&](auto on) {
        O2V_LAUNCH("k_tree_cast", s, (k_tree_cast<Src, decltype(on)::value>), blocks, dim3(kBlock), lds, s, origins, directions, n, t_max, src, hit, t, voxel_index);
    });
    O2V_CHECK(hipGetLastError());
    return finish_stages(ctx, ctx->treeray_times);
}

}  // namespace

extern "C" {

int o2v_hip_octree_raycast(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, uint64_t n_nodes, uint32_t depth,
                           uint32_t flags, const float *origins, const float *directions, uint64_t n, float t_max, int32_t *hit, float *t, int32_t *voxel_index)
{
    static const char fn[] = "o2v_hip_octree_raycast";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    // (the stage-times flag of the other octree calls is not taken here; everything else of the tree is oct_tree's to check)
    if (flags & ~kOctCollapse) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    TreeRayOct src{};
    Span spans[8] = {};
    int rc;
    bool go;
    if ((rc = oct_tree(ctx, fn, valid, full, first_child, n_nodes, depth, flags, &src.t, spans + 3))) return rc;
    if ((rc = treeray_args(ctx, fn, origins, directions, n, t_max, hit, t, voxel_index, spans, &go)) || !go) return rc;
    return treeray_launch(ctx, src, depth, !read_switches().treeray_no_stack, origins, directions, n, t_max, hit, t, voxel_index);
}

int o2v_hip_octree_dag_raycast(o2v_hip_ctx *ctx, const uint8_t *valid, const uint8_t *full, const int32_t *first_child, const int32_t *child,
                               const int32_t *skip, uint64_t n_nodes, uint64_t n_pointers, uint32_t depth, uint32_t flags, const float *origins,
                               const float *directions, uint64_t n, float t_max, int32_t *hit, float *t, int32_t *voxel_index)
{
    static const char fn[] = "o2v_hip_octree_dag_raycast";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (flags & ~kOctCollapse) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    TreeRayDag src{};
    Span spans[10] = {};
    int rc;
    bool go;
    if ((rc = dag_args(ctx, fn, valid, full, first_child, child, skip, n_nodes, n_pointers, depth, flags, &src.d, spans + 3)) ||
        (rc = dag_memory(ctx, fn, spans + 3)))
        return rc;
    if ((rc = treeray_args(ctx, fn, origins, directions, n, t_max, hit, t, voxel_index, spans, &go)) || !go) return rc;
    return treeray_launch(ctx, src, depth, !read_switches().treeray_no_stack, origins, directions, n, t_max, hit, t, voxel_index);
}

int o2v_hip_octree_raycast_times(const o2v_hip_ctx *ctx, float out_ms[1]) { return ctx ? ctx->treeray_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"
