// Host side of K8 and K15 (o2v_dev_k8_distance.hpp, o2v_dev_k15_nearest.hpp): they share the envelope stacks and their geometry.

// ---- K8: the distance transform of a label grid ------------------------------------------------------------------------

namespace {

// Lanes of an envelope pass, one line each at a time: as many as the pass has lines, at most 2^17 (8 waves per CU of the
// MI355X).  The pass's stacks take slots x (its line length) entries of the scratch.
constexpr uint64_t kDistMaxSlots = 1u << 17;

uint64_t dist_slots(uint64_t lines) { return std::min<uint64_t>(lines, kDistMaxSlots); }

// The three passes of K8 and K15 over a grid: the workgroups of pass x (four rows each, in turns), and passes y and z each with
// its own slots (the stride of its stacks) and workgroups; the lanes of the last block past the slots have no line.
struct DistPasses {
    uint64_t sy, sz;
    dim3 gx, gy, gz;
};

DistPasses dist_passes(const o2v_hip_ctx *ctx, const uint32_t dims[3])
{
    DistPasses p;
    const uint64_t rows = (uint64_t) dims[1] * dims[2];
    p.sy = dist_slots((uint64_t) dims[0] * dims[2]), p.sz = dist_slots((uint64_t) dims[0] * dims[1]);
    p.gx = dim3((uint32_t) std::min<uint64_t>((uint64_t) ctx->num_cus * 8u, (rows + 3u) / 4u));
    p.gy = dim3((uint32_t) ((p.sy + kBlock - 1) / kBlock)), p.gz = dim3((uint32_t) ((p.sz + kBlock - 1) / kBlock));
    return p;
}

// A squared distance across the grid is one int32 below the "no seed" value.
int dist2_limit(o2v_hip_ctx *ctx, const char *fn, const uint32_t dims[3])
{
    uint64_t d2max = 0;
    for (int a = 0; a < 3; ++a) d2max += (uint64_t) (dims[a] - 1u) * (dims[a] - 1u);
    if (d2max > 0x7ffffffeull)
        return refuse(ctx, O2V_HIP_ERR_LIMIT, fn,
                      "(nx-1)^2 + (ny-1)^2 + (nz-1)^2 = " + std::to_string(d2max) + " does not fit below 2^31 - 1");
    return O2V_HIP_OK;
}

// A linear index of the grid's voxels is one int32 (K15's nearest, K21's centre list).
int voxel_index_limit(o2v_hip_ctx *ctx, const char *fn, const uint32_t dims[3])
{
    if ((unsigned __int128) dims[0] * dims[1] * dims[2] > kMaxInt32)
        return refuse(ctx, O2V_HIP_ERR_LIMIT, fn,
                      std::to_string(dims[0]) + " x " + std::to_string(dims[1]) + " x " + std::to_string(dims[2]) +
                          " voxels do not fit an int32 index (at most 2^31 - 1)");
    return O2V_HIP_OK;
}

// f(format) with a set grid's format as the template argument <Format> of dt_seed, an integral constant.
template <typename F>
void with_seed_format(uint32_t format, F &&f)
{
    if (format == O2V_HIP_GRID_BITS) return f(std::integral_constant<uint32_t, kRayBits>{});
    if (format == O2V_HIP_GRID_F32_BELOW) return f(std::integral_constant<uint32_t, kRayF32Below>{});
    return f(std::integral_constant<uint32_t, kRayU8>{});
}

// The envelope along y, then along z, over the int32 grid `grid` in place (K21's depth and core stages).
void dist_envelopes_yz(o2v_hip_ctx *ctx, int32_t *grid, const DtGrid &g, const DistPasses &p)
{
    hipStream_t s = ctx->stream;
    uint2 *const stack = ctx->d_dist_stack.ptr;
    O2V_LAUNCH("k_dist_envelope", s, k_dist_envelope<kDistY>, p.gy, dim3(kBlock), 0, s, grid, g, RaySource{}, stack, p.sy);
    O2V_LAUNCH("k_dist_envelope", s, k_dist_envelope<kDistZ>, p.gz, dim3(kBlock), 0, s, grid, g, RaySource{}, stack, p.sz);
}

}  // namespace

extern "C" {

uint64_t o2v_hip_distance_scratch_bytes(const uint32_t dims[3], uint32_t format)
{
    (void) format;   // (both formats use the same stacks)
    if (!dims || !dims[0] || !dims[1] || !dims[2]) return 0;
    const uint64_t y = dist_slots((uint64_t) dims[0] * dims[2]) * dims[1], z = dist_slots((uint64_t) dims[0] * dims[1]) * dims[2];
    return std::max(y, z) * sizeof(uint2);
}

int o2v_hip_distance_dense(o2v_hip_ctx *ctx, const void *labels, const uint64_t label_strides[3], void *dst, uint32_t format,
                           const uint64_t dst_strides[3], const uint32_t dims[3])
{
    static const char fn[] = "o2v_hip_distance_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!labels || !label_strides || !dst || !dst_strides || !dims || format > O2V_HIP_DIST_SDF_F32)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument or unknown format");
    if (!dims[0] || !dims[1] || !dims[2]) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "zero dims");
    int rc;
    if ((rc = dist2_limit(ctx, fn, dims))) return rc;
    O2V_CHECK(hipSetDevice(ctx->device));
    // (one output, and the overlap named with the labels first: not check_outputs and refuse_overlap, which name the written span first)
    uint64_t lbytes = 0, dbytes = 0;
    if ((rc = check_grid(ctx, fn, "labels", labels, dims, label_strides, 1u, false, &lbytes)) ||
        (rc = check_grid(ctx, fn, "dst", dst, dims, dst_strides, 4u, true, &dbytes)))
        return rc;
    if (ranges_overlap(labels, lbytes, dst, dbytes)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "labels and dst overlap");
    if ((rc = grow_scratch(ctx, ctx->d_dist_stack, o2v_hip_distance_scratch_bytes(dims, format) / sizeof(uint2), fn, "scratch")))
        return rc;
    hipStream_t s = ctx->stream;
    const DtGrid g{dst_strides[0], dst_strides[1], dst_strides[2], dims[0], dims[1], dims[2]};
    const RaySource lab = ray_source(labels, label_strides, 0.f);
    int32_t *const out = static_cast<int32_t *>(dst);
    uint2 *const stack = ctx->d_dist_stack.ptr;
    const DistPasses p = dist_passes(ctx, dims);
    O2V_CHECK(ctx->dist_times.mark(0, s));
    O2V_LAUNCH("k_dist_x", s, k_dist_x, p.gx, dim3(kBlock), 0, s, lab, out, g);
    O2V_CHECK(ctx->dist_times.mark(1, s));
    O2V_LAUNCH("k_dist_envelope", s, k_dist_envelope<kDistY>, p.gy, dim3(kBlock), 0, s, out, g, lab, stack, p.sy);
    O2V_CHECK(ctx->dist_times.mark(2, s));
    if (format == O2V_HIP_DIST_SQ_I32)
        O2V_LAUNCH("k_dist_envelope", s, k_dist_envelope<kDistZ>, p.gz, dim3(kBlock), 0, s, out, g, lab, stack, p.sz);
    else
        O2V_LAUNCH("k_dist_envelope", s, k_dist_envelope<kDistZSdf>, p.gz, dim3(kBlock), 0, s, out, g, lab, stack, p.sz);
    O2V_CHECK(hipGetLastError());
    return finish_stages(ctx, ctx->dist_times);
}

int o2v_hip_distance_times(const o2v_hip_ctx *ctx, float out_ms[3]) { return ctx ? ctx->dist_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"

// ---- K15: the nearest seed voxel of every voxel, and its value -----------------------------------------------------------

namespace {

constexpr uint32_t kNearFlagsKnown = O2V_HIP_NEAREST_SEED_ONE | O2V_HIP_NEAREST_VALUES_INSIDE;

}  // namespace

extern "C" {

uint64_t o2v_hip_nearest_scratch_bytes(const uint32_t dims[3]) { return o2v_hip_distance_scratch_bytes(dims, O2V_HIP_DIST_SQ_I32); }

int o2v_hip_nearest_dense(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                          uint32_t flags, int32_t *nearest, const uint64_t nearest_strides[3], int32_t *dist2, const uint64_t dist2_strides[3],
                          int32_t *values, const uint64_t value_strides[3], uint32_t max_dist2)
{
    static const char fn[] = "o2v_hip_nearest_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!nearest || !nearest_strides || (dist2 && !dist2_strides) || (values && !value_strides))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    SetGrid sg;
    int rc;
    if ((rc = set_grid_args(ctx, fn, grid, format, strides, dims, level, &sg))) return rc;
    if (flags & ~kNearFlagsKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if ((rc = voxel_index_limit(ctx, fn, dims)) || (rc = dist2_limit(ctx, fn, dims))) return rc;
    if (format != O2V_HIP_GRID_U8 && flags)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "SEED_ONE and VALUES_INSIDE need a U8 grid");
    // (the size limits stand before the look at the grid's memory: a box that is too large is refused as that, whatever it reaches)
    if ((rc = set_grid_memory(ctx, fn, &sg))) return rc;
    const OutGrid outs[] = {{"nearest", nearest, nearest_strides, 4u}, {"dist2", dist2, dist2_strides, 4u}, {"values", values, value_strides, 4u}};
    Span spans[4] = {{}, {}, {}, {"grid", grid, sg.bytes}};
    if ((rc = check_outputs(ctx, fn, outs, dims, spans)) || (rc = refuse_overlap(ctx, fn, spans, 3))) return rc;
    if ((rc = grow_scratch(ctx, ctx->d_dist_stack, o2v_hip_nearest_scratch_bytes(dims) / sizeof(uint2), fn, "scratch"))) return rc;
    hipStream_t s = ctx->stream;
    const NearGrid g{sg.source(), {nearest_strides[0], nearest_strides[1], nearest_strides[2], dims[0], dims[1], dims[2]}};
    NearOut o{};
    if (dist2) o.dist2 = dist2, o.e0 = dist2_strides[0], o.e1 = dist2_strides[1], o.e2 = dist2_strides[2];
    if (values) o.values = values, o.v0 = value_strides[0], o.v1 = value_strides[1], o.v2 = value_strides[2];
    o.max_dist2 = max_dist2;
    uint2 *const stack = ctx->d_dist_stack.ptr;
    const DistPasses p = dist_passes(ctx, dims);
    O2V_CHECK(ctx->near_times.mark(0, s));
    const auto scan_x = [&](auto fmt) { O2V_LAUNCH("k_near_x", s, k_near_x<decltype(fmt)::value>, p.gx, dim3(kBlock), 0, s, nearest, g); };
    if (flags & O2V_HIP_NEAREST_SEED_ONE) scan_x(std::integral_constant<uint32_t, kSeedU8One>{});   // (a U8 grid: checked above)
    else with_seed_format(format, scan_x);
    O2V_CHECK(ctx->near_times.mark(1, s));
    O2V_LAUNCH("k_near_envelope", s, (k_near_envelope<kNearY, kNearNoPaint>), p.gy, dim3(kBlock), 0, s, nearest, g, o, stack, p.sy);
    O2V_CHECK(ctx->near_times.mark(2, s));
    if (!values)
        O2V_LAUNCH("k_near_envelope", s, (k_near_envelope<kNearZ, kNearNoPaint>), p.gz, dim3(kBlock), 0, s, nearest, g, o, stack, p.sz);
    else if (flags & O2V_HIP_NEAREST_VALUES_INSIDE)
        O2V_LAUNCH("k_near_envelope", s, (k_near_envelope<kNearZ, kNearPaintInside>), p.gz, dim3(kBlock), 0, s, nearest, g, o, stack, p.sz);
    else
        O2V_LAUNCH("k_near_envelope", s, (k_near_envelope<kNearZ, kNearPaint>), p.gz, dim3(kBlock), 0, s, nearest, g, o, stack, p.sz);
    O2V_CHECK(hipGetLastError());
    return finish_stages(ctx, ctx->near_times);
}

int o2v_hip_nearest_times(const o2v_hip_ctx *ctx, float out_ms[3]) { return ctx ? ctx->near_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"
