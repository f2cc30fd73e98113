// Host side of K19 (o2v_dev_k19_label_stats.hpp).

// ---- K19: per-label statistics of a dense grid -------------------------------------------------------------------------------

namespace {

constexpr uint32_t kLsMaxExtent = 65536;           // origin + dims per axis: a coordinate is below 2^16 ...
constexpr uint64_t kLsMaxVoxels = 0x7fffffffull;   // ... and there are fewer than 2^31 voxels, so no sum reaches 2^63 (include/o2v_hip.h)
constexpr uint32_t kLsMaxLabels = 0x7ffffffeu;     // n_labels + 1 rows, the highest value an int32
constexpr uint32_t kLsWhichKnown = O2V_HIP_STATS_BOX | O2V_HIP_STATS_SUMS | O2V_HIP_STATS_MOMENTS | O2V_HIP_STATS_FACES;

static_assert(kLsI32 == O2V_HIP_LABELS_I32 && kLsU8 == O2V_HIP_LABELS_U8 && kLsBox == O2V_HIP_STATS_BOX && kLsSums == O2V_HIP_STATS_SUMS &&
                  kLsMoments == O2V_HIP_STATS_MOMENTS && kLsFaces == O2V_HIP_STATS_FACES && kLsCols == O2V_HIP_STATS_COLUMNS,
              "one set of formats, bits and columns for the callers and the kernel");

}  // namespace

extern "C" {

int o2v_hip_label_stats(o2v_hip_ctx *ctx, const void *labels, uint32_t format, const uint64_t strides[3], const uint32_t dims[3],
                        const uint32_t origin[3], uint32_t n_labels, uint32_t which, int64_t *table, uint64_t *out_outside)
{
    static const char fn[] = "o2v_hip_label_stats";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    const Switches sw = read_switches();
    if (!origin || !table || !out_outside) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    int rc;
    if ((rc = grid_given(ctx, fn, labels, strides, dims))) return rc;
    if (format != O2V_HIP_LABELS_I32 && format != O2V_HIP_LABELS_U8)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown format " + std::to_string(format));
    if (which & ~kLsWhichKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown bits in which = " + std::to_string(which));
    if (format == O2V_HIP_LABELS_U8 && n_labels > 255u)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "n_labels " + std::to_string(n_labels) + " is above 255, the highest value of a U8 grid");
    if ((uintptr_t) table % sizeof(int64_t) || (format == O2V_HIP_LABELS_I32 && (uintptr_t) labels % sizeof(int32_t)))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "table must be 8-byte aligned and an I32 grid 4-byte aligned");
    if ((rc = axis_limit(ctx, fn, dims, origin, kLsMaxExtent, "origin + dims is above 65 536 along an axis"))) return rc;
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2];   // (below 2^48)
    if (voxels > kLsMaxVoxels) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, std::to_string(voxels) + " voxels: the sums hold at most 2^31 - 1");
    if (n_labels > kLsMaxLabels) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "n_labels is above 2^31 - 2");
    // (the limits stand before the look at the memory: a box that is too large is refused as that, whatever it reaches)
    O2V_CHECK(hipSetDevice(ctx->device));
    const uint32_t elem = format == O2V_HIP_LABELS_I32 ? 4u : 1u;
    const uint64_t rows = (uint64_t) n_labels + 1u, tbytes = rows * kLsCols * sizeof(int64_t);
    uint64_t gbytes = 0;
    if ((rc = check_grid(ctx, fn, "labels", labels, dims, strides, elem, false, &gbytes)) || (rc = check_device_range(ctx, fn, table, tbytes, "table")))
        return rc;
    const Span spans[] = {{"table", table, tbytes}, {"labels", labels, gbytes}};
    if ((rc = refuse_overlap(ctx, fn, spans, 1))) return rc;
    if ((rc = grow_scratch(ctx, ctx->d_ls_ctr, 1u, fn, "counter")) || (rc = grow_scratch(ctx, ctx->h_ls_ctr, 1u, fn, "counter"))) return rc;
    const uint32_t lane = format == O2V_HIP_LABELS_I32 ? ls_lane<kLsI32>() : ls_lane<kLsU8>();
    LsGrid g{};
    for (int a = 0; a < 3; ++a) g.n[a] = dims[a], g.o[a] = origin[a];
    g.n_labels = n_labels, g.which = which;
    g.cpr = (dims[0] + lane - 1u) / lane;
    g.chunks = (uint32_t) ((uint64_t) g.cpr * dims[1] * dims[2]);   // (at most the voxels)
    g.groups = (g.chunks + kBlock - 1u) / kBlock;
    // a range of groups per workgroup, and no more workgroups than keep every CU's LDS full (17.5 KB each)
    const uint32_t max_blocks = std::max(1u, (uint32_t) ctx->num_cus * 8u);
    g.per_wg = (g.groups + max_blocks - 1u) / max_blocks;
    const dim3 blocks((g.groups + g.per_wg - 1u) / g.per_wg);
    g.table = sw.ls_no_table ? 0u : 1u;
    const bool vec = rows_aligned16(labels, strides, elem);
    const RaySource src = ray_source(labels, strides, 0.f);
    long long *const tab = reinterpret_cast<long long *>(table);
    unsigned long long *const ctr = ctx->d_ls_ctr.ptr;
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->ls_times.mark(0, s));
    O2V_LAUNCH("k_ls_init", s, k_ls_init, dim3(stream_grid(ctx, rows * kLsCols, 8u)), dim3(kBlock), 0, s, tab, rows, which, ctr);
    O2V_CHECK(ctx->ls_times.mark(1, s));
    with_flag(format == O2V_HIP_LABELS_I32, [&](auto i32) {
        with_flag(vec, [&](auto v) {
            with_flag((which & O2V_HIP_STATS_FACES) != 0, [&](auto faces) {
                constexpr uint32_t fmt = decltype(i32)::value ? kLsI32 : kLsU8;
                O2V_LAUNCH("k_label_stats", s, (k_label_stats<fmt, decltype(v)::value, decltype(faces)::value>), blocks, dim3(kBlock), 0, s, src, g, tab, ctr);
            });
        });
    });
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(ctx->ls_times.mark(2, s));
    O2V_CHECK(hipMemcpyAsync(ctx->h_ls_ctr.ptr, ctr, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(ctx->ls_times.finish());
    *out_outside = ctx->h_ls_ctr.ptr[0];
    return O2V_HIP_OK;
}

int o2v_hip_label_stats_times(const o2v_hip_ctx *ctx, float out_ms[2]) { return ctx ? ctx->ls_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"
