// Host side of K25 (o2v_dev_k25_euler.hpp): the cell counts of a label grid.  It takes K19's formats and limits, so it comes after
// o2v_dev_host_k19_label_stats.hpp.

namespace {

static_assert(kEuCols == O2V_HIP_EULER_COLUMNS, "one set of columns for the callers and the kernel");

#ifndef O2V_EU_MAX_GROUPS
#define O2V_EU_MAX_GROUPS 8
#endif
constexpr uint32_t kEuMaxGroups = O2V_EU_MAX_GROUPS;   // groups of kBlock chunks that a workgroup takes at most

}  // namespace

extern "C" {

int o2v_hip_euler_stats(o2v_hip_ctx *ctx, const void *labels, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], uint32_t n_labels,
                        int64_t *table, uint64_t *out_outside)
{
    static const char fn[] = "o2v_hip_euler_stats";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    const Switches sw = read_switches();
    if (!table || !out_outside) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    int rc;
    if ((rc = grid_given(ctx, fn, labels, strides, dims))) return rc;
    if (format != O2V_HIP_LABELS_I32 && format != O2V_HIP_LABELS_U8)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown format " + std::to_string(format));
    if (format == O2V_HIP_LABELS_U8 && n_labels > 255u)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "n_labels " + std::to_string(n_labels) + " is above 255, the highest value of a U8 grid");
    if ((uintptr_t) table % sizeof(int64_t) || (format == O2V_HIP_LABELS_I32 && (uintptr_t) labels % sizeof(int32_t)))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "table must be 8-byte aligned and an I32 grid 4-byte aligned");
    if ((rc = axis_limit(ctx, fn, dims))) return rc;
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2];   // (below 2^48)
    if (voxels > kLsMaxVoxels) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, std::to_string(voxels) + " voxels: the grid holds at most 2^31 - 1");
    if (n_labels > kLsMaxLabels) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "n_labels is above 2^31 - 2");
    // (the limits stand before the look at the memory: a box that is too large is refused as that, whatever it reaches)
    O2V_CHECK(hipSetDevice(ctx->device));
    const uint32_t elem = format == O2V_HIP_LABELS_I32 ? 4u : 1u;
    const uint64_t rows = (uint64_t) n_labels + 1u, tbytes = rows * kEuCols * sizeof(int64_t);
    uint64_t gbytes = 0;
    if ((rc = check_grid(ctx, fn, "labels", labels, dims, strides, elem, false, &gbytes)) || (rc = check_device_range(ctx, fn, table, tbytes, "table")))
        return rc;
    const Span spans[] = {{"table", table, tbytes}, {"labels", labels, gbytes}};
    if ((rc = refuse_overlap(ctx, fn, spans, 1))) return rc;
    if ((rc = grow_scratch(ctx, ctx->d_eu_ctr, 1u, fn, "counter")) || (rc = grow_scratch(ctx, ctx->h_eu_ctr, 1u, fn, "counter"))) return rc;
    const uint32_t lane = format == O2V_HIP_LABELS_I32 ? ls_lane<kLsI32>() : ls_lane<kLsU8>();
    EuGrid g{};
    for (int a = 0; a < 3; ++a) g.n[a] = dims[a];
    g.n_labels = n_labels;
    g.cpr = (dims[0] + 1u + lane - 1u) / lane;
    g.rows_y = dims[1] + 1u;
    // cpr <= nx, and <= nx / 2 from nx = 4 on, so with at most 2^31 - 1 voxels and 2^16 along an axis the chunks stay below 2^32:
    // (ny + 1)(nz + 1) <= 2^31 + 2^17 lattice rows of one chunk for nx <= 3, (3 * 2^31 + 2^16) / 2 chunks above
    const uint64_t chunks = (uint64_t) g.cpr * g.rows_y * (dims[2] + 1u);
    if (chunks > 0xffffffffull) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 2^32 - 1 chunks of windows");   // (never, by the limits above)
    g.chunks = (uint32_t) chunks;
    g.groups = (uint32_t) ((chunks + kBlock - 1u) / kBlock);
    // a range of groups per workgroup: enough workgroups to fill every CU (8 of 15 KiB of LDS each), and ranges short enough
    // that the labels of one mostly find a slot in its table (kEuMaxGroups: DESIGN.md section 29)
    const uint32_t max_blocks = std::max(1u, (uint32_t) ctx->num_cus * 8u);
    g.per_wg = std::min((g.groups + max_blocks - 1u) / max_blocks, kEuMaxGroups);
    const dim3 blocks((g.groups + g.per_wg - 1u) / g.per_wg);
    g.table = sw.eu_no_table ? 0u : 1u;
    const bool vec = rows_aligned16(labels, strides, elem);
    const RaySource src = ray_source(labels, strides, 0.f);
    long long *const tab = reinterpret_cast<long long *>(table);
    unsigned long long *const ctr = ctx->d_eu_ctr.ptr;
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->eu_times.mark(0, s));
    O2V_LAUNCH("k_eu_init", s, k_eu_init, dim3(stream_grid(ctx, rows * kEuCols, 8u)), dim3(kBlock), 0, s, tab, rows, ctr);
    O2V_CHECK(ctx->eu_times.mark(1, s));
    with_flag(format == O2V_HIP_LABELS_I32, [&](auto i32) {
        with_flag(vec, [&](auto v) {
            constexpr uint32_t fmt = decltype(i32)::value ? kLsI32 : kLsU8;
            O2V_LAUNCH("k_euler", s, (k_euler<fmt, decltype(v)::value>), blocks, dim3(kBlock), 0, s, src, g, tab, ctr);
        });
    });
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(ctx->eu_times.mark(2, s));
    O2V_CHECK(hipMemcpyAsync(ctx->h_eu_ctr.ptr, ctr, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(ctx->eu_times.finish());
    *out_outside = ctx->h_eu_ctr.ptr[0];
    return O2V_HIP_OK;
}

int o2v_hip_euler_stats_times(const o2v_hip_ctx *ctx, float out_ms[2]) { return ctx ? ctx->eu_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"
