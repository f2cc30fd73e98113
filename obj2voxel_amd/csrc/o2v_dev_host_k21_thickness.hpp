// Host side of K21 (o2v_dev_k21_thickness.hpp): local thickness and ball morphology.  It runs K8's envelope passes on its own
// grids, so it comes after o2v_dev_host_k8_distance.hpp (dist_passes, dist_envelopes_yz, with_seed_format, the two limits,
// o2v_hip_distance_scratch_bytes).

namespace {

constexpr uint32_t kThickFlagsKnown = kThickBackground | kThickBorder | kThickF32 | kThickOpenOnly | O2V_HIP_FLAG_STAGE_TIMES;
constexpr uint64_t kThickMaxGrid = 1ull << 20;   // workgroups of k_thick_init and k_thick_list; more blocks are taken in turns

static_assert(kThickBackground == O2V_HIP_THICK_BACKGROUND && kThickBorder == O2V_HIP_THICK_BORDER && kThickF32 == O2V_HIP_THICK_F32 &&
                  kThickOpenOnly == O2V_HIP_THICK_OPEN_ONLY && kThickMaxCap == O2V_HIP_THICK_MAX_RADIUS2,
              "one set of flag values for the callers and the kernels");

// L_k[R] = 1 + max { |q - v|^2 : q in Z^3, |q|^2 < R } for v = (1, 0, 0), (1, 1, 0), (1, 1, 1) (k = 1, 2, 3) and R = 0 .. cap,
// L_k[0] = 0: out[(k - 1) * (cap + 1) + R].  The largest |q - v|^2 per |q|^2 in buckets, then a prefix max over the buckets.
void thick_cover_table(uint32_t cap, uint32_t *out)
{
    const size_t n = (size_t) cap + 1u;
    int rad = (int) std::sqrt((double) cap);
    while ((uint64_t) rad * rad >= cap && rad > 0) --rad;   // the largest |q_i| of a q with |q|^2 < cap
    std::vector<uint32_t> far(3u * cap, 0u);                // per k and |q|^2 < cap (every bucket that has a q holds at least k)
    for (int z = -rad; z <= rad; ++z)
        for (int y = -rad; y <= rad; ++y)
            for (int x = -rad; x <= rad; ++x) {
                const uint32_t q2 = (uint32_t) (x * x + y * y + z * z);
                if (q2 >= cap) continue;
                // |q - v|^2 = |q|^2 - 2 q.v + k
                const uint32_t f[3] = {(uint32_t) ((int) q2 - 2 * x + 1), (uint32_t) ((int) q2 - 2 * (x + y) + 2), (uint32_t) ((int) q2 - 2 * (x + y + z) + 3)};
                for (int k = 0; k < 3; ++k) far[(size_t) k * cap + q2] = std::max(far[(size_t) k * cap + q2], f[k]);
            }
    for (int k = 0; k < 3; ++k) {
        uint32_t best = 0;
        out[(size_t) k * n] = 0;
        for (uint32_t R = 1; R <= cap; ++R) {
            best = std::max(best, far[(size_t) k * cap + R - 1u]);
            out[(size_t) k * n + R] = best + 1u;
        }
    }
}

uint64_t thick_blocks(const uint32_t dims[3]) { return ((uint64_t) dims[0] * dims[1] * dims[2] + kBlock - 1) / kBlock; }

// The cover table of `cap` in the context's device copy: built and uploaded when the cap changes.
int thick_table(o2v_hip_ctx *ctx, const char *fn, uint32_t cap)
{
    if (ctx->thick_table_cap == cap && ctx->d_thick_table.ptr) return O2V_HIP_OK;
    ctx->thick_table_cap = 0;
    const uint64_t n = 3u * ((uint64_t) cap + 1u);
    if (int rc; (rc = grow_scratch(ctx, ctx->d_thick_table, n, fn, "cover table")) || (rc = grow_scratch(ctx, ctx->h_thick_table, n, fn, "cover table"))) return rc;
    thick_cover_table(cap, ctx->h_thick_table.ptr);
    O2V_CHECK(hipMemcpyAsync(ctx->d_thick_table.ptr, ctx->h_thick_table.ptr, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    O2V_CHECK(hipStreamSynchronize(ctx->stream));   // (the page-locked copy is free to be rebuilt)
    ctx->thick_table_cap = cap;
    return O2V_HIP_OK;
}

}  // namespace

extern "C" {

int o2v_hip_thickness_cover_table(uint32_t max_radius2, uint32_t *out)
{
    if (!out || max_radius2 == 0u || max_radius2 > kThickMaxCap) return O2V_HIP_ERR_BAD_ARGUMENT;
    thick_cover_table(max_radius2, out);
    return O2V_HIP_OK;
}

uint64_t o2v_hip_thickness_scratch_bytes(const uint32_t dims[3], uint32_t max_radius2, int have_depth2)
{
    if (!dims || !dims[0] || !dims[1] || !dims[2] || max_radius2 == 0u || max_radius2 > kThickMaxCap) return 0;
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2];
    return (have_depth2 ? 0u : 4u * voxels) + o2v_hip_distance_scratch_bytes(dims, O2V_HIP_DIST_SQ_I32) + 8u * (thick_blocks(dims) + 1u) +
           12u * ((uint64_t) max_radius2 + 1u) + 64u;
}

int o2v_hip_thickness_dense(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                            uint32_t flags, uint32_t max_radius2, void *dst, const uint64_t dst_strides[3], int32_t *depth2,
                            const uint64_t depth2_strides[3])
{
    static const char fn[] = "o2v_hip_thickness_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!dst || !dst_strides || (depth2 && !depth2_strides)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    SetGrid sg;
    int rc;
    if ((rc = set_grid(ctx, fn, grid, format, strides, dims, level, &sg))) return rc;
    if (flags & ~kThickFlagsKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if (max_radius2 == 0u) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "max_radius2 must be at least 1");
    if (max_radius2 > kThickMaxCap) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "max_radius2 " + std::to_string(max_radius2) + " is above 2^14");
    if ((rc = voxel_index_limit(ctx, fn, dims)) || (rc = dist2_limit(ctx, fn, dims))) return rc;
    const OutGrid outs[] = {{"dst", dst, dst_strides, 4u}, {"depth2", depth2, depth2_strides, 4u}};
    Span spans[3] = {{}, {}, {"grid", grid, sg.bytes}};
    if ((rc = check_outputs(ctx, fn, outs, dims, spans)) || (rc = refuse_overlap(ctx, fn, spans, 2))) return rc;

    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2], n_blocks = thick_blocks(dims);
    const bool open_only = (flags & kThickOpenOnly) != 0, count = (flags & O2V_HIP_FLAG_STAGE_TIMES) != 0;
    if ((rc = grow_scratch(ctx, ctx->d_dist_stack, o2v_hip_distance_scratch_bytes(dims, O2V_HIP_DIST_SQ_I32) / sizeof(uint2), fn, "scratch")) ||
        (!depth2 && (rc = grow_scratch(ctx, ctx->d_thick_depth, voxels, fn, "depth grid"))) ||
        (rc = grow_scratch(ctx, ctx->d_thick_boff, n_blocks + 1u, fn, "block offsets")) || (rc = grow_scratch(ctx, ctx->d_thick_ctr, 4u, fn, "counters")) ||
        (rc = grow_scratch(ctx, ctx->h_thick_ctr, 4u, fn, "counters")) || (!open_only && (rc = thick_table(ctx, fn, max_radius2))))
        return rc;

    ThickGrid g{};
    g.src = sg.source();
    g.invert = (flags & kThickBackground) ? 1u : 0u, g.border = (flags & kThickBorder) ? 1u : 0u, g.cap = max_radius2;
    if (depth2) g.e0 = depth2_strides[0], g.e1 = depth2_strides[1], g.e2 = depth2_strides[2];
    else g.e0 = 1u, g.e1 = dims[0], g.e2 = (uint64_t) dims[0] * dims[1];
    g.d0 = dst_strides[0], g.d1 = dst_strides[1], g.d2 = dst_strides[2];
    g.nx = dims[0], g.ny = dims[1], g.nz = dims[2];
    int32_t *const depth = depth2 ? depth2 : ctx->d_thick_depth.ptr;
    int32_t *const out = static_cast<int32_t *>(dst);
    const DtGrid on_depth{g.e0, g.e1, g.e2, g.nx, g.ny, g.nz}, on_dst{g.d0, g.d1, g.d2, g.nx, g.ny, g.nz};
    unsigned long long *const boff = ctx->d_thick_boff.ptr, *const ctr = ctx->d_thick_ctr.ptr;
    const uint32_t *const table = ctx->d_thick_table.ptr;
    const DistPasses p = dist_passes(ctx, dims);
    const dim3 per_block((uint32_t) std::min<uint64_t>(n_blocks, kThickMaxGrid));
    hipStream_t s = ctx->stream;

    // 1. depth2: the squared distance to the nearest voxel of the box that is not in S
    O2V_CHECK(ctx->thick_times.mark(0, s));
    with_seed_format(format, [&](auto fmt) {
        O2V_LAUNCH("k_thick_depth_x", s, k_thick_depth_x<decltype(fmt)::value>, p.gx, dim3(kBlock), 0, s, depth, g);
    });
    dist_envelopes_yz(ctx, depth, on_depth, p);
    // 2. the core M = {depth2' >= cap} and the squared distance to it
    O2V_CHECK(ctx->thick_times.mark(1, s));
    O2V_LAUNCH("k_thick_core_x", s, k_thick_core_x, p.gx, dim3(kBlock), 0, s, depth, out, g);
    dist_envelopes_yz(ctx, out, on_dst, p);
    // 3. dst initialised; the kept centres counted and listed
    O2V_CHECK(ctx->thick_times.mark(2, s));
    O2V_CHECK(hipMemsetAsync(ctr, 0, 4u * sizeof(unsigned long long), s));
    uint64_t kept = 0;
    if (open_only)
        O2V_LAUNCH("k_thick_init", s, k_thick_init<false>, per_block, dim3(kBlock), 0, s, g, depth, out, table, voxels, n_blocks, boff, ctr);
    else {
        O2V_LAUNCH("k_thick_init", s, k_thick_init<true>, per_block, dim3(kBlock), 0, s, g, depth, out, table, voxels, n_blocks, boff, ctr);
        O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, boff, n_blocks, boff + n_blocks);
        O2V_CHECK(hipGetLastError());
        O2V_CHECK(hipMemcpyAsync(ctx->h_thick_ctr.ptr, boff + n_blocks, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        O2V_CHECK(hipStreamSynchronize(s));
        kept = ctx->h_thick_ctr.ptr[0];   // (at most the voxels: an int32 index each)
        if (kept) {
            if ((rc = grow_scratch(ctx, ctx->d_thick_list, kept, fn, "centre list"))) return rc;
            O2V_LAUNCH("k_thick_list", s, k_thick_list, per_block, dim3(kBlock), 0, s, g, depth, table, voxels, n_blocks, boff, ctx->d_thick_list.ptr);
        }
    }
    // 4. the balls of the kept centres (nothing for an empty list)
    O2V_CHECK(ctx->thick_times.mark(3, s));
    if (kept) {
        const dim3 blocks((uint32_t) std::min<uint64_t>((kept + kBlock / 64u - 1) / (kBlock / 64u), (uint64_t) ctx->num_cus * 8u));
        with_flag(count, [&](auto counts) {
            O2V_LAUNCH("k_thick_balls", s, k_thick_balls<decltype(counts)::value>, blocks, dim3(kBlock), 0, s, g, depth, ctx->d_thick_list.ptr, kept, out, ctr);
        });
    }
    // 5. the float format
    O2V_CHECK(ctx->thick_times.mark(4, s));
    if (flags & kThickF32) O2V_LAUNCH("k_thick_convert", s, k_thick_convert, dim3(stream_grid(ctx, voxels, 8u)), dim3(kBlock), 0, s, g, out, voxels);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipMemcpyAsync(ctx->h_thick_ctr.ptr, ctr, 4u * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if ((rc = finish_stages(ctx, ctx->thick_times))) return rc;
    ctx->thick_counters[0] = ctx->h_thick_ctr.ptr[0], ctx->thick_counters[1] = kept, ctx->thick_counters[2] = count ? ctx->h_thick_ctr.ptr[2] : 0u;
    return O2V_HIP_OK;
}

int o2v_hip_thickness_times(const o2v_hip_ctx *ctx, float out_ms[5]) { return ctx ? ctx->thick_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

int o2v_hip_thickness_counters(const o2v_hip_ctx *ctx, uint64_t out3[3])
{
    if (!ctx || !out3) return O2V_HIP_ERR_BAD_ARGUMENT;
    std::copy(ctx->thick_counters, ctx->thick_counters + 3, out3);
    return O2V_HIP_OK;
}

}  // extern "C"
