// Host side of K27 (o2v_dev_k27_openness.hpp): sky visibility of the voxels of a set grid.  It builds K11's masks with K11's
// kernels into scratch of its own and takes K12's limits, so it comes after o2v_dev_host_k11_raycast.hpp (ray_levels) and
// o2v_dev_host_k12_components.hpp (index_limits).

namespace {

static_assert(kOpenSurface == O2V_HIP_OPEN_SURFACE && kOpenSolid == O2V_HIP_OPEN_SOLID && kOpenEmpty == O2V_HIP_OPEN_EMPTY && kOpenGrid == O2V_HIP_OPEN_GRID &&
                  kOpenMaxDirs == O2V_HIP_OPEN_MAX_DIRECTIONS && kOpenMaxComponent == O2V_HIP_OPEN_MAX_COMPONENT,
              "one set of values for the callers and the kernels");
constexpr uint32_t kOpenFlagsKnown = O2V_HIP_FLAG_STAGE_TIMES;
constexpr uint32_t kOpenMaskDirs = 64u;   // a mask holds a bit per direction

// f(mode) with the target mode (checked) as the template argument of k_open_targets
template <typename F>
void with_open_mode(uint32_t mode, F &&f)
{
    if (mode == kOpenSolid) return f(std::integral_constant<uint32_t, kOpenSolid>{});
    if (mode == kOpenEmpty) return f(std::integral_constant<uint32_t, kOpenEmpty>{});
    if (mode == kOpenGrid) return f(std::integral_constant<uint32_t, kOpenGrid>{});
    return f(std::integral_constant<uint32_t, kOpenSurface>{});
}

}  // namespace

extern "C" {

uint64_t o2v_hip_openness_scratch_bytes(const uint32_t dims[3])
{
    const uint64_t masks = o2v_hip_raycast_scratch_bytes(dims);
    if (!masks) return 0;
    // the masks, the counter, the direction table, and a list entry per voxel if every voxel is a target (a call sizes its list
    // by the targets it counted)
    return masks + 8u + 4u * kOpenDirWords * kOpenMaxDirs + 4u * (uint64_t) dims[0] * dims[1] * dims[2];
}

int o2v_hip_openness(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                     const int32_t *directions, uint32_t n_directions, uint32_t target_mode, const uint8_t *target_grid, const uint64_t target_strides[3],
                     uint32_t max_distance2, uint32_t flags, uint8_t *dst, const uint64_t dst_strides[3], int64_t *mask, const uint64_t mask_strides[3],
                     uint64_t *out_targets)
{
    static const char fn[] = "o2v_hip_openness";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    const Switches sw = read_switches();
    SetGrid sg;
    int rc;
    if ((rc = set_grid(ctx, fn, grid, format, strides, dims, level, &sg)) || (rc = index_limits(ctx, fn, dims, 0u, "targets"))) return rc;
    if (!directions || !dst || !dst_strides || !out_targets || (mask && !mask_strides)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if (n_directions == 0u) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "no directions");
    if (n_directions > kOpenMaxDirs) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 254 directions: a count is one byte, 255 marks the voxels that are no targets");
    if (mask && n_directions > kOpenMaskDirs) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "a mask holds 64 directions, not " + std::to_string(n_directions));
    OpenDir table[kOpenMaxDirs];
    for (uint32_t i = 0; i < n_directions; ++i) {
        const int32_t *d = directions + 3u * i;
        if (!d[0] && !d[1] && !d[2]) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "direction " + std::to_string(i) + " is zero");
        for (int a = 0; a < 3; ++a) {
            if (d[a] > (int32_t) kOpenMaxComponent || d[a] < -(int32_t) kOpenMaxComponent)
                return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "direction " + std::to_string(i) + " has a component above 127 in magnitude");
            table[i].s[a] = d[a] > 0 ? 1 : d[a] < 0 ? -1 : 0;
            table[i].m[a] = (uint32_t) (d[a] < 0 ? -d[a] : d[a]);
            table[i].r[a] = open_recip(table[i].m[a]);
        }
    }
    if (target_mode > kOpenGrid) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown target mode " + std::to_string(target_mode));
    if (flags & ~kOpenFlagsKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if ((uintptr_t) mask % sizeof(int64_t)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "mask must be 8-byte aligned");
    Span spans[4] = {};
    const OutGrid outs[] = {{"dst", dst, dst_strides, 1u}, {"mask", mask, mask_strides, 8u}};
    if ((rc = check_outputs(ctx, fn, outs, dims, spans))) return rc;
    spans[2] = Span{"grid", sg.key.p, sg.bytes};
    if (target_mode == kOpenGrid) {
        if (!target_grid || !target_strides) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
        spans[3] = Span{"target_grid", target_grid, 0};
        if ((rc = check_grid(ctx, fn, "target_grid", target_grid, dims, target_strides, 1u, false, &spans[3].bytes))) return rc;
    }
    if ((rc = refuse_overlap(ctx, fn, spans, 2))) return rc;

    uint64_t words[3];
    uint32_t per_axis[3][3];
    ray_levels(dims, words, per_axis);
    if ((rc = grow_scratch(ctx, ctx->d_open_masks, words[0] + words[1] + words[2], fn, "masks")) || (rc = grow_scratch(ctx, ctx->d_open_ctr, 2u, fn, "counters")) ||
        (rc = grow_scratch(ctx, ctx->h_open_ctr, 2u, fn, "counters")) || (rc = grow_scratch(ctx, ctx->d_open_dirs, (uint64_t) kOpenDirWords * kOpenMaxDirs, fn, "directions")) ||
        (rc = grow_scratch(ctx, ctx->h_open_dirs, (uint64_t) kOpenDirWords * kOpenMaxDirs, fn, "directions")))
        return rc;
    std::memcpy(ctx->h_open_dirs.ptr, table, (size_t) n_directions * sizeof(OpenDir));
    unsigned long long *const m0 = ctx->d_open_masks.ptr, *const m1 = m0 + words[0], *const m2 = m1 + words[1], *const ctr = ctx->d_open_ctr.ptr;
    RayGrid rg{};
    OpenGrid g{};
    for (int a = 0; a < 3; ++a) {
        rg.org[a] = 0, rg.dim[a] = g.dim[a] = (int32_t) dims[a];
        rg.b0[a] = g.b0[a] = per_axis[0][a], rg.b1[a] = g.b1[a] = per_axis[1][a], rg.b2[a] = g.b2[a] = per_axis[2][a];
    }
    rg.m0 = g.m0 = m0, rg.m1 = g.m1 = m1, rg.m2 = g.m2 = m2;
    OpenIo io{};
    if (target_mode == kOpenGrid) io.tgrid = target_grid, io.t0 = target_strides[0], io.t1 = target_strides[1], io.t2 = target_strides[2];
    io.dst = dst, io.d0 = dst_strides[0], io.d1 = dst_strides[1], io.d2 = dst_strides[2];
    if (mask) io.mask = reinterpret_cast<long long *>(mask), io.k0 = mask_strides[0], io.k1 = mask_strides[1], io.k2 = mask_strides[2];
    hipStream_t s = ctx->stream;

    // the masks: K11's build, the only pass over the grid
    O2V_CHECK(ctx->open_times.mark(0, s));
    O2V_CHECK(hipMemsetAsync(m1, 0, words[1] * 8u, s));
    O2V_CHECK(hipMemsetAsync(ctr, 0, 2u * sizeof(unsigned long long), s));
    O2V_CHECK(hipMemcpyAsync(ctx->d_open_dirs.ptr, ctx->h_open_dirs.ptr, (size_t) n_directions * sizeof(OpenDir), hipMemcpyHostToDevice, s));
    {
        const RaySource src = sg.source();
        const uint64_t tiles = (uint64_t) ((dims[0] + 63u) / 64u) * per_axis[0][1] * per_axis[0][2];
        const dim3 blocks(stream_grid(ctx, tiles * 64u, 8u));
        with_set_format(sg, [&](auto fmt, auto vec) {
            O2V_LAUNCH("k_ray_build", s, (k_ray_build<decltype(fmt)::value, decltype(vec)::value>), blocks, dim3(kBlock), 0, s, src, rg, m0, m1);
        });
        O2V_LAUNCH("k_ray_build_top", s, k_ray_build_top, dim3(stream_grid(ctx, words[2], 8u)), dim3(kBlock), 0, s, rg, m1, m2);
    }
    // the targets: counted, the host waits for their number, then listed (and every other voxel's 255 written)
    O2V_CHECK(ctx->open_times.mark(1, s));
    const uint64_t rows = (uint64_t) per_axis[0][0] * dims[1] * dims[2];
    const dim3 tblocks(stream_grid(ctx, rows, 8u));
    with_open_mode(target_mode, [&](auto mode) {
        O2V_LAUNCH("k_open_targets", s, (k_open_targets<decltype(mode)::value, false>), tblocks, dim3(kBlock), 0, s, g, io, (uint32_t *) nullptr, 0ull, ctr);
    });
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipMemcpyAsync(ctx->h_open_ctr.ptr, ctr, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    const uint64_t n_targets = ctx->h_open_ctr.ptr[0];
    if (n_targets > kMaxInt32) return refuse(ctx, O2V_HIP_ERR_HIP, fn, "counted " + std::to_string(n_targets) + " targets in a grid of at most 2^31 - 1 voxels");
    if ((rc = grow_scratch(ctx, ctx->d_open_list, n_targets, fn, "target list"))) return rc;
    with_open_mode(target_mode, [&](auto mode) {
        O2V_LAUNCH("k_open_targets", s, (k_open_targets<decltype(mode)::value, true>), tblocks, dim3(kBlock), 0, s, g, io, ctx->d_open_list.ptr, n_targets, ctr + 1);
    });
    // the walk
    O2V_CHECK(ctx->open_times.mark(2, s));
    if (n_targets) {
        const dim3 blocks((uint32_t) ((n_targets + kBlock - 1u) / kBlock));
        const auto launch = [&](auto skip, auto with_mask) {
            O2V_LAUNCH("k_open_walk", s, (k_open_walk<decltype(skip)::value, decltype(with_mask)::value>), blocks, dim3(kBlock), 0, s, g, ctx->d_open_dirs.ptr,
                       n_directions, max_distance2, ctx->d_open_list.ptr, (uint32_t) n_targets, io);
        };
        with_flag(!sw.open_no_skip, [&](auto skip) { with_flag(mask != nullptr, [&](auto with_mask) { launch(skip, with_mask); }); });
    }
    O2V_CHECK(hipGetLastError());
    if ((rc = finish_stages(ctx, ctx->open_times))) return rc;
    *out_targets = n_targets;
    return O2V_HIP_OK;
}

int o2v_hip_openness_times(const o2v_hip_ctx *ctx, float out_ms[3]) { return ctx ? ctx->open_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"
