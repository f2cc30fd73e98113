// Host side of K22 (o2v_dev_k22_thinning.hpp): skeletons of a dense grid by topological thinning.  It classifies with K12's
// k_cc_classify and takes K12's and K20's limits, so it comes after o2v_dev_host_k12_components.hpp (bit_grid, bit_tiles,
// launch_classify, kCcMaxGrid).

namespace {

constexpr uint32_t kThinFlagsKnown = O2V_HIP_CC_INVERT | O2V_HIP_FLAG_STAGE_TIMES;

static_assert(kThinUltimate == O2V_HIP_THIN_ULTIMATE && kThinCurve == O2V_HIP_THIN_CURVE && kThinDstMask == O2V_HIP_THIN_DST_MASK &&
                  kThinDstDegree == O2V_HIP_THIN_DST_DEGREE,
              "one set of mode and format values for the callers and the kernels");

}  // namespace

extern "C" {

uint64_t o2v_hip_thin_scratch_bytes(const uint32_t dims[3], int have_keep)
{
    if (!dims || !dims[0] || !dims[1] || !dims[2]) return 0;
    const BitGrid g = bit_grid(dims);
    return (have_keep ? 24u : 16u) * g.words + 8u * bit_tiles(g) + 64u;
}

int o2v_hip_thin_dense(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                       uint32_t flags, uint32_t mode, uint32_t max_iterations, const uint8_t *keep, const uint64_t keep_strides[3], uint8_t *dst,
                       const uint64_t dst_strides[3], uint32_t dst_format)
{
    static const char fn[] = "o2v_hip_thin_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    const Switches sw = read_switches();
    if (!dst || !dst_strides || (keep && !keep_strides)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    SetGrid sg;
    int rc;
    if ((rc = set_grid(ctx, fn, grid, format, strides, dims, level, &sg))) return rc;
    if (mode != kThinUltimate && mode != kThinCurve) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown mode " + std::to_string(mode));
    if (dst_format != kThinDstMask && dst_format != kThinDstDegree)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown dst_format " + std::to_string(dst_format));
    if (flags & ~kThinFlagsKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if ((rc = index_limits(ctx, fn, dims, 0, "voxels"))) return rc;
    const OutGrid outs[] = {{"dst", dst, dst_strides, 1u}};
    // thinning in place: dst is the grid itself, voxel for voxel (the set is classified before anything is written)
    const bool same = (const void *) dst == grid && format == O2V_HIP_GRID_U8 && std::equal(strides, strides + 3, dst_strides);
    SetGrid kg;
    Span spans[3] = {{}, {"grid", same ? nullptr : grid, sg.bytes}, {"keep", keep, 0}};
    if ((rc = check_outputs(ctx, fn, outs, dims, spans))) return rc;
    if (keep) {
        kg.key = GridKey(keep, O2V_HIP_GRID_U8, keep_strides, dims, 0.f);
        kg.vec = rows_aligned16(keep, keep_strides, 1u);
        if ((rc = check_grid(ctx, fn, "keep", keep, dims, keep_strides, 1u, false, &kg.bytes))) return rc;
        spans[2].bytes = kg.bytes;
    }
    if ((rc = refuse_overlap(ctx, fn, spans, 1))) return rc;

    const BitGrid bg = bit_grid(dims);
    const ThinGrid g{bg, bit_tiles_y(bg), bit_tiles_z(bg), mode};
    const uint64_t tiles = bit_tiles(bg);   // (at most the words, below 2^31)
    if ((rc = grow_scratch(ctx, ctx->d_thin_bits, (keep ? 3u : 2u) * g.words, fn, "set, border and keep bits")) ||
        (rc = grow_scratch(ctx, ctx->d_thin_stamps, 2u * tiles, fn, "tile stamps")) || (rc = grow_scratch(ctx, ctx->d_thin_ctr, 8u, fn, "counters")) ||
        (rc = grow_scratch(ctx, ctx->h_thin_ctr, 8u, fn, "counters")))
        return rc;
    unsigned long long *const bits = ctx->d_thin_bits.ptr, *const border = bits + g.words, *const keep_bits = keep ? bits + 2u * g.words : nullptr;
    unsigned long long *const ctr = ctx->d_thin_ctr.ptr;
    volatile unsigned long long *const h_ctr = ctx->h_thin_ctr.ptr;
    uint32_t *const stamps = ctx->d_thin_stamps.ptr;
    const bool count = (flags & O2V_HIP_FLAG_STAGE_TIMES) != 0, use_tiles = !sw.thin_no_tiles;
    const dim3 per_word(stream_grid(ctx, g.words * 64u, 16u)), per_thread(stream_grid(ctx, g.words, 16u));
    // the tiles a workgroup of k_thin_substep looks at: as many as leave 16 workgroups per CU, 1 ... kThinChunk (few tiles: a
    // workgroup each, all in flight; many: fewer workgroups that find nothing to do)
    const uint32_t chunk = (uint32_t) std::min<uint64_t>(std::max<uint64_t>(tiles / ((uint64_t) ctx->num_cus * 16u), 1u), kThinChunk);
    const dim3 per_chunk((uint32_t) std::min<uint64_t>((tiles + chunk - 1u) / chunk, kCcMaxGrid));   // (more chunks are taken in turns)
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->thin_times.mark(0, s));
    O2V_CHECK(hipMemsetAsync(ctr, 0, 8u * sizeof(unsigned long long), s));
    O2V_CHECK(hipMemsetAsync(stamps, 0, 2u * tiles * sizeof(uint32_t), s));
    launch_classify(ctx, sg, (flags & O2V_HIP_CC_INVERT) ? 1u : 0u, bits);
    if (keep) launch_classify(ctx, kg, 0u, keep_bits);
    O2V_CHECK(ctx->thin_times.mark(1, s));
    // The iterations.  No cap but the caller's: an iteration follows only one that removed a voxel, and the set is finite.
    uint64_t iterations = 0, launches = 0, removed = 0;
    for (uint32_t it = 1;; ++it) {
        with_flag(!use_tiles, [&](auto all) {
            O2V_LAUNCH("k_thin_border", s, k_thin_border<decltype(all)::value>, per_thread, dim3(kBlock), 0, s, g, bits, stamps, it, border);
        });
        for (uint32_t sub = 0; sub < 8u; ++sub) {
            if (use_tiles)
                with_flag(count, [&](auto counts) {
                    O2V_LAUNCH("k_thin_substep", s, k_thin_substep<decltype(counts)::value>, per_chunk, dim3(kBlock), 0, s, g, sub, it, chunk, bits, keep_bits, border,
                               stamps, ctr);
                });
            else
                O2V_LAUNCH("k_thin_sweep", s, k_thin_sweep, per_word, dim3(kBlock), 0, s, g, sub, bits, keep_bits, border, ctr);
        }
        O2V_CHECK(hipGetLastError());
        O2V_CHECK(hipMemcpyAsync(ctx->h_thin_ctr.ptr, ctr, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        O2V_CHECK(hipStreamSynchronize(s));
        ++iterations, launches += 9u;
        const uint64_t so_far = h_ctr[0];
        const bool none = so_far == removed;
        removed = so_far;
        if (none || (max_iterations && it == max_iterations)) break;
    }
    O2V_CHECK(ctx->thin_times.mark(2, s));
    with_flag(dst_format == kThinDstDegree, [&](auto degree) {
        O2V_LAUNCH("k_thin_write", s, k_thin_write<decltype(degree)::value>, per_word, dim3(kBlock), 0, s, g, bits, dst, dst_strides[0], dst_strides[1],
                   dst_strides[2]);
    });
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipMemcpyAsync(ctx->h_thin_ctr.ptr, ctr, 2u * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if ((rc = finish_stages(ctx, ctx->thin_times))) return rc;
    const uint64_t counters[4] = {iterations, launches, use_tiles ? h_ctr[1] : 8u * iterations * tiles, removed};
    for (int i = 0; i < 4; ++i) ctx->thin_counters[i] = count ? counters[i] : 0u;
    return O2V_HIP_OK;
}

int o2v_hip_thin_times(const o2v_hip_ctx *ctx, float out_ms[3]) { return ctx ? ctx->thin_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

int o2v_hip_thin_counters(const o2v_hip_ctx *ctx, uint64_t out4[4])
{
    if (!ctx || !out4) return O2V_HIP_ERR_BAD_ARGUMENT;
    std::copy(ctx->thin_counters, ctx->thin_counters + 4, out4);
    return O2V_HIP_OK;
}

}  // extern "C"
