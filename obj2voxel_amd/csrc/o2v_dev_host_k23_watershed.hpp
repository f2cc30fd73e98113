// Host side of K23 (o2v_dev_k23_watershed.hpp): watershed basins of a relief, merged by persistence.  It takes K12's grid, limits
// and prefix count, so it comes after o2v_dev_host_k12_components.hpp (bit_grid, bit_tiles, kCcMaxGrid).

namespace {

constexpr uint32_t kWsFlagsKnown = O2V_HIP_FLAG_STAGE_TIMES;

}  // namespace

extern "C" {

uint64_t o2v_hip_watershed_scratch_bytes(const uint32_t dims[3])
{
    if (!dims || !dims[0] || !dims[1] || !dims[2]) return 0;
    const uint64_t words = cc_words(dims), voxels = (uint64_t) dims[0] * dims[1] * dims[2];
    return 4u * voxels + 12u * words + 8u * ((words + kBlock - 1) / kBlock + 1u) + 64u;
}

int o2v_hip_watershed_dense(o2v_hip_ctx *ctx, const int32_t *relief, const uint64_t strides[3], const uint32_t dims[3], uint32_t connectivity,
                            uint32_t min_depth, uint32_t flags, int32_t *labels, const uint64_t labels_strides[3], uint32_t *count)
{
    static const char fn[] = "o2v_hip_watershed_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    const Switches sw = read_switches();
    if (!labels || !labels_strides || !count) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    int rc;
    if ((rc = grid_given(ctx, fn, relief, strides, dims))) return rc;
    if ((rc = connectivity_known(ctx, fn, connectivity))) return rc;
    if (flags & ~kWsFlagsKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if ((uintptr_t) relief % sizeof(int32_t) || (uintptr_t) labels % sizeof(int32_t))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "relief and labels must be 4-byte aligned");
    if ((rc = index_limits(ctx, fn, dims, 0, "voxels"))) return rc;
    O2V_CHECK(hipSetDevice(ctx->device));
    const OutGrid outs[] = {{"labels", labels, labels_strides, 4u}};
    Span spans[2] = {{}, {"relief", relief, 0}};
    if ((rc = check_grid(ctx, fn, "relief", relief, dims, strides, 4u, false, &spans[1].bytes)) || (rc = check_outputs(ctx, fn, outs, dims, spans)) ||
        (rc = refuse_overlap(ctx, fn, spans, 1)))
        return rc;

    const BitGrid bg = bit_grid(dims);
    const CcGrid g{bg, bit_tiles_y(bg), bit_tiles_z(bg), connectivity};
    const I32View H{relief, strides[0], strides[1], strides[2]};
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2], n_blocks = (g.words + kBlock - 1) / kBlock;
    if ((rc = grow_scratch(ctx, ctx->d_ws_parent, voxels, fn, "parents")) || (rc = grow_scratch(ctx, ctx->d_ws_flags, g.words, fn, "peak bits")) ||
        (rc = grow_scratch(ctx, ctx->d_ws_local, g.words, fn, "prefixes")) || (rc = grow_scratch(ctx, ctx->d_ws_boff, n_blocks + 1u, fn, "block offsets")) ||
        (rc = grow_scratch(ctx, ctx->d_ws_ctr, 8u, fn, "counters")) || (rc = grow_scratch(ctx, ctx->h_ws_ctr, 8u, fn, "counters")))
        return rc;
    uint32_t *const P = ctx->d_ws_parent.ptr;
    unsigned long long *const fl = ctx->d_ws_flags.ptr, *const boff = ctx->d_ws_boff.ptr, *const ctr = ctx->d_ws_ctr.ptr;
    volatile unsigned long long *const h_ctr = ctx->h_ws_ctr.ptr;
    const bool count_on = (flags & O2V_HIP_FLAG_STAGE_TIMES) != 0;
    const dim3 per_word(stream_grid(ctx, g.words * 64u, 16u));
    hipStream_t s = ctx->stream;

    // ascent
    O2V_CHECK(ctx->ws_times.mark(0, s));
    if (sw.ws_no_tiles) {
        O2V_LAUNCH("k_ws_ascent", s, k_ws_ascent, per_word, dim3(kBlock), 0, s, g, H, P);
    } else {
        const uint64_t tiles = bit_tiles(g);   // (at most the words, below 2^31)
        O2V_LAUNCH("k_ws_ascent_tiles", s, k_ws_ascent_tiles, dim3((uint32_t) std::min<uint64_t>(tiles, kCcMaxGrid)), dim3(kBlock), 0, s, g, H, P);
    }
    // flatten, the peaks' ranks, the peaks for the host
    O2V_CHECK(ctx->ws_times.mark(1, s));
    O2V_LAUNCH("k_ws_flatten", s, k_ws_flatten, per_word, dim3(kBlock), 0, s, g, P, fl);
    O2V_LAUNCH("k_cc_count", s, k_cc_count, dim3((uint32_t) n_blocks), dim3(kBlock), 0, s, fl, g.words, ctx->d_ws_local.ptr, boff);
    O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, boff, n_blocks, boff + n_blocks);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipMemcpyAsync(ctx->h_ws_ctr.ptr, boff + n_blocks, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    const uint64_t n_peaks = h_ctr[0];   // (at most the voxels, below 2^31)
    const bool merge = min_depth > 0u && n_peaks >= 2u;
    uint64_t seen = 0, n_pairs = 0, growths = 0, table_bytes = 0, survivors = n_peaks;
    if (merge) {
        if ((rc = grow_scratch(ctx, ctx->d_ws_peaks, 2u * n_peaks, fn, "peaks")) || (rc = grow_scratch(ctx, ctx->h_ws_peaks, 2u * n_peaks, fn, "peaks")) ||
            (rc = grow_scratch(ctx, ctx->d_ws_lab, n_peaks, fn, "labels of the peaks")) || (rc = grow_scratch(ctx, ctx->h_ws_lab, n_peaks, fn, "labels of the peaks")))
            return rc;
        O2V_LAUNCH("k_ws_peaks", s, k_ws_peaks, per_word, dim3(kBlock), 0, s, g, H, fl, ctx->d_ws_local.ptr, boff, ctx->d_ws_peaks.ptr,
                   reinterpret_cast<int32_t *>(ctx->d_ws_peaks.ptr + n_peaks));
        O2V_CHECK(hipMemcpyAsync(ctx->h_ws_peaks.ptr, ctx->d_ws_peaks.ptr, 2u * n_peaks * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    // pairs: the table, doubled while a probe run overflows; then its entries as a list on the host
    O2V_CHECK(ctx->ws_times.mark(2, s));
    if (merge) {
        uint32_t held = pt_first_log2(n_peaks, sw.ws_table_log2, kWsTableMaxLog2, kWsTableMaxLog2);
        rc = pt_grow(ctx, fn, kWsTableMaxLog2, &held, &growths, [&](uint32_t log2, bool &overflow) -> int {
            const uint64_t slots = 1ull << log2;
            if (int rc = grow_scratch(ctx, ctx->d_ws_keys, slots, fn, "pair table")) return rc;
            if (int rc = grow_scratch(ctx, ctx->d_ws_vals, slots, fn, "pair table")) return rc;
            O2V_CHECK(hipMemsetAsync(ctx->d_ws_keys.ptr, 0xff, slots * sizeof(unsigned long long), s));
            O2V_CHECK(hipMemsetAsync(ctx->d_ws_vals.ptr, 0, slots * sizeof(uint32_t), s));
            O2V_CHECK(hipMemsetAsync(ctr, 0, 8u * sizeof(unsigned long long), s));
            with_flag(count_on, [&](auto counts) {
                O2V_LAUNCH("k_ws_pairs", s, k_ws_pairs<decltype(counts)::value>, per_word, dim3(kBlock), 0, s, g, H, P, ctx->d_ws_keys.ptr, ctx->d_ws_vals.ptr, log2, ctr);
            });
            O2V_CHECK(hipGetLastError());
            O2V_CHECK(hipMemcpyAsync(ctx->h_ws_ctr.ptr, ctr, 3u * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
            O2V_CHECK(hipStreamSynchronize(s));
            overflow = h_ctr[0] != 0u;
            return O2V_HIP_OK;
        });
        if (rc) return rc;
        const uint64_t slots = 1ull << held;
        n_pairs = h_ctr[1], seen = h_ctr[2], table_bytes = slots * 12u;
        // (the list: keys, then values, one array each on the device and page-locked)
        if ((rc = grow_scratch(ctx, ctx->d_ws_list, n_pairs + (n_pairs + 1u) / 2u, fn, "pair list")) ||
            (rc = grow_scratch(ctx, ctx->h_ws_list, n_pairs + (n_pairs + 1u) / 2u, fn, "pair list")))
            return rc;
        O2V_LAUNCH("k_pt_list", s, (k_pt_list<uint32_t, 1u>), dim3(stream_grid(ctx, slots, 16u)), dim3(kBlock), 0, s, ctx->d_ws_keys.ptr, ctx->d_ws_vals.ptr, slots, 1u,
                   ctx->d_ws_list.ptr, reinterpret_cast<uint32_t *>(ctx->d_ws_list.ptr + n_pairs), ctr + 3);
        O2V_CHECK(hipGetLastError());
        if (n_pairs) O2V_CHECK(hipMemcpyAsync(ctx->h_ws_list.ptr, ctx->d_ws_list.ptr, n_pairs * 12u, hipMemcpyDeviceToHost, s));
        O2V_CHECK(hipStreamSynchronize(s));
    }
    // merge, on the host
    O2V_CHECK(ctx->ws_times.mark(3, s));
    if (merge) {
        survivors = ws_merge((uint32_t) n_peaks, ctx->h_ws_peaks.ptr, reinterpret_cast<const int32_t *>(ctx->h_ws_peaks.ptr + n_peaks), n_pairs, ctx->h_ws_list.ptr,
                             reinterpret_cast<const uint32_t *>(ctx->h_ws_list.ptr + n_pairs), min_depth, ctx->h_ws_lab.ptr);
        O2V_CHECK(hipMemcpyAsync(ctx->d_ws_lab.ptr, ctx->h_ws_lab.ptr, n_peaks * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    // labels
    O2V_CHECK(ctx->ws_times.mark(4, s));
    O2V_LAUNCH("k_ws_labels", s, k_ws_labels, per_word, dim3(kBlock), 0, s, g, P, fl, ctx->d_ws_local.ptr, boff, merge ? ctx->d_ws_lab.ptr : (const int32_t *) nullptr,
               labels, labels_strides[0], labels_strides[1], labels_strides[2]);
    O2V_CHECK(hipGetLastError());
    if ((rc = finish_stages(ctx, ctx->ws_times))) return rc;
    const uint64_t counters[6] = {n_peaks, seen, n_pairs, growths, table_bytes, survivors};
    for (int i = 0; i < 6; ++i) ctx->ws_counters[i] = count_on ? counters[i] : 0u;
    *count = (uint32_t) survivors;
    return O2V_HIP_OK;
}

int o2v_hip_watershed_times(const o2v_hip_ctx *ctx, float out_ms[5]) { return ctx ? ctx->ws_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

int o2v_hip_watershed_counters(const o2v_hip_ctx *ctx, uint64_t out6[6])
{
    if (!ctx || !out6) return O2V_HIP_ERR_BAD_ARGUMENT;
    std::copy(ctx->ws_counters, ctx->ws_counters + 6, out6);
    return O2V_HIP_OK;
}

}  // extern "C"
