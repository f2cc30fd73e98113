// Host side of K28 (o2v_dev_k28_grow.hpp): seeded watershed, markers grown through a relief.  It takes K12's grid and limits, K20's
// tiles and weight rules and K23's relief contract, so it comes after o2v_dev_host_k12_components.hpp.

namespace {

constexpr uint32_t kGrowFlagsKnown = O2V_HIP_FLAG_STAGE_TIMES;
constexpr uint32_t kGrowCtrWords = 16u;   // [0 .. 2] in-tile sweeps per phase, [3] reached, then as uint32 the two lists' lengths and the changed word

static_assert(kGrowCap == O2V_HIP_GROW_MAX_TICKS, "one cap for the callers and the kernels");

}  // namespace

extern "C" {

uint64_t o2v_hip_grow_scratch_bytes(const uint32_t dims[3], uint32_t which)
{
    const uint32_t all = O2V_HIP_GROW_SCRATCH_LABELS | O2V_HIP_GROW_SCRATCH_LEVEL | O2V_HIP_GROW_SCRATCH_TICKS;
    if (!dims || !dims[0] || !dims[1] || !dims[2] || (which & ~all)) return 0;
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2];
    return 4u * voxels * (1u + (uint64_t) __builtin_popcount(which)) + 16u * geo_tiles(dims) + 8u * kGrowCtrWords;
}

int o2v_hip_grow_dense(o2v_hip_ctx *ctx, const int32_t *relief, const uint64_t relief_strides[3], const int32_t *markers, const uint64_t marker_strides[3],
                       const uint32_t dims[3], const uint32_t weights[3], uint32_t flags, int32_t *labels, const uint64_t labels_strides[3], int32_t *level,
                       const uint64_t level_strides[3], int32_t *ticks, const uint64_t ticks_strides[3], uint64_t *reached)
{
    static const char fn[] = "o2v_hip_grow_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    const Switches sw = read_switches();
    if (!markers || !marker_strides || !labels || !labels_strides || !reached || !weights || (level && !level_strides) || (ticks && !ticks_strides))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    int rc;
    if ((rc = grid_given(ctx, fn, relief, relief_strides, dims)) || (rc = geo_weights(ctx, fn, weights))) return rc;
    if (flags & ~kGrowFlagsKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if (((uintptr_t) relief | (uintptr_t) markers | (uintptr_t) labels | (uintptr_t) level | (uintptr_t) ticks) % sizeof(int32_t))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "relief, markers, labels, level and ticks must be 4-byte aligned");
    if ((rc = index_limits(ctx, fn, dims, 0, "voxels"))) return rc;
    O2V_CHECK(hipSetDevice(ctx->device));
    const OutGrid outs[] = {{"labels", labels, labels_strides, 4u}, {"level", level, level_strides, 4u}, {"ticks", ticks, ticks_strides, 4u}};
    Span spans[5] = {{}, {}, {}, {"relief", relief, 0}, {"markers", markers, 0}};
    if ((rc = check_grid(ctx, fn, "relief", relief, dims, relief_strides, 4u, false, &spans[3].bytes)) ||
        (rc = check_grid(ctx, fn, "markers", markers, dims, marker_strides, 4u, false, &spans[4].bytes)) || (rc = check_outputs(ctx, fn, outs, dims, spans)) ||
        (rc = refuse_overlap(ctx, fn, spans, 3)))
        return rc;

    const BitGrid bg = bit_grid(dims);
    const GeoGrid g{bg, bit_tiles_y(bg), bit_tiles_z(bg), {weights[0], weights[1], weights[2]}, kGrowCap};
    const I32View H{relief, relief_strides[0], relief_strides[1], relief_strides[2]}, M{markers, marker_strides[0], marker_strides[1], marker_strides[2]};
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2], tiles = geo_tiles(dims);   // (tiles: at most the words, below 2^31)
    // Q, T and L live in the caller's level, ticks and labels where linear index i is element i of them
    const bool q_in_place = level && linear_layout(dims, level_strides), t_in_place = ticks && linear_layout(dims, ticks_strides),
               l_in_place = linear_layout(dims, labels_strides);
    if ((rc = grow_scratch(ctx, ctx->d_grow_mask, voxels, fn, "masks")) || (rc = grow_scratch(ctx, ctx->d_grow_tiles, 4u * tiles, fn, "tile flags and lists")) ||
        (rc = grow_scratch(ctx, ctx->d_grow_ctr, kGrowCtrWords, fn, "counters")) || (rc = grow_scratch(ctx, ctx->h_grow_ctr, kGrowCtrWords, fn, "counters")) ||
        (!q_in_place && (rc = grow_scratch(ctx, ctx->d_grow_q, voxels, fn, "levels"))) || (!t_in_place && (rc = grow_scratch(ctx, ctx->d_grow_t, voxels, fn, "ticks"))) ||
        (!l_in_place && (rc = grow_scratch(ctx, ctx->d_grow_l, voxels, fn, "labels"))))
        return rc;
    uint32_t *const Q = q_in_place ? reinterpret_cast<uint32_t *>(level) : ctx->d_grow_q.ptr;
    uint32_t *const T = t_in_place ? reinterpret_cast<uint32_t *>(ticks) : ctx->d_grow_t.ptr;
    uint32_t *const L = l_in_place ? reinterpret_cast<uint32_t *>(labels) : ctx->d_grow_l.ptr;
    uint32_t *const mask = ctx->d_grow_mask.ptr;
    unsigned long long *const ctr = ctx->d_grow_ctr.ptr;
    const TileRounds tr = tile_rounds(ctx->d_grow_tiles.ptr, tiles, ctr + 4, ctx->h_grow_ctr.ptr + 4);
    const bool count = (flags & O2V_HIP_FLAG_STAGE_TIMES) != 0, use_tiles = !sw.grow_no_tiles;
    const dim3 per_word(stream_grid(ctx, g.words * 64u, 16u));
    hipStream_t s = ctx->stream;
    uint64_t counters[9] = {};   // per phase: rounds, tile visits, in-tile sweeps

    // What a phase's round 0 needs: both flag words clear, list 0 empty.  (A phase that has ended leaves them so; the first has not.)
    auto clear_lists = [&]() -> int {
        O2V_CHECK(hipMemsetAsync(tr.cnt, 0, 4u * sizeof(uint32_t), s));
        if (use_tiles) O2V_CHECK(hipMemsetAsync(tr.tile_flags[0], 0, 2u * tiles * sizeof(uint32_t), s));
        return O2V_HIP_OK;
    };
    // the rounds of phase P on V
    auto run_rounds = [&](auto phase, uint32_t *V) -> int {
        constexpr int P = decltype(phase)::value;
        RoundCounts done;
        const int r = run_tile_rounds(
            ctx, tr, use_tiles,
            [&](uint32_t cur, uint32_t nxt, uint32_t n, dim3 blocks) {
                with_flag(count, [&](auto counts) {
                    O2V_LAUNCH("k_grow_tiles", s, (k_grow_tiles<P, decltype(counts)::value>), blocks, dim3(kBlock), 0, s, g, H, mask, V, tr.tile_list[cur], n,
                               tr.tile_flags[cur], tr.tile_flags[nxt], tr.tile_list[nxt], tr.cnt + nxt, ctr + P);
                });
            },
            [&](uint32_t *changed) { O2V_LAUNCH("k_grow_sweep", s, k_grow_sweep<P>, per_word, dim3(kBlock), 0, s, g, H, mask, V, changed); }, &done);
        counters[3 * P] = done.rounds, counters[3 * P + 1] = done.visits;
        return r;
    };
    uint32_t *const fl0 = use_tiles ? tr.tile_flags[0] : nullptr;

    O2V_CHECK(ctx->grow_times.mark(0, s));   // init
    O2V_CHECK(hipMemsetAsync(ctr, 0, kGrowCtrWords * sizeof(unsigned long long), s));
    if ((rc = clear_lists())) return rc;
    O2V_LAUNCH("k_grow_init", s, k_grow_init, per_word, dim3(kBlock), 0, s, g, H, M, Q, fl0, tr.tile_list[0], tr.cnt);
    O2V_CHECK(ctx->grow_times.mark(1, s));   // level rounds
    if ((rc = run_rounds(std::integral_constant<int, 0>{}, Q))) return rc;
    O2V_CHECK(ctx->grow_times.mark(2, s));   // sources
    if ((rc = clear_lists())) return rc;
    O2V_LAUNCH("k_grow_between", s, k_grow_between<false>, per_word, dim3(kBlock), 0, s, g, H, M, Q, T, L, mask, fl0, tr.tile_list[0], tr.cnt);
    O2V_CHECK(ctx->grow_times.mark(3, s));   // tick rounds
    if ((rc = run_rounds(std::integral_constant<int, 1>{}, T))) return rc;
    O2V_CHECK(ctx->grow_times.mark(4, s));   // tight
    if ((rc = clear_lists())) return rc;
    O2V_LAUNCH("k_grow_between", s, k_grow_between<true>, per_word, dim3(kBlock), 0, s, g, H, M, Q, T, L, mask, fl0, tr.tile_list[0], tr.cnt);
    O2V_CHECK(ctx->grow_times.mark(5, s));   // label rounds
    if ((rc = run_rounds(std::integral_constant<int, 2>{}, L))) return rc;
    O2V_CHECK(ctx->grow_times.mark(6, s));   // write
    O2V_LAUNCH("k_grow_write", s, k_grow_write, per_word, dim3(kBlock), 0, s, g, Q, T, L, labels, labels_strides[0], labels_strides[1], labels_strides[2], level,
               level ? level_strides[0] : 0u, level ? level_strides[1] : 0u, level ? level_strides[2] : 0u, ticks, ticks ? ticks_strides[0] : 0u,
               ticks ? ticks_strides[1] : 0u, ticks ? ticks_strides[2] : 0u, ctr + 3);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipMemcpyAsync(ctx->h_grow_ctr.ptr, ctr, 4u * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if ((rc = finish_stages(ctx, ctx->grow_times))) return rc;
    for (int p = 0; p < 3; ++p) counters[3 * p + 2] = ctx->h_grow_ctr.ptr[p];
    for (int i = 0; i < 9; ++i) ctx->grow_counters[i] = count ? counters[i] : 0u;
    *reached = ctx->h_grow_ctr.ptr[3];
    return O2V_HIP_OK;
}

int o2v_hip_grow_times(const o2v_hip_ctx *ctx, float out_ms[7]) { return ctx ? ctx->grow_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

int o2v_hip_grow_counters(const o2v_hip_ctx *ctx, uint64_t out9[9])
{
    if (!ctx || !out9) return O2V_HIP_ERR_BAD_ARGUMENT;
    std::copy(ctx->grow_counters, ctx->grow_counters + 9, out9);
    return O2V_HIP_OK;
}

}  // extern "C"
