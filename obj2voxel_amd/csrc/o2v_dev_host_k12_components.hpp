// Host side of K12 and K20 (o2v_dev_k12_components.hpp, o2v_dev_k20_geodesic.hpp): they share bit_grid, launch_classify and the limits.

// ---- K12: connected components and flood fill of a dense grid ---------------------------------------------------------------

namespace {

constexpr uint64_t kCcMaxGrid = 1ull << 20;   // workgroups of k_cc_tiles; more tiles are taken in turns
constexpr uint32_t kCcFlagsKnown = O2V_HIP_CC_INVERT | O2V_HIP_CC_SEED_BORDER | O2V_HIP_FLAG_STAGE_TIMES;

// The bit grid (o2v_dev_bits.hpp) of a box, for every family that reads one.  words is 64-bit: the *_scratch_bytes functions ask
// for it with dims that nothing has checked.
BitGrid bit_grid(const uint32_t dims[3])
{
    const uint32_t W = (dims[0] + 63u) / 64u;
    return BitGrid{dims[0], dims[1], dims[2], W, (uint64_t) W * dims[1] * dims[2]};
}

uint64_t cc_words(const uint32_t dims[3]) { return bit_grid(dims).words; }

// its tiles of 64 x 8 x 8 voxels: along y, along z (along x: W), all of them
uint32_t bit_tiles_y(const BitGrid &g) { return (g.ny + 7u) / 8u; }
uint32_t bit_tiles_z(const BitGrid &g) { return (g.nz + 7u) / 8u; }
uint64_t bit_tiles(const BitGrid &g) { return (uint64_t) g.W * bit_tiles_y(g) * bit_tiles_z(g); }

// k_cc_classify on the context's stream, for K12, K13 and K14: the set (its complement inside the box if invert) as one bit per
// voxel, words of 64 voxels along x, [z][y][W].
void launch_classify(o2v_hip_ctx *ctx, const SetGrid &sg, uint32_t invert, unsigned long long *bits)
{
    const BitGrid g = bit_grid(sg.key.dims);
    const RaySource src = sg.source();
    const dim3 per_group(stream_grid(ctx, (g.words + 15u) / 16u * 64u, 8u));
    hipStream_t s = ctx->stream;
    with_set_format(sg, [&](auto format, auto vec) {
        O2V_LAUNCH("k_cc_classify", s, (k_cc_classify<decltype(format)::value, decltype(vec)::value>), per_group, dim3(kBlock), 0, s, src, g, invert, bits);
    });
}

// What the two calls share.  labels != null: o2v_hip_components_dense; else o2v_hip_flood_dense.
int cc_run(o2v_hip_ctx *ctx, const char *fn, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
           uint32_t connectivity, uint32_t flags, int32_t *labels, uint8_t *out, const uint64_t out_strides[3], const int32_t *seeds,
           uint64_t n_seeds, const uint8_t values[3], uint64_t *result)
{
    const Switches sw = read_switches();
    if (!out_strides || !result || (!labels && !out) || (out && !values) || (n_seeds && !seeds))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    SetGrid sg;
    int rc;
    if ((rc = set_grid(ctx, fn, grid, format, strides, dims, level, &sg))) return rc;
    if ((rc = connectivity_known(ctx, fn, connectivity))) return rc;
    if ((flags & ~kCcFlagsKnown) || (labels && (flags & O2V_HIP_CC_SEED_BORDER)))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if ((rc = index_limits(ctx, fn, dims, n_seeds, "seeds"))) return rc;
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2];
    const OutGrid outs[] = {labels ? OutGrid{"labels", labels, out_strides, 4u} : OutGrid{"out", out, out_strides, 1u}};
    Span spans[3] = {{}, {"grid", grid, sg.bytes}, {"seeds", seeds, n_seeds * 12u}};
    if ((rc = check_outputs(ctx, fn, outs, dims, spans)) || (n_seeds && (rc = check_device_range(ctx, fn, seeds, n_seeds * 12u, "seeds"))) ||
        (rc = refuse_overlap(ctx, fn, spans, 1)))
        return rc;

    const BitGrid bg = bit_grid(dims);
    const CcGrid g{bg, bit_tiles_y(bg), bit_tiles_z(bg), connectivity};
    // the parents live in the caller's labels where linear index i is element i of them
    const bool in_place = labels && linear_layout(dims, out_strides);
    const uint64_t n_blocks = (g.words + kBlock - 1) / kBlock;
    if ((rc = grow_scratch(ctx, ctx->d_cc_bits, g.words, fn, "set bits")) || (rc = grow_scratch(ctx, ctx->d_cc_flags, g.words, fn, "flag bits")) ||
        (rc = grow_scratch(ctx, ctx->d_cc_ctr, 4u, fn, "counters")) || (rc = grow_scratch(ctx, ctx->h_cc_ctr, 4u, fn, "counters")) ||
        (labels && ((rc = grow_scratch(ctx, ctx->d_cc_local, g.words, fn, "prefixes")) ||
                    (rc = grow_scratch(ctx, ctx->d_cc_boff, n_blocks + 1u, fn, "block offsets")))) ||
        (!in_place && (rc = grow_scratch(ctx, ctx->d_cc_parent, voxels, fn, "parents"))))
        return rc;
    uint32_t *const P = in_place ? reinterpret_cast<uint32_t *>(labels) : ctx->d_cc_parent.ptr;
    unsigned long long *const bits = ctx->d_cc_bits.ptr, *const fl = ctx->d_cc_flags.ptr, *const ctr = ctx->d_cc_ctr.ptr;
    const uint32_t invert = (flags & O2V_HIP_CC_INVERT) ? 1u : 0u;
    const bool count = (flags & O2V_HIP_FLAG_STAGE_TIMES) != 0;
    const dim3 per_word(stream_grid(ctx, g.words * 64u, 16u));
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->cc_times.mark(0, s));
    O2V_CHECK(hipMemsetAsync(ctr, 0, 4u * sizeof(unsigned long long), s));
    launch_classify(ctx, sg, invert, bits);
    O2V_CHECK(ctx->cc_times.mark(1, s));
    if (sw.cc_no_tiles) {
        O2V_LAUNCH("k_cc_init", s, k_cc_init, per_word, dim3(kBlock), 0, s, g, bits, P);
    } else {
        const uint64_t tiles = bit_tiles(g);
        O2V_LAUNCH("k_cc_tiles", s, k_cc_tiles, dim3((uint32_t) std::min<uint64_t>(tiles, kCcMaxGrid)), dim3(kBlock), 0, s, g, bits, P);
    }
    O2V_CHECK(ctx->cc_times.mark(2, s));
    with_flag(sw.cc_no_tiles, [&](auto no_tiles) {
        with_flag(count, [&](auto counts) {
            O2V_LAUNCH("k_cc_seams", s, (k_cc_seams<decltype(no_tiles)::value, decltype(counts)::value>), per_word, dim3(kBlock), 0, s, g, bits, P, ctr);
        });
    });
    O2V_CHECK(ctx->cc_times.mark(3, s));
    if (labels) {
        O2V_LAUNCH("k_cc_flatten", s, k_cc_flatten, per_word, dim3(kBlock), 0, s, g, bits, P, fl);
        O2V_LAUNCH("k_cc_count", s, k_cc_count, dim3((uint32_t) n_blocks), dim3(kBlock), 0, s, fl, g.words, ctx->d_cc_local.ptr, ctx->d_cc_boff.ptr);
        O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, ctx->d_cc_boff.ptr, n_blocks, ctx->d_cc_boff.ptr + n_blocks);
        O2V_CHECK(ctx->cc_times.mark(4, s));
        O2V_LAUNCH("k_cc_labels", s, k_cc_labels, per_word, dim3(kBlock), 0, s, g, bits, P, fl, ctx->d_cc_local.ptr, ctx->d_cc_boff.ptr, labels,
                   out_strides[0], out_strides[1], out_strides[2]);
        O2V_CHECK(hipMemcpyAsync(ctx->h_cc_ctr.ptr + 2, ctx->d_cc_boff.ptr + n_blocks, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    } else {
        O2V_LAUNCH("k_cc_flatten", s, k_cc_flatten, per_word, dim3(kBlock), 0, s, g, bits, P, (unsigned long long *) nullptr);
        O2V_CHECK(ctx->cc_times.mark(4, s));
        O2V_CHECK(hipMemsetAsync(fl, 0, g.words * sizeof(unsigned long long), s));
        if (n_seeds)
            O2V_LAUNCH("k_cc_seed_list", s, k_cc_seed_list, dim3(stream_grid(ctx, n_seeds, 8u)), dim3(kBlock), 0, s, g, bits, P, seeds, n_seeds, fl);
        if (flags & O2V_HIP_CC_SEED_BORDER) O2V_LAUNCH("k_cc_seed_border", s, k_cc_seed_border, per_word, dim3(kBlock), 0, s, g, bits, P, fl);
        O2V_LAUNCH("k_cc_flood_out", s, k_cc_flood_out, per_word, dim3(kBlock), 0, s, g, bits, P, fl, (uint32_t) values[0], (uint32_t) values[1],
                   (uint32_t) values[2], out, out_strides[0], out_strides[1], out_strides[2], ctr + 2);
        O2V_CHECK(hipMemcpyAsync(ctx->h_cc_ctr.ptr + 2, ctr + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    }
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(ctx->cc_times.mark(5, s));
    O2V_CHECK(hipMemcpyAsync(ctx->h_cc_ctr.ptr, ctr, 2u * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(ctx->cc_times.finish());
    ctx->cc_counters[0] = ctx->h_cc_ctr.ptr[0];
    ctx->cc_counters[1] = ctx->h_cc_ctr.ptr[1];
    *result = ctx->h_cc_ctr.ptr[2];
    return O2V_HIP_OK;
}

}  // namespace

extern "C" {

uint64_t o2v_hip_components_scratch_bytes(const uint32_t dims[3], uint32_t which)
{
    if (!dims || !dims[0] || !dims[1] || !dims[2] || which > O2V_HIP_CC_SCRATCH_FLOOD) return 0;
    const uint64_t words = cc_words(dims), voxels = (uint64_t) dims[0] * dims[1] * dims[2];
    if (which == O2V_HIP_CC_SCRATCH_FLOOD) return 16u * words + 4u * voxels + 32u;
    return 20u * words + 8u * ((words + kBlock - 1) / kBlock + 1u) + 32u + (which == O2V_HIP_CC_SCRATCH_LABELS_STRIDED ? 4u * voxels : 0u);
}

int o2v_hip_components_dense(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                             uint32_t connectivity, uint32_t flags, int32_t *labels, const uint64_t label_strides[3], uint64_t *out_count)
{
    static const char fn[] = "o2v_hip_components_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!labels) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    return cc_run(ctx, fn, grid, format, strides, dims, level, connectivity, flags, labels, nullptr, label_strides, nullptr, 0, nullptr, out_count);
}

int o2v_hip_flood_dense(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                        uint32_t connectivity, uint32_t flags, const int32_t *seeds, uint64_t n_seeds, const uint8_t values[3], uint8_t *out,
                        const uint64_t out_strides[3], uint64_t *out_reached)
{
    static const char fn[] = "o2v_hip_flood_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!out) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    return cc_run(ctx, fn, grid, format, strides, dims, level, connectivity, flags, nullptr, out, out_strides, seeds, n_seeds, values, out_reached);
}

int o2v_hip_components_times(const o2v_hip_ctx *ctx, float out_ms[5]) { return ctx ? ctx->cc_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

int o2v_hip_components_counters(const o2v_hip_ctx *ctx, uint64_t out2[2])
{
    if (!ctx || !out2) return O2V_HIP_ERR_BAD_ARGUMENT;
    out2[0] = ctx->cc_counters[0];
    out2[1] = ctx->cc_counters[1];
    return O2V_HIP_OK;
}

}  // extern "C"

// ---- K20: geodesic distances and shortest paths through a dense grid -----------------------------------------------------------

namespace {

constexpr uint32_t kGeoFlagsKnown = O2V_HIP_CC_INVERT | O2V_HIP_CC_SEED_BORDER | O2V_HIP_FLAG_STAGE_TIMES;

static_assert(kGeoMaxDistance == O2V_HIP_GEO_MAX_DISTANCE && kGeoMaxWeight == O2V_HIP_GEO_MAX_WEIGHT, "one set of limits for the callers and the kernels");

uint64_t geo_tiles(const uint32_t dims[3]) { return bit_tiles(bit_grid(dims)); }

// The worklist of a relaxation over tiles (k_geo_tiles, k_grow_tiles): of an array of [4][tiles] words the two alternating flag
// words of every tile and the two lists; of the family's counter block three uint32 on the device and their page-locked copies:
// the lengths of the two lists and the changed word of the whole-grid sweeps.
struct TileRounds {
    uint32_t *tile_flags[2], *tile_list[2];
    uint32_t *cnt;
    volatile uint32_t *h_cnt;
};

TileRounds tile_rounds(uint32_t *words, uint64_t tiles, unsigned long long *cnt, unsigned long long *h_cnt)
{
    return TileRounds{{words, words + tiles}, {words + 2u * tiles, words + 3u * tiles}, reinterpret_cast<uint32_t *>(cnt), reinterpret_cast<volatile uint32_t *>(h_cnt)};
}

struct RoundCounts {
    uint64_t rounds, visits, reads;   // launches, listed tiles over all of them, 4-byte reads by the host
};

// The rounds of one relaxation, from round 0's list (or from nothing: the whole-grid sweeps) to its fixed point.  launch_tiles(cur,
// nxt, n, blocks) enqueues the tile kernel over list cur of n tiles; launch_sweep(changed) one sweep over the whole grid
// (O2V_*_NO_TILES).  No cap: a round is launched only if the last one moved a value on a tile's rim (tiles) or anywhere (sweeps),
// and the values are whole numbers that move one way between fixed bounds.
template <typename Tiles, typename Sweep>
int run_tile_rounds(o2v_hip_ctx *ctx, const TileRounds &tr, bool use_tiles, Tiles &&launch_tiles, Sweep &&launch_sweep, RoundCounts *out)
{
    hipStream_t s = ctx->stream;
    uint32_t *const h_cnt = const_cast<uint32_t *>(tr.h_cnt);
    *out = RoundCounts{};
    if (use_tiles) {
        O2V_CHECK(hipMemcpyAsync(h_cnt, tr.cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        O2V_CHECK(hipStreamSynchronize(s));
        ++out->reads;
        for (uint32_t cur = 0, n = tr.h_cnt[0]; n; cur ^= 1u, n = tr.h_cnt[cur]) {
            const uint32_t nxt = cur ^ 1u;
            O2V_CHECK(hipMemsetAsync(tr.cnt + nxt, 0, sizeof(uint32_t), s));
            launch_tiles(cur, nxt, n, dim3((uint32_t) std::min<uint64_t>(n, kCcMaxGrid)));
            O2V_CHECK(hipMemcpyAsync(h_cnt + nxt, tr.cnt + nxt, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            O2V_CHECK(hipStreamSynchronize(s));
            ++out->rounds, ++out->reads, out->visits += n;
        }
    } else {
        do {
            O2V_CHECK(hipMemsetAsync(tr.cnt + 2, 0, sizeof(uint32_t), s));
            launch_sweep(tr.cnt + 2);
            O2V_CHECK(hipMemcpyAsync(h_cnt + 2, tr.cnt + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            O2V_CHECK(hipStreamSynchronize(s));
            ++out->rounds, ++out->reads;
        } while (tr.h_cnt[2]);
    }
    return O2V_HIP_OK;
}

// weights: each 0 ... 65 535, not all 0
int geo_weights(o2v_hip_ctx *ctx, const char *fn, const uint32_t weights[3])
{
    for (int a = 0; a < 3; ++a)
        if (weights[a] > kGeoMaxWeight) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "a weight of " + std::to_string(weights[a]) + " is above 65 535");
    if (!(weights[0] | weights[1] | weights[2])) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "the weights are all 0: no step exists");
    return O2V_HIP_OK;
}

}  // namespace

extern "C" {

uint64_t o2v_hip_geodesic_scratch_bytes(const uint32_t dims[3], uint32_t which)
{
    if (!dims || !dims[0] || !dims[1] || !dims[2] || which > O2V_HIP_GEO_SCRATCH_STRIDED) return 0;
    return 8u * cc_words(dims) + 16u * geo_tiles(dims) + 64u + (which == O2V_HIP_GEO_SCRATCH_STRIDED ? 4u * (uint64_t) dims[0] * dims[1] * dims[2] : 0u);
}

int o2v_hip_geodesic_dense(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                           const uint32_t weights[3], uint32_t flags, const int32_t *seeds, uint64_t n_seeds, uint32_t max_distance, int32_t *dist,
                           const uint64_t dist_strides[3], uint64_t *out_reached)
{
    static const char fn[] = "o2v_hip_geodesic_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    const Switches sw = read_switches();
    if (!dist || !dist_strides || !out_reached || !weights || (n_seeds && !seeds)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    SetGrid sg;
    int rc;
    if ((rc = set_grid(ctx, fn, grid, format, strides, dims, level, &sg)) || (rc = geo_weights(ctx, fn, weights))) return rc;
    if (max_distance > kGeoMaxDistance) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "max_distance is above 2^31 - 2");
    if (flags & ~kGeoFlagsKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if ((uintptr_t) dist % sizeof(int32_t)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "dist must be 4-byte aligned");
    if ((rc = index_limits(ctx, fn, dims, n_seeds, "seeds"))) return rc;
    const OutGrid outs[] = {{"dist", dist, dist_strides, 4u}};
    Span spans[3] = {{}, {"grid", grid, sg.bytes}, {"seeds", seeds, n_seeds * 12u}};
    if ((rc = check_outputs(ctx, fn, outs, dims, spans)) || (n_seeds && (rc = check_device_range(ctx, fn, seeds, n_seeds * 12u, "seeds"))) ||
        (rc = refuse_overlap(ctx, fn, spans, 1)))
        return rc;

    const BitGrid bg = bit_grid(dims);
    const GeoGrid g{bg, bit_tiles_y(bg), bit_tiles_z(bg), {weights[0], weights[1], weights[2]}, max_distance};
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2], tiles = geo_tiles(dims);   // (tiles: at most the words, below 2^31)
    // the distances live in the caller's dist where linear index i is element i of it
    const bool in_place = linear_layout(dims, dist_strides);
    if ((rc = grow_scratch(ctx, ctx->d_geo_bits, g.words, fn, "set bits")) || (rc = grow_scratch(ctx, ctx->d_geo_tiles, 4u * tiles, fn, "tile flags and lists")) ||
        (rc = grow_scratch(ctx, ctx->d_geo_ctr, 8u, fn, "counters")) || (rc = grow_scratch(ctx, ctx->h_geo_ctr, 8u, fn, "counters")) ||
        (!in_place && (rc = grow_scratch(ctx, ctx->d_geo_dist, voxels, fn, "distances"))))
        return rc;
    uint32_t *const D = in_place ? reinterpret_cast<uint32_t *>(dist) : ctx->d_geo_dist.ptr;
    unsigned long long *const bits = ctx->d_geo_bits.ptr, *const ctr = ctx->d_geo_ctr.ptr;
    const TileRounds tr = tile_rounds(ctx->d_geo_tiles.ptr, tiles, ctr + 2, ctx->h_geo_ctr.ptr + 2);
    const bool count = (flags & O2V_HIP_FLAG_STAGE_TIMES) != 0, use_tiles = !sw.geo_no_tiles;
    const dim3 per_word(stream_grid(ctx, g.words * 64u, 16u));
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->geo_times.mark(0, s));
    O2V_CHECK(hipMemsetAsync(ctr, 0, 8u * sizeof(unsigned long long), s));
    launch_classify(ctx, sg, (flags & O2V_HIP_CC_INVERT) ? 1u : 0u, bits);
    O2V_CHECK(ctx->geo_times.mark(1, s));
    O2V_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(D), (int) kGeoInf, voxels, s));
    if (use_tiles) O2V_CHECK(hipMemsetAsync(tr.tile_flags[0], 0, 2u * tiles * sizeof(uint32_t), s));
    uint32_t *const fl0 = use_tiles ? tr.tile_flags[0] : nullptr;
    if (n_seeds)
        O2V_LAUNCH("k_geo_seed_list", s, k_geo_seed_list, dim3(stream_grid(ctx, n_seeds, 8u)), dim3(kBlock), 0, s, g, bits, seeds, n_seeds, D, fl0, tr.tile_list[0], tr.cnt);
    if (flags & O2V_HIP_CC_SEED_BORDER) O2V_LAUNCH("k_geo_seed_border", s, k_geo_seed_border, per_word, dim3(kBlock), 0, s, g, bits, D, fl0, tr.tile_list[0], tr.cnt);
    O2V_CHECK(ctx->geo_times.mark(2, s));
    RoundCounts done;
    rc = run_tile_rounds(
        ctx, tr, use_tiles,
        [&](uint32_t cur, uint32_t nxt, uint32_t n, dim3 blocks) {
            with_flag(count, [&](auto counts) {
                O2V_LAUNCH("k_geo_tiles", s, k_geo_tiles<decltype(counts)::value>, blocks, dim3(kBlock), 0, s, g, bits, D, tr.tile_list[cur], n, tr.tile_flags[cur],
                           tr.tile_flags[nxt], tr.tile_list[nxt], tr.cnt + nxt, ctr);
            });
        },
        [&](uint32_t *changed) { O2V_LAUNCH("k_geo_sweep", s, k_geo_sweep, per_word, dim3(kBlock), 0, s, g, bits, D, changed); }, &done);
    if (rc) return rc;
    O2V_CHECK(ctx->geo_times.mark(3, s));
    O2V_LAUNCH("k_geo_write", s, k_geo_write, per_word, dim3(kBlock), 0, s, g, D, dist, dist_strides[0], dist_strides[1], dist_strides[2], ctr + 1);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(ctx->geo_times.mark(4, s));
    O2V_CHECK(hipMemcpyAsync(ctx->h_geo_ctr.ptr, ctr, 2u * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(ctx->geo_times.finish());
    const uint64_t counters[4] = {done.rounds, done.visits, ctx->h_geo_ctr.ptr[0], done.reads};
    for (int i = 0; i < 4; ++i) ctx->geo_counters[i] = count ? counters[i] : 0u;
    *out_reached = ctx->h_geo_ctr.ptr[1];
    return O2V_HIP_OK;
}

int o2v_hip_geodesic_paths(o2v_hip_ctx *ctx, const int32_t *dist, const uint64_t dist_strides[3], const uint32_t dims[3], const uint32_t weights[3],
                           const int32_t *targets, uint64_t n_targets, uint32_t max_len, int32_t *paths, int32_t *lengths)
{
    static const char fn[] = "o2v_hip_geodesic_paths";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!dist || !dist_strides || !dims || !weights || (n_targets && (!targets || !lengths || (max_len && !paths))))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if (!dims[0] || !dims[1] || !dims[2]) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "zero dims");
    int rc;
    if ((rc = geo_weights(ctx, fn, weights))) return rc;
    if ((uintptr_t) dist % sizeof(int32_t)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "dist must be 4-byte aligned");
    if ((rc = index_limits(ctx, fn, dims, n_targets, "targets"))) return rc;
    O2V_CHECK(hipSetDevice(ctx->device));
    const unsigned __int128 want = (unsigned __int128) n_targets * max_len * 12u;
    if (want > (unsigned __int128) (~0ull >> 1)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "paths: n_targets rows of max_len voxels reach past any allocation");
    const uint64_t pbytes = (uint64_t) want;
    uint64_t dbytes = 0;
    if ((rc = check_grid(ctx, fn, "dist", dist, dims, dist_strides, 4u, false, &dbytes))) return rc;
    if (!n_targets) return O2V_HIP_OK;
    if ((rc = check_device_range(ctx, fn, targets, n_targets * 12u, "targets")) || (rc = check_device_range(ctx, fn, lengths, n_targets * 4u, "lengths")) ||
        (pbytes && (rc = check_device_range(ctx, fn, paths, pbytes, "paths"))))
        return rc;
    const Span spans[] = {{"paths", paths, pbytes}, {"lengths", lengths, n_targets * 4u}, {"dist", dist, dbytes}, {"targets", targets, n_targets * 12u}};
    if ((rc = refuse_overlap(ctx, fn, spans, 2))) return rc;
    GeoTrace t{};
    for (int a = 0; a < 3; ++a) t.dims[a] = dims[a], t.w[a] = weights[a], t.s[a] = dist_strides[a];
    hipStream_t s = ctx->stream;
    O2V_LAUNCH("k_geo_trace", s, k_geo_trace, dim3(stream_grid(ctx, n_targets, 8u)), dim3(kBlock), 0, s, t, dist, targets, n_targets, max_len, paths, lengths);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipStreamSynchronize(s));
    return O2V_HIP_OK;
}

int o2v_hip_geodesic_times(const o2v_hip_ctx *ctx, float out_ms[4]) { return ctx ? ctx->geo_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

int o2v_hip_geodesic_counters(const o2v_hip_ctx *ctx, uint64_t out4[4])
{
    if (!ctx || !out4) return O2V_HIP_ERR_BAD_ARGUMENT;
    std::copy(ctx->geo_counters, ctx->geo_counters + 4, out4);
    return O2V_HIP_OK;
}

}  // extern "C"
