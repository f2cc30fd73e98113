// Host side of K13, K14 and K16 (o2v_dev_k13_gather.hpp, _k14_faces.hpp, _k16_rects.hpp): they share colour modes, palette and count / write.

// ---- K13: the solid voxels of a dense grid as (x, y, z, argb) records ---------------------------------------------------------

namespace {

constexpr uint64_t kGaMaxWords = 0x7fffffffull;   // a word index is one uint32 in bits_word_at (o2v_dev_bits.hpp)
constexpr uint64_t kGaMaxGrid = 1ull << 20;       // workgroups of k_gather_count; more blocks are taken in turns
constexpr uint64_t kGaBatch = 1u << 20;           // records per batch of o2v_hip_gather_save: the batch of drain_to_sink (o2v_api.cpp)

// what the three calls check of the grid; *sg: the set grid, *g: its words
int ga_grid(o2v_hip_ctx *ctx, const char *fn, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
            SetGrid *sg, GaGrid *g)
{
    if (int rc; (rc = set_grid(ctx, fn, grid, format, strides, dims, level, sg)) || (rc = axis_limit(ctx, fn, dims))) return rc;
    const BitGrid bg = bit_grid(dims);   // (words: below 2^43)
    if (bg.words > kGaMaxWords) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, std::to_string(bg.words) + " words of 64 voxels along x (at most 2^31 - 1)");
    *g = GaGrid{bg, (bg.words + kBlock - 1) / kBlock};
    return O2V_HIP_OK;
}

// what _write and _save check of the origin and the colour mode (nothing is read through a pointer here)
int ga_mode(o2v_hip_ctx *ctx, const char *fn, uint32_t format, const uint32_t dims[3], const uint32_t origin[3], uint32_t color_mode)
{
    if (!origin) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if (color_mode != O2V_HIP_GATHER_COLOR_CONSTANT && color_mode != O2V_HIP_GATHER_COLOR_GRID && color_mode != O2V_HIP_GATHER_COLOR_PALETTE)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown color_mode " + std::to_string(color_mode));
    if (color_mode == O2V_HIP_GATHER_COLOR_PALETTE && format != O2V_HIP_GRID_U8)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "O2V_HIP_GATHER_COLOR_PALETTE needs a U8 grid");
    return extent_limit(ctx, fn, origin, dims, 1ull << 32, "origin + dims is above 2^32 along an axis");
}

// the pointers the colour mode reads; *cbytes: the reach of colors (GRID)
int ga_color_source(o2v_hip_ctx *ctx, const char *fn, const uint32_t dims[3], uint32_t color_mode, const uint32_t *colors,
                    const uint64_t color_strides[3], const uint32_t *palette, uint64_t *cbytes)
{
    *cbytes = 0;
    if (color_mode == O2V_HIP_GATHER_COLOR_GRID) {
        if (!colors || !color_strides) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
        return check_grid(ctx, fn, "colors", colors, dims, color_strides, 4u, false, cbytes);
    }
    if (color_mode == O2V_HIP_GATHER_COLOR_PALETTE && !palette) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    return O2V_HIP_OK;
}

bool ga_matches(const o2v_hip_ctx *ctx, const SetGrid &sg) { return ctx->ga.valid && ctx->ga.key == sg.key; }

// classify, count and scan; the count is kept in the context and returned
int ga_count(o2v_hip_ctx *ctx, const char *fn, const SetGrid &sg, const GaGrid &g, uint64_t *out_count)
{
    int rc;
    if ((rc = grow_scratch(ctx, ctx->d_ga_bits, g.words, fn, "set bits")) || (rc = grow_scratch(ctx, ctx->d_ga_local, g.words, fn, "prefixes")) ||
        (rc = grow_scratch(ctx, ctx->d_ga_boff, g.n_blocks + 1u, fn, "block offsets")) || (rc = grow_scratch(ctx, ctx->d_ga_first, 1u, fn, "range")) ||
        (rc = grow_scratch(ctx, ctx->h_ga_ctr, 1u, fn, "counters")))
        return rc;
    unsigned long long *const bits = ctx->d_ga_bits.ptr, *const boff = ctx->d_ga_boff.ptr;
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->ga_times.mark(0, s));
    launch_classify(ctx, sg, 0u, bits);
    O2V_CHECK(ctx->ga_times.mark(1, s));
    O2V_LAUNCH("k_gather_count", s, k_gather_count, dim3((uint32_t) std::min<uint64_t>(g.n_blocks, kGaMaxGrid)), dim3(kBlock), 0, s, bits, g,
               ctx->d_ga_local.ptr, boff);
    uint64_t total = 0;
    if ((rc = count_total(ctx, boff, g.n_blocks, ctx->h_ga_ctr, ctx->ga_times, &total))) return rc;
#ifdef O2V_GA_MUTATE_COUNT32
    total = (uint32_t) total;   // (test only: the count truncated where the host reads it)
#endif
    ctx->ga.valid = true;
    ctx->ga.key = sg.key;
    ctx->ga.total = total;
    *out_count = total;
    return O2V_HIP_OK;
}

// The 256 colours of a PALETTE call into the context's device copy, on the stream.  K13 and K14 share the copy: every call that
// reads it uploads its own palette ahead of its launches and has waited for the stream when it returns.
int upload_palette(o2v_hip_ctx *ctx, const char *fn, const uint32_t *palette)
{
    if (int rc; (rc = grow_scratch(ctx, ctx->d_palette, 256u, fn, "palette")) || (rc = grow_scratch(ctx, ctx->h_palette, 256u, fn, "palette"))) return rc;
    std::memcpy(ctx->h_palette.ptr, palette, 256u * sizeof(uint32_t));
    O2V_CHECK(hipMemcpyAsync(ctx->d_palette.ptr, ctx->h_palette.ptr, 256u * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    return O2V_HIP_OK;
}

// records [first, first + n) of the last count into `records`, enqueued on the stream (n > 0; events 2 and 3 of ga_times around it)
int ga_launch_write(o2v_hip_ctx *ctx, const GaGrid &g, uint64_t first, uint64_t n, const uint32_t origin[3], uint32_t color_mode,
                    const GaColor &col, uint32_t *records)
{
    hipStream_t s = ctx->stream;
    const unsigned long long *const boff = ctx->d_ga_boff.ptr;
    uint4 *const out = reinterpret_cast<uint4 *>(records);
    // a workgroup per block the range may touch: one per 2^14 records and the two at its ends, and no more than fill the device
    const dim3 blocks((uint32_t) std::min<uint64_t>(std::min<uint64_t>(g.n_blocks, n / 64u + 2u), (uint64_t) ctx->num_cus * 8u));
    O2V_CHECK(hipEventRecord(ctx->ga_times.ev[2], s));
    O2V_LAUNCH("k_gather_find", s, k_gather_find, dim3(1), dim3(kBlock), 0, s, boff, g.n_blocks, first, ctx->d_ga_first.ptr);
    with_color_mode(color_mode, [&](auto mode) {
        O2V_LAUNCH("k_gather_write", s, k_gather_write<decltype(mode)::value>, blocks, dim3(kBlock), 0, s, g, ctx->d_ga_bits.ptr, ctx->d_ga_local.ptr, boff,
                   ctx->d_ga_first.ptr, first, n, origin[0], origin[1], origin[2], col, out);
    });
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipEventRecord(ctx->ga_times.ev[3], s));
    return O2V_HIP_OK;
}

// *col: what the colour mode reads, as the kernels of K13 and K14 take it; PALETTE: uploaded first
int ga_color(o2v_hip_ctx *ctx, const char *fn, const SetGrid &sg, uint32_t color_mode, uint32_t argb, const uint32_t *colors,
             const uint64_t color_strides[3], const uint32_t *palette, GaColor *col)
{
    *col = GaColor{};
    col->argb = argb;
    if (color_mode == O2V_HIP_GATHER_COLOR_GRID) col->colors = colors, col->c0 = color_strides[0], col->c1 = color_strides[1], col->c2 = color_strides[2];
    if (color_mode == O2V_HIP_GATHER_COLOR_PALETTE) {
        if (int rc = upload_palette(ctx, fn, palette)) return rc;
        col->grid = static_cast<const uint8_t *>(sg.key.p);
        col->s0 = sg.key.strides[0], col->s1 = sg.key.strides[1], col->s2 = sg.key.strides[2];
        col->palette = ctx->d_palette.ptr;
    }
    return O2V_HIP_OK;
}

bool ga_output_format(FileFormat f)
{
    return f == FileFormat::VL32 || f == FileFormat::PLY || f == FileFormat::XYZRGB || f == FileFormat::QEF || f == FileFormat::VOX;
}

}  // namespace

extern "C" {

uint64_t o2v_hip_gather_scratch_bytes(const uint32_t dims[3])
{
    if (!dims || !dims[0] || !dims[1] || !dims[2]) return 0;
    const uint64_t words = cc_words(dims);
    return 12u * words + 8u * ((words + kBlock - 1) / kBlock + 1u) + 1024u + 8u;
}

int o2v_hip_gather_count(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                         uint64_t *out_count)
{
    static const char fn[] = "o2v_hip_gather_count";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    ctx->ga.valid = false;
    if (!out_count) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    SetGrid sg;
    GaGrid g{};
    if (int rc = ga_grid(ctx, fn, grid, format, strides, dims, level, &sg, &g)) return rc;
    return ga_count(ctx, fn, sg, g, out_count);
}

int o2v_hip_gather_write(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                         const uint32_t origin[3], uint32_t color_mode, uint32_t argb, const uint32_t *colors, const uint64_t color_strides[3],
                         const uint32_t *palette, uint64_t first, uint64_t n, uint32_t *records)
{
    static const char fn[] = "o2v_hip_gather_write";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    SetGrid sg;
    GaGrid g{};
    uint64_t cbytes = 0;
    int rc;
    if ((rc = ga_grid(ctx, fn, grid, format, strides, dims, level, &sg, &g)) || (rc = ga_mode(ctx, fn, format, dims, origin, color_mode))) return rc;
    if (!ga_matches(ctx, sg))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "no matching o2v_hip_gather_count (the same grid, format, strides, dims and level)");
    const uint64_t total = ctx->ga.total;
    if (first > total || n > total - first)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn,
                      "records " + std::to_string(first) + " + " + std::to_string(n) + " reach past the counted " + std::to_string(total));
    if (n == 0) return O2V_HIP_OK;
    if (!records) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((rc = ga_color_source(ctx, fn, dims, color_mode, colors, color_strides, palette, &cbytes))) return rc;
    if (n > (~0ull >> 4)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "records: n * 16 bytes reach past any allocation");
    if ((uintptr_t) records % 16u) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "records must be 16-byte aligned");
    if ((rc = check_device_range(ctx, fn, records, n * 16u, "records"))) return rc;
    const Span spans[] = {{"records", records, n * 16u}, {"grid", grid, sg.bytes}, {"colors", colors, cbytes}};
    if ((rc = refuse_overlap(ctx, fn, spans, 1))) return rc;
    GaColor col;
    if ((rc = ga_color(ctx, fn, sg, color_mode, argb, colors, color_strides, palette, &col)) ||
        (rc = ga_launch_write(ctx, g, first, n, origin, color_mode, col, records)))
        return rc;
    O2V_CHECK(hipStreamSynchronize(ctx->stream));
    O2V_CHECK(ctx->ga_times.elapsed(2, 3, ctx->ga_times.ms[2]));
    return O2V_HIP_OK;
}

int o2v_hip_gather_save(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                        const uint32_t origin[3], uint32_t color_mode, uint32_t argb, const uint32_t *colors, const uint64_t color_strides[3],
                        const uint32_t *palette, const char *path, const char *type, uint32_t resolution, uint64_t *out_count)
{
    static const char fn[] = "o2v_hip_gather_save";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    ctx->ga.valid = false;
    if (!path || !out_count) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    SetGrid sg;
    GaGrid g{};
    uint64_t cbytes = 0;
    int rc;
    if ((rc = ga_grid(ctx, fn, grid, format, strides, dims, level, &sg, &g)) || (rc = ga_mode(ctx, fn, format, dims, origin, color_mode)) ||
        (rc = ga_color_source(ctx, fn, dims, color_mode, colors, color_strides, palette, &cbytes)))
        return rc;
    for (int a = 0; a < 3; ++a)
        if ((uint64_t) origin[a] + dims[a] > resolution)
            return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "origin + dims is above the resolution " + std::to_string(resolution) + " along an axis");
    const FileFormat file_format = detect_format(path, type);
    if (!ga_output_format(file_format))
        return refuse(ctx, O2V_HIP_ERR_IO, fn, std::string("\"") + (type ? type : path) + "\" is not an output format (VL32, PLY, XYZRGB, QEF, VOX)");
    uint64_t total = 0;
    if ((rc = ga_count(ctx, fn, sg, g, &total))) return rc;
    for (int k = 0; k < 2; ++k) {
        if ((rc = grow_scratch(ctx, ctx->d_ga_rec[k], kGaBatch, fn, "record buffer")) || (rc = grow_scratch(ctx, ctx->h_ga_rec[k], kGaBatch * 4u, fn, "staging")))
            return rc;
        O2V_CHECK(ctx->ev_ga_rec[k].create_sync());
    }
    std::unique_ptr<VoxelSink> sink = open_file_sink(path, file_format, resolution);
    if (!sink) return refuse(ctx, O2V_HIP_ERR_IO, fn, std::string("cannot open \"") + path + "\" for writing");
    sink->expect(total);
    GaColor col;
    if ((rc = ga_color(ctx, fn, sg, color_mode, argb, colors, color_strides, palette, &col))) return rc;
    hipStream_t s = ctx->stream;
    const uint64_t batches = (total + kGaBatch - 1) / kGaBatch;
    // Two record buffers and two page-locked batches: while the sink consumes one batch the next is written and copied.
    auto start = [&](uint64_t k) -> int {
        const uint64_t first = k * kGaBatch, n = std::min<uint64_t>(kGaBatch, total - first);
        if (int e = ga_launch_write(ctx, g, first, n, origin, color_mode, col, reinterpret_cast<uint32_t *>(ctx->d_ga_rec[k & 1].ptr))) return e;
        O2V_CHECK(hipMemcpyAsync(ctx->h_ga_rec[k & 1].ptr, ctx->d_ga_rec[k & 1].ptr, n * 16u, hipMemcpyDeviceToHost, s));
        O2V_CHECK(hipEventRecord(ctx->ev_ga_rec[k & 1], s));
        return O2V_HIP_OK;
    };
    rc = batches ? start(0) : O2V_HIP_OK;
    for (uint64_t k = 0; k < batches && rc == O2V_HIP_OK; ++k) {
        if (!sink->can_write()) break;
        if (hipEventSynchronize(ctx->ev_ga_rec[k & 1]) != hipSuccess) {
            rc = refuse(ctx, O2V_HIP_ERR_HIP, fn, "waiting for a batch of records failed");
            break;
        }
        if (k + 1 < batches && (rc = start(k + 1))) break;
        sink->write(ctx->h_ga_rec[k & 1].ptr, (size_t) std::min<uint64_t>(kGaBatch, total - k * kGaBatch));
    }
    const hipError_t drained = hipStreamSynchronize(s);   // (nothing is on its way into the batches when the call returns)
    if (rc) return rc;
    if (drained != hipSuccess) return refuse(ctx, O2V_HIP_ERR_HIP, fn, std::string("hipStreamSynchronize: ") + hipGetErrorString(drained));
    if (batches) O2V_CHECK(ctx->ga_times.elapsed(2, 3, ctx->ga_times.ms[2]));
    if (sink->can_write()) sink->finalize();
    if (!sink->can_write()) return refuse(ctx, O2V_HIP_ERR_IO, fn, std::string("writing \"") + path + "\" failed: the sink stopped accepting voxels");
    *out_count = total;
    return O2V_HIP_OK;
}

int o2v_hip_gather_times(const o2v_hip_ctx *ctx, float out_ms[3]) { return ctx ? ctx->ga_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"

// ---- K14: the exposed voxel faces of a dense grid as coloured quads -----------------------------------------------------------

namespace {

constexpr uint64_t kFaMaxExtent = 65536;          // origin + dims per axis: a coordinate is an exact float32
constexpr uint64_t kFaMaxQuads = 0x7fffffffull / 4u;   // 4 Q <= 2^31 - 1: a vertex index is one int32
constexpr uint64_t kFaMaxGrid = 1ull << 20;       // workgroups of k_faces_count; more blocks are taken in turns

// what both calls check: the grid as the gather checks it, the merge and colour modes and the pointers the colour mode reads;
// *sg: the set grid, *g: the words and items, *cbytes: the reach of colors (GRID)
int fa_args(o2v_hip_ctx *ctx, const char *fn, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
            uint32_t merge, uint32_t color_mode, const uint32_t *colors, const uint64_t color_strides[3], const uint32_t *palette, SetGrid *sg,
            FaGrid *g, uint64_t *cbytes)
{
    GaGrid gg{};
    static const uint32_t no_origin[3] = {0, 0, 0};
    int rc;
    if ((rc = ga_grid(ctx, fn, grid, format, strides, dims, level, sg, &gg))) return rc;
    if (merge != O2V_HIP_FACES_MERGE_NONE && merge != O2V_HIP_FACES_MERGE_RUNS && merge != O2V_HIP_FACES_MERGE_RECTS)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown merge " + std::to_string(merge));
    if ((rc = ga_mode(ctx, fn, format, dims, no_origin, color_mode)) ||
        (rc = ga_color_source(ctx, fn, dims, color_mode, colors, color_strides, palette, cbytes)))
        return rc;
    const uint64_t items = 6u * gg.words;
    *g = FaGrid{gg, merge, merge != O2V_HIP_FACES_MERGE_NONE && color_mode != O2V_HIP_GATHER_COLOR_CONSTANT, items, (items + kBlock - 1) / kBlock};
    return O2V_HIP_OK;
}

bool fa_matches(const o2v_hip_ctx *ctx, const SetGrid &sg, uint32_t merge, uint32_t color_mode, uint32_t argb, const uint32_t *colors,
                const uint64_t color_strides[3], const uint32_t *palette)
{
    const o2v_hip_ctx::FacesCount &c = ctx->fa;
    if (!c.valid || !(c.key == sg.key) || c.merge != merge || c.color_mode != color_mode) return false;
    if (color_mode == O2V_HIP_GATHER_COLOR_GRID) return c.colors == colors && std::equal(color_strides, color_strides + 3, c.color_strides);
    if (color_mode == O2V_HIP_GATHER_COLOR_PALETTE) return std::equal(palette, palette + 256, c.palette);
    return c.argb == argb;
}

FaBits fa_bits(const o2v_hip_ctx *ctx) { return FaBits{ctx->d_fa_bits.ptr, ctx->d_fa_same_x.ptr, ctx->d_fa_same_y.ptr}; }

}  // namespace

extern "C" {

uint64_t o2v_hip_faces_scratch_bytes(const uint32_t dims[3], uint32_t color_mode)
{
    if (!dims || !dims[0] || !dims[1] || !dims[2]) return 0;
    const uint64_t words = cc_words(dims);
    return (color_mode == O2V_HIP_GATHER_COLOR_CONSTANT ? 8u : 24u) * words + 8u * ((6u * words + kBlock - 1) / kBlock + 1u) + 1024u;
}

uint64_t o2v_hip_faces_scratch_bytes_merge(const uint32_t dims[3], uint32_t color_mode, uint32_t merge)
{
    const uint64_t bytes = o2v_hip_faces_scratch_bytes(dims, color_mode);
    if (!bytes || merge != O2V_HIP_FACES_MERGE_RECTS) return bytes;
    return bytes + (color_mode == O2V_HIP_GATHER_COLOR_CONSTANT ? 48u : 56u) * cc_words(dims);
}

int o2v_hip_faces_count(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                        uint32_t merge, uint32_t color_mode, uint32_t argb, const uint32_t *colors, const uint64_t color_strides[3],
                        const uint32_t *palette, uint64_t *out_quads)
{
    static const char fn[] = "o2v_hip_faces_count";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    ctx->fa.valid = false;
    if (!out_quads) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    SetGrid sg;
    FaGrid g{};
    uint64_t cbytes = 0;
    int rc;
    if ((rc = fa_args(ctx, fn, grid, format, strides, dims, level, merge, color_mode, colors, color_strides, palette, &sg, &g, &cbytes))) return rc;
    const bool rects = merge == O2V_HIP_FACES_MERGE_RECTS;
    if ((rc = grow_scratch(ctx, ctx->d_fa_bits, g.words, fn, "set bits")) ||
        (g.colored && ((rc = grow_scratch(ctx, ctx->d_fa_same_x, g.words, fn, "same-colour bits")) ||
                       (rc = grow_scratch(ctx, ctx->d_fa_same_y, g.words, fn, "same-colour bits")))) ||
        (rects && ((g.colored && (rc = grow_scratch(ctx, ctx->d_rc_same_z, g.words, fn, "same-colour bits"))) ||
                   (rc = grow_scratch(ctx, ctx->d_rc_starts, g.items, fn, "rectangle starts")))) ||
        (rc = grow_scratch(ctx, ctx->d_fa_boff, g.n_blocks + 1u, fn, "block offsets")) || (rc = grow_scratch(ctx, ctx->h_fa_ctr, 1u, fn, "counters")))
        return rc;
    unsigned long long *const bits = ctx->d_fa_bits.ptr, *const boff = ctx->d_fa_boff.ptr;
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->fa_times.mark(0, s));
    launch_classify(ctx, sg, 0u, bits);
    if (g.colored) {
        // a wavefront per word in turns
        const dim3 per_word(stream_grid(ctx, g.words * 64u, 8u));
        GaColor col;
        if ((rc = ga_color(ctx, fn, sg, color_mode, argb, colors, color_strides, palette, &col))) return rc;
        // (GRID or PALETTE here: the kernels have no CONSTANT variant)
        with_flag(color_mode == O2V_HIP_GATHER_COLOR_PALETTE, [&](auto pal) {
            constexpr uint32_t mode = decltype(pal)::value ? kGaColorPalette : kGaColorGrid;
            O2V_LAUNCH("k_faces_same", s, k_faces_same<mode>, per_word, dim3(kBlock), 0, s, g, bits, col, ctx->d_fa_same_x.ptr, ctx->d_fa_same_y.ptr);
            if (rects) O2V_LAUNCH("k_rects_same_z", s, k_rects_same_z<mode>, per_word, dim3(kBlock), 0, s, g, bits, col, ctx->d_rc_same_z.ptr);
        });
    }
    O2V_CHECK(ctx->fa_times.mark(1, s));
    const dim3 count_grid((uint32_t) std::min<uint64_t>(g.n_blocks, kFaMaxGrid));
    if (rects)
        O2V_LAUNCH("k_rects_count", s, k_rects_count, count_grid, dim3(kBlock), 0, s, g, fa_bits(ctx), ctx->d_rc_same_z.ptr, ctx->d_rc_starts.ptr, boff);
    else
        O2V_LAUNCH("k_faces_count", s, k_faces_count, count_grid, dim3(kBlock), 0, s, g, fa_bits(ctx), boff);
    uint64_t total = 0;
    if ((rc = count_total(ctx, boff, g.n_blocks, ctx->h_fa_ctr, ctx->fa_times, &total))) return rc;
#ifdef O2V_FA_MUTATE_COUNT32
    total = (uint32_t) total;   // (test only: the count truncated where the host reads it)
#endif
    o2v_hip_ctx::FacesCount &c = ctx->fa;
    c.valid = true;
    c.key = sg.key;
    c.merge = merge;
    c.color_mode = color_mode;
    c.argb = argb;
    c.colors = color_mode == O2V_HIP_GATHER_COLOR_GRID ? colors : nullptr;
    if (color_mode == O2V_HIP_GATHER_COLOR_GRID) std::copy(color_strides, color_strides + 3, c.color_strides);
    if (color_mode == O2V_HIP_GATHER_COLOR_PALETTE) std::copy(palette, palette + 256, c.palette);
    c.total = total;
    *out_quads = total;
    return O2V_HIP_OK;
}

int o2v_hip_faces_write(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                        uint32_t merge, uint32_t color_mode, uint32_t argb, const uint32_t *colors, const uint64_t color_strides[3],
                        const uint32_t *palette, const uint32_t origin[3], float *positions, int32_t *faces, uint32_t *quad_argb,
                        uint64_t quad_capacity)
{
    static const char fn[] = "o2v_hip_faces_write";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    SetGrid sg;
    FaGrid g{};
    uint64_t cbytes = 0;
    int rc;
    if ((rc = fa_args(ctx, fn, grid, format, strides, dims, level, merge, color_mode, colors, color_strides, palette, &sg, &g, &cbytes))) return rc;
    if (!origin) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((rc = extent_limit(ctx, fn, origin, dims, kFaMaxExtent, "origin + dims is above 65 536 along an axis: a coordinate would not be exact in float32")))
        return rc;
    if (!fa_matches(ctx, sg, merge, color_mode, argb, colors, color_strides, palette))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn,
                      "no matching o2v_hip_faces_count (the same grid, format, strides, dims, level, merge and colour arguments)");
    const uint64_t total = ctx->fa.total;
    if (total > kFaMaxQuads)
        return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, std::to_string(total) + " quads: 4 vertices each are more than 2^31 - 1 int32 indices");
    if (quad_capacity < total)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn,
                      "quad_capacity " + std::to_string(quad_capacity) + " is below the counted " + std::to_string(total) + " quads");
    if (total == 0) return O2V_HIP_OK;
    if (!positions) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((uintptr_t) positions % 16u || (uintptr_t) faces % 8u || (uintptr_t) quad_argb % 4u)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "positions must be 16-byte, faces 8-byte and quad_argb 4-byte aligned");
    const Span spans[] = {{"positions", positions, total * 48u}, {"faces", faces, total * 24u}, {"quad_argb", quad_argb, total * 4u},
                          {"grid", grid, sg.bytes}, {"colors", colors, cbytes}};
    for (int i = 0; i < 3; ++i)
        if (spans[i].p && (rc = check_device_range(ctx, fn, spans[i].p, spans[i].bytes, spans[i].what))) return rc;
    if ((rc = refuse_overlap(ctx, fn, spans, 3))) return rc;
    GaColor col;
    if ((rc = ga_color(ctx, fn, sg, color_mode, argb, colors, color_strides, palette, &col))) return rc;
    hipStream_t s = ctx->stream;
    // a workgroup per block of items in turns, and no more than fill the device
    const dim3 blocks((uint32_t) std::min<uint64_t>(g.n_blocks, (uint64_t) ctx->num_cus * 8u));
    float4 *const pos = reinterpret_cast<float4 *>(positions);
    int2 *const tri = reinterpret_cast<int2 *>(faces);
    O2V_CHECK(hipEventRecord(ctx->fa_times.ev[2], s));
    const unsigned long long *const rstarts = ctx->d_rc_starts.ptr, *const boff = ctx->d_fa_boff.ptr;
    with_color_mode(color_mode, [&](auto mode) {
        if (merge == O2V_HIP_FACES_MERGE_RECTS)
            O2V_LAUNCH("k_rects_write", s, k_rects_write<decltype(mode)::value>, blocks, dim3(kBlock), 0, s, g, fa_bits(ctx), rstarts, boff, origin[0], origin[1],
                       origin[2], col, pos, tri, quad_argb);
        else
            O2V_LAUNCH("k_faces_write", s, k_faces_write<decltype(mode)::value>, blocks, dim3(kBlock), 0, s, g, fa_bits(ctx), boff, origin[0], origin[1], origin[2],
                       col, pos, tri, quad_argb);
    });
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipEventRecord(ctx->fa_times.ev[3], s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(ctx->fa_times.elapsed(2, 3, ctx->fa_times.ms[2]));
    return O2V_HIP_OK;
}

int o2v_hip_faces_times(const o2v_hip_ctx *ctx, float out_ms[3]) { return ctx ? ctx->fa_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"
