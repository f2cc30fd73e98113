// Host side of K9 and K18 (o2v_dev_k9_mesh_distance.hpp, o2v_dev_k18_crossings.hpp): they share the params, the box and the transform.

// ---- K9: narrow-band distance to the triangles -------------------------------------------------------------------------

namespace {

constexpr uint32_t kMdMaxDim = 65535;       // voxels per axis of one box (O2V_HIP_ERR_LIMIT above)
constexpr uint64_t kMdMaxGrid = 1ull << 24; // workgroups of k_meshdist_tiles; more tiles are taken in turns

// What K9 and K18 check of their params and their box, in this order: the supersampling and the resolution, the slab and tile
// fields, then per axis the box within the grid and its length.  *ss: the supersampling in effect.
int mesh_box_args(o2v_hip_ctx *ctx, const char *fn, const o2v_hip_params *params, const uint32_t origin[3], const uint32_t dims[3], uint32_t *ss)
{
    *ss = params->supersampling ? params->supersampling : 1u;
    if (*ss > 2u || params->resolution == 0u)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "resolution must be positive and supersampling 1 or 2");
    if (params->z_begin || params->z_end || params->x_begin || params->x_end || params->y_begin || params->y_end)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "the slab and tile fields of params must be 0 (the box is origin, dims)");
    for (int a = 0; a < 3; ++a) {
        if (!dims[a] || (uint64_t) origin[a] + dims[a] > params->resolution)
            return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "the box must have dims >= 1 and lie within the grid");
        if (dims[a] > kMdMaxDim) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "a box of more than 65 535 voxels along an axis");
    }
    return O2V_HIP_OK;
}

// The transform k_setup computes for these params (compute_mesh_transform of the caller's bounds or the mesh's own, which the
// upload reduced with k_bounds), as grid_box takes it; without triangles nothing reads it.
Affine mesh_box_transform(const o2v_hip_ctx *ctx, const o2v_hip_params *params, uint32_t ss)
{
    if (!ctx->n_tris) return Affine{};
    const float *e = params->bounds_known ? params->bounds : ctx->mesh_bounds_hint;
    return compute_mesh_transform(V3{e[0], e[1], e[2]}, V3{e[3], e[4], e[5]}, params->resolution * ss, params->unit_transform);
}

}  // namespace

extern "C" {

int o2v_hip_mesh_distance_dense(o2v_hip_ctx *ctx, const o2v_hip_params *params, float band, uint32_t format,
                                const uint32_t origin[3], const uint32_t dims[3], float *dst, const uint64_t dst_strides[3],
                                int32_t *closest, const uint64_t closest_strides[3])
{
    static const char fn[] = "o2v_hip_mesh_distance_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!params || !origin || !dims || !dst || !dst_strides || (closest && !closest_strides) || format > O2V_HIP_MESH_DIST_SIGNED_F32)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument or unknown format");
    if (!(std::isfinite(band) && band > 0.f && band <= 32.f))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "band must be finite, above 0 and at most 32 voxels");
    uint32_t ss = 0;
    int rc;
    if ((rc = mesh_box_args(ctx, fn, params, origin, dims, &ss))) return rc;
    O2V_CHECK(hipSetDevice(ctx->device));
    const OutGrid outs[] = {{"dst", dst, dst_strides, 4u}, {"closest", closest, closest_strides, 4u}};
    Span spans[2];
    if ((rc = check_outputs(ctx, fn, outs, dims, spans)) || (rc = refuse_overlap(ctx, fn, spans, 2))) return rc;

    const uint64_t T = ctx->n_tris;
    MdBox b{};
    b.x0 = origin[0], b.y0 = origin[1], b.z0 = origin[2];
    b.nx = dims[0], b.ny = dims[1], b.nz = dims[2];
    b.tx = (b.nx + kMdTile - 1) / kMdTile, b.ty = (b.ny + kMdTile - 1) / kMdTile, b.tz = (b.nz + kMdTile - 1) / kMdTile;
    b.ss = ss, b.band = band;
    b.margin = (double) band * ss + ss;
    b.bs2 = (double) band * band * ss * ss;
    b.n_tiles = (uint64_t) b.tx * b.ty * b.tz;
    const Affine xf = mesh_box_transform(ctx, params, ss);
    const uint64_t tile_blocks = (b.n_tiles + kBlock - 1) / kBlock;
    if ((rc = grow_scratch(ctx, ctx->d_md_sv, T * 9u, fn, "vertices")) || (rc = grow_scratch(ctx, ctx->d_md_counts, b.n_tiles, fn, "tile counters")) ||
        (rc = grow_scratch(ctx, ctx->d_md_first, b.n_tiles + 1u, fn, "tile offsets")) ||
        (rc = grow_scratch(ctx, ctx->d_md_blocks, tile_blocks, fn, "block sums")) || (rc = grow_scratch(ctx, ctx->d_md_ctr, 1u, fn, "counter")) ||
        (rc = grow_scratch(ctx, ctx->h_md_ctr, 1u, fn, "counter")))
        return rc;
    hipStream_t s = ctx->stream;
    const uint64_t tri_blocks = (T + kBlock - 1) / kBlock;

    // binning: (triangle, tile) pairs counted, scanned, scattered into per-tile lists
    O2V_CHECK(ctx->md_times.mark(0, s));
    O2V_CHECK(hipMemsetAsync(ctx->d_md_counts.ptr, 0, b.n_tiles * sizeof(uint32_t), s));
    if (T)
        O2V_LAUNCH("k_meshdist_bin_count", s, k_meshdist_bin_count, dim3((uint32_t) tri_blocks), dim3(kBlock), 0, s, ctx->d_verts.ptr, T, xf, b,
                   ctx->d_md_sv.ptr, ctx->d_md_counts.ptr);
    O2V_LAUNCH("k_meshdist_tile_sums", s, k_meshdist_tile_sums, dim3((uint32_t) tile_blocks), dim3(kBlock), 0, s, ctx->d_md_counts.ptr, b.n_tiles,
               ctx->d_md_blocks.ptr);
    O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, ctx->d_md_blocks.ptr, tile_blocks, ctx->d_md_ctr.ptr);
    O2V_LAUNCH("k_meshdist_tile_offsets", s, k_meshdist_tile_offsets, dim3((uint32_t) ((b.n_tiles + kBlock) / kBlock)), dim3(kBlock), 0, s,
               ctx->d_md_counts.ptr, b.n_tiles, ctx->d_md_blocks.ptr, ctx->d_md_ctr.ptr, ctx->d_md_first.ptr);
    O2V_CHECK(hipMemcpyAsync(ctx->h_md_ctr.ptr, ctx->d_md_ctr.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    const uint64_t n_pairs = ctx->h_md_ctr.ptr[0];
    if ((rc = grow_scratch(ctx, ctx->d_md_lists, n_pairs, fn, "triangle lists"))) return rc;
    if (n_pairs)
        O2V_LAUNCH("k_meshdist_bin_scatter", s, k_meshdist_bin_scatter, dim3((uint32_t) tri_blocks), dim3(kBlock), 0, s, ctx->d_md_sv.ptr, T, b,
                   ctx->d_md_first.ptr, ctx->d_md_counts.ptr, ctx->d_md_lists.ptr);
    O2V_CHECK(ctx->md_times.mark(1, s));

    // parity (signed): K6's bitmap of the box, no unmark step
    const uint32_t *bits = nullptr;
    if (format == O2V_HIP_MESH_DIST_SIGNED_F32 && T) {
        if ((rc = parity_bits(ctx, xf, fill_box(origin, dims, ss, 0u)))) {
            (void) hipGetLastError();
            return rc;
        }
        bits = ctx->d_fill_bits.ptr;
    }
    O2V_CHECK(ctx->md_times.mark(2, s));

    // distance: one workgroup per tile
    O2V_LAUNCH("k_meshdist_tiles", s, k_meshdist_tiles, dim3((uint32_t) std::min<uint64_t>(b.n_tiles, kMdMaxGrid)), dim3(kBlock), 0, s,
               ctx->d_md_sv.ptr, b, ctx->d_md_first.ptr, ctx->d_md_lists.ptr, bits, dst, dst_strides[0], dst_strides[1], dst_strides[2],
               closest, closest ? closest_strides[0] : 0u, closest ? closest_strides[1] : 0u, closest ? closest_strides[2] : 0u);
    O2V_CHECK(hipGetLastError());
    return finish_stages(ctx, ctx->md_times);
}

int o2v_hip_mesh_distance_times(const o2v_hip_ctx *ctx, float out_ms[3]) { return ctx ? ctx->md_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"

// ---- K18: signed crossing numbers ------------------------------------------------------------------------------------------

namespace {

// One axis of o2v_hip_crossings_dense, enqueued on the context's stream: the delta grid and totals cleared, the (triangle, line)
// items enumerated and marked, the lines summed into dst.
template <int A>
int crossings_axis(o2v_hip_ctx *ctx, const Switches &sw, const Affine &xf, const uint32_t origin[3], const uint32_t dims[3], uint32_t ss,
                   int32_t *dst, const uint64_t dst_strides[3], bool add)
{
    hipStream_t s = ctx->stream;
    constexpr int U = (A + 1) % 3, V = (A + 2) % 3;
    CrBox b{};
    b.u0 = origin[U], b.v0 = origin[V], b.w0 = origin[A];
    b.nu = dims[U], b.nv = dims[V], b.nw = dims[A];
    b.ss = ss;
    b.v_first = V == 0;   // (x first where a line has an x: the y rays' v)
    b.n_lines = (uint64_t) b.nu * b.nv;
    const uint64_t T = ctx->n_tris, n_blocks = (T + kBlock - 1) / kBlock;
    O2V_CHECK(hipMemsetAsync(ctx->d_cr_delta.ptr, 0, b.n_lines * b.nw * sizeof(int32_t), s));
    O2V_CHECK(hipMemsetAsync(ctx->d_cr_totals.ptr, 0, b.n_lines * sizeof(int32_t), s));
    if (T) {
        O2V_LAUNCH("k_cross_count", s, k_cross_count<A>, dim3((uint32_t) n_blocks), dim3(kBlock), 0, s, ctx->d_verts.ptr, T, xf, b, ctx->d_cr_ends.ptr,
                   ctx->d_cr_blocks.ptr);
        O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, ctx->d_cr_blocks.ptr, n_blocks, ctx->d_cr_ctr.ptr);
        O2V_LAUNCH("k_fill_offsets", s, k_fill_offsets, dim3((uint32_t) n_blocks), dim3(kBlock), 0, s, ctx->d_cr_ends.ptr, T, ctx->d_cr_blocks.ptr);
        O2V_LAUNCH("k_cross_mark", s, k_cross_mark<A>, dim3((uint32_t) ctx->num_cus * 8u), dim3(kBlock), 0, s, ctx->d_verts.ptr, T, xf, b,
                   ctx->d_cr_ends.ptr, ctx->d_cr_ctr.ptr, ctx->d_cr_delta.ptr, ctx->d_cr_totals.ptr);
    }
    const dim3 line_blocks((uint32_t) ((b.n_lines + kBlock - 1) / kBlock));
    const uint64_t s_first = dst_strides[b.v_first ? V : U], s_slow = dst_strides[b.v_first ? U : V], s_w = dst_strides[A];
    // (the ray along dst's unit stride and the lines not: the lanes of k_cross_prefix would each write a row of their own)
    const bool tile = s_w == 1u && s_first != 1u && !sw.cross_no_tile;
    with_flag(add, [&](auto adds) {
        if (tile)
            O2V_LAUNCH("k_cross_prefix_tile", s, k_cross_prefix_tile<decltype(adds)::value>, line_blocks, dim3(kBlock), 0, s, ctx->d_cr_delta.ptr,
                       ctx->d_cr_totals.ptr, b, dst, s_first, s_slow);
        else
            O2V_LAUNCH("k_cross_prefix", s, k_cross_prefix<decltype(adds)::value>, line_blocks, dim3(kBlock), 0, s, ctx->d_cr_delta.ptr,
                       ctx->d_cr_totals.ptr, b, dst, s_first, s_slow, s_w);
    });
    O2V_CHECK(hipGetLastError());
    return O2V_HIP_OK;
}

// An axis failed part-way: the runtime's error state is cleared, as o2v_hip_mesh_distance_dense does on its parity path (dst may
// hold the earlier axes' sums by then).
int axis_failed(o2v_hip_ctx *, int rc)
{
    (void) hipGetLastError();
    return rc;
}

}  // namespace

extern "C" {

int o2v_hip_crossings_dense(o2v_hip_ctx *ctx, const o2v_hip_params *params, uint32_t axes, const uint32_t origin[3], const uint32_t dims[3],
                            int32_t *dst, const uint64_t dst_strides[3])
{
    static const char fn[] = "o2v_hip_crossings_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!params || !origin || !dims || !dst || !dst_strides) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if (axes < 1u || axes > 7u) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "axes must be 1 ... 7 (bit 0 x, 1 y, 2 z), not " + std::to_string(axes));
    uint32_t ss = 0;
    int rc;
    if ((rc = mesh_box_args(ctx, fn, params, origin, dims, &ss))) return rc;
    const uint64_t T = ctx->n_tris;
    const uint32_t n_axes = (uint32_t) __builtin_popcount(axes);
    // (a voxel's value is bounded by two rays per axis and one crossing per triangle and ray)
    if (T > 0x7fffffffull / (2u * n_axes))
        return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "2 x " + std::to_string(n_axes) + " rays x " + std::to_string(T) + " triangles is above 2^31 - 1");
    O2V_CHECK(hipSetDevice(ctx->device));
    // (one output and nothing it could overlap: no check_outputs)
    if ((rc = check_grid(ctx, fn, "dst", dst, dims, dst_strides, 4u, true))) return rc;
    const Affine xf = mesh_box_transform(ctx, params, ss);
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2];
    uint64_t lines = 0;   // of the axis with the most
    for (int a = 0; a < 3; ++a)
        if (axes >> a & 1u) lines = std::max(lines, voxels / dims[a]);
    if ((rc = grow_scratch(ctx, ctx->d_cr_delta, voxels, fn, "delta grid")) || (rc = grow_scratch(ctx, ctx->d_cr_totals, lines, fn, "line totals")) ||
        (rc = grow_scratch(ctx, ctx->d_cr_ends, T, fn, "item ends")) || (rc = grow_scratch(ctx, ctx->d_cr_blocks, (T + kBlock - 1) / kBlock, fn, "block sums")) ||
        (rc = grow_scratch(ctx, ctx->d_cr_ctr, 1u, fn, "counter")))
        return rc;
    hipStream_t s = ctx->stream;
    const Switches sw = read_switches();
    bool add = false;
    O2V_CHECK(ctx->cr_times.mark(0, s));
    if (axes & 1u) {
        if ((rc = crossings_axis<0>(ctx, sw, xf, origin, dims, ss, dst, dst_strides, add))) return axis_failed(ctx, rc);
        add = true;
    }
    O2V_CHECK(ctx->cr_times.mark(1, s));
    if (axes & 2u) {
        if ((rc = crossings_axis<1>(ctx, sw, xf, origin, dims, ss, dst, dst_strides, add))) return axis_failed(ctx, rc);
        add = true;
    }
    O2V_CHECK(ctx->cr_times.mark(2, s));
    if (axes & 4u)
        if ((rc = crossings_axis<2>(ctx, sw, xf, origin, dims, ss, dst, dst_strides, add))) return axis_failed(ctx, rc);
    if ((rc = finish_stages(ctx, ctx->cr_times))) return rc;
    for (int a = 0; a < 3; ++a)
        if (!(axes >> a & 1u)) ctx->cr_times.ms[a] = 0.f;
    return O2V_HIP_OK;
}

int o2v_hip_crossings_times(const o2v_hip_ctx *ctx, float out_ms[3]) { return ctx ? ctx->cr_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"
