// Host side of K10 (o2v_dev_k10_surface.hpp).

// ---- K10: the level set of a dense grid as an indexed mesh --------------------------------------------------------------

namespace {

constexpr uint32_t kSurfMaxExtent = 65536;        // origin + dims per axis (O2V_HIP_ERR_LIMIT above): positions exact to 2^-7 voxel
constexpr uint64_t kSurfMaxVertices = 0x7fffffffull;
constexpr uint64_t kSurfMaxGrid = 1ull << 20;     // workgroups of the per-block kernels; more blocks are taken in turns

// what o2v_hip_surface_count and _write both check of the grid; *g: its words
int surf_grid(o2v_hip_ctx *ctx, const char *fn, const float *field, const uint64_t strides[3], const uint32_t dims[3], float level,
              SurfGrid *g, uint64_t *field_bytes)
{
    if (int rc = grid_given(ctx, fn, field, strides, dims)) return rc;
    if (!std::isfinite(level)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "level must be finite");
    for (int a = 0; a < 3; ++a)
        if (dims[a] > kSurfMaxExtent) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "a grid of more than 65 536 samples along an axis");
    O2V_CHECK(hipSetDevice(ctx->device));
    if (int rc = check_grid(ctx, fn, "field", field, dims, strides, 4u, false, field_bytes)) return rc;
    g->s0 = strides[0], g->s1 = strides[1], g->s2 = strides[2];
    g->nx = dims[0], g->ny = dims[1], g->nz = dims[2];
    g->W = (dims[0] + 63u) / 64u;
    g->items = (uint64_t) dims[1] * dims[2] * g->W;
    g->n_blocks = (g->items + kBlock - 1) / kBlock;
    g->level = level;
    return O2V_HIP_OK;
}

uint32_t surf_blocks(const SurfGrid &g) { return (uint32_t) std::min<uint64_t>(g.n_blocks, kSurfMaxGrid); }

}  // namespace

extern "C" {

int o2v_hip_surface_count(o2v_hip_ctx *ctx, const float *field, const uint64_t strides[3], const uint32_t dims[3], float level,
                          uint64_t *out_vertices, uint64_t *out_triangles)
{
    static const char fn[] = "o2v_hip_surface_count";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!out_vertices || !out_triangles) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    ctx->sf.valid = false;
    SurfGrid g{};
    uint64_t fbytes = 0;
    int rc;
    if ((rc = surf_grid(ctx, fn, field, strides, dims, level, &g, &fbytes))) return rc;
    if ((rc = grow_scratch(ctx, ctx->d_sf_signs, g.items, fn, "sign words")) || (rc = grow_scratch(ctx, ctx->d_sf_active, g.items, fn, "cell words")) ||
        (rc = grow_scratch(ctx, ctx->d_sf_local, g.items, fn, "prefixes")) || (rc = grow_scratch(ctx, ctx->d_sf_voff, g.n_blocks + 1u, fn, "vertex offsets")) ||
        (rc = grow_scratch(ctx, ctx->d_sf_qoff, g.n_blocks + 1u, fn, "quad offsets")) || (rc = grow_scratch(ctx, ctx->h_sf_ctr, 2u, fn, "counters")))
        return rc;
    hipStream_t s = ctx->stream;
    unsigned long long *const voff = ctx->d_sf_voff.ptr, *const qoff = ctx->d_sf_qoff.ptr;
    O2V_CHECK(ctx->sf_times.mark(0, s));
    O2V_LAUNCH("k_surf_signs", s, k_surf_signs, dim3(stream_grid(ctx, (g.items + kSurfInFlight - 1) / kSurfInFlight * 64u, 8u)), dim3(kBlock), 0, s,
               field, g, ctx->d_sf_signs.ptr);
    O2V_CHECK(ctx->sf_times.mark(1, s));
    O2V_LAUNCH("k_surf_count", s, k_surf_count, dim3(surf_blocks(g)), dim3(kBlock), 0, s, ctx->d_sf_signs.ptr, g, ctx->d_sf_active.ptr,
               ctx->d_sf_local.ptr, voff, qoff);
    // (the totals go behind the offsets: entry n_blocks)
    O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, voff, g.n_blocks, voff + g.n_blocks);
    O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, qoff, g.n_blocks, qoff + g.n_blocks);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(ctx->sf_times.mark(2, s));
    O2V_CHECK(hipMemcpyAsync(ctx->h_sf_ctr.ptr, voff + g.n_blocks, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipMemcpyAsync(ctx->h_sf_ctr.ptr + 1, qoff + g.n_blocks, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(ctx->sf_times.elapsed(0, 1, ctx->sf_times.ms[0]));
    O2V_CHECK(ctx->sf_times.elapsed(1, 2, ctx->sf_times.ms[1]));
    ctx->sf_times.ms[2] = ctx->sf_times.ms[3] = 0.f;
    const uint64_t V = ctx->h_sf_ctr.ptr[0], Q = ctx->h_sf_ctr.ptr[1];
    if (V > kSurfMaxVertices)
        return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, std::to_string(V) + " vertices do not fit an int32 index (at most 2^31 - 1)");
    ctx->sf.valid = true;
    ctx->sf.key = GridKey(field, 0u, strides, dims, level);
    ctx->sf.vertices = V;
    ctx->sf.quads = Q;
    *out_vertices = V;
    *out_triangles = 2u * Q;
    return O2V_HIP_OK;
}

int o2v_hip_surface_write(o2v_hip_ctx *ctx, const float *field, const uint64_t strides[3], const uint32_t dims[3], float level,
                          const uint32_t origin[3], float *positions, uint64_t vertex_capacity, int32_t *faces, uint64_t triangle_capacity)
{
    static const char fn[] = "o2v_hip_surface_write";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!origin) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    SurfGrid g{};
    uint64_t fbytes = 0;
    int rc;
    if ((rc = surf_grid(ctx, fn, field, strides, dims, level, &g, &fbytes))) return rc;
    if ((rc = extent_limit(ctx, fn, origin, dims, kSurfMaxExtent, "origin + dims is above 65 536 samples along an axis"))) return rc;
    const o2v_hip_ctx::SurfaceCount &c = ctx->sf;
    if (!c.valid || !(c.key == GridKey(field, 0u, strides, dims, level)))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "no matching o2v_hip_surface_count (the same field, strides, dims and level)");
    const uint64_t V = c.vertices, T = 2u * c.quads;
    if (vertex_capacity < V || triangle_capacity < T)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn,
                      "capacities " + std::to_string(vertex_capacity) + ", " + std::to_string(triangle_capacity) + " are below the counted " +
                          std::to_string(V) + " vertices, " + std::to_string(T) + " triangles");
    if ((V && !positions) || (T && !faces)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((V && (rc = check_device_range(ctx, fn, positions, V * 12u, "positions"))) || (T && (rc = check_device_range(ctx, fn, faces, T * 12u, "faces"))))
        return rc;
    const Span spans[] = {{"positions", positions, V * 12u}, {"faces", faces, T * 12u}, {"field", field, fbytes}};
    if ((rc = refuse_overlap(ctx, fn, spans, 2))) return rc;
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->sf_times.mark(2, s));
    if (V)
        with_flag(g.s0 == 1u, [&](auto unit_x) {
            O2V_LAUNCH("k_surf_vertices", s, k_surf_vertices<decltype(unit_x)::value>, dim3(surf_blocks(g)), dim3(kBlock), 0, s, field, g, ctx->d_sf_signs.ptr,
                       ctx->d_sf_active.ptr, ctx->d_sf_local.ptr, ctx->d_sf_voff.ptr, origin[0], origin[1], origin[2], positions);
        });
    O2V_CHECK(ctx->sf_times.mark(3, s));
    if (T)
        O2V_LAUNCH("k_surf_faces", s, k_surf_faces, dim3(surf_blocks(g)), dim3(kBlock), 0, s, g, ctx->d_sf_signs.ptr, ctx->d_sf_active.ptr,
                   ctx->d_sf_local.ptr, ctx->d_sf_voff.ptr, ctx->d_sf_qoff.ptr, faces);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(ctx->sf_times.mark(4, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(ctx->sf_times.elapsed(2, 3, ctx->sf_times.ms[2]));
    O2V_CHECK(ctx->sf_times.elapsed(3, 4, ctx->sf_times.ms[3]));
    return O2V_HIP_OK;
}

int o2v_hip_surface_times(const o2v_hip_ctx *ctx, float out_ms[4]) { return ctx ? ctx->sf_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"
