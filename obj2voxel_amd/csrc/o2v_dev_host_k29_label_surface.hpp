// Host side of K29 (o2v_dev_k29_label_surface.hpp): the interfaces of a label grid as one mesh.  It takes K19's formats and K10's
// limits and block grid, so it comes after o2v_dev_host_k10_surface.hpp and o2v_dev_host_k19_label_stats.hpp.

namespace {

constexpr uint32_t kLsfMaxIterations = 1024;

// what o2v_hip_label_surface_count and _write both check of the grid; *L: the labels, *g: the words of the extended lattice
int lsf_grid(o2v_hip_ctx *ctx, const char *fn, const void *labels, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], uint32_t flags,
             LsfLabels *L, SurfGrid *g, uint64_t *label_bytes)
{
    if (int rc = grid_given(ctx, fn, labels, strides, dims)) return rc;
    if (format != O2V_HIP_LABELS_I32 && format != O2V_HIP_LABELS_U8)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown format " + std::to_string(format));
    if (flags & ~(uint32_t) O2V_HIP_LABEL_SURFACE_CLOSED) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits " + std::to_string(flags));
    if (format == O2V_HIP_LABELS_I32 && (uintptr_t) labels % sizeof(int32_t))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "an I32 grid must be 4-byte aligned");
    const uint32_t E = flags & O2V_HIP_LABEL_SURFACE_CLOSED ? 1u : 0u;
    for (int a = 0; a < 3; ++a)
        if (dims[a] > kSurfMaxExtent - 2u * E)
            return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "a grid of more than " + std::to_string(kSurfMaxExtent - 2u * E) + " samples along an axis");
    O2V_CHECK(hipSetDevice(ctx->device));
    if (int rc = check_grid(ctx, fn, "labels", labels, dims, strides, format == O2V_HIP_LABELS_I32 ? 4u : 1u, false, label_bytes)) return rc;
    *L = LsfLabels{labels, strides[0], strides[1], strides[2], dims[0], dims[1], dims[2], E};
    g->nx = dims[0] + 2u * E, g->ny = dims[1] + 2u * E, g->nz = dims[2] + 2u * E;
    g->W = (g->nx + 63u) / 64u;
    g->items = (uint64_t) g->ny * g->nz * g->W;
    g->n_blocks = (g->items + kBlock - 1) / kBlock;
    return O2V_HIP_OK;
}

GridKey lsf_key(const void *labels, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], uint32_t flags)
{
    return GridKey(labels, format | flags << 8, strides, dims, 0.f);
}

}  // namespace

extern "C" {

int o2v_hip_label_surface_count(o2v_hip_ctx *ctx, const void *labels, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], uint32_t flags,
                                uint64_t *out_vertices, uint64_t *out_quads)
{
    static const char fn[] = "o2v_hip_label_surface_count";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    const Switches sw = read_switches();
    if (!out_vertices || !out_quads) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    ctx->lsf.valid = false;
    LsfLabels L{};
    SurfGrid g{};
    uint64_t lbytes = 0;
    int rc;
    if ((rc = lsf_grid(ctx, fn, labels, format, strides, dims, flags, &L, &g, &lbytes))) return rc;
    if ((rc = grow_scratch(ctx, ctx->d_lsf_diff, 3u * g.items, fn, "difference words")) ||
        (rc = grow_scratch(ctx, ctx->d_lsf_active, g.items, fn, "cell words")) || (rc = grow_scratch(ctx, ctx->d_lsf_local, g.items, fn, "prefixes")) ||
        (rc = grow_scratch(ctx, ctx->d_lsf_voff, g.n_blocks + 1u, fn, "vertex offsets")) ||
        (rc = grow_scratch(ctx, ctx->d_lsf_qoff, g.n_blocks + 1u, fn, "quad offsets")) || (rc = grow_scratch(ctx, ctx->h_lsf_ctr, 2u, fn, "counters")))
        return rc;
    hipStream_t s = ctx->stream;
    unsigned long long *const voff = ctx->d_lsf_voff.ptr, *const qoff = ctx->d_lsf_qoff.ptr;
    O2V_CHECK(ctx->lsf_times.mark(0, s));
    const uint32_t tiles_y = (g.ny + kLsfTileY - 1u) / kLsfTileY;
    const uint64_t tiles = (uint64_t) g.W * tiles_y * ((g.nz + kLsfTileZ - 1u) / kLsfTileZ);
    with_flag(format == O2V_HIP_LABELS_I32, [&](auto i32) {
        with_flag(strides[0] == 1u, [&](auto unit_x) {
            constexpr bool I32 = decltype(i32)::value, UnitX = decltype(unit_x)::value;
            if (sw.lsf_no_tile)
                O2V_LAUNCH("k_lsf_classify", s, (k_lsf_classify<I32, UnitX>), dim3(stream_grid(ctx, (g.items + kLsfInFlight - 1) / kLsfInFlight * 64u, 8u)),
                           dim3(kBlock), 0, s, L, g, ctx->d_lsf_diff.ptr);
            else
                O2V_LAUNCH("k_lsf_classify_tile", s, (k_lsf_classify_tile<I32, UnitX>), dim3((uint32_t) std::min<uint64_t>(tiles, kSurfMaxGrid)), dim3(kBlock),
                           0, s, L, g, tiles_y, tiles, ctx->d_lsf_diff.ptr);
        });
    });
    O2V_CHECK(ctx->lsf_times.mark(1, s));
    O2V_LAUNCH("k_lsf_count", s, k_lsf_count, dim3(surf_blocks(g)), dim3(kBlock), 0, s, ctx->d_lsf_diff.ptr, g, ctx->d_lsf_active.ptr, ctx->d_lsf_local.ptr,
               voff, qoff);
    // (the totals go behind the offsets: entry n_blocks)
    O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, voff, g.n_blocks, voff + g.n_blocks);
    O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, qoff, g.n_blocks, qoff + g.n_blocks);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(ctx->lsf_times.mark(2, s));
    O2V_CHECK(hipMemcpyAsync(ctx->h_lsf_ctr.ptr, voff + g.n_blocks, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipMemcpyAsync(ctx->h_lsf_ctr.ptr + 1, qoff + g.n_blocks, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(ctx->lsf_times.elapsed(0, 1, ctx->lsf_times.ms[0]));
    O2V_CHECK(ctx->lsf_times.elapsed(1, 2, ctx->lsf_times.ms[1]));
    ctx->lsf_times.ms[2] = ctx->lsf_times.ms[3] = 0.f;
    const uint64_t V = ctx->h_lsf_ctr.ptr[0], Q = ctx->h_lsf_ctr.ptr[1];
    if (V > kSurfMaxVertices) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, std::to_string(V) + " vertices do not fit an int32 index (at most 2^31 - 1)");
    if (2u * Q > kSurfMaxVertices) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, std::to_string(Q) + " quads: more than 2^31 - 1 triangles");
    ctx->lsf.valid = true;
    ctx->lsf.key = lsf_key(labels, format, strides, dims, flags);
    ctx->lsf.vertices = V;
    ctx->lsf.quads = Q;
    *out_vertices = V;
    *out_quads = Q;
    return O2V_HIP_OK;
}

int o2v_hip_label_surface_write(o2v_hip_ctx *ctx, const void *labels, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], uint32_t flags,
                                int32_t *cells, int32_t *links, uint64_t vertex_capacity, int32_t *faces, int32_t *pairs, uint64_t quad_capacity)
{
    static const char fn[] = "o2v_hip_label_surface_write";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    LsfLabels L{};
    SurfGrid g{};
    uint64_t lbytes = 0;
    int rc;
    if ((rc = lsf_grid(ctx, fn, labels, format, strides, dims, flags, &L, &g, &lbytes))) return rc;
    const o2v_hip_ctx::SurfaceCount &c = ctx->lsf;
    if (!c.valid || !(c.key == lsf_key(labels, format, strides, dims, flags)))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "no matching o2v_hip_label_surface_count (the same labels, format, strides, dims and flags)");
    const uint64_t V = c.vertices, Q = c.quads;
    if (vertex_capacity < V || quad_capacity < Q)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn,
                      "capacities " + std::to_string(vertex_capacity) + ", " + std::to_string(quad_capacity) + " are below the counted " +
                          std::to_string(V) + " vertices, " + std::to_string(Q) + " quads");
    if ((V && (!cells || !links)) || (Q && (!faces || !pairs))) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if (((uintptr_t) cells | (uintptr_t) links | (uintptr_t) faces | (uintptr_t) pairs) % sizeof(int32_t))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "cells, links, faces and pairs must be 4-byte aligned");
    if ((V && ((rc = check_device_range(ctx, fn, cells, V * 12u, "cells")) || (rc = check_device_range(ctx, fn, links, V * 24u, "links")))) ||
        (Q && ((rc = check_device_range(ctx, fn, faces, Q * 24u, "faces")) || (rc = check_device_range(ctx, fn, pairs, Q * 8u, "pairs")))))
        return rc;
    const Span spans[] = {{"cells", cells, V * 12u}, {"links", links, V * 24u}, {"faces", faces, Q * 24u}, {"pairs", pairs, Q * 8u}, {"labels", labels, lbytes}};
    if ((rc = refuse_overlap(ctx, fn, spans, 4))) return rc;
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->lsf_times.mark(2, s));
    if (V)
        O2V_LAUNCH("k_lsf_vertices", s, k_lsf_vertices, dim3(surf_blocks(g)), dim3(kBlock), 0, s, g, L.E, ctx->d_lsf_diff.ptr, ctx->d_lsf_active.ptr,
                   ctx->d_lsf_local.ptr, ctx->d_lsf_voff.ptr, cells, links);
    O2V_CHECK(ctx->lsf_times.mark(3, s));
    if (Q)
        with_flag(format == O2V_HIP_LABELS_I32, [&](auto i32) {
            O2V_LAUNCH("k_lsf_faces", s, k_lsf_faces<decltype(i32)::value>, dim3(surf_blocks(g)), dim3(kBlock), 0, s, L, g, ctx->d_lsf_diff.ptr,
                       ctx->d_lsf_active.ptr, ctx->d_lsf_local.ptr, ctx->d_lsf_voff.ptr, ctx->d_lsf_qoff.ptr, faces, pairs);
        });
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(ctx->lsf_times.mark(4, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(ctx->lsf_times.elapsed(2, 3, ctx->lsf_times.ms[2]));
    O2V_CHECK(ctx->lsf_times.elapsed(3, 4, ctx->lsf_times.ms[3]));
    return O2V_HIP_OK;
}

int o2v_hip_label_surface_relax(o2v_hip_ctx *ctx, const int32_t *cells, const int32_t *links, uint64_t n_vertices, const uint32_t origin[3],
                                uint32_t iterations, float relaxation, float reach, float *positions)
{
    static const char fn[] = "o2v_hip_label_surface_relax";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!origin || (n_vertices && (!cells || !links || !positions))) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if (!(relaxation > 0.f && relaxation <= 1.f)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "relaxation must be above 0 and at most 1");
    if (!(reach >= 0.f && reach <= 0.5f)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "reach must be 0 ... 0.5");
    if (((uintptr_t) cells | (uintptr_t) links | (uintptr_t) positions) % 4u)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "cells, links and positions must be 4-byte aligned");
    if (iterations > kLsfMaxIterations) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 1024 iterations");
    if (n_vertices > kSurfMaxVertices) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 2^31 - 1 vertices");
    for (int a = 0; a < 3; ++a)
        if (origin[a] > kSurfMaxExtent) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "an origin above 65 536");
    ctx->lsf_times.ms[4] = 0.f;
    if (!n_vertices) return O2V_HIP_OK;
    O2V_CHECK(hipSetDevice(ctx->device));
    int rc;
    const uint64_t V = n_vertices;
    if ((rc = check_device_range(ctx, fn, cells, V * 12u, "cells")) || (rc = check_device_range(ctx, fn, links, V * 24u, "links")) ||
        (rc = check_device_range(ctx, fn, positions, V * 12u, "positions")))
        return rc;
    const Span spans[] = {{"positions", positions, V * 12u}, {"cells", cells, V * 12u}, {"links", links, V * 24u}};
    if ((rc = refuse_overlap(ctx, fn, spans, 1))) return rc;
    if (iterations && (rc = grow_scratch(ctx, ctx->d_lsf_pos, V * 3u, fn, "the second position buffer"))) return rc;
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->lsf_times.create());
    O2V_CHECK(ctx->lsf_times.mark(4, s));
    // p_0 goes where an even number of steps from it ends in the caller's array
    float *from = iterations % 2u ? ctx->d_lsf_pos.ptr : positions, *to = iterations % 2u ? positions : ctx->d_lsf_pos.ptr;
    const uint32_t n = (uint32_t) V;
    O2V_LAUNCH("k_lsf_centres", s, k_lsf_centres, dim3(stream_grid(ctx, V * 3u, 8u)), dim3(kBlock), 0, s, cells, n, origin[0], origin[1], origin[2], from);
    for (uint32_t t = 0; t < iterations; ++t, std::swap(from, to))
        O2V_LAUNCH("k_lsf_relax", s, k_lsf_relax, dim3(stream_grid(ctx, V, 8u)), dim3(kBlock), 0, s, cells, links, n, origin[0], origin[1], origin[2],
                   relaxation, reach, from, to);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(ctx->lsf_times.mark(5, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(ctx->lsf_times.elapsed(4, 5, ctx->lsf_times.ms[4]));
    return O2V_HIP_OK;
}

int o2v_hip_label_surface_times(const o2v_hip_ctx *ctx, float out_ms[5]) { return ctx ? ctx->lsf_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"
