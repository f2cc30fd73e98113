// Host side of K11 (o2v_dev_k11_raycast.hpp).

// ---- K11: rays through a dense grid ----------------------------------------------------------------------------------------

namespace {

constexpr uint32_t kRayMaxExtent = 65536;        // origin + dims per axis (O2V_HIP_ERR_LIMIT above)
constexpr uint64_t kRayMaxRays = 0x7fffffffull;

// the words of the three levels over dims: 4^3 bricks, 16^3 blocks, 64^3 blocks
void ray_levels(const uint32_t dims[3], uint64_t words[3], uint32_t per_axis[3][3])
{
    for (int l = 0; l < 3; ++l) {
        words[l] = 1;
        for (int a = 0; a < 3; ++a) {
            const uint32_t step = 4u << (2 * l);
            per_axis[l][a] = (uint32_t) (((uint64_t) dims[a] + step - 1u) / step);
            words[l] *= per_axis[l][a];
        }
    }
}

RayGrid ray_grid(const o2v_hip_ctx *ctx)
{
    RayGrid g{};
    uint64_t words[3];
    uint32_t per_axis[3][3];
    ray_levels(ctx->ray.dims, words, per_axis);
    for (int a = 0; a < 3; ++a) {
        g.org[a] = (int32_t) ctx->ray.origin[a];
        g.dim[a] = (int32_t) ctx->ray.dims[a];
        g.b0[a] = per_axis[0][a];
        g.b1[a] = per_axis[1][a];
        g.b2[a] = per_axis[2][a];
    }
    g.m0 = ctx->d_ray_masks.ptr;
    g.m1 = g.m0 + words[0];
    g.m2 = g.m1 + words[1];
    return g;
}

}  // namespace

extern "C" {

uint64_t o2v_hip_raycast_scratch_bytes(const uint32_t dims[3])
{
    if (!dims || !dims[0] || !dims[1] || !dims[2]) return 0;
    uint64_t words[3];
    uint32_t per_axis[3][3];
    ray_levels(dims, words, per_axis);
    return 8u * (words[0] + words[1] + words[2]);
}

int o2v_hip_raycast_build(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                          const uint32_t origin[3])
{
    static const char fn[] = "o2v_hip_raycast_build";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    ctx->ray.valid = false;
    ++ctx->ray.generation;
    SetGrid sg;
    int rc;
    if ((rc = set_grid(ctx, fn, grid, format, strides, dims, level, &sg))) return rc;
    if (!origin) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((rc = extent_limit(ctx, fn, origin, dims, kRayMaxExtent, "origin + dims is above 65 536 voxels along an axis"))) return rc;
    if ((rc = grow_scratch(ctx, ctx->d_ray_masks, o2v_hip_raycast_scratch_bytes(dims) / 8u, fn, "snapshot"))) return rc;
    std::copy(dims, dims + 3, ctx->ray.dims);
    std::copy(origin, origin + 3, ctx->ray.origin);
    const RayGrid g = ray_grid(ctx);
    uint64_t words[3];
    uint32_t per_axis[3][3];
    ray_levels(dims, words, per_axis);
    unsigned long long *const m0 = ctx->d_ray_masks.ptr, *const m1 = m0 + words[0], *const m2 = m1 + words[1];
    const RaySource src = sg.source();
    const uint64_t tiles = (uint64_t) ((dims[0] + 63u) / 64u) * per_axis[0][1] * per_axis[0][2];
    const dim3 blocks(stream_grid(ctx, tiles * 64u, 8u));
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->ray_build_times.mark(0, s));
    O2V_CHECK(hipMemsetAsync(m1, 0, words[1] * 8u, s));
    with_set_format(sg, [&](auto fmt, auto vec) {
        O2V_LAUNCH("k_ray_build", s, (k_ray_build<decltype(fmt)::value, decltype(vec)::value>), blocks, dim3(kBlock), 0, s, src, g, m0, m1);
    });
    O2V_LAUNCH("k_ray_build_top", s, k_ray_build_top, dim3(stream_grid(ctx, words[2], 8u)), dim3(kBlock), 0, s, g, m1, m2);
    O2V_CHECK(hipGetLastError());
    if ((rc = finish_stages(ctx, ctx->ray_build_times))) return rc;
    ctx->ray.valid = true;
    return O2V_HIP_OK;
}

int o2v_hip_raycast(o2v_hip_ctx *ctx, const float *origins, const float *directions, uint64_t n, float t_max, int32_t *hit, float *t)
{
    static const char fn[] = "o2v_hip_raycast";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    const Switches sw = read_switches();
    if (!(t_max >= 0.f)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "t_max must be >= 0 or +inf");
    if (n > kRayMaxRays) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "more than 2^31 - 1 rays");
    if (!ctx->ray.valid) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "no o2v_hip_raycast_build");
    if (n == 0) return O2V_HIP_OK;
    if (!origins || !directions || !hit || !t) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    O2V_CHECK(hipSetDevice(ctx->device));
    int rc;
    if ((rc = check_device_range(ctx, fn, origins, n * 12u, "origins")) || (rc = check_device_range(ctx, fn, directions, n * 12u, "directions")) ||
        (rc = check_device_range(ctx, fn, hit, n * 16u, "hit")) || (rc = check_device_range(ctx, fn, t, n * 4u, "t")))
        return rc;
    const Span spans[] = {{"hit", hit, n * 16u}, {"t", t, n * 4u}, {"origins", origins, n * 12u}, {"directions", directions, n * 12u}};
    if ((rc = refuse_overlap(ctx, fn, spans, 2))) return rc;
    const RayGrid g = ray_grid(ctx);
    const dim3 blocks((uint32_t) ((n + kBlock - 1) / kBlock));
    hipStream_t s = ctx->stream;
    O2V_CHECK(ctx->ray_cast_times.mark(0, s));
    with_flag(!sw.ray_no_skip, [&](auto skip) {
        O2V_LAUNCH("k_ray_cast", s, k_ray_cast<decltype(skip)::value>, blocks, dim3(kBlock), 0, s, origins, directions, n, t_max, g, hit, t);
    });
    O2V_CHECK(hipGetLastError());
    return finish_stages(ctx, ctx->ray_cast_times);
}

int o2v_hip_raycast_times(const o2v_hip_ctx *ctx, float out_ms[2])
{
    if (!ctx || !out_ms) return O2V_HIP_ERR_BAD_ARGUMENT;
    out_ms[0] = ctx->ray_build_times.ms[0];
    out_ms[1] = ctx->ray_cast_times.ms[0];
    return O2V_HIP_OK;
}

uint64_t o2v_hip_raycast_generation(const o2v_hip_ctx *ctx) { return ctx ? ctx->ray.generation : 0; }

}  // extern "C"
