// Host side of K17 (o2v_dev_k17_downsample.hpp).

// ---- K17: a dense grid merged into a coarser one ------------------------------------------------------------------------------

namespace {

static_assert(kDsValueMin == O2V_HIP_DOWN_VALUE_MIN && kDsValueMax == O2V_HIP_DOWN_VALUE_MAX, "one set of value modes for the callers and the kernel");

}  // namespace

extern "C" {

int o2v_hip_downsample_box(const uint32_t origin[3], const uint32_t dims[3], uint32_t factor, uint32_t out_origin[3], uint32_t out_dims[3])
{
    if (!origin || !dims || !out_origin || !out_dims || factor < kDsMinFactor || factor > kDsMaxFactor || !dims[0] || !dims[1] || !dims[2])
        return O2V_HIP_ERR_BAD_ARGUMENT;
    for (int a = 0; a < 3; ++a)
        if ((uint64_t) origin[a] + dims[a] > (1ull << 32)) return O2V_HIP_ERR_LIMIT;
    for (int a = 0; a < 3; ++a) {
        out_origin[a] = ds_corigin(origin[a], factor);
        out_dims[a] = ds_cdim(origin[a], dims[a], factor);
    }
    return O2V_HIP_OK;
}

int o2v_hip_downsample(o2v_hip_ctx *ctx, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                       const uint32_t origin[3], uint32_t factor, uint32_t min_count, uint32_t value_mode, const uint32_t *colors,
                       const uint64_t color_strides[3], int16_t *count, const uint64_t count_strides[3], uint8_t *solid,
                       const uint64_t solid_strides[3], uint8_t *values, const uint64_t value_strides[3], uint32_t *argb,
                       const uint64_t argb_strides[3])
{
    static const char fn[] = "o2v_hip_downsample";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    SetGrid sg;
    int rc;
    if ((rc = set_grid_args(ctx, fn, grid, format, strides, dims, level, &sg))) return rc;
    if (!origin || (count && !count_strides) || (solid && !solid_strides) || (values && !value_strides) || (argb && !argb_strides) ||
        (colors && !color_strides))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if (!count && !solid && !values && !argb) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "no output: count, solid, values and argb are all null");
    if (factor < kDsMinFactor || factor > kDsMaxFactor)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "factor must be 2 ... 8, not " + std::to_string(factor));
    if (min_count < 1u || min_count > factor * factor * factor)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn,
                      "min_count must be 1 ... factor^3 = " + std::to_string(factor * factor * factor) + ", not " + std::to_string(min_count));
    if (values && format != O2V_HIP_GRID_U8) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "values needs a U8 grid");
    if (values && value_mode != O2V_HIP_DOWN_VALUE_MIN && value_mode != O2V_HIP_DOWN_VALUE_MAX)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown value_mode " + std::to_string(value_mode));
    if (argb && !colors) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "argb needs colors");
    if ((rc = axis_limit(ctx, fn, dims, origin, 1ull << 32, "origin + dims is above 2^32 along an axis"))) return rc;
    // (the limits stand before the look at the memory: a box that is too large is refused as that, whatever it reaches)
    if ((rc = set_grid_memory(ctx, fn, &sg))) return rc;
    DsGrid g{};
    for (int a = 0; a < 3; ++a) g.n[a] = dims[a], g.o[a] = origin[a], g.cn[a] = ds_cdim(origin[a], dims[a], factor);
    g.f = factor, g.min_count = min_count, g.value_mode = value_mode;
    g.spans = (g.cn[0] + kDsSpan - 1u) / kDsSpan;
    g.ry = std::max(1u, kDsRows / (factor * factor));
    g.ygroups = (g.cn[1] + g.ry - 1u) / g.ry;
    g.items = (uint64_t) g.spans * g.ygroups * g.cn[2];
    // colours are read only where argb is written
    const OutGrid outs[] = {{"count", count, count_strides, 2u}, {"solid", solid, solid_strides, 1u}, {"values", values, value_strides, 1u},
                            {"argb", argb, argb_strides, 4u}};
    Span spans[6] = {{}, {}, {}, {}, {"grid", grid, sg.bytes}, {"colors", nullptr, 0}};
    if (argb) {
        spans[5].p = colors;
        if ((rc = check_grid(ctx, fn, "colors", colors, dims, color_strides, 4u, false, &spans[5].bytes))) return rc;
    }
    if ((rc = check_outputs(ctx, fn, outs, g.cn, spans)) || (rc = refuse_overlap(ctx, fn, spans, 4))) return rc;
    DsOut o{};
    if (count) o.count = count, o.k0 = count_strides[0], o.k1 = count_strides[1], o.k2 = count_strides[2];
    if (solid) o.solid = solid, o.s0 = solid_strides[0], o.s1 = solid_strides[1], o.s2 = solid_strides[2];
    if (values) o.values = values, o.v0 = value_strides[0], o.v1 = value_strides[1], o.v2 = value_strides[2];
    if (argb) {
        o.argb = argb, o.a0 = argb_strides[0], o.a1 = argb_strides[1], o.a2 = argb_strides[2];
        o.colors = colors, o.c0 = color_strides[0], o.c1 = color_strides[1], o.c2 = color_strides[2];
    }
    hipStream_t s = ctx->stream;
    // a workgroup per item, and no more than keep every CU's LDS full (16.6 KB each)
    const dim3 blocks((uint32_t) std::min<uint64_t>(g.items, (uint64_t) ctx->num_cus * 8u));
    O2V_CHECK(ctx->ds_times.mark(0, s));
    with_set_format(sg, [&](auto fmt, auto vec) {
        O2V_LAUNCH("k_downsample", s, (k_downsample<decltype(fmt)::value, decltype(vec)::value>), blocks, dim3(kBlock), 0, s, sg.source(), g, o);
    });
    O2V_CHECK(hipGetLastError());
    return finish_stages(ctx, ctx->ds_times);
}

int o2v_hip_downsample_times(const o2v_hip_ctx *ctx, float out_ms[1]) { return ctx ? ctx->ds_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

}  // extern "C"
