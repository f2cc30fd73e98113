// Host side of K7 (o2v_dev_k7_dense.hpp).

// ---- K7: device-resident input, dense output -------------------------------------------------------------------------

extern "C" {

int o2v_hip_set_triangles_device(o2v_hip_ctx *ctx, const float *positions, uint64_t n_positions, const void *faces,
                                 uint32_t index_bytes, const float *uvs, const uint32_t *types, const float *colors,
                                 const int32_t *texids, uint64_t count)
{
    static const char fn[] = "o2v_hip_set_triangles_device";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (count && !positions) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "positions is null");
    if (faces && index_bytes != 4 && index_bytes != 8) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "index_bytes must be 4 or 8");
    if (count >= (1ull << 29)) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "triangle count must be below 2^29");
    if (faces && count && n_positions == 0) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "n_positions is 0 but there are faces");
    if (faces && n_positions > (~0ull >> 4)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "n_positions is too large");
    O2V_CHECK(hipSetDevice(ctx->device));
    int rc;
    if (count) {
        if ((rc = check_device_range(ctx, fn, positions, faces ? n_positions * 12u : count * 36u, "positions")) ||
            (faces && (rc = check_device_range(ctx, fn, faces, count * 3u * index_bytes, "faces"))) ||
            (uvs && (rc = check_device_range(ctx, fn, uvs, count * 24u, "uvs"))) ||
            (types && (rc = check_device_range(ctx, fn, types, count * 4u, "types"))) ||
            (colors && (rc = check_device_range(ctx, fn, colors, count * 12u, "colors"))) ||
            (texids && (rc = check_device_range(ctx, fn, texids, count * 4u, "texids"))) ||
            (rc = grow_scratch(ctx, ctx->d_dense, 1, fn, "counters")) || (rc = grow_scratch(ctx, ctx->h_dense, 1, fn, "counters")))
            return rc;
    }
    if ((rc = o2v::ctx_alloc_triangles(ctx, count, uvs != nullptr, types != nullptr, colors != nullptr, texids != nullptr))) return rc;
    if (count) {
        hipStream_t s = ctx->stream;
        DenseCtr *const ctr = ctx->d_dense.ptr;
        O2V_CHECK(hipMemsetAsync(ctr, 0, sizeof(DenseCtr), s));
        if (!faces) O2V_CHECK(hipMemcpyAsync(ctx->d_verts.ptr, positions, count * 36u, hipMemcpyDeviceToDevice, s));
        else {
            const uint32_t grid = stream_grid(ctx, (count + 3u) / 4u * 64u, 8u);  // (one wave per 64 triangles)
            if (index_bytes == 4)
                O2V_LAUNCH("k_gather_tris", s, k_gather_tris<int32_t>, dim3(grid), dim3(kBlock), 0, s, positions, n_positions,
                           static_cast<const int32_t *>(faces), count, ctx->d_verts.ptr, ctr);
            else
                O2V_LAUNCH("k_gather_tris", s, k_gather_tris<int64_t>, dim3(grid), dim3(kBlock), 0, s, positions, n_positions,
                           static_cast<const int64_t *>(faces), count, ctx->d_verts.ptr, ctr);
        }
        if (uvs) O2V_CHECK(hipMemcpyAsync(ctx->d_uvs.ptr, uvs, count * 24u, hipMemcpyDeviceToDevice, s));
        if (types) {
            O2V_CHECK(hipMemcpyAsync(ctx->d_types.ptr, types, count * 4u, hipMemcpyDeviceToDevice, s));
            O2V_LAUNCH("k_any_textured", s, k_any_textured, dim3(stream_grid(ctx, count, 4u)), dim3(kBlock), 0, s, types, count, ctr);
        }
        if (colors) O2V_CHECK(hipMemcpyAsync(ctx->d_colors.ptr, colors, count * 12u, hipMemcpyDeviceToDevice, s));
        if (texids) O2V_CHECK(hipMemcpyAsync(ctx->d_texids.ptr, texids, count * 4u, hipMemcpyDeviceToDevice, s));
        O2V_CHECK(hipGetLastError());
        O2V_CHECK(hipMemcpyAsync(ctx->h_dense.ptr, ctr, sizeof(DenseCtr), hipMemcpyDeviceToHost, s));
    }
    // (the flags come back in the round trip the upload's hints make anyway)
    if ((rc = o2v::ctx_finish_triangles(ctx, false, nullptr))) return rc;
    if (!count) return O2V_HIP_OK;
    if (ctx->h_dense.ptr->bad_index) {
        if ((rc = o2v::ctx_alloc_triangles(ctx, 0, false, false, false, false)) || (rc = o2v::ctx_finish_triangles(ctx, false, nullptr)))
            return rc;
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "face index out of range: an index is negative, not below n_positions (" +
                      std::to_string(n_positions) + ") or not below 2^32; the context holds no triangles");
    }
    ctx->any_textured = ctx->h_dense.ptr->textured != 0;
    return O2V_HIP_OK;
}

int o2v_hip_write_dense(o2v_hip_ctx *ctx, void *dst, uint32_t format, const uint32_t origin[3], const uint32_t dims[3],
                        const uint64_t strides[3], uint64_t *out_outside)
{
    static const char fn[] = "o2v_hip_write_dense";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!dst || !origin || !dims || !strides || format > O2V_HIP_DENSE_BITS)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument or unknown format");
    if (!dims[0] || !dims[1] || !dims[2]) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "zero dims");
    if (format == O2V_HIP_DENSE_BITS && strides[0] != 1) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "BITS needs strides[0] == 1");
    O2V_CHECK(hipSetDevice(ctx->device));
    // (BITS: x counted in 32-bit words; aliasing strides are the caller's business here)
    const uint32_t box[3] = {format == O2V_HIP_DENSE_BITS ? (dims[0] - 1u) / 32u + 1u : dims[0], dims[1], dims[2]};
    int rc;
    if ((rc = check_grid(ctx, fn, "dst", dst, box, strides, format == O2V_HIP_DENSE_U8 ? 1u : 4u, false)) ||
        (rc = grow_scratch(ctx, ctx->d_dense, 1, fn, "counters")) || (rc = grow_scratch(ctx, ctx->h_dense, 1, fn, "counters")))
        return rc;
    if (out_outside) *out_outside = 0;
    const uint64_t n = ctx->n_vox;
    if (!n) return O2V_HIP_OK;
    hipStream_t s = ctx->stream;
    DenseCtr *const ctr = ctx->d_dense.ptr;
    const DenseBox b{origin[0], origin[1], origin[2], dims[0], dims[1], dims[2], strides[0], strides[1], strides[2]};
    const uint64_t n_surf = n - std::min<uint64_t>(n, ctx->stats.interior_voxels);
    O2V_CHECK(hipMemsetAsync(&ctr->outside, 0, sizeof(ctr->outside), s));
    const dim3 grid(stream_grid(ctx, n, 8u));
    if (format == O2V_HIP_DENSE_U8)
        O2V_LAUNCH("k_dense_scatter", s, k_dense_scatter<kDenseU8>, grid, dim3(kBlock), 0, s, ctx->d_out.ptr, n, n_surf, b, dst, ctr);
    else if (format == O2V_HIP_DENSE_ARGB32)
        O2V_LAUNCH("k_dense_scatter", s, k_dense_scatter<kDenseArgb32>, grid, dim3(kBlock), 0, s, ctx->d_out.ptr, n, n_surf, b, dst, ctr);
    else
        O2V_LAUNCH("k_dense_scatter", s, k_dense_scatter<kDenseBits>, grid, dim3(kBlock), 0, s, ctx->d_out.ptr, n, n_surf, b, dst, ctr);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipMemcpyAsync(&ctx->h_dense.ptr->outside, &ctr->outside, sizeof(ctr->outside), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    if (out_outside) *out_outside = ctx->h_dense.ptr->outside;
    return O2V_HIP_OK;
}

int o2v_hip_voxels_box(o2v_hip_ctx *ctx, uint32_t lo[3], uint32_t hi[3])
{
    if (!ctx || !lo || !hi) return O2V_HIP_ERR_BAD_ARGUMENT;
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = 0;
    const uint64_t n = ctx->n_vox;
    if (!n) return O2V_HIP_OK;
    O2V_CHECK(hipSetDevice(ctx->device));
    static const char fn[] = "o2v_hip_voxels_box";
    if (int rc; (rc = grow_scratch(ctx, ctx->d_dense, 1, fn, "counters")) || (rc = grow_scratch(ctx, ctx->h_dense, 1, fn, "counters")))
        return rc;
    hipStream_t s = ctx->stream;
    DenseCtr *const ctr = ctx->d_dense.ptr;
    O2V_CHECK(hipMemsetAsync(ctr->lo, 0xff, sizeof(ctr->lo), s));
    O2V_CHECK(hipMemsetAsync(ctr->hi, 0, sizeof(ctr->hi), s));
    O2V_LAUNCH("k_dense_box", s, k_dense_box, dim3(stream_grid(ctx, n, 4u)), dim3(kBlock), 0, s, ctx->d_out.ptr, n, ctr);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(hipMemcpyAsync(ctx->h_dense.ptr->lo, ctr->lo, sizeof(ctr->lo) + sizeof(ctr->hi), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    for (int a = 0; a < 3; ++a) lo[a] = ctx->h_dense.ptr->lo[a], hi[a] = ctx->h_dense.ptr->hi[a] + 1u;
    return O2V_HIP_OK;
}

}  // extern "C"
