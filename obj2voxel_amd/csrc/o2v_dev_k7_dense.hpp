// o2v_dev_k7_dense.hpp -- K7: device-resident input and dense output (o2v_hip_set_triangles_device, o2v_hip_write_dense,
// o2v_hip_voxels_box).  Included from o2v_device.hip inside its anonymous namespace; none of the pipeline's kernels use it.
//
//   k_gather_tris<Index>  positions [n][3] + faces [T][3] -> the [T][9] vertex array of the context.  One wave per 64
//                         triangles, one output word per lane and step (9 steps): the stores of a wave are 256 contiguous
//                         bytes.  Every index is clamped into [0, n) before its load; an index that was out of range sets a flag.
//   k_any_textured        the host call's scan of `types` for a TEXTURED triangle, as a flag
//   k_dense_scatter<F>    records of the last call -> a caller's dense grid (U8: 1 surface / 2 interior, ARGB32: the argb,
//                         BITS: one atomicOr per record); records outside the box are counted
//   k_dense_box           the records' [lo, hi] box: wave and block reduction, one atomic per block and axis

// The flags and sums of these kernels, one small array of the context (reset by the host before each use).
struct DenseCtr {
    unsigned long long outside;  // k_dense_scatter: records outside the box
    uint32_t bad_index;          // k_gather_tris: a face index was out of range
    uint32_t textured;           // k_any_textured: some triangle is TEXTURED
    uint32_t lo[3], hi[3];       // k_dense_box: min and max of x, y, z (lo starts at ~0, hi at 0)
};

// A box of output voxels and the layout of the grid it is written to (include/o2v_hip.h, o2v_hip_write_dense).
struct DenseBox {
    uint32_t ox, oy, oz;  // origin
    uint32_t dx, dy, dz;  // extent
    uint64_t s0, s1, s2;  // strides: elements (U8, ARGB32) or 32-bit words (BITS; s0 unused)
};
constexpr uint32_t kDenseU8 = 0, kDenseArgb32 = 1, kDenseBits = 2;

constexpr uint64_t kBadIndex = 1ull << 32;  // the first index that is refused whatever n_positions is

template <typename Index>
__global__ __launch_bounds__(kBlock) void k_gather_tris(const float *__restrict__ pos, uint64_t n_pos, const Index *__restrict__ faces,
                                                        uint64_t count, float *__restrict__ verts, DenseCtr *__restrict__ ctr)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t) gridDim.x * (kBlock / 64u);
    const uint64_t limit = n_pos < kBadIndex ? n_pos : kBadIndex;
    bool bad = false;
    for (uint64_t t0 = ((uint64_t) blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6)) * 64u; t0 < count; t0 += waves * 64u) {
#pragma unroll
        for (uint32_t k = 0; k < 9; ++k) {
            const uint32_t li = k * 64u + lane;           // word of the wave's 64 triangles
            const uint32_t tl = li / 9u, c = li - tl * 9u;  // triangle, corner * 3 + axis
            const uint64_t t = t0 + tl;
            if (t >= count) continue;
            const long long idx = (long long) faces[t * 3u + c / 3u];
            const bool in = idx >= 0 && (unsigned long long) idx < limit;
            bad |= !in;
            const uint64_t j = in ? (uint64_t) idx : idx < 0 ? 0u : n_pos - 1u;
            verts[t * 9u + c] = pos[j * 3u + (c - c / 3u * 3u)];
        }
    }
    if (__ballot(bad) && lane == 0) atomicOr(&ctr->bad_index, 1u);
}

__global__ __launch_bounds__(kBlock) void k_any_textured(const uint32_t *__restrict__ types, uint64_t count, DenseCtr *__restrict__ ctr)
{
    bool tex = false;
    for (uint64_t t = (uint64_t) blockIdx.x * kBlock + threadIdx.x; t < count; t += (uint64_t) gridDim.x * kBlock)
        tex |= types[t] == (uint32_t) O2V_HIP_TRI_TEXTURED;
    if (__ballot(tex) && (threadIdx.x & 63u) == 0) atomicOr(&ctr->textured, 1u);
}

// Records [0, n) of d_out, the first n_surf of them surface records.  BITS: one device-scope atomicOr per record.  Combining
// the lanes of a wave that hit the same word first (a ballot loop over the distinct words, an OR reduction each) was measured
// and not kept: 0.41 ms against 0.20 ms for the bench mesh's 4.6 M records at 1024.
template <uint32_t Fmt>
__global__ __launch_bounds__(kBlock) void k_dense_scatter(const uint4 *__restrict__ out, uint64_t n, uint64_t n_surf, DenseBox b,
                                                          void *__restrict__ dst, DenseCtr *__restrict__ ctr)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n_outside = 0;
    for (uint64_t r0 = (uint64_t) blockIdx.x * kBlock + (threadIdx.x & ~63u); r0 < n; r0 += (uint64_t) gridDim.x * kBlock) {
        const uint64_t r = r0 + lane;
        const bool valid = r < n;
        const uint4 v = valid ? out[r] : make_uint4(0u, 0u, 0u, 0u);
        const uint32_t x = v.x - b.ox, y = v.y - b.oy, z = v.z - b.oz;  // (wraps above the box for a coordinate below it)
        const bool inside = valid && x < b.dx && y < b.dy && z < b.dz;
        n_outside += valid && !inside;
        if (Fmt == kDenseU8) {
            if (inside) static_cast<uint8_t *>(dst)[x * b.s0 + y * b.s1 + z * b.s2] = r < n_surf ? 1u : 2u;
        }
        else if (Fmt == kDenseArgb32) {
            if (inside) static_cast<uint32_t *>(dst)[x * b.s0 + y * b.s1 + z * b.s2] = v.w;
        }
        else {
            if (inside) atomicOr(&static_cast<uint32_t *>(dst)[(x >> 5) + y * b.s1 + z * b.s2], 1u << (x & 31u));
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) n_outside += __shfl_xor(n_outside, o);
    if (n_outside && lane == 0) atomicAdd(&ctr->outside, (unsigned long long) n_outside);
}

__global__ __launch_bounds__(kBlock) void k_dense_box(const uint4 *__restrict__ out, uint64_t n, DenseCtr *__restrict__ ctr)
{
    __shared__ uint32_t part[kBlock / 64u][6];
    uint32_t m[6] = {~0u, ~0u, ~0u, 0u, 0u, 0u};  // min x, y, z, max x, y, z
    for (uint64_t r = (uint64_t) blockIdx.x * kBlock + threadIdx.x; r < n; r += (uint64_t) gridDim.x * kBlock) {
        const uint4 v = out[r];
        m[0] = min(m[0], v.x), m[1] = min(m[1], v.y), m[2] = min(m[2], v.z);
        m[3] = max(m[3], v.x), m[4] = max(m[4], v.y), m[5] = max(m[5], v.z);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            m[a] = min(m[a], (uint32_t) __shfl_xor(m[a], o));
            m[a + 3] = max(m[a + 3], (uint32_t) __shfl_xor(m[a + 3], o));
        }
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0)
        for (int a = 0; a < 6; ++a) part[wave][a] = m[a];
    __syncthreads();
    if (threadIdx.x < 6) {
        const uint32_t a = threadIdx.x;
        uint32_t q = part[0][a];
        for (uint32_t w = 1; w < kBlock / 64u; ++w) q = a < 3 ? min(q, part[w][a]) : max(q, part[w][a]);
        if (a < 3 && q != ~0u) atomicMin(&ctr->lo[a], q);
        if (a >= 3 && q != 0u) atomicMax(&ctr->hi[a - 3], q);
    }
}
