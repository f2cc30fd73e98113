// o2v_dev_k17_downsample.hpp -- K17: a dense grid merged into a coarser one, f^3 fine voxels per coarse voxel
// (o2v_hip_downsample).  Included from o2v_device.hip inside its anonymous namespace, after K16; it reads the grid through K11's
// ray_read16, as K12's classify pass does.
//
// Blocks are aligned to the global lattice (include/o2v_hip.h): coarse voxel X of the coarse box covers the global fine
// coordinates [(corigin + X) f, (corigin + X + 1) f) per axis, clipped to the box (ds_block_range); what lies outside is empty.
//
//   k_downsample<Format, Vec>   the one launch.  A workgroup takes a span of kDsSpan coarse voxels of kDsRows / f^2 (at least
//                   one) coarse rows that follow each other along y (items in turns), so that f = 2 has as many loads in
//                   flight as f = 8.  Load: the up to kDsRows fine rows under them - only those inside the box - are read once, 16
//                   voxels a lane (one 16-byte load for U8, four for F32 where rows are aligned, half a word for BITS),
//                   classified into one bit per voxel and put into LDS as 16-bit chunks, chunk c of a row holding the box's
//                   voxels 16 (c0 + c) ... + 15, with a zero chunk behind the last.  Reduce: a lane per coarse voxel takes its
//                   clipped range [lo, hi) along x, extracts that field of at most 8 bits from every row (ds_field: two chunks,
//                   a shift and a mask - blocks of f = 3, 5, 6, 7 straddle chunks) and adds the popcounts: c(X).  Stores are a
//                   lane per coarse voxel along x.  values and argb walk the set bits of the fields: the grid's bytes (in
//                   cache: the workgroup has just read them) and the colours are read only where the fine voxel is solid.
// No atomics, no scratch, no private segment; every sum is an integer, so the result does not depend on any order.

constexpr uint32_t kDsMinFactor = 2, kDsMaxFactor = 8;
constexpr uint32_t kDsSpan = 256;                                   // coarse voxels of a workgroup's span along x
constexpr uint32_t kDsRows = kDsMaxFactor * kDsMaxFactor;           // fine rows of an item, at most: those under a coarse row of f = 8
// 16-bit chunks of a row in LDS: the span's kDsSpan * 8 fine voxels from any offset within a chunk, and the zero chunk
constexpr uint32_t kDsChunks = kDsSpan * kDsMaxFactor / 16u + 2u;
constexpr uint32_t kDsValueMin = 0, kDsValueMax = 1;                // O2V_HIP_DOWN_VALUE_*

#ifndef O2V_DS_HOST
#define O2V_DS_FN __host__ __device__ __forceinline__
O2V_DS_FN uint32_t ds_popc(uint32_t v) { return (uint32_t) __builtin_popcount(v); }
#endif

// ---- the coarse box, a block's fine range, its bits and the mean -----------------------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_downsample.py compiles this part for the host, with O2V_DS_FN and ds_popc
// of its own, and runs it against the reference.)

// Per axis: the coarse origin, floor(origin / f), and the coarse extent, ceil((origin + dim) / f) - floor(origin / f).
O2V_DS_FN uint32_t ds_corigin(uint32_t origin, uint32_t f) { return origin / f; }
O2V_DS_FN uint32_t ds_cdim(uint32_t origin, uint32_t dim, uint32_t f)
{
    return (uint32_t) (((uint64_t) origin + dim + f - 1u) / f) - origin / f;
}

// The fine voxels of coarse voxel X (below the axis' coarse extent) along one axis, in box coordinates and clipped to the box:
// [lo, hi) with lo < hi <= dim.  Global coordinates take 33 bits (origin + dim may be 2^32).
O2V_DS_FN void ds_block_range(uint32_t origin, uint32_t dim, uint32_t f, uint32_t X, uint32_t &lo, uint32_t &hi)
{
    const uint64_t g0 = ((uint64_t) (origin / f) + X) * f;   // the block's first global coordinate; g0 + f > origin
    lo = g0 > origin ? (uint32_t) (g0 - origin) : 0u;
    const uint64_t end = g0 + f - origin;
#ifdef O2V_DS_MUTATE_NO_END_CLIP
    hi = (uint32_t) end;   // (test only: the last block reaches past the box)
#else
    hi = end < dim ? (uint32_t) end : dim;
#endif
}

// Bits [off, off + width) of a row of 16-bit chunks (bit i of chunk c is voxel 16 c + i), width <= 8: they lie in the chunk of
// `off` and the one behind it, which exists (the zero chunk behind a row's last).
O2V_DS_FN uint32_t ds_field(const uint16_t *row, uint32_t off, uint32_t width)
{
    const uint32_t c = off >> 4;
    const uint32_t two = (uint32_t) row[c] | (uint32_t) row[c + 1u] << 16;
    return (two >> (off & 15u)) & ((1u << width) - 1u);
}

// The mean of c >= 1 values with the sum `sum`, rounded half up.
O2V_DS_FN uint32_t ds_mean(uint32_t sum, uint32_t c) { return (2u * sum + c) / (2u * c); }

// The four 8-bit channels of a colour added to their sums (at most 512 x 255 each).
O2V_DS_FN void ds_add_argb(uint32_t (&sum)[4], uint32_t argb)
{
    sum[0] += argb & 0xffu;
    sum[1] += (argb >> 8) & 0xffu;
    sum[2] += (argb >> 16) & 0xffu;
    sum[3] += argb >> 24;
}
O2V_DS_FN uint32_t ds_mean_argb(const uint32_t (&sum)[4], uint32_t c)
{
    return ds_mean(sum[0], c) | ds_mean(sum[1], c) << 8 | ds_mean(sum[2], c) << 16 | ds_mean(sum[3], c) << 24;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_DS_HOST

struct DsGrid {
    uint32_t n[3], o[3], cn[3];   // the fine box, its origin, the coarse box
    uint32_t f, min_count, value_mode;
    uint32_t spans;               // ceil(cn[0] / kDsSpan)
    uint32_t ry, ygroups;         // coarse rows of an item along y: kDsRows / f^2, at least 1; ceil(cn[1] / ry)
    uint64_t items;               // spans * ygroups * cn[2]
};

// The outputs (null: not asked for) and the colours, element strides (x, y, z).
struct DsOut {
    int16_t *count;
    uint64_t k0, k1, k2;
    uint8_t *solid;
    uint64_t s0, s1, s2;
    uint8_t *values;
    uint64_t v0, v1, v2;
    uint32_t *argb;
    uint64_t a0, a1, a2;
    const uint32_t *colors;
    uint64_t c0, c1, c2;
};

template <uint32_t Format, bool Vec>
__global__ __launch_bounds__(kBlock) void k_downsample(RaySource src, DsGrid g, DsOut o)
{
    __shared__ uint16_t s_bits[kDsRows * kDsChunks];
    for (uint64_t item = blockIdx.x; item < g.items; item += gridDim.x) {
        const uint64_t crow = item / g.spans;
        const uint32_t sp = (uint32_t) (item - crow * g.spans);
        const uint32_t Z = (uint32_t) (crow / g.ygroups), Y0 = (uint32_t) (crow - (uint64_t) Z * g.ygroups) * g.ry;
        const uint32_t X0 = sp * kDsSpan, nX = min(kDsSpan, g.cn[0] - X0), nY = min(g.ry, g.cn[1] - Y0);
        uint32_t ylo, yhi, zlo, zhi, flo, fhi, unused;
        ds_block_range(g.o[1], g.n[1], g.f, Y0, ylo, unused);
        ds_block_range(g.o[1], g.n[1], g.f, Y0 + nY - 1u, unused, yhi);
        ds_block_range(g.o[2], g.n[2], g.f, Z, zlo, zhi);
        ds_block_range(g.o[0], g.n[0], g.f, X0, flo, unused);
        ds_block_range(g.o[0], g.n[0], g.f, X0 + nX - 1u, unused, fhi);
        const uint32_t c0 = flo >> 4, nc = ((fhi + 15u) >> 4) - c0;   // at most kDsChunks - 1
        const uint32_t nry = yhi - ylo, nrz = zhi - zlo, nr = nry * nrz;   // nry <= ry f, nrz <= f: at most kDsRows rows
        __syncthreads();   // (the rows of the item before have been read)
        for (uint32_t u = threadIdx.x; u < nr * (nc + 1u); u += kBlock) {
            const uint32_t r = u / (nc + 1u), c = u - r * (nc + 1u);
            uint32_t bits = 0;
            if (c < nc) {
                const uint32_t rz = r / nry, x0 = (c0 + c) * 16u;   // x0 < fhi <= nx
                const uint64_t at = (uint64_t) (ylo + (r - rz * nry)) * src.s1 + (uint64_t) (zlo + rz) * src.s2;
                bits = ray_read16<Format, Vec>(src, at, x0, min(16u, g.n[0] - x0));
            }
            s_bits[r * kDsChunks + c] = (uint16_t) bits;
        }
        __syncthreads();
        for (uint32_t u = threadIdx.x; u < nY * nX; u += kBlock) {
            const uint32_t Yi = u / nX, X = X0 + (u - Yi * nX), Y = Y0 + Yi;
            uint32_t lo, hi, y0, y1;
            ds_block_range(g.o[0], g.n[0], g.f, X, lo, hi);
            ds_block_range(g.o[1], g.n[1], g.f, Y, y0, y1);
            const uint32_t off = lo - c0 * 16u, width = hi - lo;
            uint32_t cnt = 0;
            for (uint32_t rz = 0; rz < nrz; ++rz)
                for (uint32_t y = y0; y < y1; ++y) cnt += ds_popc(ds_field(s_bits + (rz * nry + y - ylo) * kDsChunks, off, width));
            const bool solid = cnt >= g.min_count;
            if (o.count) o.count[(uint64_t) X * o.k0 + (uint64_t) Y * o.k1 + (uint64_t) Z * o.k2] = (int16_t) cnt;
            if (o.solid) o.solid[(uint64_t) X * o.s0 + (uint64_t) Y * o.s1 + (uint64_t) Z * o.s2] = solid ? 1u : 0u;
            if (o.values) {   // (U8 only: a solid fine voxel is a non-zero byte)
                uint32_t best = 0;
                if (solid) {
                    best = g.value_mode == kDsValueMin ? 255u : 0u;
                    for (uint32_t rz = 0; rz < nrz; ++rz)
                        for (uint32_t y = y0; y < y1; ++y) {
                            const uint8_t *p = static_cast<const uint8_t *>(src.p) + (uint64_t) y * src.s1 + (uint64_t) (zlo + rz) * src.s2;
                            for (uint32_t m = ds_field(s_bits + (rz * nry + y - ylo) * kDsChunks, off, width); m; m &= m - 1u) {
                                const uint32_t v = p[(uint64_t) (lo + (uint32_t) __builtin_ctz(m)) * src.s0];
                                best = g.value_mode == kDsValueMin ? min(best, v) : max(best, v);
                            }
                        }
                }
                o.values[(uint64_t) X * o.v0 + (uint64_t) Y * o.v1 + (uint64_t) Z * o.v2] = (uint8_t) best;
            }
            if (o.argb) {
                uint32_t mean = 0;
                if (solid) {
                    uint32_t sum[4] = {0u, 0u, 0u, 0u};
                    for (uint32_t rz = 0; rz < nrz; ++rz)
                        for (uint32_t y = y0; y < y1; ++y) {
                            const uint32_t *p = o.colors + (uint64_t) y * o.c1 + (uint64_t) (zlo + rz) * o.c2;
                            for (uint32_t m = ds_field(s_bits + (rz * nry + y - ylo) * kDsChunks, off, width); m; m &= m - 1u)
                                ds_add_argb(sum, p[(uint64_t) (lo + (uint32_t) __builtin_ctz(m)) * o.c0]);
                        }
                    mean = ds_mean_argb(sum, cnt);
                }
                o.argb[(uint64_t) X * o.a0 + (uint64_t) Y * o.a1 + (uint64_t) Z * o.a2] = mean;
            }
        }
    }
}

#endif   // O2V_DS_HOST
