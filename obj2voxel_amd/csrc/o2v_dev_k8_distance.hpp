// o2v_dev_k8_distance.hpp -- K8: the exact Euclidean distance transform of a U8 label grid (o2v_hip_distance_dense).
// Included from o2v_device.hip inside its anonymous namespace; none of the pipeline's kernels use it.
//
// Seeds are the surface voxels (label 1).  The transform is separable:
//   k_dist_x                 per row along x: the squared distance to the nearest seed of the row, g(x)^2, or kDistInf.
//                            One wave per row, lanes over x in chunks of 64; a chunk's seeds are a ballot mask, so the last
//                            seed at or left of a lane (the inclusive max-scan) and the first at or right of it (the min-scan
//                            from the right) are bit scans of the mask, with the last seed of the chunks before as the left
//                            carry and a look-ahead over the chunks after (each chunk is read at most once by it) as the right.
//   k_dist_envelope<Mode>    per line along y (Mode 0) or z (1: DIST2, 2: SDF): d(u) = min over v of f(v) + (u - v)^2, the
//                            lower envelope of parabolas of Meijster et al. 2000 in 64-bit integers.  One lane per line,
//                            consecutive lanes on consecutive x, so every grid access of a wave is contiguous when the x stride
//                            is 1.  The line's values are read and written in place in dst; the envelope's stack lives in the
//                            context's scratch, entry k of slot s at stack[k * slots + s] (a wave's entries of equal depth are
//                            contiguous), with its top two entries in registers.

constexpr int32_t kDistInf = 0x7fffffff;
constexpr uint32_t kDistNone = 0xffffffffu;
constexpr uint32_t kDistChunk = 8;  // values of a line loaded ahead of the envelope's forward sweep

// The label grid and the destination: strides in elements, per axis x, y, z.
struct DistGrid {
    uint64_t l0, l1, l2;
    uint64_t d0, d1, d2;
    uint32_t nx, ny, nz;
};

__global__ __launch_bounds__(kBlock) void k_dist_x(const uint8_t *__restrict__ lab, int32_t *__restrict__ dst, DistGrid g)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t) gridDim.x * (kBlock / 64u);
    const uint64_t rows = (uint64_t) g.ny * g.nz;
    const unsigned long long upto = lane == 63u ? ~0ull : (2ull << lane) - 1ull;  // bits 0 .. lane
    for (uint64_t row = (uint64_t) blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6); row < rows; row += waves) {
        const uint64_t y = row % g.ny, z = row / g.ny;
        const uint8_t *lrow = lab + y * g.l1 + z * g.l2;
        int32_t *drow = dst + y * g.d1 + z * g.d2;
        uint32_t left = kDistNone;   // the last seed of the chunks before
        uint32_t ahead = 0;          // the first seed at or after the next chunk when >= x0 + 64 (kDistNone: none to the end)
        for (uint32_t x0 = 0; x0 < g.nx; x0 += 64u) {
            const uint32_t x = x0 + lane;
            const unsigned long long m = __ballot(x < g.nx && lrow[(uint64_t) x * g.l0] == 1u);
            if (ahead < x0 + 64u) {   // (wave-uniform) look ahead for the first seed behind this chunk
                ahead = kDistNone;
                for (uint32_t c = x0 + 64u; c < g.nx; c += 64u) {
                    const unsigned long long mc = __ballot(c + lane < g.nx && lrow[(uint64_t) (c + lane) * g.l0] == 1u);
                    if (mc) {
                        ahead = c + (uint32_t) __builtin_ctzll(mc);
                        break;
                    }
                }
            }
            const unsigned long long ml = m & upto, mr = m >> lane;
            const uint32_t l = ml ? x0 + 63u - (uint32_t) __builtin_clzll(ml) : left;
            const uint32_t r = mr ? x + (uint32_t) __builtin_ctzll(mr) : ahead;
            uint32_t d = kDistNone;
            if (l != kDistNone) d = x - l;
            if (r != kDistNone) d = min(d, r - x);
            if (x < g.nx) drow[(uint64_t) x * g.d0] = d == kDistNone ? kDistInf : (int32_t) (d * d);
            if (m) left = x0 + 63u - (uint32_t) __builtin_clzll(m);
        }
    }
}

constexpr uint32_t kDistY = 0, kDistZ = 1, kDistZSdf = 2;

// One stack entry: the parabola's vertex s and the first position t where it is the lowest (both below 2^16), and f(s).
__device__ __forceinline__ uint2 dist_entry(uint32_t s, uint32_t t, uint32_t f) { return make_uint2(s | (t << 16), f); }

template <uint32_t Mode>
__global__ __launch_bounds__(kBlock) void k_dist_envelope(int32_t *__restrict__ dst, const uint8_t *__restrict__ lab, DistGrid g,
                                                          uint2 *__restrict__ stack, uint64_t slots)
{
    const uint64_t slot = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n = Mode == kDistY ? g.ny : g.nz;
    const uint64_t step = Mode == kDistY ? g.d1 : g.d2;
    const uint64_t lines = (uint64_t) g.nx * (Mode == kDistY ? g.nz : g.ny);
    uint2 *const st = stack + slot;
    for (uint64_t line = slot; line < lines; line += slots) {
        const uint64_t x = line % g.nx, w = line / g.nx;
        int32_t *const col = dst + x * g.d0 + w * (Mode == kDistY ? g.d2 : g.d1);
        // forward: the lower envelope of the parabolas of the finite f(v).  Entries 0 .. q - 1 are in the scratch, entry q
        // (ts, tt, tf) and entry q - 1 (bs, bt, bf) also in registers.
        int32_t q = -1;
        uint32_t ts = 0, tt = 0, tf = 0, bs = 0, bt = 0, bf = 0;
        for (uint32_t u0 = 0; u0 < n; u0 += kDistChunk) {
            int32_t fv[kDistChunk];
#pragma unroll
            for (uint32_t k = 0; k < kDistChunk; ++k) fv[k] = u0 + k < n ? col[(uint64_t) (u0 + k) * step] : kDistInf;
#pragma unroll
            for (uint32_t k = 0; k < kDistChunk; ++k) {
                const uint32_t u = u0 + k;
                const int32_t fu = fv[k];
                if (fu == kDistInf) continue;
                while (q >= 0) {
                    const int64_t a = (int64_t) ((int32_t) tt - (int32_t) ts) * ((int32_t) tt - (int32_t) ts) + tf;
                    const int64_t b = (int64_t) ((int32_t) tt - (int32_t) u) * ((int32_t) tt - (int32_t) u) + fu;
                    if (a <= b) break;
                    --q;   // pop: entry q - 1 becomes the top, entry q - 2 is loaded behind it
                    ts = bs, tt = bt, tf = bf;
                    if (q >= 1) {
                        const uint2 e = st[(uint64_t) (q - 1) * slots];
                        bs = e.x & 0xffffu, bt = e.x >> 16, bf = e.y;
                    }
                }
                if (q < 0) {
                    q = 0, ts = u, tt = 0, tf = (uint32_t) fu;
                    continue;
                }
                // where u's parabola goes below the top's: 1 + floor(Sep); the numerator is >= 0 (the top is not above u's
                // parabola at tt >= 0), and below 2^33
                const uint64_t num = (uint64_t) ((int64_t) u * u - (int64_t) ts * ts + fu - (int64_t) tf);
                const uint64_t sep = num / (uint64_t) (2u * (u - ts));
                if (sep + 1u < n) {
                    st[(uint64_t) q * slots] = dist_entry(ts, tt, tf);
                    bs = ts, bt = tt, bf = tf;
                    ++q, ts = u, tt = (uint32_t) sep + 1u, tf = (uint32_t) fu;
                }
            }
        }
        // backward: each position takes the parabola whose range holds it; the t of the entries rise strictly, so there is
        // at most one pop per position, and the entry below is loaded a position (or more) before it is needed
        for (uint32_t u = n; u-- > 0;) {
            int32_t d = kDistInf;
            if (q >= 0) d = (int32_t) ((u - ts) * (u - ts)) + (int32_t) tf;   // (the exact minimum: below 2^31 - 1)
            int32_t *const p = col + (uint64_t) u * step;
            if (Mode == kDistZSdf) {
                const bool inside = lab[x * g.l0 + w * g.l1 + (uint64_t) u * g.l2] == 2u;
                const float r = d == kDistInf ? __int_as_float(0x7f800000) : (float) sqrt((double) d);
                *p = __float_as_int(inside ? -r : r);
            }
            else
                *p = d;
            if (q >= 0 && u == tt) {
                --q;
                ts = bs, tt = bt, tf = bf;
                if (q >= 1) {
                    const uint2 e = st[(uint64_t) (q - 1) * slots];
                    bs = e.x & 0xffffu, bt = e.x >> 16, bf = e.y;
                }
            }
        }
    }
}
