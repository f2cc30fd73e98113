// o2v_dev_k15_nearest.hpp -- K15: the nearest-voxel (feature) transform of a dense grid (o2v_hip_nearest_dense).
// Included from o2v_device.hip inside its anonymous namespace, after K8 (whose constants and stack entry it uses); none of the
// pipeline's kernels use it.
//
// K8's three separable passes (DESIGN.md sections 11 and 18), carrying the nearest seed's coordinates instead of its distance:
//   k_near_x<Format>         per row along x: the x coordinate of the nearest seed of the row (the left one on a tie), or
//                            kNearNone.  k_dist_x's ballot masks, left carry and look-ahead; the seed test is per format.
//   k_near_envelope<Pass, Paint>
//                            per line along y (kNearY) or z (kNearZ): k_dist_envelope's lower envelope with a payload per
//                            voxel in place of f - fx before the y pass, fx | fy << 16 before the z pass, kNearNone where
//                            the row (the plane) has no seed - and f recomputed from it.  The z pass writes the linear
//                            index of the seed, d2 if asked for and (Paint) the value of the seed into the voxels that take it.

constexpr uint32_t kNearNone = 0xffffffffu;   // (free: an axis is at most 46 341 long, so fx | fy << 16 <= 0xb504b504)
constexpr uint32_t kNearU8 = 0, kNearBits = 1, kNearF32Below = 2, kNearU8One = 3;   // O2V_HIP_GRID_*; 3: U8 with SEED_ONE
constexpr uint32_t kNearY = 0, kNearZ = 1;
constexpr uint32_t kNearNoPaint = 0, kNearPaint = 1, kNearPaintInside = 2;

// The seed grid and `nearest`: strides in elements (words for BITS), per axis x, y, z.
struct NearGrid {
    const void *src;
    uint64_t l0, l1, l2;
    float level;
    uint64_t d0, d1, d2;
    uint32_t nx, ny, nz;
};

// The optional outputs of the z pass.
struct NearOut {
    int32_t *dist2;
    uint64_t e0, e1, e2;
    int32_t *values;
    uint64_t v0, v1, v2;
    uint32_t max_dist2;
};

// Whether voxel x of the row at `row` (its offset y * l1 + z * l2) is a seed.
template <uint32_t Format>
__device__ __forceinline__ bool near_seed(const NearGrid &g, uint64_t row, uint32_t x)
{
    if (Format == kNearBits) return (static_cast<const uint32_t *>(g.src)[row + (x >> 5)] >> (x & 31u)) & 1u;
    if (Format == kNearF32Below) return static_cast<const float *>(g.src)[row + (uint64_t) x * g.l0] < g.level;
    const uint8_t v = static_cast<const uint8_t *>(g.src)[row + (uint64_t) x * g.l0];
    return Format == kNearU8One ? v == 1u : v != 0u;
}

template <uint32_t Format>
__global__ __launch_bounds__(kBlock) void k_near_x(int32_t *__restrict__ dst, NearGrid g)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t) gridDim.x * (kBlock / 64u);
    const uint64_t rows = (uint64_t) g.ny * g.nz;
    const unsigned long long upto = lane == 63u ? ~0ull : (2ull << lane) - 1ull;  // bits 0 .. lane
    for (uint64_t row = (uint64_t) blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6); row < rows; row += waves) {
        const uint64_t y = row % g.ny, z = row / g.ny;
        const uint64_t lrow = y * g.l1 + z * g.l2;
        int32_t *drow = dst + y * g.d1 + z * g.d2;
        uint32_t left = kNearNone;   // the last seed of the chunks before
        uint32_t ahead = 0;          // the first seed at or after the next chunk when >= x0 + 64 (kNearNone: none to the end)
        for (uint32_t x0 = 0; x0 < g.nx; x0 += 64u) {
            const uint32_t x = x0 + lane;
            const unsigned long long m = __ballot(x < g.nx && near_seed<Format>(g, lrow, x));
            if (ahead < x0 + 64u) {   // (wave-uniform) look ahead for the first seed behind this chunk
                ahead = kNearNone;
                for (uint32_t c = x0 + 64u; c < g.nx; c += 64u) {
                    const unsigned long long mc = __ballot(c + lane < g.nx && near_seed<Format>(g, lrow, c + lane));
                    if (mc) {
                        ahead = c + (uint32_t) __builtin_ctzll(mc);
                        break;
                    }
                }
            }
            const unsigned long long ml = m & upto, mr = m >> lane;
            const uint32_t l = ml ? x0 + 63u - (uint32_t) __builtin_clzll(ml) : left;
            const uint32_t r = mr ? x + (uint32_t) __builtin_ctzll(mr) : ahead;
            // the nearer of the two; the left one - the smaller x - on a tie
            uint32_t fx = l;
            if (r != kNearNone && (l == kNearNone || r - x < x - l)) fx = r;
            if (x < g.nx) drow[(uint64_t) x * g.d0] = (int32_t) fx;
            if (m) left = x0 + 63u - (uint32_t) __builtin_clzll(m);
        }
    }
}

// f of the parabola at the line's position of payload p, on the line (x, w): what the passes before left of the squared
// distance - (x - fx)^2 in the y pass (p = fx), (x - fx)^2 + (w - fy)^2 in the z pass (p = fx | fy << 16, w = y).
template <uint32_t Pass>
__device__ __forceinline__ uint32_t near_f(uint32_t p, uint32_t x, uint32_t w)
{
    const int32_t dx = (int32_t) x - (int32_t) (p & 0xffffu);
    uint32_t f = (uint32_t) (dx * dx);
    if (Pass == kNearZ) {
        const int32_t dy = (int32_t) w - (int32_t) (p >> 16);
        f += (uint32_t) (dy * dy);
    }
    return f;
}

template <uint32_t Pass, uint32_t Paint>
__global__ __launch_bounds__(kBlock) void k_near_envelope(int32_t *__restrict__ dst, NearGrid g, NearOut o, uint2 *__restrict__ stack,
                                                          uint64_t slots)
{
    const uint64_t slot = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n = Pass == kNearY ? g.ny : g.nz;
    const uint64_t step = Pass == kNearY ? g.d1 : g.d2;
    const uint64_t lines = (uint64_t) g.nx * (Pass == kNearY ? g.nz : g.ny);
    uint2 *const st = stack + slot;
    for (uint64_t line = slot; line < lines; line += slots) {
        const uint32_t x = (uint32_t) (line % g.nx), w = (uint32_t) (line / g.nx);
        int32_t *const col = dst + (uint64_t) x * g.d0 + (uint64_t) w * (Pass == kNearY ? g.d2 : g.d1);
        // forward: the lower envelope of the parabolas of the positions with a payload.  Entries 0 .. q - 1 are in the
        // scratch (s | t << 16, payload), entry q (ts, tt, tp; tf = f of tp) and entry q - 1 (bs, bt, bp, bf) also in registers.
        //
        // Ties.  On a <= b the top - the lower vertex - stays, and u's parabola takes over at 1 + floor(Sep), past every
        // position where the two are equal, so a position takes the smallest vertex among those that give its minimum.
        // In the z pass that is the smallest z with a nearest seed in its plane.  The payload at (x, y) of that plane came
        // from the y pass by the same rule: the smallest y of that plane whose row holds a seed at the plane's minimum; and
        // the payload there from the x pass: the left of two seeds equally far.  Each of them is a nearest seed of the
        // voxel, so together they are the smallest (z, y, x), the smallest linear index, among its nearest seeds.
        int32_t q = -1;
        uint32_t ts = 0, tt = 0, tp = 0, tf = 0, bs = 0, bt = 0, bp = 0, bf = 0;
        for (uint32_t u0 = 0; u0 < n; u0 += kDistChunk) {
            uint32_t pv[kDistChunk];
#pragma unroll
            for (uint32_t k = 0; k < kDistChunk; ++k) pv[k] = u0 + k < n ? (uint32_t) col[(uint64_t) (u0 + k) * step] : kNearNone;
#pragma unroll
            for (uint32_t k = 0; k < kDistChunk; ++k) {
                const uint32_t u = u0 + k;
                const uint32_t pu = pv[k];
                if (pu == kNearNone) continue;
                const uint32_t fu = near_f<Pass>(pu, x, w);
                while (q >= 0) {
                    const int64_t a = (int64_t) ((int32_t) tt - (int32_t) ts) * ((int32_t) tt - (int32_t) ts) + tf;
                    const int64_t b = (int64_t) ((int32_t) tt - (int32_t) u) * ((int32_t) tt - (int32_t) u) + fu;
                    if (a <= b) break;
                    --q;   // pop: entry q - 1 becomes the top, entry q - 2 is loaded behind it
                    ts = bs, tt = bt, tp = bp, tf = bf;
                    if (q >= 1) {
                        const uint2 e = st[(uint64_t) (q - 1) * slots];
                        bs = e.x & 0xffffu, bt = e.x >> 16, bp = e.y, bf = near_f<Pass>(e.y, x, w);
                    }
                }
                if (q < 0) {
                    q = 0, ts = u, tt = 0, tp = pu, tf = fu;
                    continue;
                }
                // where u's parabola goes below the top's: 1 + floor(Sep); the numerator is >= 0 (the top is not above u's
                // parabola at tt >= 0), and below 2^33
                const uint64_t num = (uint64_t) ((int64_t) u * u - (int64_t) ts * ts + (int64_t) fu - (int64_t) tf);
                const uint64_t sep = num / (uint64_t) (2u * (u - ts));
                if (sep + 1u < n) {
                    st[(uint64_t) q * slots] = dist_entry(ts, tt, tp);
                    bs = ts, bt = tt, bp = tp, bf = tf;
                    ++q, ts = u, tt = (uint32_t) sep + 1u, tp = pu, tf = fu;
                }
            }
        }
        // backward: each position takes the parabola whose range holds it; the t of the entries rise strictly, so there is
        // at most one pop per position, and the entry below is loaded a position (or more) before it is needed
        for (uint32_t u = n; u-- > 0;) {
            if (Pass == kNearY) {
                col[(uint64_t) u * step] = q >= 0 ? (int32_t) (tp | (ts << 16)) : (int32_t) kNearNone;
            } else {
                const uint32_t fx = tp & 0xffffu, fy = tp >> 16;
                int32_t d = kDistInf, near = -1;
                if (q >= 0) {
                    d = (int32_t) ((u - ts) * (u - ts)) + (int32_t) tf;              // (the exact minimum: below 2^31 - 1)
                    near = (int32_t) (((uint64_t) ts * g.ny + fy) * g.nx + fx);      // (below nx * ny * nz <= 2^31 - 1)
                }
                col[(uint64_t) u * step] = near;
                if (o.dist2) o.dist2[(uint64_t) x * o.e0 + (uint64_t) w * o.e1 + (uint64_t) u * o.e2] = d;
                // a voxel is a seed where d is 0: seeds are only read, the others only written
                if (Paint != kNearNoPaint && q >= 0 && d != 0 && (uint32_t) d <= o.max_dist2) {
                    bool take = true;
                    if (Paint == kNearPaintInside)
                        take = static_cast<const uint8_t *>(g.src)[(uint64_t) x * g.l0 + (uint64_t) w * g.l1 + (uint64_t) u * g.l2] != 0u;
                    if (take)
                        o.values[(uint64_t) x * o.v0 + (uint64_t) w * o.v1 + (uint64_t) u * o.v2] =
                            o.values[(uint64_t) fx * o.v0 + (uint64_t) fy * o.v1 + (uint64_t) ts * o.v2];
                }
            }
            if (q >= 0 && u == tt) {
                --q;
                ts = bs, tt = bt, tp = bp, tf = bf;
                if (q >= 1) {
                    const uint2 e = st[(uint64_t) (q - 1) * slots];
                    bs = e.x & 0xffffu, bt = e.x >> 16, bp = e.y, bf = near_f<Pass>(e.y, x, w);
                }
            }
        }
    }
}
