// o2v_dev_k8_distance.hpp -- the two passes of the separable distance transforms, and K8: the exact Euclidean distance
// transform of a U8 label grid (o2v_hip_distance_dense).
// Included from o2v_device.hip inside its anonymous namespace, after K11 (RaySource and the kRay* formats of a set grid); none
// of the pipeline's kernels use it.
//
// K8, K15 (o2v_dev_k15_nearest.hpp) and K21 (o2v_dev_k21_thickness.hpp) are one algorithm: a scan per row
// along x, then the lower envelope of parabolas per line along y and along z.  The first part of this file holds it once:
//   dt_seed<Format>          whether a voxel of a set grid is a seed
//   dt_scan_row              one row along x: the nearest seed at or left and at or right of every voxel
//   dt_envelope<Axis, Carry> the lines along y or z: the parabola that is lowest at every position
// and the kernels of the three families are what they plug in.  K8's seeds are the surface voxels (label 1):
//   k_dist_x                 per row: the squared distance to the nearest seed of the row, g(x)^2, or kDistInf.
//   k_dist_envelope<Mode>    per line along y (Mode 0) or z (1: DIST2, 2: SDF): d(u) = min over v of f(v) + (u - v)^2, in place
//                            in dst; the z pass of the SDF writes the signed root, negative where the label is 2.

constexpr int32_t kDistInf = 0x7fffffff;
constexpr uint32_t kDistNone = 0xffffffffu;
constexpr uint32_t kDistChunk = 8;  // values of a line loaded ahead of the envelope's forward sweep

// An int32 grid that the passes write (and the envelope reads): strides in elements and voxels per axis x, y, z.
struct DtGrid {
    uint64_t s0, s1, s2;
    uint32_t nx, ny, nz;
};

// ---- the seed test ----------------------------------------------------------------------------------------------------------

constexpr uint32_t kSeedU8One = 3;   // beside kRayU8, kRayBits, kRayF32Below: a U8 grid whose seeds are the voxels equal to 1

// Whether voxel x of the row at `row` (its offset y * s1 + z * s2) is a seed.
template <uint32_t Format>
__device__ __forceinline__ bool dt_seed(const RaySource &src, uint64_t row, uint32_t x)
{
    if (Format == kRayBits) return (static_cast<const uint32_t *>(src.p)[row + (x >> 5)] >> (x & 31u)) & 1u;
    if (Format == kRayF32Below) return static_cast<const float *>(src.p)[row + (uint64_t) x * src.s0] < src.level;
    const uint8_t v = static_cast<const uint8_t *>(src.p)[row + (uint64_t) x * src.s0];
    return Format == kSeedU8One ? v == 1u : v != 0u;
}

// ---- the row scan -----------------------------------------------------------------------------------------------------------

// One row of nx voxels, by one wave: lanes over x in chunks of 64.  seed(x, ahead) says whether voxel x < nx is a seed, and
// out[x * stride] = value(x, l, r) of the last seed at or left of x and the first at or right of it (kDistNone: none).  A
// chunk's seeds are a ballot mask, so l (the inclusive max-scan) and r (the min-scan from the right) are bit scans of the mask,
// with the last seed of the chunks before as the left carry and a look-ahead over the chunks after as the right.  The look-ahead
// asks with ahead = true and reads each chunk at most once; every voxel is asked with ahead = false exactly once, in its own
// chunk's turn, so a seed test that also writes does it there.  (value is formed for the lanes past the row's end too, and
// dropped: the store alone is under the bounds test.)
template <typename Seed, typename Value>
__device__ __forceinline__ void dt_scan_row(uint32_t nx, uint32_t lane, Seed seed, Value value, int32_t *out, uint64_t stride)
{
    const unsigned long long upto = lane == 63u ? ~0ull : (2ull << lane) - 1ull;  // bits 0 .. lane
    uint32_t left = kDistNone;   // the last seed of the chunks before
    uint32_t ahead = 0;          // the first seed at or after the next chunk when >= x0 + 64 (kDistNone: none to the end)
    for (uint32_t x0 = 0; x0 < nx; x0 += 64u) {
        const uint32_t x = x0 + lane;
        const unsigned long long m = __ballot(x < nx && seed(x, false));
        if (ahead < x0 + 64u) {   // (wave-uniform) look ahead for the first seed behind this chunk
            ahead = kDistNone;
            for (uint32_t c = x0 + 64u; c < nx; c += 64u) {
                const unsigned long long mc = __ballot(c + lane < nx && seed(c + lane, true));
                if (mc) {
                    ahead = c + (uint32_t) __builtin_ctzll(mc);
                    break;
                }
            }
        }
        const unsigned long long ml = m & upto, mr = m >> lane;
        const uint32_t l = ml ? x0 + 63u - (uint32_t) __builtin_clzll(ml) : left;
        const uint32_t r = mr ? x + (uint32_t) __builtin_ctzll(mr) : ahead;
        const int32_t v = value(x, l, r);
        if (x < nx) out[(uint64_t) x * stride] = v;
        if (m) left = x0 + 63u - (uint32_t) __builtin_clzll(m);
    }
}

// g(x)^2 from the seeds l and r around x: the squared distance to the nearer one, kDistInf without a seed in the row.
__device__ __forceinline__ int32_t dt_row_d2(uint32_t x, uint32_t l, uint32_t r)
{
    uint32_t d = kDistNone;
    if (l != kDistNone) d = x - l;
    if (r != kDistNone) d = min(d, r - x);
    return d == kDistNone ? kDistInf : (int32_t) (d * d);
}

// The waves of the grid take the rows (y, z) in turns: the first row of this wave, and its stride.
__device__ __forceinline__ uint64_t dt_first_row() { return (uint64_t) blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6); }
__device__ __forceinline__ uint64_t dt_row_stride() { return (uint64_t) gridDim.x * (kBlock / 64u); }

// ---- the envelope -----------------------------------------------------------------------------------------------------------

constexpr uint32_t kDtY = 0, kDtZ = 1;

// One stack entry: the parabola's vertex s and the first position t where it is the lowest (both below 2^16), and the word
// its carry is made from.
__device__ __forceinline__ uint2 dist_entry(uint32_t s, uint32_t t, uint32_t word) { return make_uint2(s | (t << 16), word); }

// K8's carry: the grid holds f itself.  (K15's, with a payload that f is recomputed from: o2v_dev_k15_nearest.hpp.)
struct DistCarry {
    static constexpr uint32_t kNone = (uint32_t) kDistInf;   // the grid's word of a position without a parabola
    uint32_t f;
    static __device__ __forceinline__ DistCarry of(uint32_t word, uint32_t, uint32_t) { return DistCarry{word}; }
    __device__ __forceinline__ uint32_t word() const { return f; }
};

// The lines of g along y (Axis kDtY) or z (kDtZ): the lower envelope of parabolas of Meijster et al. 2000 in 64-bit integers,
// d(u) = min over v of f(v) + (u - v)^2.  One lane per line, consecutive lanes on consecutive x, so every grid access of a wave
// is contiguous when the x stride is 1.  The line (x, w) - w its z in the y pass, its y in the z pass - holds a word per
// position, Carry::kNone where there is no parabola; Carry::of(word, x, w) is what the sweep keeps of a parabola: its f, and
// what else the emit needs.  The stack lives in the context's scratch, entry k of slot s at stack[k * slots + s] (a wave's
// entries of equal depth are contiguous), with its top two entries in registers.  Backward, emit(p, x, w, u, found, s, c) writes
// position u of the line, at p: s and c are the vertex and the carry of the parabola that is lowest there, d(u) = (u - s)^2 + c.f
// (the exact minimum: below 2^31 - 1); found is false on a line without any.
template <uint32_t Axis, typename Carry, typename Emit>
__device__ __forceinline__ void dt_envelope(int32_t *__restrict__ grid, const DtGrid &g, uint2 *__restrict__ stack, uint64_t slots, Emit emit)
{
    const uint64_t slot = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n = Axis == kDtY ? g.ny : g.nz;
    const uint64_t step = Axis == kDtY ? g.s1 : g.s2;
    const uint64_t lines = (uint64_t) g.nx * (Axis == kDtY ? g.nz : g.ny);
    uint2 *const st = stack + slot;
    for (uint64_t line = slot; line < lines; line += slots) {
        const uint32_t x = (uint32_t) (line % g.nx), w = (uint32_t) (line / g.nx);
        int32_t *const col = grid + (uint64_t) x * g.s0 + (uint64_t) w * (Axis == kDtY ? g.s2 : g.s1);
        // forward: the lower envelope of the parabolas of the positions that have one.  Entries 0 .. q - 1 are in the scratch,
        // entry q (ts, tt, tc) and entry q - 1 (bs, bt, bc) also in registers.
        //
        // Ties.  On a <= b the top - the lower vertex - stays, and u's parabola takes over at 1 + floor(Sep), past every
        // position where the two are equal, so a position takes the smallest vertex among those that give its minimum.
        // (K15's smallest-index guarantee rests on it: o2v_dev_k15_nearest.hpp.)
        int32_t q = -1;
        uint32_t ts = 0, tt = 0, bs = 0, bt = 0;
        Carry tc{}, bc{};
        for (uint32_t u0 = 0; u0 < n; u0 += kDistChunk) {
            uint32_t wv[kDistChunk];
#pragma unroll
            for (uint32_t k = 0; k < kDistChunk; ++k) wv[k] = u0 + k < n ? (uint32_t) col[(uint64_t) (u0 + k) * step] : Carry::kNone;
#pragma unroll
            for (uint32_t k = 0; k < kDistChunk; ++k) {
                const uint32_t u = u0 + k;
                if (wv[k] == Carry::kNone) continue;
                const Carry cu = Carry::of(wv[k], x, w);
                while (q >= 0) {
                    const int64_t a = (int64_t) ((int32_t) tt - (int32_t) ts) * ((int32_t) tt - (int32_t) ts) + tc.f;
                    const int64_t b = (int64_t) ((int32_t) tt - (int32_t) u) * ((int32_t) tt - (int32_t) u) + cu.f;
                    if (a <= b) break;
                    --q;   // pop: entry q - 1 becomes the top, entry q - 2 is loaded behind it
                    ts = bs, tt = bt, tc = bc;
                    if (q >= 1) {
                        const uint2 e = st[(uint64_t) (q - 1) * slots];
                        bs = e.x & 0xffffu, bt = e.x >> 16, bc = Carry::of(e.y, x, w);
                    }
                }
                if (q < 0) {
                    q = 0, ts = u, tt = 0, tc = cu;
                    continue;
                }
                // where u's parabola goes below the top's: 1 + floor(Sep); the numerator is >= 0 (the top is not above u's
                // parabola at tt >= 0), and below 2^33
                const uint64_t num = (uint64_t) ((int64_t) u * u - (int64_t) ts * ts + (int64_t) cu.f - (int64_t) tc.f);
                const uint64_t sep = num / (uint64_t) (2u * (u - ts));
                if (sep + 1u < n) {
                    st[(uint64_t) q * slots] = dist_entry(ts, tt, tc.word());
                    bs = ts, bt = tt, bc = tc;
                    ++q, ts = u, tt = (uint32_t) sep + 1u, tc = cu;
                }
            }
        }
        // backward: each position takes the parabola whose range holds it; the t of the entries rise strictly, so there is
        // at most one pop per position, and the entry below is loaded a position (or more) before it is needed
        for (uint32_t u = n; u-- > 0;) {
            emit(col + (uint64_t) u * step, x, w, u, q >= 0, ts, tc);
            if (q >= 0 && u == tt) {
                --q;
                ts = bs, tt = bt, tc = bc;
                if (q >= 1) {
                    const uint2 e = st[(uint64_t) (q - 1) * slots];
                    bs = e.x & 0xffffu, bt = e.x >> 16, bc = Carry::of(e.y, x, w);
                }
            }
        }
    }
}

// ---- K8 ---------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void k_dist_x(RaySource lab, int32_t *__restrict__ dst, DtGrid g)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t rows = (uint64_t) g.ny * g.nz;
    for (uint64_t row = dt_first_row(); row < rows; row += dt_row_stride()) {
        const uint64_t y = row % g.ny, z = row / g.ny;
        const uint64_t lrow = y * lab.s1 + z * lab.s2;
        int32_t *drow = dst + y * g.s1 + z * g.s2;
        dt_scan_row(g.nx, lane, [&](uint32_t x, bool) { return dt_seed<kSeedU8One>(lab, lrow, x); }, dt_row_d2, drow, g.s0);
    }
}

constexpr uint32_t kDistY = 0, kDistZ = 1, kDistZSdf = 2;

// The labels are read by kDistZSdf alone: K21 runs kDistY and kDistZ on its own grids, without any.
template <uint32_t Mode>
__global__ __launch_bounds__(kBlock) void k_dist_envelope(int32_t *__restrict__ dst, DtGrid g, RaySource lab, uint2 *__restrict__ stack,
                                                          uint64_t slots)
{
    dt_envelope<Mode == kDistY ? kDtY : kDtZ, DistCarry>(dst, g, stack, slots, [&](int32_t *p, uint32_t x, uint32_t w, uint32_t u, bool found, uint32_t s, DistCarry c) {
        const int32_t d = found ? (int32_t) ((u - s) * (u - s)) + (int32_t) c.f : kDistInf;
        if (Mode == kDistZSdf) {
            const bool inside = static_cast<const uint8_t *>(lab.p)[(uint64_t) x * lab.s0 + (uint64_t) w * lab.s1 + (uint64_t) u * lab.s2] == 2u;
            const float r = d == kDistInf ? __int_as_float(0x7f800000) : (float) sqrt((double) d);
            *p = __float_as_int(inside ? -r : r);
        }
        else
            *p = d;
    });
}
