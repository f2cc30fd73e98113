// o2v_dev_k15_nearest.hpp -- K15: the nearest-voxel (feature) transform of a dense grid (o2v_hip_nearest_dense).
// Included from o2v_device.hip inside its anonymous namespace, after K8 (whose row scan and envelope it runs); none of the
// pipeline's kernels use it.
//
// K8's three separable passes (DESIGN.md sections 11 and 18), carrying the nearest seed's coordinates instead of its distance:
//   k_near_x<Format>         dt_scan_row with the seed test per format; stores the x coordinate of the nearest seed of the row
//                            (the left one on a tie), or kNearNone.
//   k_near_envelope<Pass, Paint>
//                            dt_envelope along y (kNearY) or z (kNearZ) with a payload per voxel in place of f - fx before the
//                            y pass, fx | fy << 16 before the z pass, kNearNone where the row (the plane) has no seed - and f
//                            recomputed from it (NearCarry).  The y pass stores fx | fy << 16; the z pass the linear index of
//                            the seed, d2 if asked for and (Paint) the value of the seed into the voxels that take it.

constexpr uint32_t kNearNone = 0xffffffffu;   // (free: an axis is at most 46 341 long, so fx | fy << 16 <= 0xb504b504)
constexpr uint32_t kNearY = kDtY, kNearZ = kDtZ;
constexpr uint32_t kNearNoPaint = 0, kNearPaint = 1, kNearPaintInside = 2;

// The seed grid (strides in words for BITS) and `nearest`.
struct NearGrid {
    RaySource src;
    DtGrid out;
};

// The optional outputs of the z pass.
struct NearOut {
    int32_t *dist2;
    uint64_t e0, e1, e2;
    int32_t *values;
    uint64_t v0, v1, v2;
    uint32_t max_dist2;
};

template <uint32_t Format>
__global__ __launch_bounds__(kBlock) void k_near_x(int32_t *__restrict__ dst, NearGrid g)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t rows = (uint64_t) g.out.ny * g.out.nz;
    for (uint64_t row = dt_first_row(); row < rows; row += dt_row_stride()) {
        const uint64_t y = row % g.out.ny, z = row / g.out.ny;
        const uint64_t lrow = y * g.src.s1 + z * g.src.s2;
        int32_t *drow = dst + y * g.out.s1 + z * g.out.s2;
        dt_scan_row(
            g.out.nx, lane, [&](uint32_t x, bool) { return dt_seed<Format>(g.src, lrow, x); },
            [](uint32_t x, uint32_t l, uint32_t r) {
                // the nearer of the two; the left one - the smaller x - on a tie
                uint32_t fx = l;
                if (r != kNearNone && (l == kNearNone || r - x < x - l)) fx = r;
                return (int32_t) fx;
            },
            drow, g.out.s0);
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

// The envelope's carry of a parabola: its payload, and f from it.
template <uint32_t Pass>
struct NearCarry {
    static constexpr uint32_t kNone = kNearNone;
    uint32_t p, f;
    static __device__ __forceinline__ NearCarry of(uint32_t word, uint32_t x, uint32_t w) { return NearCarry{word, near_f<Pass>(word, x, w)}; }
    __device__ __forceinline__ uint32_t word() const { return p; }
};

// Ties.  A position takes the smallest vertex among those that give its minimum (dt_envelope).  In the z pass that is the smallest
// z with a nearest seed in its plane.  The payload at (x, y) of that plane came from the y pass by the same rule: the smallest y
// of that plane whose row holds a seed at the plane's minimum; and the payload there from the x pass: the left of two seeds
// equally far.  Each of them is a nearest seed of the voxel, so together they are the smallest (z, y, x), the smallest linear
// index, among its nearest seeds.
template <uint32_t Pass, uint32_t Paint>
__global__ __launch_bounds__(kBlock) void k_near_envelope(int32_t *__restrict__ dst, NearGrid g, NearOut o, uint2 *__restrict__ stack,
                                                          uint64_t slots)
{
    using Carry = NearCarry<Pass>;
    dt_envelope<Pass, Carry>(dst, g.out, stack, slots, [&](int32_t *p, uint32_t x, uint32_t w, uint32_t u, bool found, uint32_t s, Carry c) {
        if (Pass == kNearY) {
            *p = found ? (int32_t) (c.p | (s << 16)) : (int32_t) kNearNone;
            return;
        }
        const uint32_t fx = c.p & 0xffffu, fy = c.p >> 16;
        int32_t d = kDistInf, near = -1;
        if (found) {
            d = (int32_t) ((u - s) * (u - s)) + (int32_t) c.f;
            near = (int32_t) (((uint64_t) s * g.out.ny + fy) * g.out.nx + fx);   // (below nx * ny * nz <= 2^31 - 1)
        }
        *p = near;
        if (o.dist2) o.dist2[(uint64_t) x * o.e0 + (uint64_t) w * o.e1 + (uint64_t) u * o.e2] = d;
        // a voxel is a seed where d is 0: seeds are only read, the others only written
        if (Paint != kNearNoPaint && found && d != 0 && (uint32_t) d <= o.max_dist2) {
            bool take = true;
            if (Paint == kNearPaintInside)
                take = static_cast<const uint8_t *>(g.src.p)[(uint64_t) x * g.src.s0 + (uint64_t) w * g.src.s1 + (uint64_t) u * g.src.s2] != 0u;
            if (take)
                o.values[(uint64_t) x * o.v0 + (uint64_t) w * o.v1 + (uint64_t) u * o.v2] =
                    o.values[(uint64_t) fx * o.v0 + (uint64_t) fy * o.v1 + (uint64_t) s * o.v2];
        }
    });
}
