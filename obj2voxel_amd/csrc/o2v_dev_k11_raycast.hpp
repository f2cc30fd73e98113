// o2v_dev_k11_raycast.hpp -- K11: rays through a dense voxel grid (o2v_hip_raycast_build / o2v_hip_raycast).
// Included from o2v_device.hip inside its anonymous namespace; compiled with -ffp-contract=off (o2v_math.h): every plane
// parameter T_a(i) = ((double) i - o_a) * inv_a is evaluated op by op in double exactly as include/o2v_hip.h writes it, so a
// numpy restatement of the fine walk reproduces every bit.
//
// The snapshot (local coordinates l = voxel - origin; a word is 64 bits):
//   m0[brick]   per 4^3 voxels: bit (lx & 3) + 4 (ly & 3) + 16 (lz & 3) is the voxel's solid predicate (0 past the box)
//   m1[block]   per 16^3 voxels: the same bit of (l >> 2) says that brick is not empty
//   m2[block]   per 64^3 voxels: the same bit of (l >> 4) says that 16^3 block is not empty
// each level stored [z][y][x] over ceil(dims / 4, 16, 64).
// Build:
//   k_ray_build       the only pass over the grid.  A wavefront takes 64 x 4 x 4 voxels (16 bricks along x): lane = q + 4 r
//                     reads 16 voxels along x (q: which 16 of the 64, so four lanes cover 64 contiguous voxels of a row;
//                     r = (y & 3) + 4 (z & 3): the row), as one 16-byte load (U8), four (F32) or half a word (BITS) where
//                     the x stride is 1 and the rows are 16-byte aligned, else element by element.  Its 16 bits are four
//                     nibbles of four bricks at bit 4 r; an OR over the 16 rows (four xor-shuffles) gives the four brick
//                     words, stored by 16 lanes as 128 contiguous bytes.  m1: one atomicOr per (wavefront, 16^3 block) that
//                     has a non-empty brick, at most four per wavefront (the vector global_atomic_or_x2).
//   k_ray_build_top   m2 from m1, a lane per word, no atomics.
// Cast:
//   k_ray_cast        a ray per lane, everything in registers.  The walk of the header is the merge of the three plane
//                     sequences in order of (T, axis).  In an empty aligned block (64^3, 16^3 or 4^3, found by the descent
//                     m2 -> m1 -> m0) the ray advances to the block's least exit event E; outside the box to the greatest
//                     entry event of the axes on which it is still outside.  ray_advance puts every other axis b at the first
//                     plane with (T_b(j), b) > E: an estimate floor(o_b + T d_b), corrected by comparing T_b itself, so the
//                     state after a skip is the state the fine walk has there.  Inside a non-empty brick the walk is the
//                     fine one, on the brick's word in registers.  Skip = false (O2V_RAY_NO_SKIP=1): every fine cell.

constexpr uint32_t kRayU8 = 0, kRayBits = 1, kRayF32Below = 2;   // O2V_HIP_RAY_GRID_*
// The two rules that make the skipping walk equal to the fine one (DESIGN.md section 14 names the tests that catch a change):
constexpr bool kRayTieLowestAxis = true;   // of planes with equal T the lowest axis is crossed first
constexpr bool kRayFixUp = true;           // after a skip, the estimate of an axis' next plane is corrected by T_b itself

struct RaySource {
    const void *p;
    uint64_t s0, s1, s2;   // strides (x, y, z): elements, words for BITS
    float level;
};

struct RayGrid {
    int32_t org[3], dim[3];
    uint32_t b0[3], b1[3], b2[3];   // bricks, 16^3 blocks, 64^3 blocks per axis
    const unsigned long long *m0, *m1, *m2;
};

__device__ __forceinline__ uint32_t ray_bit(int32_t x, int32_t y, int32_t z) { return (uint32_t) ((x & 3) + 4 * (y & 3) + 16 * (z & 3)); }

// ---- build ----------------------------------------------------------------------------------------------------------------

// The solid bits of the n <= 16 voxels x0 .. x0 + n - 1 (x0 a multiple of 16) of the row at element offset `at`: bit i is
// voxel x0 + i.  Vec: the x stride is 1 and every row 16-byte aligned.  (K12's classify pass reads the grid through it too.)
template <uint32_t Format, bool Vec>
__device__ __forceinline__ uint32_t ray_read16(const RaySource &src, uint64_t at, uint32_t x0, uint32_t n)
{
    uint32_t bits = 0;
    if (Format == kRayBits) {
        const uint32_t w = static_cast<const uint32_t *>(src.p)[at + (x0 >> 5)];
        bits = (w >> (x0 & 16u)) & ((1u << n) - 1u);
    } else if (Format == kRayU8) {
        const uint8_t *p = static_cast<const uint8_t *>(src.p) + at;
        if (Vec && n == 16u) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p + x0);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t i = 0; i < 16u; ++i) bits |= (uint32_t) ((w[i >> 2] >> (8u * (i & 3u)) & 0xffu) != 0u) << i;
        } else {
            for (uint32_t i = 0; i < n; ++i) bits |= (uint32_t) (p[(uint64_t) (x0 + i) * src.s0] != 0) << i;
        }
    } else {
        const float *p = static_cast<const float *>(src.p) + at;
        if (Vec && n == 16u) {
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                const float4 v = *reinterpret_cast<const float4 *>(p + x0 + 4u * i);
                bits |= ((uint32_t) (v.x < src.level) | (uint32_t) (v.y < src.level) << 1 | (uint32_t) (v.z < src.level) << 2 |
                         (uint32_t) (v.w < src.level) << 3) << (4u * i);
            }
        } else {
            for (uint32_t i = 0; i < n; ++i) bits |= (uint32_t) (p[(uint64_t) (x0 + i) * src.s0] < src.level) << i;
        }
    }
    return bits;
}

// The n <= 16 / Elem elements x0 .. x0 + n - 1 (x0 a multiple of 16 / Elem) of the row at element offset `at`, of Elem = 1 or 4
// bytes each, as they are: element i in bits [8 Elem i, 8 Elem (i + 1)) of the 16 bytes, zero behind the n-th.  Vec as above.
// (K19 reads its label grid through it.)
template <uint32_t Elem, bool Vec>
__device__ __forceinline__ uint4 ray_read16_raw(const RaySource &src, uint64_t at, uint32_t x0, uint32_t n)
{
    constexpr uint32_t K = 16u / Elem;
    const uint8_t *p = static_cast<const uint8_t *>(src.p) + at * Elem;
    if (Vec && n == K) return *reinterpret_cast<const uint4 *>(p + (uint64_t) x0 * Elem);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t i = 0; i < K; ++i)
        if (i < n) {
            const uint8_t *q = p + (uint64_t) (x0 + i) * src.s0 * Elem;
            w[i * Elem / 4u] |= Elem == 4u ? *reinterpret_cast<const uint32_t *>(q) : (uint32_t) *q << (8u * (i & 3u));
        }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <uint32_t Format, bool Vec>
__global__ __launch_bounds__(kBlock) void k_ray_build(RaySource src, RayGrid g, unsigned long long *__restrict__ m0, unsigned long long *__restrict__ m1)
{
    const uint32_t lane = threadIdx.x & 63u, q = lane & 3u, r = lane >> 2;
    const uint32_t nx = (uint32_t) g.dim[0], ny = (uint32_t) g.dim[1], nz = (uint32_t) g.dim[2];
    const uint32_t tx_n = (nx + 63u) / 64u;
    const uint64_t tiles = (uint64_t) tx_n * g.b0[1] * g.b0[2];
    const uint64_t wave = (uint64_t) blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6), n_waves = (uint64_t) gridDim.x * (kBlock / 64u);
    for (uint64_t tile = wave; tile < tiles; tile += n_waves) {
        const uint64_t row = tile / tx_n;
        const uint32_t tx = (uint32_t) (tile - row * tx_n), bz = (uint32_t) (row / g.b0[1]), by = (uint32_t) (row - (uint64_t) bz * g.b0[1]);
        const uint32_t x0 = tx * 64u + q * 16u, y = by * 4u + (r & 3u), z = bz * 4u + (r >> 2);
        uint32_t bits = 0;
        if (x0 < nx && y < ny && z < nz) {
            const uint64_t at = (uint64_t) y * src.s1 + (uint64_t) z * src.s2;
            bits = ray_read16<Format, Vec>(src, at, x0, min(16u, nx - x0));
        }
        // the nibble of brick j of this lane's four, at its row's place; OR over the 16 rows (lane bits 2 .. 5)
        unsigned long long m[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) m[j] = (unsigned long long) ((bits >> (4u * j)) & 15u) << (4u * r);
#pragma unroll
        for (uint32_t off = 4u; off < 64u; off <<= 1)
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) m[j] |= __shfl_xor(m[j], (int) off);
        const uint32_t bx0 = tx * 16u + q * 4u;
        if (r < 4u && bx0 + r < g.b0[0]) {
            const unsigned long long mine = r == 0u ? m[0] : r == 1u ? m[1] : r == 2u ? m[2] : m[3];
            m0[((uint64_t) bz * g.b0[1] + by) * g.b0[0] + bx0 + r] = mine;
        }
        if (r == 0u) {
            unsigned long long up = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) up |= (unsigned long long) (m[j] != 0ull) << (j + 4u * (by & 3u) + 16u * (bz & 3u));
            if (up) atomicOr(&m1[((uint64_t) (bz >> 2) * g.b1[1] + (by >> 2)) * g.b1[0] + tx * 4u + q], up);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_ray_build_top(RayGrid g, const unsigned long long *__restrict__ m1, unsigned long long *__restrict__ m2)
{
    const uint64_t n = (uint64_t) g.b2[0] * g.b2[1] * g.b2[2];
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
        const uint64_t row = i / g.b2[0];
        const uint32_t X = (uint32_t) (i - row * g.b2[0]), Z = (uint32_t) (row / g.b2[1]), Y = (uint32_t) (row - (uint64_t) Z * g.b2[1]);
        unsigned long long word = 0;
        for (uint32_t c = 0; c < 64u; ++c) {
            const uint32_t x = X * 4u + (c & 3u), y = Y * 4u + ((c >> 2) & 3u), z = Z * 4u + (c >> 4);
            if (x < g.b1[0] && y < g.b1[1] && z < g.b1[2] && m1[((uint64_t) z * g.b1[1] + y) * g.b1[0] + x] != 0ull) word |= 1ull << c;
        }
        m2[i] = word;
    }
}

// ---- the walk ------------------------------------------------------------------------------------------------------------
// (Plain C++ from here to the cast kernel, like the declarations above the build: tests/test_host_raycast.py compiles these two
// parts for the host and holds the walk against the reference there, with each of the two rules above changed as well.)

struct Ray {
    double o[3], d[3], inv[3];
    int32_t c[3], nxt[3], s[3];   // the cell, the index of the next plane per axis, sgn d
    double T;                     // of the last plane crossed
    int32_t face;
};

// T_b(j); b is a constant wherever this is called (unrolled loops), so the ray stays in registers
__device__ __forceinline__ double ray_T(const Ray &r, int b, int32_t j) { return ((double) j - r.o[b]) * r.inv[b]; }

// One step of the fine walk; false: the ray misses (no axis can step, or the next plane lies past t_max).
__device__ __forceinline__ bool ray_step(Ray &r, double tmax)
{
    double best = 0.0;
    int a = -1;
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (r.s[b] != 0) {
            const double Tb = ray_T(r, b, r.nxt[b]);
            if (a < 0 || Tb < best || (!kRayTieLowestAxis && Tb == best)) best = Tb, a = b;
        }
    if (a < 0 || best > tmax) return false;
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (b == a) {
            r.c[b] += r.s[b];
            r.nxt[b] += r.s[b];
            r.face = 2 * b + (r.s[b] > 0 ? 0 : 1);
        }
    r.T = best;
    return true;
}

// Crosses every plane whose event (T, axis) lies before E = (TE, aE), then plane x of axis aE itself.  lim[b] is a plane of
// axis b at or after nxt[b] whose event is known to lie behind E: the next plane of b after the skip is searched up to it.
__device__ __forceinline__ void ray_advance(Ray &r, double TE, int aE, int32_t xE, const int32_t lim[3])
{
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        if (b == aE) {
            r.nxt[b] = xE + r.s[b];
            r.c[b] = r.s[b] > 0 ? xE : xE - 1;
            r.face = 2 * b + (r.s[b] > 0 ? 0 : 1);
        } else if (r.s[b] != 0) {
            const int32_t sb = r.s[b], first = r.nxt[b], last = lim[b];
            double p = r.o[b] + TE * r.d[b];
            p = fmin(fmax(p, -1073741824.0), 1073741824.0);
            int32_t j = (int32_t) floor(p) + (sb > 0 ? 1 : 0);
            j = sb > 0 ? min(max(j, first), last) : max(min(j, first), last);
            if (kRayFixUp) {
                auto before = [&](int32_t k) {
                    const double Tk = ray_T(r, b, k);
                    return Tk < TE || (Tk == TE && (kRayTieLowestAxis ? b < aE : b > aE));
                };
                while (j != last && before(j)) j += sb;
                while (j != first && !before(j - sb)) j -= sb;
            }
            r.nxt[b] = j;
            r.c[b] = sb > 0 ? j - 1 : j;
        }
    }
    r.T = TE;
}

// true: r.c is solid, entered at r.T through r.face
template <bool Skip>
__device__ __forceinline__ bool ray_walk(Ray &r, double tmax, const RayGrid &g)
{
    for (;;) {
        const int32_t lx = r.c[0] - g.org[0], ly = r.c[1] - g.org[1], lz = r.c[2] - g.org[2];
        const bool in = (uint32_t) lx < (uint32_t) g.dim[0] && (uint32_t) ly < (uint32_t) g.dim[1] && (uint32_t) lz < (uint32_t) g.dim[2];
        int32_t x[3], lim[3];   // per axis: the plane of its event; the plane the search ends at
        bool takes[3];          // the axis has an event
        if (in) {
            int k = 0;   // the empty block around the cell has 2^k voxels along an axis; 0: its brick is not empty
            if (Skip) {
                const unsigned long long w2 = g.m2[((uint64_t) (lz >> 6) * g.b2[1] + (uint32_t) (ly >> 6)) * g.b2[0] + (uint32_t) (lx >> 6)];
                if (w2 == 0ull) k = 6;
                else if (!((w2 >> ray_bit(lx >> 4, ly >> 4, lz >> 4)) & 1ull)) k = 4;
                else {
                    const unsigned long long w1 = g.m1[((uint64_t) (lz >> 4) * g.b1[1] + (uint32_t) (ly >> 4)) * g.b1[0] + (uint32_t) (lx >> 4)];
                    if (!((w1 >> ray_bit(lx >> 2, ly >> 2, lz >> 2)) & 1ull)) k = 2;
                }
            }
            if (k == 0) {
                // the fine walk on the brick's word
                const int32_t bx = lx >> 2, by = ly >> 2, bz = lz >> 2;
                const unsigned long long w0 = g.m0[((uint64_t) bz * g.b0[1] + (uint32_t) by) * g.b0[0] + (uint32_t) bx];
                for (;;) {
                    const int32_t ux = r.c[0] - g.org[0], uy = r.c[1] - g.org[1], uz = r.c[2] - g.org[2];
                    if ((ux >> 2) != bx || (uy >> 2) != by || (uz >> 2) != bz) break;
                    if ((w0 >> ray_bit(ux, uy, uz)) & 1ull) return true;
                    if (!ray_step(r, tmax)) return false;
                }
                continue;
            }
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int32_t l = r.c[b] - g.org[b];
                x[b] = lim[b] = g.org[b] + (((l >> k) + (r.s[b] > 0 ? 1 : 0)) << k);
                takes[b] = r.s[b] != 0;
            }
        } else {
            bool gone = false;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int32_t lo = g.org[b], hi = g.org[b] + g.dim[b];
                const bool below = r.c[b] < lo, above = r.c[b] >= hi;
                gone = gone || (r.s[b] > 0 ? above : r.s[b] < 0 ? below : (below || above));   // left on this axis for good
                takes[b] = (r.s[b] > 0 && below) || (r.s[b] < 0 && above);
                x[b] = r.s[b] > 0 ? lo : hi;     // the plane it enters through
                lim[b] = r.s[b] > 0 ? hi : lo;   // the plane it leaves through
            }
            if (gone) return false;
            if (!Skip) {
                if (!ray_step(r, tmax)) return false;
                continue;
            }
        }
        // E: inside, the least of the block's exit events; outside, the greatest of the entry events still ahead
        double TE = 0.0;
        int aE = -1;
        int32_t xE = 0;
#pragma unroll
        for (int b = 0; b < 3; ++b)
            if (takes[b]) {
                const double Tb = ray_T(r, b, x[b]);
                const bool better = in ? (Tb < TE || (!kRayTieLowestAxis && Tb == TE)) : (Tb > TE || (kRayTieLowestAxis && Tb == TE));
                if (aE < 0 || better) TE = Tb, aE = b, xE = x[b];
            }
        if (aE < 0 || TE > tmax) return false;
        if (!in) {
            // an axis whose exit plane comes before E has left the box before the ray is inside on every axis
            bool gone = false;
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (b != aE && r.s[b] != 0) {
                    const double Tl = ray_T(r, b, lim[b]);
                    gone = gone || Tl < TE || (Tl == TE && (kRayTieLowestAxis ? b < aE : b > aE));
                }
            if (gone) return false;
        }
        ray_advance(r, TE, aE, xE, lim);
    }
}

// ---- the cast kernel ---------------------------------------------------------------------------------------------------------

template <bool Skip>
__global__ __launch_bounds__(kBlock) void k_ray_cast(const float *__restrict__ origins, const float *__restrict__ directions, uint64_t n, float t_max,
                                                     RayGrid g, int32_t *__restrict__ hit, float *__restrict__ t_out)
{
    const uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Ray r;
    bool valid = true;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const float of = origins[i * 3u + b], df = directions[i * 3u + b];
        valid = valid && isfinite(of) && isfinite(df) && fabsf(of) <= 4194304.f;
        r.o[b] = (double) of;
        r.d[b] = (double) df;
    }
    int32_t out[4] = {-1, -1, -1, -2};
    float t = __builtin_nanf("");
    if (valid) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            r.s[b] = r.d[b] > 0.0 ? 1 : r.d[b] < 0.0 ? -1 : 0;
            r.inv[b] = r.s[b] != 0 ? 1.0 / r.d[b] : 0.0;
            r.c[b] = (int32_t) floor(r.o[b]);
            r.nxt[b] = r.c[b] + (r.s[b] > 0 ? 1 : 0);
        }
        r.T = 0.0;
        r.face = -1;
        if (ray_walk<Skip>(r, (double) t_max, g)) {
            out[0] = r.c[0], out[1] = r.c[1], out[2] = r.c[2], out[3] = r.face;
            t = (float) r.T;
        } else {
            out[3] = -1;
            t = __builtin_inff();
        }
    }
    if ((reinterpret_cast<uintptr_t>(hit) & 15u) == 0u)
        reinterpret_cast<int4 *>(hit)[i] = make_int4(out[0], out[1], out[2], out[3]);
    else
        hit[i * 4u] = out[0], hit[i * 4u + 1u] = out[1], hit[i * 4u + 2u] = out[2], hit[i * 4u + 3u] = out[3];
    t_out[i] = t;
}
