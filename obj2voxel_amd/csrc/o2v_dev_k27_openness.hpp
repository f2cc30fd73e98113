// o2v_dev_k27_openness.hpp -- K27: sky visibility of the voxels of a dense grid (o2v_hip_openness).
// Included from o2v_device.hip inside its anonymous namespace, behind K11, whose build kernels (k_ray_build, k_ray_build_top) make
// the three levels of masks it walks: m0 per 4^3 voxels, m1 per 16^3, m2 per 64^3 (o2v_dev_k11_raycast.hpp), here in scratch of
// its own with the box at origin 0.
//
// The definition is in include/o2v_hip.h: from the centre of a target voxel c0 along an integer direction d the ray crosses the
// planes of axis a at T_a(k) = (2 k + 1) / (2 |d_a|), k = 0, 1, ...; a step takes the least event and crosses every axis whose event
// equals it, together; the cell after it is c0 + sgn(d) * k.  Events are compared by cross-multiplication: every product is
// below 2^25, so everything is uint32 / int32.
//
//   k_open_targets<Mode, false>   a lane per row of four voxels along x of a brick (64 lanes: 256 voxels of a row of the grid): the
//                                 target bits of the row from the brick words - SURFACE from the row's own nibble and its six
//                                 neighbours' -, their number added up per wavefront, one atomicAdd per wavefront.
//   k_open_targets<Mode, true>    the same bits again: 255 (and mask 0) to every voxel that is no target, and the targets' linear
//                                 indices into the list, a wavefront's in one contiguous piece (one atomicAdd per wavefront; the
//                                 order of the pieces decides nothing: every target's result is its own).
//   k_open_walk<Skip, Mask>       a lane per target, a loop over the directions inside: the wavefront walks 64 neighbouring targets
//                                 along one direction at a time, the direction's constants (signs, magnitudes, reciprocals) uniform
//                                 over it, read from a table in LDS (a broadcast read: no bank conflict).  In an empty aligned block
//                                 (64^3, 16^3 or 4^3, by the descent m2 -> m1 -> m0) the ray advances to the block's least exit
//                                 event in one skip (open_skip); in a brick that is not empty it walks cell by cell on the brick's
//                                 word in a register.  Skip = false (O2V_OPEN_NO_SKIP=1): every fine cell.
// The work is targets x directions; the grid itself is read once, by k_ray_build.  Integers only, vector stores only.

constexpr uint32_t kOpenSurface = 0u, kOpenSolid = 1u, kOpenEmpty = 2u, kOpenGrid = 3u;   // O2V_HIP_OPEN_*
constexpr uint32_t kOpenNear2 = 32u * 32u;   // a cut-off up to 32 voxels: the descent goes bottom up (open_walk)
constexpr uint32_t kOpenMaxDirs = 254u, kOpenMaxComponent = 127u, kOpenDirWords = 9u;

#ifndef O2V_OPEN_HOST
#define O2V_OPEN_FN __device__ __forceinline__
#define O2V_OPEN_HD __host__ __device__ __forceinline__   // (what the host side makes the direction table with)
O2V_OPEN_FN uint32_t open_mulhi(uint32_t a, uint32_t b) { return __umulhi(a, b); }
#endif

// ---- the step, the skip, the short division ---------------------------------------------------------------------------------------
// (Plain C++ from here to the kernels: tests/test_host_openness.py compiles this part for the host, with O2V_OPEN_FN, O2V_OPEN_HD
// and open_mulhi of its own, and runs it against the reference.)

// A direction as the walk takes it: sgn d_a, |d_a| and the reciprocal of |d_a| per axis (0 where d_a is 0).
struct OpenDir {
    int32_t s[3];
    uint32_t m[3], r[3];
};
static_assert(sizeof(OpenDir) == 4u * kOpenDirWords, "a direction is nine words of the table");

// The three levels of masks over the box [0, dim) (o2v_dev_k11_raycast.hpp) and the bricks / blocks per axis of each.
struct OpenGrid {
    int32_t dim[3];
    uint32_t b0[3], b1[3], b2[3];
    const unsigned long long *m0, *m1, *m2;
};

// floor(n / d) for n < 2^25 and 1 <= d <= 127 is open_div(n, open_recip(d)) = ((n + 1) * floor((2^32 - 1) / d)) >> 32.
// With r = floor((2^32 - 1) / d) and e = 2^32 - r d, 1 <= e <= d; for n = q d + t, 0 <= t < d:
// (n + 1) r / 2^32 = q + (t + 1) / d - (n + 1) e / (d 2^32), and (n + 1) e <= 2^25 * 2^7 = 2^32 <= (t + 1) 2^32 keeps that in
// [q, q + 1).  One add and one v_mul_hi_u32; d = 1 and the powers of two need no case of their own.
O2V_OPEN_HD uint32_t open_recip(uint32_t d) { return d ? 0xffffffffu / d : 0u; }
O2V_OPEN_FN uint32_t open_div(uint32_t n, uint32_t r) { return open_mulhi(n + 1u, r); }

// Of two events that are equal, both are taken: the rule that makes the walk commute with the symmetries of the lattice.
// (O2V_OPEN_MUTATE_TIE_LESS: the mutation of the host test - only the lowest axis of a tie crosses, as in K11's walk.)
O2V_OPEN_FN bool open_tie(uint32_t event_b, uint32_t event_a)
{
#ifdef O2V_OPEN_MUTATE_TIE_LESS
    return event_b < event_a;
#else
    return event_b <= event_a;
#endif
}

O2V_OPEN_FN uint32_t open_bit(int32_t x, int32_t y, int32_t z) { return (uint32_t) ((x & 3) + 4 * (y & 3) + 16 * (z & 3)); }

// One step of the fine walk: a, the axis of the least event (2 k_a + 1) / (2 m_a) - the lowest of equal ones -, crosses, and with
// it every axis b whose event is not later: (2 k_b + 1) m_a <= (2 k_a + 1) m_b.
O2V_OPEN_FN void open_step(const OpenDir &d, uint32_t k[3])
{
    int a = -1;
    uint32_t na = 0, ma = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (d.m[b] != 0u) {
            const uint32_t nb = 2u * k[b] + 1u;
            if (a < 0 || nb * ma < na * d.m[b]) a = b, na = nb, ma = d.m[b];
        }
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (d.m[b] != 0u && (b == a || open_tie((2u * k[b] + 1u) * ma, na * d.m[b]))) ++k[b];
}

// The skip out of the empty aligned block of side 2^L around the cell c = c0 + s k.  Per axis the crossing that leaves the block
// is K_a = k_a + (s_a > 0 ? hi - c_a : c_a - lo + 1); E, the least (2 K_a - 1) / (2 m_a), is the event at which the ray leaves,
// on axis e with N = 2 K_e - 1, M = m_e.  Axis b has made every crossing whose event is at or before E: those with
// (2 j + 1) / (2 m_b) <= N / (2 M), j = 0 ... k_b - 1, so k_b = (floor(N m_b / M) + 1) / 2 - for an axis that ties with e this
// is K_b itself.  The state is that of the fine walk after event E.  K <= 65 536, so N m_b < 2^24.
O2V_OPEN_FN void open_skip(const OpenDir &d, const int32_t c[3], uint32_t L, uint32_t k[3])
{
    uint32_t K[3] = {0u, 0u, 0u}, N = 0, M = 0, R = 0;
    int e = -1;
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (d.m[b] != 0u) {
            const int32_t lo = (c[b] >> L) << L;
            K[b] = k[b] + (uint32_t) (d.s[b] > 0 ? lo + (int32_t) (1u << L) - c[b] : c[b] - lo + 1);
            const uint32_t nb = 2u * K[b] - 1u;
            if (e < 0 || nb * M < N * d.m[b]) e = b, N = nb, M = d.m[b], R = d.r[b];
        }
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (d.m[b] != 0u) k[b] = b == e ? K[b] : (open_div(N * d.m[b], R) + 1u) >> 1;
}

// The cell after a step or a skip; true: the ray is open there - the cell is outside the box, or k^2 is past the cut-off (md2 != 0).
O2V_OPEN_FN bool open_after(const OpenGrid &g, const int32_t c0[3], const OpenDir &d, const uint32_t k[3], uint32_t md2, int32_t c[3])
{
#pragma unroll
    for (int b = 0; b < 3; ++b) c[b] = c0[b] + d.s[b] * (int32_t) k[b];
    if ((uint32_t) c[0] >= (uint32_t) g.dim[0] || (uint32_t) c[1] >= (uint32_t) g.dim[1] || (uint32_t) c[2] >= (uint32_t) g.dim[2]) return true;
    // (inside the box k_a < 2^16: a square fits 32 bits, the sum of three does not)
    return md2 != 0u && (uint64_t) (k[0] * k[0]) + (uint64_t) (k[1] * k[1]) + (uint64_t) (k[2] * k[2]) > (uint64_t) md2;
}

// true: the ray from the centre of c0 (inside the box) along d is open.  The start cell is never tested.
template <bool Skip>
O2V_OPEN_FN bool open_walk(const OpenGrid &g, const int32_t c0[3], const OpenDir &d, uint32_t md2)
{
    uint32_t k[3] = {0u, 0u, 0u};
    int32_t c[3] = {c0[0], c0[1], c0[2]};
    bool first = true;
    const bool near = md2 != 0u && md2 <= kOpenNear2;   // (uniform over the wavefront)
    for (;;) {
        // c is inside the box.  L: the empty block around it has 2^L voxels along an axis; 0: its brick is not empty
        uint32_t L = 0;
        const int32_t bx = c[0] >> 2, by = c[1] >> 2, bz = c[2] >> 2;
        const uint64_t brick = ((uint64_t) bz * g.b0[1] + (uint32_t) by) * g.b0[0] + (uint32_t) bx;
        unsigned long long w0 = 0;
        if (Skip && near) {
            // bottom up: a ray with a short cut-off stays near the surface, where most bricks hold something - one load, as in the
            // fine walk - and a zero word of a level says that the whole block of the next is empty
            w0 = g.m0[brick];
            if (w0 == 0ull) {
                L = 2;
                if (g.m1[((uint64_t) (c[2] >> 4) * g.b1[1] + (uint32_t) (c[1] >> 4)) * g.b1[0] + (uint32_t) (c[0] >> 4)] == 0ull) {
                    L = 4;
                    if (g.m2[((uint64_t) (c[2] >> 6) * g.b2[1] + (uint32_t) (c[1] >> 6)) * g.b2[0] + (uint32_t) (c[0] >> 6)] == 0ull) L = 6;
                }
            }
        } else if (Skip) {
            const unsigned long long w2 = g.m2[((uint64_t) (c[2] >> 6) * g.b2[1] + (uint32_t) (c[1] >> 6)) * g.b2[0] + (uint32_t) (c[0] >> 6)];
            if (w2 == 0ull) L = 6;
            else if (!((w2 >> open_bit(c[0] >> 4, c[1] >> 4, c[2] >> 4)) & 1ull)) L = 4;
            else {
                const unsigned long long w1 = g.m1[((uint64_t) (c[2] >> 4) * g.b1[1] + (uint32_t) (c[1] >> 4)) * g.b1[0] + (uint32_t) (c[0] >> 4)];
                if (!((w1 >> open_bit(c[0] >> 2, c[1] >> 2, c[2] >> 2)) & 1ull)) L = 2;
            }
        }
        if (L != 0u) {
            open_skip(d, c, L, k);
            if (open_after(g, c0, d, k, md2, c)) return true;
            first = false;
            continue;
        }
        // the fine walk on the brick's word
        if (!(Skip && near)) w0 = g.m0[brick];
        if (!first && ((w0 >> open_bit(c[0], c[1], c[2])) & 1ull)) return false;
        for (;;) {
            open_step(d, k);
            if (open_after(g, c0, d, k, md2, c)) return true;
            if ((c[0] >> 2) != bx || (c[1] >> 2) != by || (c[2] >> 2) != bz) break;
            if ((w0 >> open_bit(c[0], c[1], c[2])) & 1ull) return false;
        }
        first = false;
    }
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------

// The grids a call reads besides the set and writes: the target grid (GRID), dst and mask with their element strides (x, y, z).
struct OpenIo {
    const uint8_t *tgrid;
    uint64_t t0, t1, t2;
    uint8_t *dst;
    uint64_t d0, d1, d2;
    long long *mask;
    uint64_t k0, k1, k2;
};

// The solid bits of the four voxels 4 bx ... 4 bx + 3 of row (y, z): a nibble of the brick's word; 0 outside the box.
__device__ __forceinline__ uint32_t open_row(const OpenGrid &g, int32_t bx, int32_t y, int32_t z)
{
    if ((uint32_t) bx >= g.b0[0] || (uint32_t) y >= (uint32_t) g.dim[1] || (uint32_t) z >= (uint32_t) g.dim[2]) return 0u;
    const unsigned long long w = g.m0[((uint64_t) (z >> 2) * g.b0[1] + (uint32_t) (y >> 2)) * g.b0[0] + (uint32_t) bx];
    return (uint32_t) (w >> (4u * ((uint32_t) y & 3u) + 16u * ((uint32_t) z & 3u))) & 15u;
}

template <uint32_t Mode, bool Write>
__global__ __launch_bounds__(kBlock) void k_open_targets(OpenGrid g, OpenIo io, uint32_t *__restrict__ list, uint64_t cap, unsigned long long *__restrict__ counter)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nx = (uint32_t) g.dim[0], ny = (uint32_t) g.dim[1];
    const uint64_t rows = (uint64_t) g.b0[0] * ny * (uint32_t) g.dim[2];
    const uint64_t stride = (uint64_t) gridDim.x * kBlock;
    // (the bound is the wavefront's: every lane takes part in the scan)
    for (uint64_t base = (uint64_t) blockIdx.x * kBlock + (threadIdx.x & ~63u); base < rows; base += stride) {
        const uint64_t i = base + lane;
        uint32_t T = 0, n = 0, x0 = 0, y = 0, z = 0;
        if (i < rows) {
            // (the rows are no more than the voxels, below 2^31: 32-bit divisions)
            const uint32_t row = (uint32_t) i / g.b0[0];
            const int32_t bx = (int32_t) ((uint32_t) i - row * g.b0[0]);
            z = row / ny, y = row - z * ny;
            x0 = 4u * (uint32_t) bx, n = min(4u, nx - x0);
            const uint32_t in_box = (1u << n) - 1u;
            const uint32_t S = open_row(g, bx, (int32_t) y, (int32_t) z);
            if (Mode == kOpenSolid) T = S;
            else if (Mode == kOpenEmpty) T = ~S & in_box;
            else if (Mode == kOpenGrid) {
                const uint8_t *p = io.tgrid + (uint64_t) y * io.t1 + (uint64_t) z * io.t2;
                for (uint32_t j = 0; j < n; ++j) T |= (uint32_t) (p[(uint64_t) (x0 + j) * io.t0] != 0) << j;
            } else if (S != 0u) {
                const uint32_t left = open_row(g, bx - 1, (int32_t) y, (int32_t) z) >> 3, right = open_row(g, bx + 1, (int32_t) y, (int32_t) z) & 1u;
                uint32_t inner = ((S << 1) | left) & ((S >> 1) | (right << 3));
                inner &= open_row(g, bx, (int32_t) y - 1, (int32_t) z) & open_row(g, bx, (int32_t) y + 1, (int32_t) z);
                inner &= open_row(g, bx, (int32_t) y, (int32_t) z - 1) & open_row(g, bx, (int32_t) y, (int32_t) z + 1);
                T = S & ~inner;
            }
        }
        const uint32_t cnt = (uint32_t) __popc(T);
        uint32_t inc = cnt;
#pragma unroll
        for (uint32_t off = 1u; off < 64u; off <<= 1) {
            const uint32_t o = __shfl_up(inc, off, 64);
            if (lane >= off) inc += o;
        }
        const uint32_t total = __shfl(inc, 63, 64);
        if (!Write) {
            if (lane == 0u && total != 0u) atomicAdd(counter, (unsigned long long) total);
            continue;
        }
        unsigned long long first = 0;
        if (lane == 0u && total != 0u) first = atomicAdd(counter, (unsigned long long) total);
        first = __shfl(first, 0, 64);
        uint64_t at = first + inc - cnt;
        for (uint32_t j = 0; j < n; ++j)
            if ((T >> j) & 1u) {
                if (at < cap) list[at] = x0 + j + nx * (y + ny * z);   // (below 2^31; the bound holds unless the grid changed under the call)
                ++at;
            }
        // 255 and mask 0 where no target is.  A whole row of four at unit stride goes out as one word (two 16-byte stores for the
        // mask): the wavefront then writes 256 contiguous bytes; the targets' places in it are written again by the walk, behind
        // this kernel on the stream.
        uint8_t *const drow = io.dst + (uint64_t) y * io.d1 + (uint64_t) z * io.d2;
        if (n == 4u && io.d0 == 1u && ((uintptr_t) (drow + x0) & 3u) == 0u) {
            uint32_t w = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) w |= ((T >> j) & 1u) ? 0u : 255u << (8u * j);
            *reinterpret_cast<uint32_t *>(drow + x0) = w;
        } else {
            for (uint32_t j = 0; j < n; ++j)
                if (!((T >> j) & 1u)) drow[(uint64_t) (x0 + j) * io.d0] = 255u;
        }
        if (io.mask) {
            long long *const mrow = io.mask + (uint64_t) y * io.k1 + (uint64_t) z * io.k2;
            if (n == 4u && io.k0 == 1u && ((uintptr_t) (mrow + x0) & 15u) == 0u) {
                reinterpret_cast<longlong2 *>(mrow + x0)[0] = make_longlong2(0ll, 0ll);
                reinterpret_cast<longlong2 *>(mrow + x0)[1] = make_longlong2(0ll, 0ll);
            } else {
                for (uint32_t j = 0; j < n; ++j)
                    if (!((T >> j) & 1u)) mrow[(uint64_t) (x0 + j) * io.k0] = 0ll;
            }
        }
    }
}

template <bool Skip, bool Mask>
__global__ __launch_bounds__(kBlock) void k_open_walk(OpenGrid g, const uint32_t *__restrict__ dirs, uint32_t n_dirs, uint32_t md2,
                                                      const uint32_t *__restrict__ list, uint32_t n_targets, OpenIo io)
{
    __shared__ uint32_t s_dir[kOpenMaxDirs * kOpenDirWords];
    for (uint32_t i = threadIdx.x; i < n_dirs * kOpenDirWords; i += kBlock) s_dir[i] = dirs[i];
    __syncthreads();
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_targets) return;
    const uint32_t nx = (uint32_t) g.dim[0], ny = (uint32_t) g.dim[1];
    const uint32_t idx = list[t], row = idx / nx, z = row / ny;
    if (z >= (uint32_t) g.dim[2]) return;   // (never, unless the grid changed under the call: no walk starts outside the box)
    const int32_t c0[3] = {(int32_t) (idx - row * nx), (int32_t) (row - z * ny), (int32_t) z};
    uint32_t count = 0;
    unsigned long long bits = 0;
    for (uint32_t i = 0; i < n_dirs; ++i) {
        const uint32_t *w = s_dir + i * kOpenDirWords;
        const OpenDir d{{(int32_t) w[0], (int32_t) w[1], (int32_t) w[2]}, {w[3], w[4], w[5]}, {w[6], w[7], w[8]}};
        if (open_walk<Skip>(g, c0, d, md2)) {
            ++count;
            if (Mask) bits |= 1ull << (i & 63u);
        }
    }
    io.dst[(uint64_t) c0[0] * io.d0 + (uint64_t) c0[1] * io.d1 + (uint64_t) c0[2] * io.d2] = (uint8_t) count;
    if (Mask) io.mask[(uint64_t) c0[0] * io.k0 + (uint64_t) c0[1] * io.k1 + (uint64_t) c0[2] * io.k2] = (long long) bits;
}
