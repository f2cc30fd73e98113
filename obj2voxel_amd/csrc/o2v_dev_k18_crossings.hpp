// o2v_dev_k18_crossings.hpp -- K18: signed crossing numbers along x, y and z (o2v_hip_crossings_dense).
// Included from o2v_device.hip inside its anonymous namespace, after K17; compiled with -ffp-contract=off (o2v_math.h).
//
// The definition (include/o2v_hip.h): for a ray axis a the vertices are read as (u, v, w) - (x, y, z) for
// z, (y, z, x) for x, (z, x, y) for y -, K6's column test on (u, v) at a line's centre keeps the common sign sigma of the three
// edge functions, and K6's crossing height with w in place of z gives k0, the first layer whose centre lies above the crossing.
// For the voxel at k the crossing lies below it if k0 <= k, else above; D = -sum of sigma below, U = +sum of sigma above, and the
// voxel's value is the sum of D + U over the axes asked for.
//
// Per axis, on an int32 delta grid of the box laid out [w][line] and one int32 total per line:
//   k_cross_count<A> / k_fill_scan_blocks / k_fill_offsets   lines of each triangle's projected box within the box (K6's cull, on
//                                                             u and v only: a triangle above or below the box along w counts)
//                                                             and their inclusive prefix sum (K6's own scan kernels)
//   k_cross_mark<A>   one lane per (triangle, line): K6's column test (fill_edge), which keeps sigma, K6's height (fill_e), one
//                     atomicAdd of -sigma into the delta grid at k0 clamped to the box's first layer - none for a crossing above the
//                     box's last centre - and one into the line's total T
//   k_cross_prefix    one lane per line, walking w: the running sum of the deltas is D, U = D - T, the voxel gets 2 D - T: stored
//                     for the first axis, added for the later ones, through the caller's strides
//   k_cross_prefix_tile   the same where the ray runs along dst's unit stride: 64 lines x 32 layers staged through LDS per wave
// The lines of an axis are indexed with x running first where x is one of the line's coordinates (z rays: (x, y), y rays: (x, z)),
// so that a wave reads 256 consecutive bytes of the delta grid and, for a tensor of unit x stride, writes 256 consecutive bytes;
// the x rays' lines run along y first, and their rows of dst are written from the LDS tile.

// ---- plain C++: a crossing's place on its line and a voxel's value ---------------------------------------------------------
// (tests/test_host_crossings.py compiles this part for the host, with O2V_CR_FN of its own, and runs it against the reference.)
#ifndef O2V_CR_HOST
#define O2V_CR_FN __host__ __device__ __forceinline__
#endif

// The layer of a box of nw layers from w0 (output voxels, supersampling ss) that a crossing at the height hgt (sample space,
// finite) is first below: k0 - w0 for k0 the first k with k ss + ss/2 > hgt, 0 for a crossing below the box's first centre
// (it lies below every voxel of the line), nw for one at or above the box's last centre (above every voxel).
O2V_CR_FN uint32_t cr_layer(double hgt, uint32_t w0, uint32_t nw, uint32_t ss)
{
    const double h = 0.5 * ss;
    const uint32_t last = w0 + nw - 1u;
    if (hgt >= (double) last * ss + h) return nw;
    if (!(hgt >= (double) w0 * ss + h)) return 0u;
    uint32_t k = (uint32_t) fmin(fmax(floor((hgt - h) / ss) + 1.0, (double) w0), (double) last);  // (a guess, then exact steps)
    while (k > w0 && (double) (k - 1u) * ss + h > hgt) --k;
    while ((double) k * ss + h <= hgt) ++k;  // (ends at `last` at the latest: last ss + ss/2 > hgt)
    return k - w0;
}

// What a crossing of sign sigma adds: `delta` to the delta grid at `layer` (nothing if layer == nw) and `total` to its line's T.
struct CrAdd {
    uint32_t layer;
    int32_t delta, total;
};
O2V_CR_FN CrAdd cr_add(double hgt, int sigma, uint32_t w0, uint32_t nw, uint32_t ss)
{
    CrAdd a;
    a.layer = cr_layer(hgt, w0, nw, ss);
    a.delta = a.layer < nw ? -sigma : 0;
#ifdef O2V_CR_MUTATE_DROP_ABOVE
    a.total = a.delta;   // (test only: a crossing above the box is lost from T)
#else
    a.total = -sigma;
#endif
    return a;
}

// D + U of a voxel whose line has the total T and the running sum D up to its layer: U = D - T.
O2V_CR_FN int32_t cr_value(int32_t d, int32_t total) { return 2 * d - total; }

// ---- kernels -----------------------------------------------------------------------------------------------------------------
#ifndef O2V_CR_HOST

// The box as one axis' rays see it.
struct CrBox {
    uint32_t u0, v0, w0;   // origin along the line coordinates u, v and along the ray (output voxels)
    uint32_t nu, nv, nw;   // extent
    uint32_t ss;           // supersampling
    uint32_t v_first;      // the line index runs along v first: (i - u0) nv + (j - v0); else (j - v0) nu + (i - u0)
    uint64_t n_lines;      // nu * nv
};

// a sample-space vertex read as (u, v, w) of ray axis A (0 x, 1 y, 2 z)
template <int A>
__device__ __forceinline__ V3 cr_perm(V3 p)
{
    if (A == 0) return V3{p.y, p.z, p.x};
    if (A == 1) return V3{p.z, p.x, p.y};
    return p;
}

// K6's fill_tri for ray axis A: the vertices as (u, v, w) in x, y, z, and the lines of the box its projected box meets.  No cull
// along w.
template <int A>
__device__ __forceinline__ FillTri cr_tri(const float *__restrict__ verts, uint64_t tri, const Affine &xf, const CrBox &b)
{
    FillTri t;
    const float *q = verts + tri * 9;
    t.v0 = cr_perm<A>(affine_apply(xf, V3{q[0], q[1], q[2]}));
    t.v1 = cr_perm<A>(affine_apply(xf, V3{q[3], q[4], q[5]}));
    t.v2 = cr_perm<A>(affine_apply(xf, V3{q[6], q[7], q[8]}));
    t.i0 = t.j0 = t.wi = 0;
    t.count = 0;
    const float c[9] = {t.v0.x, t.v0.y, t.v0.z, t.v1.x, t.v1.y, t.v1.z, t.v2.x, t.v2.y, t.v2.z};
    for (int k = 0; k < 9; ++k)
        if (!isfinite(c[k])) return t;  // (a non-finite coordinate: the triangle contributes nothing)
    const float umin = fminf(t.v0.x, fminf(t.v1.x, t.v2.x)), umax = fmaxf(t.v0.x, fmaxf(t.v1.x, t.v2.x));
    const float vmin = fminf(t.v0.y, fminf(t.v1.y, t.v2.y)), vmax = fmaxf(t.v0.y, fmaxf(t.v1.y, t.v2.y));
    // the lines whose centre lies in [min, max] (closed, as K6's), within the box
    const uint32_t i_lo = fill_first_col(umin, b.u0, b.u0 + b.nu, b.ss, false), i_end = fill_first_col(umax, b.u0, b.u0 + b.nu, b.ss, true);
    const uint32_t j_lo = fill_first_col(vmin, b.v0, b.v0 + b.nv, b.ss, false), j_end = fill_first_col(vmax, b.v0, b.v0 + b.nv, b.ss, true);
    if (i_end <= i_lo || j_end <= j_lo) return t;
    t.i0 = i_lo;
    t.j0 = j_lo;
    t.wi = i_end - i_lo;
    t.count = (uint64_t) t.wi * (j_end - j_lo);
    return t;
}

// lines per triangle -> lines[tri]; per block of kBlock triangles their sum -> block_sums[block]
template <int A>
__global__ __launch_bounds__(kBlock) void k_cross_count(const float *__restrict__ verts, uint64_t n_tris, Affine xf, CrBox b,
                                                        unsigned long long *__restrict__ lines, unsigned long long *__restrict__ block_sums)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    const uint64_t tri = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    uint64_t n = 0;
    if (tri < n_tris) {
        n = cr_tri<A>(verts, tri, xf, b).count;
        lines[tri] = n;
    }
    uint64_t total;
    (void) fill_block_exscan64(n, s_wave, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// One lane per (triangle, line) item: the column test with its sign, the crossing height, -sigma into the delta grid at the first
// layer above the crossing and into the line's total.
template <int A>
__global__ __launch_bounds__(kBlock) void k_cross_mark(const float *__restrict__ verts, uint64_t n_tris, Affine xf, CrBox b,
                                                       const unsigned long long *__restrict__ ends,
                                                       const unsigned long long *__restrict__ n_items, int32_t *__restrict__ delta,
                                                       int32_t *__restrict__ totals)
{
    const uint64_t total = *n_items;
    const double h = 0.5 * b.ss;
    for (uint64_t w = (uint64_t) blockIdx.x * kBlock + threadIdx.x; w < total; w += (uint64_t) gridDim.x * kBlock) {
        // the triangle: the first whose inclusive end is above w
        uint64_t lo = 0, hi = n_tris - 1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (ends[mid] > w) hi = mid;
            else lo = mid + 1;
        }
        const uint64_t tri = lo;
        const uint64_t local = w - (tri ? ends[tri - 1] : 0u);
        const FillTri t = cr_tri<A>(verts, tri, xf, b);
        const uint32_t i = t.i0 + (uint32_t) (local % t.wi), j = t.j0 + (uint32_t) (local / t.wi);
        const double px = (double) i * b.ss + h, py = (double) j * b.ss + h;
        const int s0 = fill_edge(t.v0, t.v1, px, py);
        if (s0 == 0 || fill_edge(t.v1, t.v2, px, py) != s0 || fill_edge(t.v2, t.v0, px, py) != s0) continue;
        const double w0 = fill_e(t.v1, t.v2, px, py), w1 = fill_e(t.v2, t.v0, px, py), w2 = fill_e(t.v0, t.v1, px, py);
        const double den = (w0 + w1) + w2;
        double z = ((w0 * (double) t.v0.z + w1 * (double) t.v1.z) + w2 * (double) t.v2.z) / den;
        if (den == 0.0 || !isfinite(z)) z = fmin(fmin((double) t.v0.z, (double) t.v1.z), (double) t.v2.z);
        const CrAdd a = cr_add(z, s0, b.w0, b.nw, b.ss);
        const uint64_t line = b.v_first ? (uint64_t) (i - b.u0) * b.nv + (j - b.v0) : (uint64_t) (j - b.v0) * b.nu + (i - b.u0);
        if (a.layer < b.nw) atomicAdd(&delta[(uint64_t) a.layer * b.n_lines + line], a.delta);
        atomicAdd(&totals[line], a.total);
    }
}

// One lane per line: the running sum of the deltas along w is D, the voxel's value 2 D - T.  The voxel at layer k of the line
// (first, slow) is dst[first s_first + slow s_slow + k s_w]: stored, or added to what is there (ADD: the later axes of a call).
template <bool ADD>
__global__ __launch_bounds__(kBlock) void k_cross_prefix(const int32_t *__restrict__ delta, const int32_t *__restrict__ totals, CrBox b,
                                                         int32_t *__restrict__ dst, uint64_t s_first, uint64_t s_slow, uint64_t s_w)
{
    const uint64_t line = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (line >= b.n_lines) return;
    const uint32_t n_first = b.v_first ? b.nv : b.nu;
    const uint64_t slow = line / n_first, first = line - slow * n_first;
    int32_t *q = dst + first * s_first + slow * s_slow;
    const int32_t *p = delta + line;
    const int32_t T = totals[line];
    int32_t d = 0;
#pragma unroll 4
    for (uint32_t k = 0; k < b.nw; ++k) {
        d += p[(uint64_t) k * b.n_lines];
        const int32_t v = cr_value(d, T);
        if (ADD) q[(uint64_t) k * s_w] += v;
        else q[(uint64_t) k * s_w] = v;
    }
}

// k_cross_prefix where the ray runs along dst's unit stride (s_w == 1: the x rays of a tensor stored [z][y][x]), so that the lanes of
// k_cross_prefix would each store 4 bytes into a row of their own.  A wave walks kCrTile layers of its 64 lines into LDS, a lane
// per line, then writes the tile out a row at a time, 32 lanes to 128 consecutive bytes of a line's row.
constexpr uint32_t kCrTile = 32;
template <bool ADD>
__global__ __launch_bounds__(kBlock) void k_cross_prefix_tile(const int32_t *__restrict__ delta, const int32_t *__restrict__ totals, CrBox b,
                                                              int32_t *__restrict__ dst, uint64_t s_first, uint64_t s_slow)
{
    __shared__ int32_t s_tile[kBlock / 64][64][kCrTile + 1];   // (+ 1: a lane per row writes without bank conflicts)
    __shared__ uint64_t s_off[kBlock / 64][64];                // where each line's row begins in dst
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t wave_base = (uint64_t) blockIdx.x * kBlock + wave * 64u, line = wave_base + lane;
    const bool live = line < b.n_lines;
    const uint32_t rows = wave_base < b.n_lines ? (uint32_t) (b.n_lines - wave_base < 64u ? b.n_lines - wave_base : 64u) : 0u;
    int32_t T = 0, d = 0;
    if (live) {
        const uint32_t n_first = b.v_first ? b.nv : b.nu;
        const uint64_t slow = line / n_first, first = line - slow * n_first;
        s_off[wave][lane] = first * s_first + slow * s_slow;
        T = totals[line];
    }
    const uint32_t j = lane & (kCrTile - 1u), half = lane / kCrTile;
    for (uint32_t k0 = 0; k0 < b.nw; k0 += kCrTile) {   // (every thread of the workgroup makes every trip: the barriers)
        const uint32_t n = b.nw - k0 < kCrTile ? b.nw - k0 : kCrTile;
        if (live) {
            const int32_t *p = delta + (uint64_t) k0 * b.n_lines + line;
#pragma unroll 8
            for (uint32_t i = 0; i < n; ++i) {
                d += p[(uint64_t) i * b.n_lines];
                s_tile[wave][lane][i] = cr_value(d, T);
            }
        }
        __syncthreads();
        if (j < n)
            for (uint32_t r = half; r < rows; r += 64u / kCrTile) {
                int32_t *q = dst + s_off[wave][r] + k0 + j;
                const int32_t v = s_tile[wave][r][j];
                if (ADD) *q += v;
                else *q = v;
            }
        __syncthreads();
    }
}

#endif   // O2V_CR_HOST
