// o2v_dev_k6_fill.hpp -- K6: solid fill (O2V_HIP_FLAG_FILL_INTERIOR), the stage behind a pass' final surface records.
// Included from o2v_device.hip inside its anonymous namespace; compiled with -ffp-contract=off (o2v_math.h).
//
// The parity set (include/o2v_hip.h): the column of output voxel (i, j) is the vertical line through
// P = (i ss + ss/2, j ss + ss/2) in sample space.  A triangle covers it if the exact signs of its three 2-D edge functions
// (symbolic perturbation P + (eps, eps^2) for exact zeros) are all +1 or all -1; it then toggles every voxel k >= k0 of the
// column, k0 the first layer whose centre lies above the crossing height z (barycentric, in double, op by op).  A voxel is
// interior when it is toggled an odd number of times and is not a surface voxel.
//
// The stage, on a toggle bitmap of the pass box (one bit per cell, 32-bit words along z, laid out [z-word][y][x]):
//   k_fill_count / k_fill_scan_blocks / k_fill_offsets   columns of each triangle's projected box within the pass box, and
//                                                         their inclusive prefix sum: a flat (triangle, column) enumeration;
//                                                         k_fill_count also reduces the mesh's top (largest finite z)
//   k_fill_cross      one lane per (triangle, column): exact column test, crossing height, atomicXor of one bit at k0
//   k_fill_prefix     one lane per column: prefix XOR along z (in-word by shifts, a carry across words), cut at the mesh's
//                     top layer
//   k_fill_unmark     the pass' surface records cleared from the bitmap (atomicAnd)
//   k_fill_count_words / k_fill_emit   popcounts, wave prefix sums and one atomic per wave for the base; then 16-byte records,
//                     written by all 64 lanes of a wave side by side

// Bitmap words per wave in the count and emit kernels: 32 steps of one word per lane.  One atomic per chunk for its base: with
// 64-word chunks the 500 k atomics on one address of the bench mesh took 3.7 ms, with 2048-word chunks the kernel reads at
// streaming rate.
constexpr uint32_t kFillSteps = 32;
constexpr uint32_t kFillChunk = 64 * kFillSteps;

// The pass box in output space and what the fill needs of the call.
struct FillBox {
    uint32_t x0, y0, z0;   // origin (output voxels)
    uint32_t nx, ny, nz;   // extent
    uint32_t nzw;          // 32-bit words per column: ceil(nz / 32)
    uint32_t ss;           // supersampling
    uint32_t argb;         // colour of the interior records
    uint64_t n_cols;       // nx * ny
    uint64_t n_words;      // nzw * n_cols
};

// ---- exact sign of the 2-D edge function --------------------------------------------------------------------------

__device__ __forceinline__ void fill_two_sum(double a, double b, double &s, double &e)
{
    s = a + b;
    const double bv = s - a, av = s - bv;
    e = (a - av) + (b - bv);
}
__device__ __forceinline__ void fill_two_prod(double a, double b, double &p, double &e)
{
    p = a * b;
    e = fma(a, b, -p);  // explicit fma: exact error of the product (no underflow: every factor is 0 or above 2^-150)
}

// Sign of the exact value of (vx - ux)(py - uy) - (vy - uy)(px - ux) for float32 u, v and half-integer p (all exact in double).
// A floating-point filter first (the error bound of Shewchuk's orient2d, ccwerrboundA = (3 + 16 eps) eps), then, for the rare
// values near zero, the exact value as a non-overlapping expansion of the 16 error-free partial products.
__device__ __noinline__ int fill_exact_sign(double ux, double uy, double vx, double vy, double px, double py)
{
    double a[2], b[2], c[2], d[2];
    fill_two_sum(vx, -ux, a[1], a[0]);
    fill_two_sum(py, -uy, b[1], b[0]);
    fill_two_sum(vy, -uy, c[1], c[0]);
    fill_two_sum(px, -ux, d[1], d[0]);
    double e[16];
    int n = 0;
    auto grow = [&](double x) {  // grow_expansion with zero elimination (Shewchuk 1997)
        double q = x;
        int m = 0;
        for (int i = 0; i < n; ++i) {
            double s, h;
            fill_two_sum(q, e[i], s, h);
            q = s;
            if (h != 0.0) e[m++] = h;
        }
        if (q != 0.0) e[m++] = q;
        n = m;
    };
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            double pp, pe;
            fill_two_prod(a[i], b[j], pp, pe);
            grow(pp);
            grow(pe);
            fill_two_prod(c[i], d[j], pp, pe);
            grow(-pp);
            grow(-pe);
        }
    return n == 0 ? 0 : (e[n - 1] > 0.0 ? 1 : -1);  // (the largest component carries the sign)
}

__device__ __forceinline__ int fill_sign(double ux, double uy, double vx, double vy, double px, double py)
{
    const double l = (vx - ux) * (py - uy), r = (vy - uy) * (px - ux), det = l - r;
    const double bound = 3.3306690738754716e-16 * (fabs(l) + fabs(r));  // (3 + 16 * 2^-53) * 2^-53
    if (det > bound) return 1;
    if (-det > bound) return -1;
    return fill_exact_sign(ux, uy, vx, vy, px, py);
}

// The column test's sign of edge u -> v: exact sign, an exact zero resolved by the perturbation P + (eps, eps^2), 0 for an
// edge whose projected endpoints coincide.
__device__ __forceinline__ int fill_edge(V3 u, V3 v, double px, double py)
{
    if (u.x == v.x && u.y == v.y) return 0;
    const int s = fill_sign(u.x, u.y, v.x, v.y, px, py);
    if (s) return s;
    return v.y != u.y ? (v.y > u.y ? -1 : 1) : (v.x > u.x ? 1 : -1);
}

// e(U, V, P) in double, as written (the barycentric weights of the crossing height)
__device__ __forceinline__ double fill_e(V3 u, V3 v, double px, double py)
{
    return ((double) v.x - (double) u.x) * (py - (double) u.y) - ((double) v.y - (double) u.y) * (px - (double) u.x);
}

// ---- per triangle: its vertices in sample space and the columns of the box its projected box meets --------------------

struct FillTri {
    V3 v0, v1, v2;
    uint32_t i0, j0;  // first column (output x, y)
    uint32_t wi;      // columns per row of the triangle's range
    uint64_t count;   // columns in all (0: the triangle contributes nothing to this box)
};

// the first index i in [lo, hi) whose column centre i ss + ss/2 is >= x (> x if `strict`); hi if there is none
__device__ __forceinline__ uint32_t fill_first_col(float x, uint32_t lo, uint32_t hi, uint32_t ss, bool strict)
{
    const double h = 0.5 * ss, xd = x;
    auto after = [&](uint32_t i) { return strict ? (double) i * ss + h > xd : (double) i * ss + h >= xd; };
    uint32_t i = (uint32_t) fmin(fmax(floor((xd - h) / ss), (double) lo), (double) hi);  // (a guess, then exact steps)
    while (i > lo && after(i - 1u)) --i;
    while (i < hi && !after(i)) ++i;
    return i;
}

__device__ __forceinline__ FillTri fill_tri(const float *__restrict__ verts, uint64_t tri, const Affine &xf, const FillBox &b)
{
    FillTri t;
    const float *q = verts + tri * 9;
    t.v0 = affine_apply(xf, V3{q[0], q[1], q[2]});
    t.v1 = affine_apply(xf, V3{q[3], q[4], q[5]});
    t.v2 = affine_apply(xf, V3{q[6], q[7], q[8]});
    t.i0 = t.j0 = t.wi = 0;
    t.count = 0;
    const float c[9] = {t.v0.x, t.v0.y, t.v0.z, t.v1.x, t.v1.y, t.v1.z, t.v2.x, t.v2.y, t.v2.z};
    for (int k = 0; k < 9; ++k)
        if (!isfinite(c[k])) return t;  // (a non-finite coordinate: the triangle contributes nothing)
    // a triangle whose z range starts at or above the box's top cannot toggle a layer of it
    const float zmin = fminf(t.v0.z, fminf(t.v1.z, t.v2.z));
    if ((double) zmin >= (double) (b.z0 + b.nz) * b.ss) return t;
    const float xmin = fminf(t.v0.x, fminf(t.v1.x, t.v2.x)), xmax = fmaxf(t.v0.x, fmaxf(t.v1.x, t.v2.x));
    const float ymin = fminf(t.v0.y, fminf(t.v1.y, t.v2.y)), ymax = fmaxf(t.v0.y, fmaxf(t.v1.y, t.v2.y));
    // the columns whose centre lies in [min, max] (closed: a column through the box's edge may be covered), within the box
    const uint32_t i_lo = fill_first_col(xmin, b.x0, b.x0 + b.nx, b.ss, false), i_end = fill_first_col(xmax, b.x0, b.x0 + b.nx, b.ss, true);
    const uint32_t j_lo = fill_first_col(ymin, b.y0, b.y0 + b.ny, b.ss, false), j_end = fill_first_col(ymax, b.y0, b.y0 + b.ny, b.ss, true);
    if (i_end <= i_lo || j_end <= j_lo) return t;
    t.i0 = i_lo;
    t.j0 = j_lo;
    t.wi = i_end - i_lo;
    t.count = (uint64_t) t.wi * (j_end - j_lo);
    return t;
}

// ---- 64-bit scans ------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint64_t fill_wave_scan64(uint64_t v)
{
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// exclusive scan of one uint64 per thread over a kBlock-thread block; `total` receives the block's sum
__device__ __forceinline__ uint64_t fill_block_exscan64(uint64_t v, uint64_t *s_wave /*[kBlock / 64]*/, uint64_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t inc = fill_wave_scan64(v);
    __syncthreads();
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint64_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64; ++w) {
        if (w < wave) base += s_wave[w];
        tot += s_wave[w];
    }
    total = tot;
    return base + inc - v;
}

// ---- kernels ------------------------------------------------------------------------------------------------------

// columns per triangle -> cols[tri]; per block of kBlock triangles their sum -> block_sums[block].  Also the largest sample-space
// z of every triangle with finite coordinates, before any cull by the box -> *zmax_enc (f2ord, zero-initialised: the mesh's top,
// which bounds the parity set from above, k_fill_prefix)
__global__ __launch_bounds__(kBlock) void k_fill_count(const float *__restrict__ verts, uint64_t n_tris, Affine xf, FillBox b,
                                                       unsigned long long *__restrict__ cols, unsigned long long *__restrict__ block_sums,
                                                       unsigned long long *__restrict__ zmax_enc)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    __shared__ float s_zmax[kBlock / 64];
    const uint64_t tri = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    uint64_t n = 0;
    float ztop = -__builtin_inff();
    if (tri < n_tris) {
        const FillTri t = fill_tri(verts, tri, xf, b);
        n = t.count;
        const float c[9] = {t.v0.x, t.v0.y, t.v0.z, t.v1.x, t.v1.y, t.v1.z, t.v2.x, t.v2.y, t.v2.z};
        bool finite = true;
        for (int k = 0; k < 9; ++k) finite = finite && isfinite(c[k]);
        if (finite) ztop = fmaxf(t.v0.z, fmaxf(t.v1.z, t.v2.z));
        cols[tri] = n;
    }
    uint64_t total;
    (void) fill_block_exscan64(n, s_wave, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
    for (int d = 32; d >= 1; d >>= 1) ztop = fmaxf(ztop, __shfl_xor(ztop, d, 64));
    if ((threadIdx.x & 63u) == 0) s_zmax[threadIdx.x >> 6] = ztop;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kBlock / 64; ++w) ztop = fmaxf(ztop, s_zmax[w]);
        const unsigned long long e = f2ord(ztop);
        if (ztop > -__builtin_inff() && e > *zmax_enc) atomicMax(zmax_enc, e);  // (a plain read first: few atomics contend)
    }
}

// exclusive scan of the block sums in place (one workgroup); the grand total -> *total
__global__ __launch_bounds__(kBlock) void k_fill_scan_blocks(unsigned long long *__restrict__ block_sums, uint64_t n_blocks,
                                                             unsigned long long *__restrict__ total)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_blocks; base += kBlock) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < n_blocks ? block_sums[i] : 0u;
        uint64_t sum;
        const uint64_t ex = fill_block_exscan64(v, s_wave, sum);
        if (i < n_blocks) block_sums[i] = carry + ex;
        carry += sum;
    }
    if (threadIdx.x == 0) *total = carry;
}

// cols[tri] -> the inclusive end of the triangle's items in the flat enumeration
__global__ __launch_bounds__(kBlock) void k_fill_offsets(unsigned long long *__restrict__ cols, uint64_t n_tris,
                                                         const unsigned long long *__restrict__ block_offsets)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    const uint64_t tri = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    const uint64_t n = tri < n_tris ? cols[tri] : 0u;
    uint64_t total;
    const uint64_t ex = fill_block_exscan64(n, s_wave, total);
    if (tri < n_tris) cols[tri] = block_offsets[blockIdx.x] + ex + n;
}

// One lane per (triangle, column) item: the column test, the crossing height and one toggled bit at the first layer above it.
__global__ __launch_bounds__(kBlock) void k_fill_cross(const float *__restrict__ verts, uint64_t n_tris, Affine xf, FillBox b,
                                                       const unsigned long long *__restrict__ ends,
                                                       const unsigned long long *__restrict__ n_items, uint32_t *__restrict__ bits)
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
        const FillTri t = fill_tri(verts, tri, xf, b);
        const uint32_t i = t.i0 + (uint32_t) (local % t.wi), j = t.j0 + (uint32_t) (local / t.wi);
        const double px = (double) i * b.ss + h, py = (double) j * b.ss + h;
        const int s0 = fill_edge(t.v0, t.v1, px, py);
        if (s0 == 0 || fill_edge(t.v1, t.v2, px, py) != s0 || fill_edge(t.v2, t.v0, px, py) != s0) continue;
        const double w0 = fill_e(t.v1, t.v2, px, py), w1 = fill_e(t.v2, t.v0, px, py), w2 = fill_e(t.v0, t.v1, px, py);
        const double den = (w0 + w1) + w2;
        double z = ((w0 * (double) t.v0.z + w1 * (double) t.v1.z) + w2 * (double) t.v2.z) / den;
        if (den == 0.0 || !isfinite(z)) z = fmin(fmin((double) t.v0.z, (double) t.v1.z), (double) t.v2.z);
        // k0: the first k >= 0 with k ss + ss/2 > z; a crossing below the box's first layer toggles from that layer up
        const uint32_t zlast = b.z0 + b.nz - 1u;
        if (z >= (double) zlast * b.ss + h) continue;  // (k0 beyond the box)
        uint32_t k = b.z0;
        if (z >= (double) b.z0 * b.ss + h) {
            k = (uint32_t) fmin(fmax(floor((z - h) / b.ss) + 1.0, (double) b.z0), (double) zlast);
            while (k > b.z0 && (double) (k - 1u) * b.ss + h > z) --k;
            while ((double) k * b.ss + h <= z) ++k;  // (ends at zlast at the latest: zlast ss + ss/2 > z)
        }
        const uint32_t kz = k - b.z0;
        atomicXor(&bits[(uint64_t) (kz >> 5) * b.n_cols + (uint64_t) (j - b.y0) * b.nx + (i - b.x0)], 1u << (kz & 31u));
    }
}

// One lane per column: every toggle bit becomes the parity of the toggles at and below it; the bits above the box and above
// the mesh's top layer floor(zmax / ss) cleared (the set does not depend on how far the box reaches above the mesh).
__global__ __launch_bounds__(kBlock) void k_fill_prefix(uint32_t *__restrict__ bits, FillBox b, const unsigned long long *__restrict__ zmax_enc)
{
    const uint64_t col = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (col >= b.n_cols) return;
    // layers of the box at or below the top layer (0 if no triangle is finite or the mesh lies below the box)
    const float zmax = ord2f((uint32_t) *zmax_enc);   // (*zmax_enc == 0, no finite triangle: NaN)
    const double top = floor((double) zmax / b.ss);
    const uint32_t n_valid = !(zmax >= 0.f) || top < (double) b.z0 ? 0u : (uint32_t) fmin(top - (double) b.z0 + 1.0, (double) b.nz);
    uint32_t carry = 0;
    for (uint32_t zw = 0; zw < b.nzw; ++zw) {
        uint32_t *q = bits + (uint64_t) zw * b.n_cols + col;
        uint32_t w = *q;
        w ^= w << 1;
        w ^= w << 2;
        w ^= w << 4;
        w ^= w << 8;
        w ^= w << 16;
        w ^= carry;
        carry = (uint32_t) ((int32_t) w >> 31);
        const uint32_t valid = n_valid > zw * 32u ? n_valid - zw * 32u : 0u;
        if (valid < 32u) w &= (1u << valid) - 1u;
        *q = w;
    }
}

// the pass' surface records out of the bitmap
__global__ __launch_bounds__(kBlock) void k_fill_unmark(const uint4 *__restrict__ out, uint64_t n_surf, FillBox b, uint32_t *__restrict__ bits)
{
    for (uint64_t r = (uint64_t) blockIdx.x * kBlock + threadIdx.x; r < n_surf; r += (uint64_t) gridDim.x * kBlock) {
        const uint4 v = out[r];
        const uint32_t x = v.x - b.x0, y = v.y - b.y0, z = v.z - b.z0;  // (wraps above the box for a coordinate below it)
        if (x >= b.nx || y >= b.ny || z >= b.nz) continue;
        atomicAnd(&bits[(uint64_t) (z >> 5) * b.n_cols + (uint64_t) y * b.nx + x], ~(1u << (z & 31u)));
    }
}

// Per chunk of kFillChunk words (one wave, one word per lane): its records' base, by one atomic per wave; *n_interior the sum.
__global__ __launch_bounds__(kBlock) void k_fill_count_words(const uint32_t *__restrict__ bits, FillBox b,
                                                             unsigned long long *__restrict__ chunk_base,
                                                             unsigned long long *__restrict__ n_interior)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = (b.n_words + kFillChunk - 1) / kFillChunk;
    const uint64_t waves = (uint64_t) gridDim.x * (kBlock / 64u);
    for (uint64_t c = (uint64_t) blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6); c < n_chunks; c += waves) {
        uint32_t n = 0;
#pragma unroll 8
        for (uint32_t k = 0; k < kFillSteps; ++k) {
            const uint64_t wi = c * kFillChunk + k * 64u + lane;
            n += wi < b.n_words ? (uint32_t) __popc(bits[wi]) : 0u;
        }
        const uint32_t inc = wave_inclusive_scan(n);
        const uint32_t sum = __shfl(inc, 63, 64);
        unsigned long long base = 0;
        if (lane == 0 && sum) base = atomicAdd(n_interior, (unsigned long long) sum);
        if (lane == 0) chunk_base[c] = base;
    }
}

// Per chunk: the records of its set bits at first + chunk_base[c], in the order of its words; the wave's 64 lanes write 64
// consecutive records a step.
__global__ __launch_bounds__(kBlock) void k_fill_emit(const uint32_t *__restrict__ bits, FillBox b,
                                                      const unsigned long long *__restrict__ chunk_base, uint64_t first,
                                                      uint4 *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = (b.n_words + kFillChunk - 1) / kFillChunk;
    const uint64_t waves = (uint64_t) gridDim.x * (kBlock / 64u);
    for (uint64_t c = (uint64_t) blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6); c < n_chunks; c += waves) {
        uint64_t base = first + chunk_base[c];
        for (uint32_t k = 0; k < kFillSteps; ++k) {
            const uint64_t wi = c * kFillChunk + k * 64u + lane;
            const uint32_t word = wi < b.n_words ? bits[wi] : 0u;
            const uint32_t inc = wave_inclusive_scan((uint32_t) __popc(word));
            const uint32_t sum = __shfl(inc, 63, 64);
            if (!sum) continue;
            // this lane's word's place in the box (one 64-bit division per word, not per record)
            const uint64_t zw = wi / b.n_cols, rem = wi - zw * b.n_cols;
            const uint32_t y = (uint32_t) (rem / b.nx), x = (uint32_t) (rem - (uint64_t) y * b.nx);
            const uint32_t ox = b.x0 + x, oy = b.y0 + y, oz = b.z0 + (uint32_t) zw * 32u;
            for (uint32_t t = 0; t < sum; t += 64u) {
                const uint32_t r = t + lane;
                // the word holding record r: the first lane whose inclusive count is above r
                uint32_t src = 0;
#pragma unroll
                for (uint32_t step = 32; step; step >>= 1)
                    if ((uint32_t) __shfl(inc, (int) (src + step - 1u), 64) <= r) src += step;
                const uint32_t m0 = (uint32_t) __shfl(word, (int) src, 64);
                const uint32_t before = (uint32_t) __shfl(inc, (int) src, 64) - (uint32_t) __popc(m0);
                const uint32_t rx = (uint32_t) __shfl(ox, (int) src, 64), ry = (uint32_t) __shfl(oy, (int) src, 64);
                const uint32_t rz = (uint32_t) __shfl(oz, (int) src, 64);
                if (r >= sum) continue;
                // the (r - before)-th set bit of the word
                uint32_t rank = r - before, m = m0, pos = 0;
#pragma unroll
                for (uint32_t s = 16; s; s >>= 1) {
                    const uint32_t low = (uint32_t) __popc(m & ((1u << s) - 1u));
                    if (rank >= low) {
                        rank -= low;
                        m >>= s;
                        pos += s;
                    }
                }
                uint4 *dst = out + base + r;
                __builtin_nontemporal_store(rx, &dst->x);
                __builtin_nontemporal_store(ry, &dst->y);
                __builtin_nontemporal_store(rz + pos, &dst->z);
                __builtin_nontemporal_store(b.argb, &dst->w);
            }
            base += sum;
        }
    }
}
