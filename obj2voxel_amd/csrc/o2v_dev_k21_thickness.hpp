// o2v_dev_k21_thickness.hpp -- K21: local thickness and ball morphology of a dense grid (o2v_hip_thickness_dense).
// Included from o2v_device.hip inside its anonymous namespace, after K6 (the block scans) and K8 (the seed tests, the row scan
// and the envelope passes); none of the pipeline's kernels use it.
//
// T(p) = max { R(c) : c in S, |p - c|^2 < R(c) } with R(c) = min(depth2(c), cap): the largest (capped) inscribed ball that holds
// the voxel (include/o2v_hip.h).  Exact integers; the same bits on every run.
//   k_thick_depth_x<Format>  dt_scan_row with the per-format seed test negated (plain with BACKGROUND): g^2 to the nearest voxel of
//                            the row that is NOT in S.  K8's k_dist_envelope<kDistY> and <kDistZ> on the depth grid follow: depth2.
//   k_thick_core_x           dt_scan_row on the depth grid with M = {depth2' >= cap} as seeds, g^2 into dst; the seed test
//                            applies the border's min and writes depth2' back.  The two envelope passes on dst give the
//                            squared distance to M: a voxel of S is in the opening where that is below cap.
//   k_thick_init<List>       per voxel: dst = 0 outside S, cap inside the opening, R(p) elsewhere.  List: a voxel of S with
//                            depth2' < cap is a ball centre unless a 26-neighbour's ball covers its own (thick_keep); the kept
//                            centres of a block of kBlock voxels are counted (k_fill_scan_blocks turns the counts into offsets).
//   k_thick_list             the kept centres' linear indices, ascending, into the list: the keep test again, the block's scan, a
//                            store.  No atomics, so the list is the same on every run.
//   k_thick_balls<Count>     a wave per centre, in turns: the cube around the centre row by row, lanes along x (a row of up to 64
//                            voxels per wave-instruction, several short rows side by side), a plain load and an atomicMax where
//                            the stored value is smaller.  max is order-independent, so the bits are fixed.
//   k_thick_convert          in place: int32 T -> float32 2 sqrt(T) - 1, 0 where T is 0.

constexpr uint32_t kThickMaxCap = 1u << 14;   // the largest max_radius2: a ball of 255 voxels across
constexpr uint32_t kThickBackground = 16u, kThickBorder = 32u, kThickF32 = 64u, kThickOpenOnly = 128u;   // O2V_HIP_THICK_*

// The set grid (strides in words for BITS), the depth grid and dst: strides in elements, per axis x, y, z.
struct ThickGrid {
    RaySource src;
    uint32_t invert;        // BACKGROUND: S is the complement
    uint32_t border;        // BORDER: the voxels outside the box are not in S
    uint32_t cap;
    uint64_t e0, e1, e2;    // depth
    uint64_t d0, d1, d2;    // dst
    uint32_t nx, ny, nz;
};

// depth2' of a voxel of depth2 d: the min with the squared distances to the nearest voxel outside the box along the axes
__device__ __forceinline__ uint32_t thick_border(const ThickGrid &g, uint32_t x, uint32_t y, uint32_t z, uint32_t d)
{
    if (!g.border || d == 0u) return d;
    const uint32_t m = min(min(min(x + 1u, g.nx - x), min(y + 1u, g.ny - y)), min(z + 1u, g.nz - z));   // (at most 23 171)
    return min(d, m * m);
}

template <uint32_t Format>
__global__ __launch_bounds__(kBlock) void k_thick_depth_x(int32_t *__restrict__ depth, ThickGrid g)
{
    const bool in_set = g.invert == 0u;   // a voxel is in S where its seed test gives this
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t rows = (uint64_t) g.ny * g.nz;
    for (uint64_t row = dt_first_row(); row < rows; row += dt_row_stride()) {
        const uint64_t y = row % g.ny, z = row / g.ny;
        const uint64_t lrow = y * g.src.s1 + z * g.src.s2;
        int32_t *drow = depth + y * g.e1 + z * g.e2;
        dt_scan_row(g.nx, lane, [&](uint32_t x, bool) { return dt_seed<Format>(g.src, lrow, x) != in_set; }, dt_row_d2, drow, g.e0);
    }
}

// depth -> depth2' in place; dst = g^2 to the nearest voxel of the row with depth2' >= cap.  (The look-ahead reads chunks that
// are written only later, by this wave, and the border's min is idempotent: a voxel tests the same both times.)
__global__ __launch_bounds__(kBlock) void k_thick_core_x(int32_t *__restrict__ depth, int32_t *__restrict__ dst, ThickGrid g)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t rows = (uint64_t) g.ny * g.nz;
    for (uint64_t row = dt_first_row(); row < rows; row += dt_row_stride()) {
        const uint32_t y = (uint32_t) (row % g.ny), z = (uint32_t) (row / g.ny);
        int32_t *erow = depth + (uint64_t) y * g.e1 + (uint64_t) z * g.e2;
        int32_t *drow = dst + (uint64_t) y * g.d1 + (uint64_t) z * g.d2;
        dt_scan_row(
            g.nx, lane,
            [&](uint32_t x, bool ahead) {
                const uint32_t r = thick_border(g, x, y, z, (uint32_t) erow[(uint64_t) x * g.e0]);
                if (!ahead) erow[(uint64_t) x * g.e0] = (int32_t) r;
                return r >= g.cap;
            },
            dt_row_d2, drow, g.d0);
    }
}

// Whether the centre (x, y, z) of radius^2 r (1 <= r < cap) keeps its ball: no neighbour c + v in the box has
// R(c + v) >= L_k[r], k = |v|^2, the smallest radius^2 at which the neighbour's discrete ball contains this one (table:
// [3][cap + 1], o2v_hip_thickness_cover_table).  L_k[r] > r, so of a chain of covered balls the last is kept or lies in the
// opening.  depth2' of a voxel outside S is 0 and covers nothing; min(depth2', cap) need not be formed: an entry above cap is
// above every R, and one at most cap is reached by depth2' exactly when it is by R.
__device__ __forceinline__ bool thick_keep(const ThickGrid &g, const int32_t *__restrict__ depth, const uint32_t *__restrict__ table, uint32_t x,
                                           uint32_t y, uint32_t z, uint32_t r)
{
    const uint32_t need[3] = {table[r], table[(g.cap + 1u) + r], table[2u * (g.cap + 1u) + r]};
    if (need[0] > g.cap) return true;   // (L_1 <= L_2 <= L_3: no neighbour can cover it)
    for (int dz = -1; dz <= 1; ++dz) {
        const uint32_t zz = z + (uint32_t) dz;   // (wraps below 0: >= nz)
        if (zz >= g.nz) continue;
        for (int dy = -1; dy <= 1; ++dy) {
            const uint32_t yy = y + (uint32_t) dy;
            if (yy >= g.ny) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const uint32_t xx = x + (uint32_t) dx;
                const int k = dx * dx + dy * dy + dz * dz;
                if (xx >= g.nx || k == 0) continue;
                const uint32_t rn = (uint32_t) depth[(uint64_t) xx * g.e0 + (uint64_t) yy * g.e1 + (uint64_t) zz * g.e2];
                if (min(rn, g.cap) >= need[k - 1]) return false;
            }
        }
    }
    return true;
}

// dst (the squared distance to M) -> 0 outside S, cap in the opening, R(p) elsewhere.  List: block_sums[b] = the kept centres of
// block b of kBlock voxels in linear order, ctr[0] += the candidates (the voxels of S with depth2' < cap).
template <bool List>
__global__ __launch_bounds__(kBlock) void k_thick_init(ThickGrid g, const int32_t *__restrict__ depth, int32_t *__restrict__ dst,
                                                       const uint32_t *__restrict__ table, uint64_t voxels, uint64_t n_blocks,
                                                       unsigned long long *__restrict__ block_sums, unsigned long long *__restrict__ ctr)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint64_t i = b * kBlock + threadIdx.x;
        bool cand = false, keep = false;
        if (i < voxels) {
            const uint64_t row = i / g.nx;
            const uint32_t x = (uint32_t) (i - row * g.nx), y = (uint32_t) (row % g.ny), z = (uint32_t) (row / g.ny);
            const uint32_t r = (uint32_t) depth[(uint64_t) x * g.e0 + (uint64_t) y * g.e1 + (uint64_t) z * g.e2];
            int32_t *const p = dst + (uint64_t) x * g.d0 + (uint64_t) y * g.d1 + (uint64_t) z * g.d2;
            const uint32_t dm = (uint32_t) *p;
            *p = r == 0u ? 0 : dm < g.cap ? (int32_t) g.cap : (int32_t) r;   // (r >= cap: the voxel is in M, dm = 0)
            cand = r != 0u && r < g.cap;
            if (List && cand) keep = thick_keep(g, depth, table, x, y, z, r);
        }
        if (List) {
            const unsigned long long mc = __ballot(cand);
            if ((threadIdx.x & 63u) == 0u && mc) atomicAdd(ctr, (unsigned long long) __popcll(mc));
            uint64_t total;
            (void) fill_block_exscan64(keep ? 1u : 0u, s_wave, total);
            if (threadIdx.x == 0) block_sums[b] = total;
        }
    }
}

// list[boff[b] + (the kept centres of block b before i)] = i for every kept centre i
__global__ __launch_bounds__(kBlock) void k_thick_list(ThickGrid g, const int32_t *__restrict__ depth, const uint32_t *__restrict__ table,
                                                       uint64_t voxels, uint64_t n_blocks, const unsigned long long *__restrict__ boff,
                                                       int32_t *__restrict__ list)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        if (boff[b + 1] == boff[b]) continue;   // (uniform over the workgroup)
        const uint64_t i = b * kBlock + threadIdx.x;
        bool keep = false;
        if (i < voxels) {
            const uint64_t row = i / g.nx;
            const uint32_t x = (uint32_t) (i - row * g.nx), y = (uint32_t) (row % g.ny), z = (uint32_t) (row / g.ny);
            const uint32_t r = (uint32_t) depth[(uint64_t) x * g.e0 + (uint64_t) y * g.e1 + (uint64_t) z * g.e2];
            keep = r != 0u && r < g.cap && thick_keep(g, depth, table, x, y, z, r);
        }
        uint64_t total;
        const uint64_t ex = fill_block_exscan64(keep ? 1u : 0u, s_wave, total);
        if (keep) list[boff[b] + ex] = (int32_t) i;
    }
}

// dst = max(dst, R(c)) over the ball {|q - c|^2 < R(c)} of every centre c of the list, clipped to the box (every voxel of it
// is in S: depth2' is the squared distance to the nearest voxel that is not).  A wave per centre.  The cube of side
// 2 rad + 1 around the centre, rad = floor(sqrt(R - 1)), is walked row by row (dy, dz); a wave-instruction covers wx = 64 lanes
// of one row, or 64 / wx rows of wx (a power of two >= the side) lanes side by side, so its accesses are runs along x.
// ctr[2] += the voxels visited (Count: O2V_HIP_FLAG_STAGE_TIMES).
template <bool Count>
__global__ __launch_bounds__(kBlock) void k_thick_balls(ThickGrid g, const int32_t *__restrict__ depth, const int32_t *__restrict__ list, uint64_t n,
                                                        int32_t *__restrict__ dst, unsigned long long *__restrict__ ctr)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t) gridDim.x * (kBlock / 64u);
    uint64_t visited = 0;
    for (uint64_t ci = (uint64_t) blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6); ci < n; ci += waves) {
        const uint32_t c = (uint32_t) list[ci];
        const uint32_t crow = c / g.nx;
        const int32_t cx = (int32_t) (c - crow * g.nx), cy = (int32_t) (crow % g.ny), cz = (int32_t) (crow / g.ny);
        const int32_t R = depth[(uint64_t) cx * g.e0 + (uint64_t) cy * g.e1 + (uint64_t) cz * g.e2];   // (1 <= R < cap <= 2^14)
        if (R < 1) continue;   // (never: the list holds voxels of S)
        int32_t rad = (int32_t) sqrtf((float) (R - 1));
        while (rad * rad > R - 1) --rad;
        while ((rad + 1) * (rad + 1) <= R - 1) ++rad;
        const uint32_t side = 2u * (uint32_t) rad + 1u;   // (at most 255)
        uint32_t wx = 1u;
        while (wx < side && wx < 64u) wx <<= 1;
        const uint32_t per = 64u / wx, sub = lane / wx, xi = lane & (wx - 1u);
        const uint32_t rows = side * side;
        for (uint32_t row0 = 0; row0 < rows; row0 += per) {
            const uint32_t row = row0 + sub;
            const int32_t dz = (int32_t) (row / side) - rad, dy = (int32_t) (row % side) - rad;
            const int32_t rem = R - dy * dy - dz * dz;   // dx^2 must be below it
            const int32_t y = cy + dy, z = cz + dz;
            const bool row_in = row < rows && rem > 0 && y >= 0 && y < (int32_t) g.ny && z >= 0 && z < (int32_t) g.nz;
            for (uint32_t xo = xi; xo < side; xo += 64u) {   // (one turn where the side is at most 64)
                const int32_t dx = (int32_t) xo - rad, x = cx + dx;
                const bool in = row_in && dx * dx < rem && x >= 0 && x < (int32_t) g.nx;
                if (in) {
                    int32_t *const p = dst + (uint64_t) x * g.d0 + (uint64_t) y * g.d1 + (uint64_t) z * g.d2;
                    if (*p < R) atomicMax(p, R);   // (a stale smaller value only costs an atomic: dst only rises)
                }
                if (Count) visited += in ? 1u : 0u;
            }
        }
    }
    if (Count) {
        for (int d = 32; d >= 1; d >>= 1) visited += __shfl_xor(visited, d, 64);
        if (lane == 0u && visited) atomicAdd(ctr + 2, (unsigned long long) visited);
    }
}

// int32 T -> float32 2 sqrt(T) - 1 in place (0 stays 0): the diameter in voxels of the largest inscribed ball
__global__ __launch_bounds__(kBlock) void k_thick_convert(ThickGrid g, int32_t *__restrict__ dst, uint64_t voxels)
{
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < voxels; i += (uint64_t) gridDim.x * kBlock) {
        const uint64_t row = i / g.nx;
        const uint64_t x = i - row * g.nx, y = row % g.ny, z = row / g.ny;
        int32_t *const p = dst + x * g.d0 + y * g.d1 + z * g.d2;
        const int32_t t = *p;
        *p = __float_as_int(t == 0 ? 0.f : (float) (2.0 * sqrt((double) t) - 1.0));
    }
}
