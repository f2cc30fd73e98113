// o2v_dev_k9_mesh_distance.hpp -- K9: narrow-band distance from voxel centres to the triangles (o2v_hip_mesh_distance_dense).
// Included from o2v_device.hip inside its anonymous namespace; compiled with -ffp-contract=off (o2v_math.h): d2 is evaluated
// op by op in double exactly as include/o2v_hip.h writes it, so a numpy restatement reproduces every bit.
//
// The box is cut into tiles of kMdTile^3 voxels.  Binning (counting sort of (triangle, tile) pairs):
//   k_meshdist_bin_count     per triangle: its sample-space vertices -> the context array sv[t][9]; the tiles that its AABB,
//                            dilated by band ss + ss, reaches (a superset of the voxels md_in_reach admits); one atomicAdd per
//                            (triangle, tile) on the tile's counter
//   k_meshdist_tile_sums / k_fill_scan_blocks / k_meshdist_tile_offsets
//                            the counters' exclusive prefix sum -> first[tile], first[n_tiles] = the pairs in all
//   k_meshdist_bin_scatter   per triangle again: its id into each of its tiles' lists (the counter counts down to 0); the order
//                            inside a list is whatever the atomics give: min and the smallest-index tie rule do not depend on it
// Distance:
//   k_meshdist_tiles         one 256-lane workgroup per tile, lane -> (x, y) of the tile and two voxels z, z + 4.  The tile's
//                            triangles are staged through LDS kMdChunk at a time with their double vertices, normal and dilated
//                            AABB; each lane keeps its two voxels' best d2 and index in registers, then applies band, sign (one
//                            bit of K6's parity bitmap of the box) and closest, and writes with x fastest.  A tile without
//                            triangles writes +-band and -1 (its list loop is empty).
// Crowded tiles (a fan of many triangles meeting in one tile) are left to one workgroup: its cost is pairs / 256 lanes, about
// 10 ms for 20 000 triangles in one tile, and every other tile runs beside it.

constexpr uint32_t kMdTile = 8;     // voxels per tile edge
constexpr uint32_t kMdChunk = 128;  // triangles staged in LDS at a time

struct MdBox {
    uint32_t x0, y0, z0;      // origin (output voxels)
    uint32_t nx, ny, nz;      // extent
    uint32_t tx, ty, tz;      // tiles per axis
    uint32_t ss;
    double margin;            // band ss + ss (sample units): the AABB dilation
    double bs2;               // band^2 ss^2
    float band;
    uint64_t n_tiles;
};

// the voxel index range [lo, hi] of the box whose centres can lie within [a, b] (sample space; conservative by one voxel
// either side); false if it misses the box
__device__ __forceinline__ bool md_range(double a, double b, uint32_t o, uint32_t n, uint32_t ss, uint32_t &lo, uint32_t &hi)
{
    const double h = 0.5 * ss;
    const double l = floor((a - h) / ss) - 1.0, u = floor((b - h) / ss) + 1.0;
    if (!(u >= (double) o) || !(l <= (double) (o + n - 1u))) return false;
    lo = (uint32_t) fmax(l, (double) o);
    hi = (uint32_t) fmin(u, (double) (o + n - 1u));
    return true;
}

// the triangle's sample-space vertices (K6's affine_apply) and, if they are finite, its tile range in the box
__device__ __forceinline__ bool md_tri_tiles(const float *__restrict__ sv, uint64_t tri, const MdBox &b, uint32_t lo[3], uint32_t hi[3])
{
    const float *q = sv + tri * 9;
    for (int k = 0; k < 9; ++k)
        if (!isfinite(q[k])) return false;
    const uint32_t o[3] = {b.x0, b.y0, b.z0}, n[3] = {b.nx, b.ny, b.nz};
    for (int a = 0; a < 3; ++a) {
        const float mn = fminf(q[a], fminf(q[3 + a], q[6 + a])), mx = fmaxf(q[a], fmaxf(q[3 + a], q[6 + a]));
        uint32_t l, h;
        if (!md_range((double) mn - b.margin, (double) mx + b.margin, o[a], n[a], b.ss, l, h)) return false;
        lo[a] = (l - o[a]) / kMdTile;
        hi[a] = (h - o[a]) / kMdTile;
    }
    return true;
}

__global__ __launch_bounds__(kBlock) void k_meshdist_bin_count(const float *__restrict__ verts, uint64_t n_tris, Affine xf, MdBox b,
                                                               float *__restrict__ sv, uint32_t *__restrict__ counts)
{
    const uint64_t tri = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (tri >= n_tris) return;
    const float *q = verts + tri * 9;
    float *o = sv + tri * 9;
    for (int v = 0; v < 3; ++v) {
        const V3 p = affine_apply(xf, V3{q[v * 3], q[v * 3 + 1], q[v * 3 + 2]});
        o[v * 3] = p.x;
        o[v * 3 + 1] = p.y;
        o[v * 3 + 2] = p.z;
    }
    uint32_t lo[3], hi[3];
    if (!md_tri_tiles(sv, tri, b, lo, hi)) return;
    for (uint32_t z = lo[2]; z <= hi[2]; ++z)
        for (uint32_t y = lo[1]; y <= hi[1]; ++y)
            for (uint32_t x = lo[0]; x <= hi[0]; ++x) atomicAdd(&counts[((uint64_t) z * b.ty + y) * b.tx + x], 1u);
}

// per block of kBlock tiles: the sum of their counters
__global__ __launch_bounds__(kBlock) void k_meshdist_tile_sums(const uint32_t *__restrict__ counts, uint64_t n_tiles,
                                                               unsigned long long *__restrict__ block_sums)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    const uint64_t t = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    uint64_t total;
    (void) fill_block_exscan64(t < n_tiles ? counts[t] : 0u, s_wave, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// first[t]: the pairs of the tiles before t (block_offsets: k_fill_scan_blocks of the sums); first[n_tiles]: all of them
__global__ __launch_bounds__(kBlock) void k_meshdist_tile_offsets(const uint32_t *__restrict__ counts, uint64_t n_tiles,
                                                                  const unsigned long long *__restrict__ block_offsets,
                                                                  const unsigned long long *__restrict__ n_pairs,
                                                                  unsigned long long *__restrict__ first)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    const uint64_t t = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    uint64_t total;
    const uint64_t ex = fill_block_exscan64(t < n_tiles ? counts[t] : 0u, s_wave, total);
    if (t < n_tiles) first[t] = block_offsets[blockIdx.x] + ex;
    if (t == n_tiles) first[t] = *n_pairs;
}

__global__ __launch_bounds__(kBlock) void k_meshdist_bin_scatter(const float *__restrict__ sv, uint64_t n_tris, MdBox b,
                                                                 const unsigned long long *__restrict__ first,
                                                                 uint32_t *__restrict__ counts, uint32_t *__restrict__ lists)
{
    const uint64_t tri = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
    if (tri >= n_tris) return;
    uint32_t lo[3], hi[3];
    if (!md_tri_tiles(sv, tri, b, lo, hi)) return;
    for (uint32_t z = lo[2]; z <= hi[2]; ++z)
        for (uint32_t y = lo[1]; y <= hi[1]; ++y)
            for (uint32_t x = lo[0]; x <= hi[0]; ++x) {
                const uint64_t t = ((uint64_t) z * b.ty + y) * b.tx + x;
                lists[first[t] + (atomicSub(&counts[t], 1u) - 1u)] = (uint32_t) tri;
            }
}

// ---- d2 of one (centre, triangle) pair, as include/o2v_hip.h defines it -------------------------------------------------

struct MdTri {
    double a[3], b[3], c[3];  // vertices
    double n[3], nn;          // cross(B - A, C - A) and its squared norm
    double lo[3], hi[3];      // the AABB dilated by band ss + ss
};

__device__ __forceinline__ double md_dot(double ax, double ay, double az, double bx, double by, double bz)
{
    return (ax * bx + ay * by) + az * bz;
}

// n . cross(V - U, P - U)
__device__ __forceinline__ double md_side(const double n[3], const double u[3], const double v[3], double px, double py, double pz)
{
    const double ex = v[0] - u[0], ey = v[1] - u[1], ez = v[2] - u[2];
    const double wx = px - u[0], wy = py - u[1], wz = pz - u[2];
    return md_dot(n[0], n[1], n[2], ey * wz - ez * wy, ez * wx - ex * wz, ex * wy - ey * wx);
}

__device__ __forceinline__ double md_seg(const double u[3], const double v[3], double px, double py, double pz)
{
    const double ex = v[0] - u[0], ey = v[1] - u[1], ez = v[2] - u[2];
    const double wx = px - u[0], wy = py - u[1], wz = pz - u[2];
    const double ee = md_dot(ex, ey, ez, ex, ey, ez);
    double t = 0.0;
    if (ee != 0.0) {
        t = md_dot(wx, wy, wz, ex, ey, ez) / ee;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
    const double qx = wx - t * ex, qy = wy - t * ey, qz = wz - t * ez;
    return md_dot(qx, qy, qz, qx, qy, qz);
}

__device__ __forceinline__ double md_d2(const MdTri &t, double px, double py, double pz)
{
    if (t.nn > 0.0) {
        const double s0 = md_side(t.n, t.a, t.b, px, py, pz), s1 = md_side(t.n, t.b, t.c, px, py, pz), s2 = md_side(t.n, t.c, t.a, px, py, pz);
        if (s0 >= 0.0 && s1 >= 0.0 && s2 >= 0.0) {
            const double h = md_dot(t.n[0], t.n[1], t.n[2], px - t.a[0], py - t.a[1], pz - t.a[2]);
            return (h * h) / t.nn;
        }
    }
    return fmin(fmin(md_seg(t.a, t.b, px, py, pz), md_seg(t.b, t.c, px, py, pz)), md_seg(t.c, t.a, px, py, pz));
}

__device__ __forceinline__ void md_take(double d2, uint32_t id, double &best, uint32_t &best_id)
{
    if (d2 < best || (d2 == best && id < best_id)) {
        best = d2;
        best_id = id;
    }
}

// bits: K6's parity bitmap of the box ([z-word][y][x], FillBox layout), or null (unsigned)
__global__ __launch_bounds__(kBlock) void k_meshdist_tiles(const float *__restrict__ sv, MdBox b, const unsigned long long *__restrict__ first,
                                                           const uint32_t *__restrict__ lists, const uint32_t *__restrict__ bits,
                                                           float *__restrict__ dst, uint64_t ds0, uint64_t ds1, uint64_t ds2,
                                                           int32_t *__restrict__ closest, uint64_t cs0, uint64_t cs1, uint64_t cs2)
{
    __shared__ MdTri s_tri[kMdChunk];
    __shared__ uint32_t s_id[kMdChunk];
    const uint32_t lx = threadIdx.x & 7u, ly = (threadIdx.x >> 3) & 7u, lz = threadIdx.x >> 6;
    const double h = 0.5 * b.ss;
    const uint64_t n_cols = (uint64_t) b.nx * b.ny;
    for (uint64_t tile = blockIdx.x; tile < b.n_tiles; tile += gridDim.x) {
        const uint64_t txy = (uint64_t) b.tx * b.ty;
        const uint32_t tz = (uint32_t) (tile / txy), rem = (uint32_t) (tile - (uint64_t) tz * txy);
        const uint32_t ty = rem / b.tx, tx = rem - ty * b.tx;
        const uint32_t x = tx * kMdTile + lx, y = ty * kMdTile + ly, z0 = tz * kMdTile + lz, z1 = z0 + 4u;  // (box coordinates)
        const double px = (double) (b.x0 + x) * b.ss + h, py = (double) (b.y0 + y) * b.ss + h;
        const double pz0 = (double) (b.z0 + z0) * b.ss + h, pz1 = (double) (b.z0 + z1) * b.ss + h;
        double best0 = __builtin_inf(), best1 = __builtin_inf();
        uint32_t id0 = 0xffffffffu, id1 = 0xffffffffu;
        const uint64_t begin = first[tile], end = first[tile + 1];
        for (uint64_t c = begin; c < end; c += kMdChunk) {
            const uint32_t n = (uint32_t) min<uint64_t>(kMdChunk, end - c);
            __syncthreads();   // (the previous chunk has been read)
            if (threadIdx.x < n) {
                const uint32_t id = lists[c + threadIdx.x];
                const float *q = sv + (uint64_t) id * 9;
                MdTri t;
                for (int k = 0; k < 3; ++k) {
                    t.a[k] = q[k];
                    t.b[k] = q[3 + k];
                    t.c[k] = q[6 + k];
                }
                const double abx = t.b[0] - t.a[0], aby = t.b[1] - t.a[1], abz = t.b[2] - t.a[2];
                const double acx = t.c[0] - t.a[0], acy = t.c[1] - t.a[1], acz = t.c[2] - t.a[2];
                t.n[0] = aby * acz - abz * acy;
                t.n[1] = abz * acx - abx * acz;
                t.n[2] = abx * acy - aby * acx;
                t.nn = md_dot(t.n[0], t.n[1], t.n[2], t.n[0], t.n[1], t.n[2]);
                for (int k = 0; k < 3; ++k) {
                    t.lo[k] = (double) fminf(q[k], fminf(q[3 + k], q[6 + k])) - b.margin;
                    t.hi[k] = (double) fmaxf(q[k], fmaxf(q[3 + k], q[6 + k])) + b.margin;
                }
                s_tri[threadIdx.x] = t;
                s_id[threadIdx.x] = id;
            }
            __syncthreads();
            for (uint32_t k = 0; k < n; ++k) {
                const MdTri &t = s_tri[k];
                if (px < t.lo[0] || px > t.hi[0] || py < t.lo[1] || py > t.hi[1]) continue;
                const uint32_t id = s_id[k];
                if (pz0 >= t.lo[2] && pz0 <= t.hi[2]) md_take(md_d2(t, px, py, pz0), id, best0, id0);
                if (pz1 >= t.lo[2] && pz1 <= t.hi[2]) md_take(md_d2(t, px, py, pz1), id, best1, id1);
            }
        }
        if (x >= b.nx || y >= b.ny) continue;
        const uint32_t zs[2] = {z0, z1};
        const double bests[2] = {best0, best1};
        const uint32_t ids[2] = {id0, id1};
        for (int v = 0; v < 2; ++v) {
            const uint32_t z = zs[v];
            if (z >= b.nz) continue;
            const bool in = bests[v] < b.bs2;
            float u = in ? (float) (sqrt(bests[v]) / (double) b.ss) : b.band;
            if (bits && ((bits[(uint64_t) (z >> 5) * n_cols + (uint64_t) y * b.nx + x] >> (z & 31u)) & 1u)) u = -u;
            dst[x * ds0 + y * ds1 + z * ds2] = u;
            if (closest) closest[x * cs0 + y * cs1 + z * cs2] = in ? (int32_t) ids[v] : -1;
        }
    }
}
