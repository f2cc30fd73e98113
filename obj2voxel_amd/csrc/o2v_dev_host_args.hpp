// Host side of the dense-grid entry points (K7 - K24): what they share.  Refusals, the checks of the caller's memory, scratch,
// the set grid, the limits, run-time values as template arguments, the pair table's grow loop.  Included by o2v_device.hip only, once, like the kernels'
// headers: it needs the context and the launch macros defined there.

namespace {

// The refusal of a call of the entry point fn: "fn: why" becomes the context's error, rc is returned.
int refuse(o2v_hip_ctx *ctx, int rc, const char *fn, const std::string &why)
{
    ctx->err = std::string(fn) + ": " + why;
    return rc;
}

// [p, p + bytes) must be device (or managed) memory of the context's device and lie inside one allocation.  A pointer the
// runtime does not know leaves an error in its per-thread state, which is cleared here so that the next call does not see it.
int check_device_range(o2v_hip_ctx *ctx, const char *fn, const void *p, uint64_t bytes, const char *what)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void) hipGetLastError();
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, std::string(what) + " is not memory the HIP runtime knows");
    }
    if ((a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged && !a.isManaged) || a.device != ctx->device)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn,
                      std::string(what) + " is not device memory of the context's device " + std::to_string(ctx->device));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess) {
        (void) hipGetLastError();
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, std::string(what) + ": the runtime does not know its allocation");
    }
    const uint64_t offset = (uint64_t) ((const char *) p - (const char *) base);
    if (offset > size || bytes > size - offset)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn,
                      std::string(what) + ": " + std::to_string(bytes) + " bytes from its address extend past its allocation");
    return O2V_HIP_OK;
}

// Along the axes of more than one voxel, taken by rising stride, each stride must step past everything the axes before it
// reach, or two voxels of the box share an element (a stride of 0, as of an expanded tensor, fails this).
bool strides_distinct(const uint32_t dims[3], const uint64_t strides[3])
{
    int ax[3] = {0, 1, 2};
    std::sort(ax, ax + 3, [&](int a, int b) { return strides[a] < strides[b]; });
    unsigned __int128 reach = 0;   // the highest element offset the axes so far reach
    for (int a : ax) {
        if (dims[a] == 1) continue;
        if ((unsigned __int128) strides[a] <= reach) return false;
        reach += (unsigned __int128) (dims[a] - 1u) * strides[a];
    }
    return true;
}

// A grid the caller owns, passed to the entry point fn as `what`: dims voxels at these element strides (x, y, z) from p, of
// elem bytes each.  Refused if its reach (in 128 bits: the strides are the caller's) is above 2^63 - 1 bytes, if `distinct`
// and two voxels share an element, or if check_device_range refuses it.  out_bytes: the reach, the bytes past p it touches.
int check_grid(o2v_hip_ctx *ctx, const char *fn, const char *what, const void *p, const uint32_t dims[3], const uint64_t strides[3],
               uint32_t elem, bool distinct, uint64_t *out_bytes = nullptr)
{
    unsigned __int128 last = 0;
    for (int a = 0; a < 3; ++a) last += (unsigned __int128) (dims[a] - 1u) * strides[a];
    const unsigned __int128 bytes = (last + 1u) * elem;
    if (bytes > (unsigned __int128) (~0ull >> 1))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, std::string(what) + ": the box and strides reach past any allocation");
    if (distinct && !strides_distinct(dims, strides))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, std::string(what) + ": strides map two voxels of the box to one element");
    if (out_bytes) *out_bytes = (uint64_t) bytes;
    return check_device_range(ctx, fn, p, (uint64_t) bytes, what);
}

bool ranges_overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes)
{
    const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
    return x < y + b_bytes && y < x + a_bytes;
}

// Room for n elements (at least one) of an array of the entry point fn.  A failed allocation leaves the array empty, the
// runtime's error state clear and the context usable.  (The voxelize pipeline grows its arrays with grow / grow_keep.)
template <typename T, bool P>
int grow_scratch(o2v_hip_ctx *ctx, DevArray<T, P> &a, uint64_t n, const char *fn, const char *what)
{
    n = std::max<uint64_t>(n, 1);
    if (a.ptr && n <= a.cap) return O2V_HIP_OK;
    if (const hipError_t e = a.alloc(n); e != hipSuccess) {
        (void) hipGetLastError();
        return refuse(ctx, e == hipErrorOutOfMemory ? O2V_HIP_ERR_OUT_OF_MEMORY : O2V_HIP_ERR_HIP, fn,
                      std::string(what) + " of " + std::to_string(n * sizeof(T)) + " bytes: " + hipGetErrorString(e));
    }
    return O2V_HIP_OK;
}

uint32_t stream_grid(const o2v_hip_ctx *ctx, uint64_t items, uint32_t per_cu)
{
    return (uint32_t) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) ctx->num_cus * per_cu, (items + kBlock - 1) / kBlock));
}

// A range of device memory that an entry point reads or writes, as refuse_overlap takes it.
struct Span {
    const char *what;
    const void *p;
    uint64_t bytes;
};

// Refuses the first pair of spans that overlap, among the pairs with a written span: the first n_out are written, the others
// only read (and may share memory).  A span with a null pointer or no bytes is not there.
template <size_t N>
int refuse_overlap(o2v_hip_ctx *ctx, const char *fn, const Span (&spans)[N], size_t n_out)
{
    for (size_t i = 0; i < n_out; ++i)
        for (size_t j = i + 1; j < N; ++j) {
            const Span &a = spans[i], &b = spans[j];
            if (a.p && a.bytes && b.p && b.bytes && ranges_overlap(a.p, a.bytes, b.p, b.bytes))
                return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, std::string(a.what) + " and " + b.what + " overlap");
        }
    return O2V_HIP_OK;
}

// The first checks of a grid argument, in this order: null argument, zero dims.
int grid_given(o2v_hip_ctx *ctx, const char *fn, const void *grid, const uint64_t strides[3], const uint32_t dims[3])
{
    if (!grid || !strides || !dims) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if (!dims[0] || !dims[1] || !dims[2]) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "zero dims");
    return O2V_HIP_OK;
}

// The neighbourhoods of K12, K23 and K24.
int connectivity_known(o2v_hip_ctx *ctx, const char *fn, uint32_t connectivity)
{
    if (connectivity == 6u || connectivity == 18u || connectivity == 26u) return O2V_HIP_OK;
    return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "connectivity must be 6, 18 or 26, not " + std::to_string(connectivity));
}

// 16-byte loads from a grid of elem-byte elements: unit x stride and every row 16-byte aligned
bool rows_aligned16(const void *grid, const uint64_t strides[3], uint32_t elem)
{
    return strides[0] == 1u && (uintptr_t) grid % 16u == 0 && strides[1] * elem % 16u == 0 && strides[2] * elem % 16u == 0;
}

RaySource ray_source(const void *grid, const uint64_t strides[3], float level) { return RaySource{grid, strides[0], strides[1], strides[2], level}; }

// Linear index i (x fastest) is element i: a grid that an int32 array of the voxels can stand in for (K12's parents, K20's distances).
bool linear_layout(const uint32_t dims[3], const uint64_t strides[3])
{
    return (dims[0] == 1u || strides[0] == 1u) && (dims[1] == 1u || strides[1] == dims[0]) && (dims[2] == 1u || strides[2] == (uint64_t) dims[0] * dims[1]);
}

// A grid that a call writes, as check_outputs takes it; a null p: the caller did not ask for it.
struct OutGrid {
    const char *what;
    const void *p;
    const uint64_t *strides;
    uint32_t elem;   // bytes per element
};

// The output grids of a call of the entry point fn, each of dims voxels: check_grid on those that are there, in order, no two
// voxels of one sharing an element.  spans[0, N): the outputs with their reach, as refuse_overlap takes the written spans.
template <size_t N>
int check_outputs(o2v_hip_ctx *ctx, const char *fn, const OutGrid (&outs)[N], const uint32_t dims[3], Span *spans)
{
    for (size_t i = 0; i < N; ++i) {
        spans[i] = Span{outs[i].what, outs[i].p, 0};
        if (!outs[i].p) continue;
        if (int rc = check_grid(ctx, fn, outs[i].what, outs[i].p, dims, outs[i].strides, outs[i].elem, true, &spans[i].bytes)) return rc;
    }
    return O2V_HIP_OK;
}

// ---- limits ------------------------------------------------------------------------------------------------------------------

constexpr uint32_t kMaxAxis = 65536;   // voxels along an axis of the grids of K12, K13, K14, K17, K19 and K20 (O2V_HIP_ERR_LIMIT above)

// origin + dims along every axis is at most `limit`, or the call is refused in the caller's words.
int extent_limit(o2v_hip_ctx *ctx, const char *fn, const uint32_t origin[3], const uint32_t dims[3], uint64_t limit, const char *why)
{
    for (int a = 0; a < 3; ++a)
        if ((uint64_t) origin[a] + dims[a] > limit) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, why);
    return O2V_HIP_OK;
}

// No axis above kMaxAxis voxels.  With an origin (K17, K19) each axis' extent is tried right behind its length, as extent_limit does.
int axis_limit(o2v_hip_ctx *ctx, const char *fn, const uint32_t dims[3], const uint32_t *origin = nullptr, uint64_t limit = 0, const char *why = nullptr)
{
    for (int a = 0; a < 3; ++a) {
        if (dims[a] > kMaxAxis) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "a grid of more than 65 536 voxels along an axis");
        if (origin && (uint64_t) origin[a] + dims[a] > limit) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, why);
    }
    return O2V_HIP_OK;
}

constexpr uint64_t kMaxInt32 = 0x7fffffffull;   // a linear index, a label, a place in a list are one int32 (K12, K20)

// The voxels of the grid and the n entries of the list `what` each fit an int32 (behind axis_limit: K12, K20).
int index_limits(o2v_hip_ctx *ctx, const char *fn, const uint32_t dims[3], uint64_t n, const char *what)
{
    if (int rc = axis_limit(ctx, fn, dims)) return rc;
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2];   // (below 2^48)
    if (voxels > kMaxInt32) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, std::to_string(voxels) + " voxels do not fit an int32 index (at most 2^31 - 1)");
    if (n > kMaxInt32) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, std::string("more than 2^31 - 1 ") + what);
    return O2V_HIP_OK;
}

// ---- the set grid: the input of K11 - K15, K17 and K20 -----------------------------------------------------------------------

// Which voxels of a box are solid (include/o2v_hip.h, o2v_hip_raycast_build), as set_grid checked it.
struct SetGrid {
    GridKey key;          // the caller's pointer, format, strides, dims and level
    uint64_t bytes = 0;   // the reach: the bytes from key.p on that the box touches
    uint32_t elem = 1;    // bytes per element: 1 (U8) or 4 (a word of BITS, a float of F32_BELOW)
    bool vec = false;     // 16-byte loads (rows_aligned16)

    RaySource source() const { return ray_source(key.p, key.strides, key.level); }
};

static_assert((int) O2V_HIP_RAY_GRID_U8 == (int) O2V_HIP_GRID_U8 && (int) O2V_HIP_RAY_GRID_BITS == (int) O2V_HIP_GRID_BITS &&
                  (int) O2V_HIP_RAY_GRID_F32_BELOW == (int) O2V_HIP_GRID_F32_BELOW && kRayU8 == O2V_HIP_GRID_U8 && kRayBits == O2V_HIP_GRID_BITS &&
                  kRayF32Below == O2V_HIP_GRID_F32_BELOW,
              "one set of format values for the callers of K11 and of K12 - K15 and for the kernels");

// The checks of a set grid that look at the arguments alone, in this order: null argument, zero dims, unknown format, a BITS
// grid's x stride, a level that is not finite (F32_BELOW).  *g: everything but the reach.
int set_grid_args(o2v_hip_ctx *ctx, const char *fn, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
                  SetGrid *g)
{
    if (int rc = grid_given(ctx, fn, grid, strides, dims)) return rc;
    if (format != O2V_HIP_GRID_U8 && format != O2V_HIP_GRID_BITS && format != O2V_HIP_GRID_F32_BELOW)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown format " + std::to_string(format));
    if (format == O2V_HIP_GRID_BITS && strides[0] != 1u) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "a BITS grid needs strides[0] == 1");
    if (format == O2V_HIP_GRID_F32_BELOW && !std::isfinite(level)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "level must be finite");
    g->key = GridKey(grid, format, strides, dims, level);
    g->elem = format == O2V_HIP_GRID_U8 ? 1u : 4u;
    g->vec = rows_aligned16(grid, strides, g->elem);
    return O2V_HIP_OK;
}

// ... and the one that looks at its memory (check_grid; the context's device is made current for it).  *g: the reach.
int set_grid_memory(o2v_hip_ctx *ctx, const char *fn, SetGrid *g)
{
    O2V_CHECK(hipSetDevice(ctx->device));
    // (the elements the box reaches: 32-bit words along x for BITS)
    const uint32_t *const dims = g->key.dims;
    const uint32_t reach[3] = {g->key.format == O2V_HIP_GRID_BITS ? (dims[0] + 31u) / 32u : dims[0], dims[1], dims[2]};
    return check_grid(ctx, fn, "grid", g->key.p, reach, g->key.strides, g->elem, false, &g->bytes);
}

// The set grid of the entry point fn, checked: set_grid_args, then set_grid_memory.  An entry point's own limits and modes come
// after it (o2v_hip_nearest_dense alone has its size limits between the two).
int set_grid(o2v_hip_ctx *ctx, const char *fn, const void *grid, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], float level,
             SetGrid *g)
{
    if (int rc = set_grid_args(ctx, fn, grid, format, strides, dims, level, g)) return rc;
    return set_grid_memory(ctx, fn, g);
}

// f(format, vec) with the template arguments <Format, Vec> of the kernels that read a set grid, as integral constants.
template <typename F>
void with_set_format(const SetGrid &g, F &&f)
{
    using Bits = std::integral_constant<uint32_t, kRayBits>;
    using U8 = std::integral_constant<uint32_t, kRayU8>;
    using F32Below = std::integral_constant<uint32_t, kRayF32Below>;
    if (g.key.format == O2V_HIP_GRID_BITS) return f(Bits{}, std::false_type{});   // (words: no 16-byte variant)
    if (g.key.format == O2V_HIP_GRID_U8) return g.vec ? f(U8{}, std::true_type{}) : f(U8{}, std::false_type{});
    return g.vec ? f(F32Below{}, std::true_type{}) : f(F32Below{}, std::false_type{});
}

// f(flag) with a run-time bool as std::true_type / std::false_type, for the kernels with a bool template argument.
template <typename F>
void with_flag(bool on, F &&f)
{
    on ? f(std::true_type{}) : f(std::false_type{});
}

// f(mode) with the colour mode of K13 and K14 (checked by ga_mode) as the template argument of their kernels.
template <typename F>
void with_color_mode(uint32_t color_mode, F &&f)
{
    if (color_mode == O2V_HIP_GATHER_COLOR_GRID) return f(std::integral_constant<uint32_t, kGaColorGrid>{});
    if (color_mode == O2V_HIP_GATHER_COLOR_PALETTE) return f(std::integral_constant<uint32_t, kGaColorPalette>{});
    return f(std::integral_constant<uint32_t, kGaColorConstant>{});
}

// The tail of a call whose N stages are all enqueued on the context's stream: the end of the last stage marked, the stream waited
// for, the stages' times read.
template <int N>
int finish_stages(o2v_hip_ctx *ctx, StageTimes<N> &times)
{
    hipStream_t s = ctx->stream;
    O2V_CHECK(times.mark(N, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(times.finish());
    return O2V_HIP_OK;
}

// The pair table of K23 and K24 (o2v_dev_pair_table.hpp), doubled while a probe run overflows.  pass(log2, overflow) gives the
// table 2^log2 slots, clears it, runs the family's pass and reads its counters back: a code that is not 0 ends the call, `overflow`
// asks for the next size.  *log2: the first size, then the one that held every pair; *growths: the doublings.  Above 2^max_log2: refused.
template <typename Pass>
int pt_grow(o2v_hip_ctx *ctx, const char *fn, uint32_t max_log2, uint32_t *log2, uint64_t *growths, Pass &&pass)
{
    for (*growths = 0;; ++*log2, ++*growths) {
        if (*log2 > max_log2) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "the pair table would pass 2^" + std::to_string(max_log2) + " slots");
        bool overflow = false;
        if (int rc = pass(*log2, overflow)) return rc;
        if (!overflow) return O2V_HIP_OK;
    }
}

// The tail of a count of K13 and K14, whose stage marks 0 and 1 the caller has set: the block sums boff[0, n_blocks) scanned in
// place, their total into entry n_blocks and from there to the host, which waits for it.  Stage 2 (the write) has not run.
int count_total(o2v_hip_ctx *ctx, unsigned long long *boff, uint64_t n_blocks, PinnedArray<unsigned long long> &h_ctr, StageTimes<3> &times,
                uint64_t *total)
{
    hipStream_t s = ctx->stream;
    O2V_LAUNCH("k_fill_scan_blocks", s, k_fill_scan_blocks, dim3(1), dim3(kBlock), 0, s, boff, n_blocks, boff + n_blocks);
    O2V_CHECK(hipGetLastError());
    O2V_CHECK(times.mark(2, s));
    O2V_CHECK(hipMemcpyAsync(h_ctr.ptr, boff + n_blocks, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    O2V_CHECK(hipStreamSynchronize(s));
    O2V_CHECK(times.elapsed(0, 1, times.ms[0]));
    O2V_CHECK(times.elapsed(1, 2, times.ms[1]));
    times.ms[2] = 0.f;
    *total = h_ctr.ptr[0];
    return O2V_HIP_OK;
}

}  // namespace
