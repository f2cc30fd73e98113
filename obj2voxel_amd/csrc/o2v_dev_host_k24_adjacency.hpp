// Host side of K24 (o2v_dev_k24_adjacency.hpp): the region adjacency of a label grid.  It takes K19's formats and limits, so it
// comes after o2v_dev_host_k19_label_stats.hpp.

namespace {

constexpr uint32_t kAdjFlagsKnown = O2V_HIP_FLAG_STAGE_TIMES | O2V_HIP_ADJ_ZERO;
constexpr uint32_t kAdjFirstMaxLog2 = 24u;   // the table's first size is 2^24 slots (768 MiB) at most: more only after an overflow

static_assert(kAdjCols == O2V_HIP_ADJ_COLUMNS, "one set of columns for the callers and the kernel");

// The order that sorts m distinct keys ascending: a radix sort of (key, index) by 16-bit digits from the lowest, the digits that
// all keys share left out (labels are small numbers: most of a key's 64 bits are zero).
std::vector<uint64_t> adj_sorted_order(const unsigned long long *keys, uint64_t m)
{
    struct Entry {
        uint64_t key, index;
    };
    std::vector<Entry> a(m), b(m);
    for (uint64_t i = 0; i < m; ++i) a[i] = Entry{keys[i], i};
    std::vector<uint64_t> first(65536u + 1u);
    for (uint32_t shift = 0; shift < 64u; shift += 16u) {
        std::fill(first.begin(), first.end(), 0u);
        for (const Entry &e : a) ++first[((e.key >> shift) & 0xffffu) + 1u];
        if (m && first[((a[0].key >> shift) & 0xffffu) + 1u] == m) continue;   // (one digit for all)
        for (uint32_t d = 0; d < 65536u; ++d) first[d + 1u] += first[d];
        for (const Entry &e : a) b[first[(e.key >> shift) & 0xffffu]++] = e;
        a.swap(b);
    }
    std::vector<uint64_t> order(m);
    for (uint64_t i = 0; i < m; ++i) order[i] = a[i].index;
    return order;
}

}  // namespace

extern "C" {

uint64_t o2v_hip_adjacency_scratch_bytes(uint64_t pairs) { return 48u * std::max<uint64_t>(pairs, 1u) + kAdjCtrs * sizeof(unsigned long long); }

int o2v_hip_adjacency_count(o2v_hip_ctx *ctx, const void *labels, uint32_t format, const uint64_t strides[3], const uint32_t dims[3], uint32_t n_labels,
                            uint32_t connectivity, uint32_t flags, const int32_t *values, const uint64_t value_strides[3], uint64_t *out_pairs,
                            uint64_t *out_outside)
{
    static const char fn[] = "o2v_hip_adjacency_count";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    ctx->adj_counted = false;   // (another count, refused or not, replaces the last one)
    const Switches sw = read_switches();
    if (!out_pairs || !out_outside || (values && !value_strides)) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    int rc;
    if ((rc = grid_given(ctx, fn, labels, strides, dims))) return rc;
    if (format != O2V_HIP_LABELS_I32 && format != O2V_HIP_LABELS_U8)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown format " + std::to_string(format));
    if ((rc = connectivity_known(ctx, fn, connectivity))) return rc;
    if (flags & ~kAdjFlagsKnown) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "unknown flag bits in " + std::to_string(flags));
    if (format == O2V_HIP_LABELS_U8 && n_labels > 255u)
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "n_labels " + std::to_string(n_labels) + " is above 255, the highest value of a U8 grid");
    if ((format == O2V_HIP_LABELS_I32 && (uintptr_t) labels % sizeof(int32_t)) || (uintptr_t) values % sizeof(int32_t))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "an I32 grid and values must be 4-byte aligned");
    if ((rc = index_limits(ctx, fn, dims, 0, "voxels"))) return rc;
    if (n_labels > kLsMaxLabels) return refuse(ctx, O2V_HIP_ERR_LIMIT, fn, "n_labels is above 2^31 - 2");
    // (the limits stand before the look at the memory: a box that is too large is refused as that, whatever it reaches)
    O2V_CHECK(hipSetDevice(ctx->device));
    const uint32_t elem = format == O2V_HIP_LABELS_I32 ? 4u : 1u;
    if ((rc = check_grid(ctx, fn, "labels", labels, dims, strides, elem, false))) return rc;
    if (values && (rc = check_grid(ctx, fn, "values", values, dims, value_strides, 4u, false))) return rc;
    if ((rc = grow_scratch(ctx, ctx->d_adj_ctr, kAdjCtrs, fn, "counters")) || (rc = grow_scratch(ctx, ctx->h_adj_ctr, kAdjCtrs, fn, "counters"))) return rc;

    const uint32_t lane = format == O2V_HIP_LABELS_I32 ? ls_lane<kLsI32>() : ls_lane<kLsU8>();
    const uint64_t voxels = (uint64_t) dims[0] * dims[1] * dims[2];
    AdjGrid g{};
    for (int a = 0; a < 3; ++a) g.n[a] = dims[a];
    g.n_labels = n_labels, g.lo = flags & O2V_HIP_ADJ_ZERO ? 0u : 1u;
    g.cpr = (dims[0] + lane - 1u) / lane;
    g.chunks = (uint32_t) ((uint64_t) g.cpr * dims[1] * dims[2]);   // (at most the voxels)
    g.groups = (g.chunks + kBlock - 1u) / kBlock;
    // a range of groups per workgroup, as K19 cuts them: the fewer workgroups, the fewer tables are added up at the end
    const uint32_t max_blocks = std::max(1u, (uint32_t) ctx->num_cus * 8u);
    g.per_wg = (g.groups + max_blocks - 1u) / max_blocks;
    const dim3 blocks((g.groups + g.per_wg - 1u) / g.per_wg);
    g.table = sw.adj_no_table ? 0u : 1u;
    const bool count_on = (flags & O2V_HIP_FLAG_STAGE_TIMES) != 0;
    g.count = count_on ? 1u : 0u;
    const bool vec = rows_aligned16(labels, strides, elem);
    const RaySource src = ray_source(labels, strides, 0.f);
    const I32View V{values, values ? value_strides[0] : 0u, values ? value_strides[1] : 0u, values ? value_strides[2] : 0u};
    unsigned long long *const ctr = ctx->d_adj_ctr.ptr;
    volatile unsigned long long *const h_ctr = ctx->h_adj_ctr.ptr;
    hipStream_t s = ctx->stream;
    uint64_t growths = 0;
    // the table, doubled while a probe run overflows: 16 slots a label that can occur at first, 2^kAdjFirstMaxLog2 at most
    uint32_t held = pt_first_log2(std::min<uint64_t>((uint64_t) n_labels + 1u, voxels), sw.adj_table_log2, kAdjFirstMaxLog2, kAdjTableMaxLog2);
    rc = pt_grow(ctx, fn, kAdjTableMaxLog2, &held, &growths, [&](uint32_t log2, bool &overflow) -> int {
        const uint64_t slots = 1ull << log2;
        if (int rc = grow_scratch(ctx, ctx->d_adj_keys, slots, fn, "pair table")) return rc;
        if (int rc = grow_scratch(ctx, ctx->d_adj_rows, slots * kAdjCols, fn, "pair table")) return rc;
        g.log2 = log2;
        O2V_CHECK(ctx->adj_times.mark(0, s));
        O2V_CHECK(hipMemsetAsync(ctr, 0, kAdjCtrs * sizeof(unsigned long long), s));
        O2V_LAUNCH("k_adj_init", s, k_adj_init, dim3(stream_grid(ctx, slots * kAdjCols, 8u)), dim3(kBlock), 0, s, ctx->d_adj_keys.ptr, ctx->d_adj_rows.ptr, slots);
        O2V_CHECK(ctx->adj_times.mark(1, s));
        with_flag(format == O2V_HIP_LABELS_I32, [&](auto i32) {
            with_flag(vec, [&](auto v) {
                with_flag(values != nullptr, [&](auto vals) {
                    constexpr uint32_t fmt = decltype(i32)::value ? kLsI32 : kLsU8;
                    constexpr bool vc = decltype(v)::value, vl = decltype(vals)::value;
                    if (connectivity == 6u)
                        O2V_LAUNCH("k_adj_pairs", s, (k_adj_pairs<fmt, 6u, vl, vc>), blocks, dim3(kBlock), 0, s, src, V, g, ctx->d_adj_keys.ptr, ctx->d_adj_rows.ptr, ctr);
                    else if (connectivity == 18u)
                        O2V_LAUNCH("k_adj_pairs", s, (k_adj_pairs<fmt, 18u, vl, vc>), blocks, dim3(kBlock), 0, s, src, V, g, ctx->d_adj_keys.ptr, ctx->d_adj_rows.ptr, ctr);
                    else
                        O2V_LAUNCH("k_adj_pairs", s, (k_adj_pairs<fmt, 26u, vl, vc>), blocks, dim3(kBlock), 0, s, src, V, g, ctx->d_adj_keys.ptr, ctx->d_adj_rows.ptr, ctr);
                });
            });
        });
        O2V_CHECK(hipGetLastError());
        O2V_CHECK(ctx->adj_times.mark(2, s));
        O2V_CHECK(hipMemcpyAsync(ctx->h_adj_ctr.ptr, ctr, kAdjCtrs * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        O2V_CHECK(hipStreamSynchronize(s));
        overflow = h_ctr[0] != 0u;
        return O2V_HIP_OK;
    });
    if (rc) return rc;
    const uint64_t slots = 1ull << held;
    const uint64_t outside = h_ctr[1], to_lds = h_ctr[2], to_global = h_ctr[3], m = h_ctr[5];
    // the list: keys [m], then rows [m][5] - first as the table gives them, then sorted by key, as pairs [m][2] and rows
    if ((rc = grow_scratch(ctx, ctx->d_adj_list, 6u * m, fn, "pair list")) || (rc = grow_scratch(ctx, ctx->h_adj_list, 12u * m, fn, "pair list"))) return rc;
    O2V_LAUNCH("k_pt_list", s, (k_pt_list<long long, kAdjCols>), dim3(stream_grid(ctx, slots, 16u)), dim3(kBlock), 0, s, ctx->d_adj_keys.ptr, ctx->d_adj_rows.ptr, slots, values ? kAdjCols : 3u,
               ctx->d_adj_list.ptr, reinterpret_cast<long long *>(ctx->d_adj_list.ptr + m), ctr + 4);
    O2V_CHECK(hipGetLastError());
    if (m) O2V_CHECK(hipMemcpyAsync(ctx->h_adj_list.ptr, ctx->d_adj_list.ptr, 48u * m, hipMemcpyDeviceToHost, s));
    O2V_CHECK(ctx->adj_times.mark(3, s));
    O2V_CHECK(hipStreamSynchronize(s));
    // the sort, on the host
    if (m) {
        const unsigned long long *const keys = ctx->h_adj_list.ptr, *const rows = keys + m;
        const std::vector<uint64_t> order = adj_sorted_order(keys, m);
        int32_t *const pairs = reinterpret_cast<int32_t *>(ctx->h_adj_list.ptr + 6u * m);
        unsigned long long *const sorted = ctx->h_adj_list.ptr + 7u * m;
        for (uint64_t i = 0; i < m; ++i) {
            const uint64_t e = order[i];
            pairs[2u * i] = (int32_t) (keys[e] >> 32), pairs[2u * i + 1u] = (int32_t) (uint32_t) keys[e];
            std::copy(rows + e * kAdjCols, rows + (e + 1u) * kAdjCols, sorted + i * kAdjCols);
        }
        O2V_CHECK(hipMemcpyAsync(ctx->d_adj_list.ptr, ctx->h_adj_list.ptr + 6u * m, 48u * m, hipMemcpyHostToDevice, s));
    }
    if ((rc = finish_stages(ctx, ctx->adj_times))) return rc;
    const uint64_t counters[4] = {to_lds, to_global, growths, slots * 48u};
    for (int i = 0; i < 4; ++i) ctx->adj_counters[i] = count_on ? counters[i] : 0u;
    ctx->adj_pairs = m, ctx->adj_counted = true;
    *out_pairs = m, *out_outside = outside;
    return O2V_HIP_OK;
}

int o2v_hip_adjacency_write(o2v_hip_ctx *ctx, int32_t *pairs, int64_t *table, uint64_t capacity)
{
    static const char fn[] = "o2v_hip_adjacency_write";
    if (!ctx) return O2V_HIP_ERR_BAD_ARGUMENT;
    if (!ctx->adj_counted) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "no o2v_hip_adjacency_count before it");
    const uint64_t m = ctx->adj_pairs;
    if (capacity < m) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "capacity " + std::to_string(capacity) + " is below the " + std::to_string(m) + " pairs counted");
    if (!m) return O2V_HIP_OK;
    if (!pairs || !table) return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "null argument");
    if ((uintptr_t) pairs % sizeof(int32_t) || (uintptr_t) table % sizeof(int64_t))
        return refuse(ctx, O2V_HIP_ERR_BAD_ARGUMENT, fn, "pairs must be 4-byte aligned and table 8-byte aligned");
    O2V_CHECK(hipSetDevice(ctx->device));
    int rc;
    if ((rc = check_device_range(ctx, fn, pairs, 8u * m, "pairs")) || (rc = check_device_range(ctx, fn, table, 40u * m, "table"))) return rc;
    const Span spans[] = {{"pairs", pairs, 8u * m}, {"table", table, 40u * m}};
    if ((rc = refuse_overlap(ctx, fn, spans, 2))) return rc;
    hipStream_t s = ctx->stream;
    O2V_CHECK(hipMemcpyAsync(pairs, ctx->d_adj_list.ptr, 8u * m, hipMemcpyDeviceToDevice, s));
    O2V_CHECK(hipMemcpyAsync(table, ctx->d_adj_list.ptr + m, 40u * m, hipMemcpyDeviceToDevice, s));
    O2V_CHECK(hipStreamSynchronize(s));
    return O2V_HIP_OK;
}

int o2v_hip_adjacency_times(const o2v_hip_ctx *ctx, float out_ms[4]) { return ctx ? ctx->adj_times.read(out_ms) : O2V_HIP_ERR_BAD_ARGUMENT; }

int o2v_hip_adjacency_counters(const o2v_hip_ctx *ctx, uint64_t out4[4])
{
    if (!ctx || !out4) return O2V_HIP_ERR_BAD_ARGUMENT;
    std::copy(ctx->adj_counters, ctx->adj_counters + 4, out4);
    return O2V_HIP_OK;
}

}  // extern "C"
