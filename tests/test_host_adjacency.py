"""Region adjacency without a GPU: the numpy reference (tests/adjacency_ref.py) against the definition as a
scalar loop, known answers, the plain C++ of o2v_dev_k24_adjacency.hpp compiled for the host behind K19's and the pair table's
(o2v_dev_pair_table.hpp, through tests/pair_table_host.py) and run chunk by chunk
and wavefront by wavefront against the reference (with a tiny slot count, so that the probe limit is met, and one mutation seen to
fail), and obj2voxel_amd.dense's label_adjacency, adjacency_neighbours, coordination and skeleton_graph against a stub of the device
calls that computes with the references; the K24 kernels' metadata in the gfx950 code object."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import adjacency_ref as R
from tests import label_stats_ref as LR
from tests import pair_table_host

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, device_asm, on_cpu  # noqa: E402,F401
from tests.test_host_label_stats import LsStub, _strided  # noqa: E402

K19 = os.path.join(SRC, "o2v_dev_k19_label_stats.hpp")
K24 = os.path.join(SRC, "o2v_dev_k24_adjacency.hpp")


def same(got, want, what):
    assert got[2] == want[2], (what, "outside", got[2], want[2])
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), (what, "pairs", got[0][:8].tolist(), want[0][:8].tolist())
    bad = np.argwhere(got[1] != want[1])
    assert not len(bad), (what, len(bad), "elements differ, the first at", bad[0].tolist(), got[1][tuple(bad[0])], want[1][tuple(bad[0])])


# ---- the reference ----------------------------------------------------------------------------------------------------------------

def test_reference_against_a_scalar_loop():
    rng = np.random.default_rng(24)
    cases = 0
    for dims in ((1, 1, 1), (1, 4, 3), (5, 1, 2), (4, 3, 1), (2, 2, 2), (3, 3, 3), (7, 3, 2), (6, 5, 4)):
        for n in (1, 3, 9):
            for outside in (0.0, 0.2):
                g = LR.blobs(rng, dims, n, outside)
                if cases % 3 == 0:
                    g = rng.integers(-1 if outside else 0, n + 2 if outside else n + 1, g.shape).astype(np.int32)   # no coherence at all
                conn = (6, 18, 26)[cases % 3]
                zero = bool(cases // 3 % 2)
                values = rng.integers(-50, 50, g.shape).astype(np.int32) if cases % 2 else None
                a = R.adjacency(g, n, conn, zero, values)
                b = R.adjacency_loop(g, n, conn, zero, values)
                assert a[0].dtype == np.int32 and a[1].dtype == np.int64
                same(a, b, (dims, n, outside, conn, zero, values is not None))
                assert a[2] == int(((g < 0) | (g > n)).sum())
                if conn < 26:
                    assert not a[1][:, 2].any() and (conn == 18 or not a[1][:, 1].any())
                cases += 1
    assert cases == 48
    # every connectivity, zero on and off and values on and off on one noisy grid; uint8 and bool grids
    g = rng.integers(-1, 6, (4, 5, 6)).astype(np.int32)
    v = rng.integers(-9, 9, g.shape).astype(np.int32)
    for conn in (6, 18, 26):
        for zero in (False, True):
            for values in (None, v):
                same(R.adjacency(g, 4, conn, zero, values), R.adjacency_loop(g, 4, conn, zero, values), (conn, zero))
    u = rng.integers(0, 256, (3, 4, 5)).astype(np.uint8)
    same(R.adjacency(u, 200, 26, True), R.adjacency_loop(u, 200, 26, True), "uint8")
    m = rng.random((4, 4, 4)) < 0.5
    same(R.adjacency(m, 1, 18, True), R.adjacency_loop(m, 1, 18, True), "bool")
    assert len(R.adjacency(m, 1, 18, False)[0]) == 0


# ---- known answers ---------------------------------------------------------------------------------------------------------------

def test_known_answer_two_boxes():
    g = np.ones((3, 4, 12), np.int32)
    g[:, :, 6:] = 2
    pairs, table, outside = R.adjacency(g, 2, 26)
    assert pairs.tolist() == [[1, 2]] and table.tolist() == [[12, 34, 24, 0, 0]] and outside == 0
    assert R.box_pair_row(6, 4, 3) == [12, 34, 24]
    for b, c in ((1, 1), (2, 5), (7, 3)):
        g = np.ones((c, b, 4), np.int32)
        g[:, :, 2:] = 2
        assert R.adjacency(g, 2, 26)[1][0, :3].tolist() == R.box_pair_row(2, b, c)


def test_known_answer_octants():
    z, y, x = np.indices((4, 4, 4))
    g = (1 + (x >= 2) + 2 * (y >= 2) + 4 * (z >= 2)).astype(np.int32)
    rows = {}
    for conn, m in ((26, 28), (18, 24), (6, 12)):
        pairs, table, _ = R.adjacency(g, 8, conn)
        assert len(pairs) == m
        rows[conn] = {tuple(p): t[:3].tolist() for p, t in zip(pairs.tolist(), table)}
    assert rows[26][(1, 2)] == [4, 8, 4] and rows[26][(1, 4)] == [0, 2, 2] and rows[26][(1, 8)] == [0, 0, 1]
    assert rows[18][(1, 2)] == [4, 8, 0] and rows[18][(1, 4)] == [0, 2, 0] and (1, 8) not in rows[18] and rows[6][(1, 2)] == [4, 0, 0]


def test_known_answer_hollow_box_and_distinct_labels():
    H = np.ones((10, 10, 10), bool)
    H[1:-1, 1:-1, 1:-1] = False
    pairs, table, _ = R.adjacency(H, 1, 26, True)
    assert pairs.tolist() == [[0, 1]] and table[0, :3].tolist() == [384, 1440, 1352]
    assert len(R.adjacency(H, 1, 26, False)[0]) == 0
    g = np.arange(1, 28, dtype=np.int32).reshape(3, 3, 3)
    assert [len(R.adjacency(g, 27, c)[0]) for c in (6, 18, 26)] == [54, 126, 158] == list(R.grid_pair_counts(3, 3, 3))
    for dims in ((5, 1, 1), (4, 3, 1), (2, 3, 5)):
        nx, ny, nz = dims
        g = np.arange(1, nx * ny * nz + 1, dtype=np.int32).reshape(nz, ny, nx)
        got = [len(R.adjacency(g, g.size, c)[0]) for c in (6, 18, 26)]
        assert got == list(R.grid_pair_counts(*dims)) and got[0] == (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1)
    assert R.alternating_row(2048, 1024, 1023) == [2144338944, 8568975358, 8560603128]
    z, y, x = np.indices((3, 4, 7))
    assert R.adjacency((x & 1) + 1, 2, 26)[1][0, :3].tolist() == R.alternating_row(7, 4, 3)


# ---- the kernel's own algebra on the host ------------------------------------------------------------------------------------------

HOST_ADJ = r"""
#include <cstdint>
#include <stddef.h>
#include <vector>
#define O2V_LS_HOST
#define O2V_LS_FN static inline
#define O2V_ADJ_HOST
#define O2V_ADJ_FN static inline
%s
// k_adj_pairs' steps for one workgroup that takes the whole grid (contiguous, [z][y][x]), a wavefront of 64 chunks at a time: the
// lanes' chunks, then the chunk's end as the wavefront settles it.  out: the global table's occupied slots, unsorted.
static uint64_t cas64(unsigned long long *p, uint64_t expected, uint64_t desired)
{
    const uint64_t was = *p;
    if (was == expected) *p = desired;
    return was;
}
template <uint32_t Format, uint32_t Conn, typename T>
static int adj_host_t(const T *grid, const int32_t *values, const uint32_t *dims, uint32_t n_labels, uint32_t lo, uint32_t use_table, uint32_t log2,
                      unsigned long long *keys, long long *rows, uint64_t *ctr)
{
    constexpr uint32_t K = ls_lane<Format>();
    const uint32_t nx = dims[0], ny = dims[1], nz = dims[2], cpr = (nx + K - 1u) / K;
    const uint64_t chunks = (uint64_t) cpr * ny * nz, slots = 1ull << log2;
    const bool with_values = values != nullptr;
    std::vector<unsigned long long> s_key(kAdjSlots, kPtEmpty);
    std::vector<long long> s_tab(kAdjSlots * kAdjCols);
    for (uint32_t i = 0; i < kAdjSlots * kAdjCols; ++i) s_tab[i] = adj_init_value(i %% kAdjCols);
    for (uint64_t i = 0; i < slots; ++i) keys[i] = kPtEmpty;
    for (uint64_t i = 0; i < slots * kAdjCols; ++i) rows[i] = adj_init_value((uint32_t) (i %% kAdjCols));
    for (int i = 0; i < 6; ++i) ctr[i] = 0;
    auto at = [&](uint32_t x, uint32_t y, uint32_t z) { return ((size_t) z * ny + y) * nx + x; };
    auto into = [&](long long *row, const AdjPending &p) {
        adj_apply(p, with_values, [&](uint32_t c, uint64_t v) { row[c] += (long long) v; }, [&](uint32_t c, long long v) { if (v > row[c]) row[c] = v; },
                  [&](uint32_t c, long long v) { if (v < row[c]) row[c] = v; });
    };
    auto to_global = [&](const AdjPending &p) {
        bool fresh;
        const uint64_t slot = pt_slot(keys, log2, p.key, cas64, fresh);
        ctr[5] += fresh;
        if (slot == kPtNoPlace) ctr[0] = 1;
        else into(rows + slot * kAdjCols, p);
    };
    auto flush = [&](const AdjPending &p) {
        const uint32_t slot = use_table ? adj_find_slot(s_key.data(), p.key, cas64) : kAdjNoSlot;
        if (slot != kAdjNoSlot) into(s_tab.data() + slot * kAdjCols, p), ++ctr[2];
        else to_global(p), ++ctr[3];
    };
    for (uint64_t base = 0; base < chunks; base += 64u) {
        AdjPending pend[64];
        for (uint32_t l = 0; l < 64u; ++l) {
            adj_pending_clear(pend[l]);
            if (base + l >= chunks) continue;
            const uint32_t ci = (uint32_t) (base + l), row = ci / cpr, x0 = (ci - row * cpr) * K, z = row / ny, y = row - z * ny;
            AdjChunk c;
            c.n = nx - x0 < K ? nx - x0 : K;
            c.has_before = adj_has_before(x0) && at(x0, y, z) > 0, c.has_behind = adj_has_behind(x0, c.n, nx);
            c.have = 1u | (y > 0u ? 2u : 0u) | (y > 0u && z > 0u ? 4u : 0u) | (z > 0u ? 8u : 0u) | (z > 0u && y + 1u < ny ? 16u : 0u);
            for (uint32_t r = 0; r < kAdjRows; ++r) {
                c.row[r] = LsVec{{0u, 0u, 0u, 0u}}, c.before[r] = c.behind[r] = 0;
                if (!adj_row_on(Conn, r) || !((c.have >> r) & 1u)) continue;
                const uint32_t Y = (uint32_t) ((int) y + adj_row_dy(r)), Z = (uint32_t) ((int) z + adj_row_dz(r));
                for (uint32_t i = 0; i < c.n; ++i) {
                    const uint32_t e = (uint32_t) grid[at(x0 + i, Y, Z)];
                    if (Format == kLsI32) c.row[r].w[i] = e;
                    else c.row[r].w[i >> 2] |= (e & 0xffu) << (8u * (i & 3u));
                }
                if (r == 0u || adj_ends_on(Conn, r)) {
                    if (c.has_before) c.before[r] = (int32_t) grid[at(x0, Y, Z) - 1u];     // (linear memory: what a mutation would read)
                    if (c.has_behind && r > 0u) c.behind[r] = (int32_t) grid[at(x0 + c.n, Y, Z)];
                }
            }
            for (uint32_t j = 0; j < c.n; ++j) ctr[1] += adj_outside(ls_value<Format>(c.row[0], j), n_labels);
            uint32_t masks[3u * kAdjRows];
            if (!adj_chunk_masks<Format, Conn>(c, masks)) continue;
            adj_chunk_contacts<Format>(c, masks, [&](uint32_t j, uint32_t r, int dx, int32_t a, int32_t b, uint32_t cls) {
                if (!adj_counted(a, lo, n_labels) || !adj_counted(b, lo, n_labels)) return;
                int32_t va = 0, vb = 0;
                if (with_values) {
                    const int64_t X = (int64_t) x0 + j + dx;   // (a mutation's neighbour may lie before the row)
                    va = values[at(x0 + j, y, z)];
                    vb = X >= 0 ? values[at((uint32_t) X, (uint32_t) ((int) y + adj_row_dy(r)), (uint32_t) ((int) z + adj_row_dz(r)))] : 0;
                }
                adj_merge(pend[l], pt_key((uint32_t) a, (uint32_t) b), cls, with_values, va, vb, flush);
            });
        }
        // the chunk's end: one flush for the wavefront if all its pending pairs are one pair
        uint32_t with = 0, first = 64u;
        bool one = true;
        for (uint32_t l = 0; l < 64u; ++l)
            if (pend[l].key != kPtEmpty) {
                if (first == 64u) first = l;
                one = one && pend[l].key == pend[first].key;
                ++with;
            }
        if (with > 1u && one) {
            AdjPending sum = pend[first];
            for (uint32_t l = first + 1u; l < 64u; ++l) {
                if (pend[l].key == kPtEmpty) continue;
                for (int c = 0; c < 3; ++c) sum.cnt[c] += pend[l].cnt[c];
                sum.hi = pend[l].hi > sum.hi ? pend[l].hi : sum.hi, sum.lo = pend[l].lo < sum.lo ? pend[l].lo : sum.lo;
            }
            flush(sum);
        } else {
            for (uint32_t l = 0; l < 64u; ++l)
                if (pend[l].key != kPtEmpty) flush(pend[l]);
        }
    }
    for (uint32_t slot = 0; slot < kAdjSlots; ++slot) {
        if (s_key[slot] == kPtEmpty) continue;
        bool fresh;
        const uint64_t place = pt_slot(keys, log2, s_key[slot], cas64, fresh);
        ctr[5] += fresh;
        if (place == kPtNoPlace) {
            ctr[0] = 1;
            continue;
        }
        long long *dst = rows + place * kAdjCols;
        const long long *src = s_tab.data() + slot * kAdjCols;
        for (int c = 0; c < 3; ++c) dst[c] += src[c];
        if (with_values) dst[3] = src[3] > dst[3] ? src[3] : dst[3], dst[4] = src[4] < dst[4] ? src[4] : dst[4];
    }
    return 0;
}
extern "C" int adj_host(const void *grid, uint32_t format, const int32_t *values, const uint32_t *dims, uint32_t n_labels, uint32_t lo, uint32_t conn,
                        uint32_t use_table, uint32_t log2, unsigned long long *keys, long long *rows, uint64_t *ctr)
{
#define RUN(F, T, C) adj_host_t<F, C>(static_cast<const T *>(grid), values, dims, n_labels, lo, use_table, log2, keys, rows, ctr)
    if (format == kLsI32) return conn == 6u ? RUN(kLsI32, int32_t, 6u) : conn == 18u ? RUN(kLsI32, int32_t, 18u) : RUN(kLsI32, int32_t, 26u);
    return conn == 6u ? RUN(kLsU8, uint8_t, 6u) : conn == 18u ? RUN(kLsU8, uint8_t, 18u) : RUN(kLsU8, uint8_t, 26u);
}
extern "C" uint32_t adj_slots(void) { return kAdjSlots; }
extern "C" uint32_t adj_class_of(int dx, int dy, int dz) { return adj_class(dx, dy, dz); }
"""


@pytest.fixture(scope="module")
def host_adj(tmp_path_factory):
    """build(defines) -> run(grid, n, conn, zero, values, use_table, log2) -> (pairs, table, outside, counters): the plain C++
    part of o2v_dev_k24_adjacency.hpp (behind K19's and the pair table's), compiled for the host; the table's list is sorted here as the host side does."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    k19, k24 = open(K19).read(), open(K24).read()
    text = (k19[k19.index("constexpr uint32_t kLsI32"):k19.index("#ifndef O2V_LS_HOST")] + k19[k19.index("// ---- runs:"):k19.index("// ---- kernels")] +
            pair_table_host.plain_part() +
            k24[k24.index("constexpr uint32_t kAdjCols"):k24.index("#ifndef O2V_ADJ_HOST")] + k24[k24.index("// ---- contacts:"):k24.index("// ---- kernels")])
    tmp = tmp_path_factory.mktemp("host_adj")

    def build(defines=()):
        name = "adj_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_ADJ % text)
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = C.CDLL(str(tmp / (name + ".so")))
        L.adj_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p] * 3
        L.adj_slots.restype = L.adj_class_of.restype = C.c_uint32

        def run(g, n, conn=26, zero=False, values=None, use_table=1, log2=12):
            g = np.ascontiguousarray(g)
            assert g.dtype in (np.int32, np.uint8)
            nz, ny, nx = g.shape
            v = None if values is None else np.ascontiguousarray(values, np.int32)
            keys = np.zeros(1 << log2, np.uint64)
            rows = np.zeros((1 << log2, R.COLUMNS), np.int64)
            ctr = np.zeros(6, np.uint64)
            L.adj_host(g.ctypes.data, 0 if g.dtype == np.int32 else 1, None if v is None else v.ctypes.data, (C.c_uint32 * 3)(nx, ny, nz), n, 0 if zero else 1,
                       conn, use_table, log2, keys.ctypes.data, rows.ctypes.data, ctr.ctypes.data)
            taken = np.flatnonzero(keys != np.uint64(2 ** 64 - 1))
            order = taken[np.argsort(keys[taken], kind="stable")]
            k = keys[order].astype(np.int64)
            table = rows[order].copy()
            if v is None:
                table[:, 3:] = 0
            pairs = np.stack([k >> 32, k & 0xffffffff], 1).astype(np.int32).reshape(-1, 2)
            counters = dict(overflow=int(ctr[0]), to_lds=int(ctr[2]), to_global=int(ctr[3]), fresh=int(ctr[5]))
            assert counters["overflow"] or counters["fresh"] == len(taken)
            return pairs, table, int(ctr[1]), counters
        run.slots = int(L.adj_slots())
        run.class_of = L.adj_class_of
        return run
    return build


def test_the_class_of_a_contact_on_the_host(host_adj):
    run = host_adj()
    for dx, dy, dz in R.OFFSETS:
        assert run.class_of(dx, dy, dz) == R.offset_class(dx, dy, dz) == run.class_of(-dx, -dy, -dz)
    assert sorted(R.offset_class(*o) for o in R.OFFSETS) == [1] * 3 + [2] * 6 + [3] * 4


def test_every_row_length_on_the_host(host_adj):
    run = host_adj()
    rng = np.random.default_rng(240)
    n_cases = 0
    for nx in list(range(1, 40)) + [63, 64, 65, 255, 256, 257]:
        for n in (2, 7):
            g = LR.blobs(rng, (nx, 3, 2), n, 0.05)
            v = rng.integers(-100, 100, g.shape).astype(np.int32)
            conn = (6, 18, 26)[n_cases % 3]
            zero = bool(n_cases % 2)
            same(run(g, n, conn, zero, v)[:3], R.adjacency(g, n, conn, zero, v), (nx, n, "int32", conn, zero))
            u = np.where((g < 0) | (g > n), n + 1, g).astype(np.uint8)
            for use_table in (1, 0):
                same(run(u, n, 26, not zero, None, use_table)[:3], R.adjacency(u, n, 26, not zero), (nx, n, "uint8", use_table))
            n_cases += 1
    assert n_cases == 90
    # pure noise at every connectivity, dims that include 1, both formats
    for dims in ((1, 1, 1), (1, 5, 4), (9, 1, 3), (17, 4, 1), (5, 3, 3), (33, 2, 2)):
        g = rng.integers(-1, 7, dims[::-1]).astype(np.int32)
        v = rng.integers(-5, 5, g.shape).astype(np.int32)
        for conn in (6, 18, 26):
            for zero in (False, True):
                same(run(g, 5, conn, zero, v)[:3], R.adjacency(g, 5, conn, zero, v), (dims, conn, zero))
                u = (g & 0xff).astype(np.uint8)
                same(run(u, 5, conn, zero)[:3], R.adjacency(u, 5, conn, zero), (dims, conn, zero, "uint8"))
    # all-distinct labels: the row ends - nothing pairs the last voxel of a row with the first of the next
    for nx in (5, 17):
        g = np.arange(1, nx * 3 * 2 + 1, dtype=np.int32).reshape(2, 3, nx)
        for conn, want in zip((6, 18, 26), R.grid_pair_counts(nx, 3, 2)):
            got = run(g, g.size, conn)
            same(got[:3], R.adjacency(g, g.size, conn), ("row ends", nx, conn))
            assert len(got[0]) == want
    # one pair for whole wavefronts: the alternating grid's closed form, with and without the table
    z, y, x = np.indices((3, 4, 300))
    for dtype in (np.int32, np.uint8):
        for use_table in (1, 0):
            pairs, table, _, counters = run(((x & 1) + 1).astype(dtype), 2, 26, use_table=use_table)
            assert pairs.tolist() == [[1, 2]] and table[0, :3].tolist() == R.alternating_row(300, 4, 3)
            assert counters["to_lds" if use_table else "to_global"] > 0 and counters["to_global" if use_table else "to_lds"] == 0


def test_a_full_slot_table_on_the_host(host_adj):
    run = host_adj(("O2V_ADJ_SLOT_BITS=2",))
    assert run.slots == 4
    rng = np.random.default_rng(241)
    g = rng.integers(1, 40, (4, 6, 50)).astype(np.int32)
    v = rng.integers(0, 1000, g.shape).astype(np.int32)
    got = run(g, 39, 26, False, v)
    same(got[:3], R.adjacency(g, 39, 26, False, v), "four slots")
    assert got[3]["to_lds"] > 0 and got[3]["to_global"] > 0 and not got[3]["overflow"]
    # a global table too small for the pairs reports it
    assert run(g, 39, 26, False, v, log2=4)[3]["overflow"] == 1
    # ... and one that just holds them, probe runs around the table's end included, is right
    m = len(R.adjacency(g, 39, 6)[0])
    log2 = int(np.ceil(np.log2(m)))
    got = run(g, 39, 6, log2=log2 + 1)
    assert not got[3]["overflow"]
    same(got[:3], R.adjacency(g, 39, 6), "a tight table")


def test_the_row_start_mutation_is_caught_on_the_host(host_adj):
    """With the element before a chunk at x = 0 taken from linear memory (O2V_ADJ_MUTATE_WRAP_BEFORE) the last voxel of a row
    touches the first of the next: pairs that the definition does not have."""
    run = host_adj(("O2V_ADJ_MUTATE_WRAP_BEFORE",))
    g = np.arange(1, 5 * 3 * 2 + 1, dtype=np.int32).reshape(2, 3, 5)
    got, want = run(g, g.size, 6), R.adjacency(g, g.size, 6)
    assert len(got[0]) > len(want[0]) and [5, 6] in got[0].tolist() and [5, 6] not in want[0].tolist()
    # a grid of one row has no row starts but its own
    line = np.arange(1, 20, dtype=np.int32).reshape(1, 1, 19)
    same(run(line, 19, 26)[:3], R.adjacency(line, 19, 26), "one row")


# ---- dense.* against a stub ----------------------------------------------------------------------------------------------------------

class AdjStub(LsStub):
    """adjacency_count computes the list with the reference and adjacency_write hands it out; label_stats and components_dense are
    LsStub's."""

    def adjacency_count(self, labels_ptr, fmt, strides, dims, n_labels, connectivity, flags, values_ptr=None, value_strides=None):
        self.calls.append(dict(labels=labels_ptr, fmt=fmt, strides=tuple(strides), dims=tuple(dims), n=n_labels, connectivity=connectivity, flags=flags,
                               values=values_ptr, value_strides=None if value_strides is None else tuple(value_strides)))
        g = _strided(labels_ptr, C.c_int32 if fmt == hip.LABELS_I32 else C.c_uint8, tuple(dims), tuple(strides))
        v = None if values_ptr is None else _strided(values_ptr, C.c_int32, tuple(dims), tuple(value_strides))
        self.pairs, self.table, outside = R.adjacency(g, n_labels, connectivity, bool(flags & hip.ADJ_ZERO), v)
        return len(self.pairs), outside

    def adjacency_write(self, pairs_ptr, table_ptr, capacity):
        m = len(self.pairs)
        assert capacity >= m
        if m:
            np.ctypeslib.as_array(C.cast(pairs_ptr, C.POINTER(C.c_int32)), shape=(2 * m,))[:] = self.pairs.reshape(-1)
            np.ctypeslib.as_array(C.cast(table_ptr, C.POINTER(C.c_int64)), shape=(R.COLUMNS * m,))[:] = self.table.reshape(-1)


def test_label_adjacency_formats_strides_and_n():
    dv = AdjStub()
    rng = np.random.default_rng(242)
    g = torch.from_numpy(LR.blobs(rng, (7, 6, 5), 9, 0.1))
    v = torch.from_numpy(rng.integers(-20, 20, (5, 6, 7)).astype(np.int32))
    adj = dense.label_adjacency(dv, g, connectivity=26, values=v)
    c = dv.calls[-1]
    assert (c["labels"], c["fmt"], c["strides"], c["dims"]) == (g.data_ptr(), hip.LABELS_I32, (1, 7, 42), (7, 6, 5))
    assert c["n"] == int(g.max()) == adj.n and c["connectivity"] == 26 == adj.connectivity and c["flags"] == 0 and c["values"] == v.data_ptr()
    pairs, table, outside = R.adjacency(g.numpy(), adj.n, 26, False, v.numpy())
    assert adj.pairs.dtype == torch.int32 and np.array_equal(adj.pairs.numpy(), pairs) and adj.outside == outside
    assert adj.faces.dtype == torch.int64 and np.array_equal(adj.faces.numpy(), table[:, 0]) and np.array_equal(adj.edges.numpy(), table[:, 1])
    assert np.array_equal(adj.corners.numpy(), table[:, 2]) and np.array_equal(adj.contacts.numpy(), table[:, :3].sum(1))
    assert adj.pass_high.dtype == torch.int32 and np.array_equal(adj.pass_high.numpy(), table[:, 3]) and np.array_equal(adj.pass_low.numpy(), table[:, 4])
    # without values; background; n=None per dtype
    adj = dense.label_adjacency(dv, g, 9, background=True)
    assert dv.calls[-1]["flags"] == hip.ADJ_ZERO and dv.calls[-1]["values"] is None and adj.pass_high is None and adj.pass_low is None
    assert int(adj.pairs[:, 0].min()) == 0 and not adj.edges.any() and not adj.corners.any()
    assert dense.label_adjacency(dv, g.to(torch.uint8)).n == 255 and dv.calls[-1]["fmt"] == hip.LABELS_U8
    adj = dense.label_adjacency(dv, g > 3, background=True)
    assert adj.n == 1 and dv.calls[-1]["fmt"] == hip.LABELS_U8 and adj.pairs.tolist() == [[0, 1]]
    # no pairs: empty tensors
    adj = dense.label_adjacency(dv, torch.ones((3, 3, 3), dtype=torch.int32), values=torch.ones((3, 3, 3), dtype=torch.int32))
    assert tuple(adj.pairs.shape) == (0, 2) and tuple(adj.faces.shape) == (0,) and tuple(adj.pass_high.shape) == (0,) and adj.pass_high.dtype == torch.int32
    assert tuple(adj.contacts.shape) == (0,) and dense.coordination(adj).tolist() == [0, 0]
    # any view: a slice of a batch with x and z swapped, values with strides of their own
    batch = torch.from_numpy(LR.blobs(rng, (4, 6, 10), 5)).reshape(2, 5, 6, 4)
    view = batch[1].permute(2, 1, 0)
    vals = torch.from_numpy(rng.integers(0, 9, (4, 12, 5)).astype(np.int32))[:, ::2, :]
    adj = dense.label_adjacency(dv, view, 5, connectivity=18, values=vals)
    assert dv.calls[-1]["strides"] == (24, 4, 1) and dv.calls[-1]["dims"] == (5, 6, 4) and dv.calls[-1]["value_strides"] == (1, 10, 60)
    want = R.adjacency(view.numpy(), 5, 18, False, vals.numpy())
    assert np.array_equal(adj.pairs.numpy(), want[0]) and np.array_equal(adj.pass_high.numpy(), want[1][:, 3])


def test_the_wait_comes_before_the_library_call(monkeypatch):
    dv = AdjStub()
    order = []
    monkeypatch.setattr(dense, "_sync", lambda device: order.append("sync"))
    monkeypatch.setattr(dv, "adjacency_count", lambda *a, **kw: order.append("adjacency_count") or (0, 0))
    monkeypatch.setattr(dv, "adjacency_write", lambda *a, **kw: order.append("adjacency_write"))
    dense.label_adjacency(dv, torch.zeros((4, 4, 4), dtype=torch.uint8), 2)
    assert order == ["sync", "adjacency_count", "adjacency_write"]


def test_neighbours_and_coordination():
    dv = AdjStub()
    z, y, x = np.indices((4, 4, 4))
    g = torch.from_numpy((1 + (x >= 2) + 2 * (y >= 2) + 4 * (z >= 2)).astype(np.int32))
    adj = dense.label_adjacency(dv, g, 9, connectivity=6)
    assert dense.coordination(adj).tolist() == [0] + [3] * 8 + [0]
    row_ptr, neighbour, pair = dense.adjacency_neighbours(adj)
    assert row_ptr.dtype == torch.int64 and neighbour.dtype == torch.int32 and pair.dtype == torch.int64
    assert row_ptr.tolist() == [0, 0] + [3 * k for k in range(1, 9)] + [24] and len(neighbour) == 24 == 2 * len(adj.pairs)
    assert neighbour[row_ptr[1]:row_ptr[2]].tolist() == [2, 3, 5] and neighbour[row_ptr[8]:row_ptr[9]].tolist() == [4, 6, 7]
    for L in range(1, 9):
        for k in range(int(row_ptr[L]), int(row_ptr[L + 1])):
            assert sorted(adj.pairs[pair[k]].tolist()) == sorted([L, int(neighbour[k])])
    adj = dense.label_adjacency(dv, g, 8, connectivity=26)
    assert dense.coordination(adj).tolist() == [0] + [7] * 8
    for fn in (dense.coordination, dense.adjacency_neighbours):
        with pytest.raises(TypeError):
            fn((1, 2))


def degree_of(mask):
    """uint8: 0 outside the mask, else 1 + the 26-neighbours in it (skeletonize's fmt="degree")."""
    m = np.pad(mask.astype(np.int64), 1)
    s = sum(m[1 + dz:m.shape[0] - 1 + dz, 1 + dy:m.shape[1] - 1 + dy, 1 + dx:m.shape[2] - 1 + dx]
            for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    return np.where(mask, s, 0).astype(np.uint8)


def ring(n=7):
    """A closed 8-connected voxel ring in a plane: every voxel has two neighbours."""
    m = np.zeros((3, n, n), bool)
    m[1, 1, 2:n - 2] = m[1, n - 2, 2:n - 2] = m[1, 2:n - 2, 1] = m[1, 2:n - 2, n - 2] = True
    return m


def test_skeleton_graph_known_shapes():
    dv = AdjStub()
    L = 9
    line = np.zeros((3, 3, L + 2), bool)
    line[1, 1, 1:L + 1] = True
    gr = dense.skeleton_graph(dv, torch.from_numpy(degree_of(line)))
    assert (gr.n_nodes, gr.n_branches) == (2, 1) and gr.branch_voxels.tolist() == [L - 2] and gr.node_voxels.tolist() == [1, 1]
    assert gr.incidence.tolist() == [[1, 1], [2, 1]] and gr.incidence.dtype == torch.int32 and gr.node_contacts.tolist() == []
    assert gr.labels.dtype == torch.int32 and sorted(torch.unique(gr.labels).tolist()) == [0, 1, 2, 3]
    plus = np.zeros((3, 11, 11), bool)
    plus[1, 5, 1:10] = plus[1, 1:10, 5] = True
    gr = dense.skeleton_graph(dv, torch.from_numpy(degree_of(plus)))
    assert (gr.n_nodes, gr.n_branches) == (5, 4) and sorted(gr.node_voxels.tolist()) == [1, 1, 1, 1, 5] and gr.branch_voxels.tolist() == [2] * 4
    junction = int(torch.argmax(gr.node_voxels)) + 1
    assert sorted(gr.incidence[:, 1].tolist()) == [1, 1, 2, 2, 3, 3, 4, 4] and int((gr.incidence[:, 0] == junction).sum()) == 4
    assert gr.node_contacts.tolist() == []
    m = ring()
    d = degree_of(m)
    assert set(d[m].tolist()) == {3}
    gr = dense.skeleton_graph(dv, torch.from_numpy(d))
    assert (gr.n_nodes, gr.n_branches) == (0, 1) and tuple(gr.incidence.shape) == (0, 2) and gr.branch_voxels.tolist() == [int(m.sum())]
    # a spur of one voxel at the ring's corner: an end, and the ring voxel it touches a junction - one node of two voxels, since
    # nodes are 26-components (so no two nodes ever touch: node_contacts stays empty); the reference agrees on all of them
    m[1, 0, 1] = True
    gr = dense.skeleton_graph(dv, torch.from_numpy(degree_of(m)))
    assert (gr.n_nodes, gr.n_branches) == (1, 1) and gr.node_voxels.tolist() == [2] and gr.incidence.tolist() == [[1, 1]]
    for mask in (line, plus, ring(), m):
        d = degree_of(mask)
        gr = dense.skeleton_graph(dv, torch.from_numpy(d))
        labels, n_nodes, n_branches, incidence, contacts = R.skeleton_graph(d)
        assert np.array_equal(gr.labels.numpy(), labels) and (gr.n_nodes, gr.n_branches) == (n_nodes, n_branches)
        assert np.array_equal(gr.incidence.numpy(), incidence) and np.array_equal(gr.node_contacts.numpy(), contacts)
        assert len(contacts) == 0


_U8 = torch.zeros((4, 4, 4), dtype=torch.uint8)
_I32 = torch.zeros((4, 4, 4), dtype=torch.int32)


@pytest.mark.parametrize("args, kw, exc", [
    ((torch.zeros((4, 4, 4), dtype=torch.int64),), {}, TypeError),
    ((torch.zeros((4, 4, 4)),), {}, TypeError),
    ((torch.zeros((4, 4), dtype=torch.uint8),), {}, ValueError),
    ((np.zeros((4, 4, 4), np.uint8),), {}, ValueError),
    ((torch.zeros((4, 0, 4), dtype=torch.uint8),), {}, ValueError),
    ((torch.zeros((4, 4, 4), device="meta", dtype=torch.uint8),), {}, ValueError),
    ((torch.zeros((1, 1, 65537), dtype=torch.uint8),), {}, ValueError),
    ((torch.zeros((1, 1, 1), dtype=torch.uint8).expand(2048, 1024, 1024),), {}, ValueError),      # 2^31 voxels
    ((_U8, 256), {}, ValueError),
    ((_U8, -1), {}, ValueError),
    ((_U8, 1.0), {}, ValueError),
    ((_U8, True), {}, ValueError),
    ((_U8 != 0, 2), {}, ValueError),
    ((_I32, 2 ** 31 - 1), {}, ValueError),
    ((_U8,), dict(connectivity=8), ValueError),
    ((_U8,), dict(connectivity=True), ValueError),
    ((_U8,), dict(connectivity="6"), ValueError),
    ((_U8,), dict(background=1), ValueError),
    ((_U8,), dict(background=None), ValueError),
    ((_U8,), dict(values=np.zeros((4, 4, 4), np.int32)), TypeError),
    ((_U8,), dict(values=torch.zeros((4, 4, 4))), TypeError),
    ((_U8,), dict(values=torch.zeros((4, 4, 5), dtype=torch.int32)), ValueError),
    ((_U8,), dict(values=torch.zeros((4, 4, 4), device="meta", dtype=torch.int32)), ValueError),
])
def test_rejects_before_any_device_call(args, kw, exc):
    dv = AdjStub()
    with pytest.raises(exc):
        dense.label_adjacency(dv, *args, **kw)
    assert not dv.calls


@pytest.mark.parametrize("degree", [torch.zeros((4, 4, 4), dtype=torch.bool), torch.zeros((4, 4), dtype=torch.uint8), np.zeros((4, 4, 4), np.uint8),
                                    torch.zeros((4, 0, 4), dtype=torch.uint8), torch.zeros((4, 4, 4), device="meta", dtype=torch.uint8)])
def test_skeleton_graph_rejects_before_any_device_call(degree):
    dv = AdjStub()
    with pytest.raises(ValueError):
        dense.skeleton_graph(dv, degree)
    assert not dv.calls


def test_the_docstrings_and_constants():
    assert "section 27" in dense.__doc__ and "o2v_hip_adjacency_count" in dense.__doc__ and "section 27" in dense.label_adjacency.__doc__
    assert hip.ADJ_COLUMNS == R.COLUMNS == 5 and hip.ADJ_ZERO != hip.FLAG_STAGE_TIMES and hip.ADJ_ZERO & (hip.ADJ_ZERO - 1) == 0
    header = open(os.path.join(os.path.dirname(SRC), "..", "include", "o2v_hip.h")).read()
    assert "O2V_HIP_ADJ_ZERO = %du" % hip.ADJ_ZERO in header and "O2V_HIP_ADJ_COLUMNS = %d" % hip.ADJ_COLUMNS in header
    for name in ("adjacency_count", "adjacency_write", "adjacency_times", "adjacency_counters", "adjacency_scratch_bytes"):
        assert callable(getattr(hip.DeviceVoxelizer, name))


# ---- the code object ---------------------------------------------------------------------------------------------------------------

K24_KERNELS = (["k_adj_pairsILj%dELj%dELb%dELb%dEE" % (f, c, v, vec) for f in (0, 1) for c in (6, 18, 26) for v in (0, 1) for vec in (0, 1)] +
               ["k_pt_listIxLj5EE", "k_adj_initE"])
PAIRS_LDS = 512 * 8 + 512 * 5 * 8   # a workgroup's table: 512 keys and their rows of five int64 (the kernel's comment)


@pytest.mark.parametrize("kernel", K24_KERNELS)
def test_k24_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    """From the code object's metadata only: no private segment, and the 24 KiB of LDS of the pass alone."""
    meta = device_asm[device_asm.index("amdhsa.kernels:"):]
    entry = [e for e in meta.split("\n  - ") if re.search(r"\.name: +_ZN\S*" + kernel + r"\S*\n", e)]
    assert len(entry) == 1, kernel + " is not in the gfx950 code object"
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
    assert int(re.search(r"\.wavefront_size: +(\d+)", entry[0]).group(1)) == 64 and int(re.search(r"\.max_flat_workgroup_size: +(\d+)", entry[0]).group(1)) == 256
    lds = int(re.search(r"\.group_segment_fixed_size: +(\d+)", entry[0]).group(1))
    assert lds == (PAIRS_LDS if "pairs" in kernel else 0) and PAIRS_LDS == 24576
