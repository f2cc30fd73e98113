"""Euler numbers without a GPU: the numpy reference (tests/topology_ref.py) against the definition as a scalar
loop over the lattice's cells, the known answers, the duality of the two connectivities and the exposed-faces identity against
tests/label_stats_ref.py; the plain C++ of o2v_dev_k25_euler.hpp compiled for the host behind K19's and run chunk by chunk and
wavefront by wavefront against the reference (with a tiny slot count, so that the probes run out, and one mutation seen to fail);
obj2voxel_amd.dense's euler_stats, euler_numbers, intrinsic_volumes and betti_numbers against a stub of the device calls that
computes with the references; the K25 kernels' metadata in the gfx950 code object."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import components_ref as CR
from tests import label_stats_ref as LR
from tests import topology_ref as R

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip, topology  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, device_asm, on_cpu  # noqa: E402,F401
from tests.test_host_label_stats import LsStub, _strided  # noqa: E402

K19 = os.path.join(SRC, "o2v_dev_k19_label_stats.hpp")
K25 = os.path.join(SRC, "o2v_dev_k25_euler.hpp")


def same(got, want, what):
    assert got[1] == want[1], (what, "outside", got[1], want[1])
    assert got[0].dtype == np.int64 and got[0].shape == want[0].shape, what
    bad = np.argwhere(got[0] != want[0])
    assert not len(bad), (what, len(bad), "elements differ, the first at", bad[0].tolist(), int(got[0][tuple(bad[0])]), int(want[0][tuple(bad[0])]))


# ---- the reference ----------------------------------------------------------------------------------------------------------------

def test_reference_against_a_scalar_loop():
    rng = np.random.default_rng(25)
    cases = 0
    for dims in ((1, 1, 1), (1, 4, 3), (5, 1, 2), (4, 3, 1), (2, 2, 2), (3, 3, 3), (7, 3, 2), (6, 5, 4)):
        for n in (0, 1, 7, 255):
            for outside in (0.0, 0.2):
                g = R.blobs(rng, dims, n, outside)
                if cases % 3 == 0:
                    g = rng.integers(-1 if outside else 0, n + 2 if outside else n + 1, g.shape).astype(np.int32)   # no coherence at all
                a, b = R.euler_stats(g, n), R.euler_stats_loop(g, n)
                assert a[0].dtype == np.int64 and a[0].shape == (n + 1, R.COLUMNS)
                same(a, b, (dims, n, outside))
                assert a[1] == int(((g < 0) | (g > n)).sum()) and int(a[0][:, 0].sum()) + a[1] == g.size
                cases += 1
    assert cases == 64
    u = rng.integers(0, 256, (3, 4, 5)).astype(np.uint8)
    for n in (0, 7, 200, 255):
        same(R.euler_stats(u, n), R.euler_stats_loop(u, n), ("uint8", n))
    m = rng.random((4, 4, 4)) < 0.5
    same(R.euler_stats(m, 1), R.euler_stats_loop(m, 1), "bool")
    assert R.euler_stats(m, 0)[1] == int(m.sum())


# ---- known answers ---------------------------------------------------------------------------------------------------------------

def test_known_answer_solid_boxes():
    for a, b, c in ((1, 1, 1), (2, 3, 4), (5, 1, 1), (1, 6, 2), (7, 5, 3)):
        t, outside = R.euler_stats(np.ones((c, b, a), bool), 1)
        assert t[1].tolist() == R.box_row(a, b, c) and not t[0].any() and outside == 0
        assert R.euler_numbers(t, 26)[1] == R.euler_numbers(t, 6)[1] == 1
        assert R.intrinsic_volumes(t)[1].tolist() == [1, a + b + c, a * b + b * c + a * c, a * b * c]
    assert R.box_row(1, 1, 1) == R.SINGLE_VOXEL


def test_known_answer_hollow_box_ring_and_plate():
    t, _ = R.euler_stats(R.hollow_box(10), 1)
    assert t[1].tolist() == [488, 1956, 2454, 988, 972, 486, 0] and t[0].tolist() == [512, 1728, 1944, 729, 1344, 1176, 343]
    assert R.euler_numbers(t, 26).tolist() == [1, 2] == R.euler_numbers(t, 6).tolist() and R.exposed_faces(t)[1] == 984
    assert t[0].tolist() == R.box_row(8, 8, 8)
    t, _ = R.euler_stats(R.square_ring(), 1)
    assert t[1].tolist() == [16, 80, 128, 64, 16, 0, 0] and R.euler_numbers(t, 26)[1] == R.euler_numbers(t, 6)[1] == 0
    t, _ = R.euler_stats(R.plate_with_two_holes(), 1)
    assert R.euler_numbers(t, 26)[1] == R.euler_numbers(t, 6)[1] == -1


def test_known_answer_pairs_and_checkerboard():
    t, _ = R.euler_stats(R.edge_pair(), 1)
    assert t[1].tolist() == [2, 12, 23, 14, 0, 0, 0] and (R.euler_numbers(t, 26)[1], R.euler_numbers(t, 6)[1]) == (1, 2)
    t, _ = R.euler_stats(R.corner_pair(), 1)
    assert t[1].tolist() == [2, 12, 24, 15, 0, 0, 0] and (R.euler_numbers(t, 26)[1], R.euler_numbers(t, 6)[1]) == (1, 2)
    t, _ = R.euler_stats(R.checkerboard(4), 1)
    assert t[1].tolist() == [32, 192, 276, 121, 0, 0, 0] and (R.euler_numbers(t, 26)[1], R.euler_numbers(t, 6)[1]) == (5, 32)


def test_duality_on_random_padded_grids():
    """chi_6 of the background = chi_26 of the set + 1 and the other way round, for a 0 / 1 grid padded with one layer of zeros."""
    rng = np.random.default_rng(251)
    for i in range(30):
        dims = rng.integers(1, 7, 3)
        g = np.pad(rng.random(tuple(dims)) < (0.2, 0.5, 0.8)[i % 3], 1)
        t, _ = R.euler_stats(g, 1)
        x26, x6 = R.euler_numbers(t, 26), R.euler_numbers(t, 6)
        assert x6[0] == x26[1] + 1 and x26[0] == x6[1] + 1, (i, x26.tolist(), x6.tolist())


def test_exposed_faces_are_label_stats_faces():
    rng = np.random.default_rng(252)
    for dims, n, outside in (((6, 5, 4), 3, 0.0), ((9, 1, 3), 7, 0.2), ((1, 1, 5), 1, 0.0), ((8, 8, 8), 20, 0.1)):
        g = R.blobs(rng, dims, n, outside)
        t, out = R.euler_stats(g, n)
        want, want_out = LR.label_stats(g, n, which=LR.FACES)
        assert np.array_equal(R.exposed_faces(t), want[:, 16]) and np.array_equal(t[:, 0], want[:, 0]) and out == want_out


def test_betti_numbers_of_the_reference():
    assert R.betti_numbers(R.ball()) == (1, 0, 0) and R.betti_numbers(R.square_ring()) == (1, 1, 0)
    assert R.betti_numbers(R.plate_with_two_holes()) == (1, 2, 0) and R.betti_numbers(R.hollow_box()) == (1, 0, 1)
    assert R.betti_numbers(R.edge_pair(), 26) == (1, 0, 0) and R.betti_numbers(R.edge_pair(), 6) == (2, 0, 0)


# ---- the kernel's own algebra on the host ------------------------------------------------------------------------------------------

HOST_EU = r"""
#include <cstdint>
#include <stddef.h>
#include <vector>
#define O2V_LS_HOST
#define O2V_LS_FN static inline
#define O2V_EU_HOST
#define O2V_EU_FN static inline
%s
// k_euler's steps for one workgroup that takes the whole grid (contiguous, [z][y][x]), a wavefront of 64 chunks at a time: the
// lanes' chunks, the runs as the wavefront settles them, then the other chunks label by label.
// ctr: [0] outside, [1] rows into the table of the workgroup, [2] rows to global memory, [3] chains of more than one run,
// [4] labels of a chunk whose columns are not the sum of their windows' increments
static int32_t cas32(int32_t *p, int32_t expected, int32_t desired)
{
    const int32_t was = *p;
    if (was == expected) *p = desired;
    return was;
}
template <uint32_t Format, typename T>
static int eu_host_t(const T *grid, const uint32_t *dims, uint32_t n_labels, uint32_t use_table, long long *table, uint64_t *ctr)
{
    constexpr uint32_t K = ls_lane<Format>();
    const uint32_t nx = dims[0], ny = dims[1], nz = dims[2], cpr = (nx + 1u + K - 1u) / K, rows_y = ny + 1u;
    const uint64_t chunks = (uint64_t) cpr * rows_y * (nz + 1u), total = (uint64_t) nx * ny * nz;
    std::vector<int32_t> s_key(kEuSlots, kLsEmptyKey);
    std::vector<long long> s_tab(kEuSlots * kEuCols, 0);
    for (uint64_t i = 0; i < ((uint64_t) n_labels + 1u) * kEuCols; ++i) table[i] = 0;
    for (int i = 0; i < 5; ++i) ctr[i] = 0;
    auto at = [&](uint32_t x, uint32_t y, uint32_t z) { return ((uint64_t) z * ny + y) * nx + x; };
    auto add = [&](int32_t label, const uint32_t col[kEuCols]) {
        const uint32_t slot = use_table ? eu_find_slot(s_key.data(), label, cas32) : kEuNoSlot;
        long long *row = slot != kEuNoSlot ? s_tab.data() + slot * kEuCols : table + (uint64_t) (uint32_t) label * kEuCols;
        for (uint32_t c = 0; c < kEuCols; ++c) row[c] += col[c];
        ++ctr[slot != kEuNoSlot ? 1 : 2];
    };
    for (uint64_t base = 0; base < chunks; base += 64u) {
        EuChunk ch[64];
        bool active[64], run[64];
        int32_t run_label[64];
        for (uint32_t l = 0; l < 64u; ++l) {
            EuChunk &c = ch[l];
            c.have = c.n = c.nw = 0u, c.has_before = false;
            for (uint32_t r = 0; r < kEuRows; ++r) c.row[r] = LsVec{{0u, 0u, 0u, 0u}}, c.before[r] = 0;
            active[l] = base + l < chunks, run[l] = false, run_label[l] = 0;
            if (!active[l]) continue;
            const uint32_t ci = (uint32_t) (base + l), lrow = ci / cpr, x0 = (ci - lrow * cpr) * K, vz = lrow / rows_y, vy = lrow - vz * rows_y;
            c.n = eu_voxels(x0, nx, K), c.nw = eu_windows(x0, nx, K);
            c.has_before = x0 > 0u;
            c.have = eu_rows_in_box(vy, vz, ny, nz);
            // (linear memory: what a mutation would read behind a row is the next row's first element; behind the grid's last row
            // there is nothing, and the chunk has the elements of its longest row)
            uint32_t longest = 0;
            for (uint32_t r = 0; r < kEuRows; ++r) {
                if (!((c.have >> r) & 1u)) continue;
                const uint32_t y = vy - 1u + (r & 1u), z = vz - 1u + (r >> 1);
                uint32_t n_r = 0;
                for (uint32_t i = 0; i < c.n && at(x0, y, z) + i < total; ++i, ++n_r) {
                    const uint32_t e = (uint32_t) grid[at(x0, y, z) + i];
                    if (Format == kLsI32) c.row[r].w[i] = e;
                    else c.row[r].w[i >> 2] |= (e & 0xffu) << (8u * (i & 3u));
                }
                longest = n_r > longest ? n_r : longest;
                if (c.has_before) c.before[r] = (int32_t) grid[at(x0 - 1u, y, z)];
            }
            c.n = longest;
            run[l] = eu_uniform<Format>(c, run_label[l]);
        }
        // the runs: a chain of runs of one label in lanes that follow each other is added once, by its first lane
        uint64_t runs = 0, heads = 0;
        for (uint32_t l = 0; l < 64u; ++l) {
            const bool head = run[l] && !(l > 0u && eu_joins(run[l - 1u], run_label[l - 1u], run_label[l]));
            runs |= (uint64_t) run[l] << l, heads |= (uint64_t) head << l;
        }
        for (uint32_t l = 0; l < 64u; ++l) {
            if (!active[l]) continue;
            const EuChunk &c = ch[l];
            if (run[l]) {
                if (!((heads >> l) & 1u)) continue;
                const uint32_t len = eu_chain(runs, heads, l) * K;
                ctr[3] += len > K;
                if (eu_counted(run_label[l], n_labels)) {
                    uint32_t col[kEuCols];
                    eu_run_columns(len, col);
                    add(run_label[l], col);
                } else {
                    ctr[0] += len;
                }
                continue;
            }
            uint32_t todo[kEuRows], before;
            eu_todo_init<Format>(c, todo, before);
            int32_t label = 0;
            while (eu_next<Format>(c, todo, before, label)) {
                uint32_t E[8];
                eu_label_masks<Format>(c, label, E);
                eu_taken(E, todo, before);
                if (!eu_counted(label, n_labels)) {
                    ctr[0] += (uint32_t) __builtin_popcount(E[7]);
                    continue;
                }
                uint32_t col[kEuCols], sum[kEuCols] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
                eu_columns(E, col);
                for (uint32_t w = 0; w < c.nw; ++w) {
                    const uint32_t inc = eu_increments(eu_config(E, w));
                    for (uint32_t k = 0; k < kEuCols; ++k) sum[k] += (inc >> (4u * k)) & 15u;
                }
                for (uint32_t k = 0; k < kEuCols; ++k) ctr[4] += sum[k] != col[k];
                add(label, col);
            }
        }
    }
    for (uint32_t slot = 0; slot < kEuSlots; ++slot) {
        if (s_key[slot] == kLsEmptyKey) continue;
        for (uint32_t c = 0; c < kEuCols; ++c) table[(uint64_t) (uint32_t) s_key[slot] * kEuCols + c] += s_tab[slot * kEuCols + c];
    }
    return 0;
}
extern "C" int eu_host(const void *grid, uint32_t format, const uint32_t *dims, uint32_t n_labels, uint32_t use_table, long long *table, uint64_t *ctr)
{
    if (format == kLsI32) return eu_host_t<kLsI32>(static_cast<const int32_t *>(grid), dims, n_labels, use_table, table, ctr);
    return eu_host_t<kLsU8>(static_cast<const uint8_t *>(grid), dims, n_labels, use_table, table, ctr);
}
extern "C" uint32_t eu_slots(void) { return kEuSlots; }
extern "C" uint32_t eu_increments_of(uint32_t config) { return eu_increments(config); }
"""


@pytest.fixture(scope="module")
def host_eu(tmp_path_factory):
    """build(defines) -> run(grid, n, use_table) -> (table, outside, counters): the plain C++ part of o2v_dev_k25_euler.hpp (behind
    K19's), compiled for the host."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    k19, k25 = open(K19).read(), open(K25).read()
    text = (k19[k19.index("constexpr uint32_t kLsI32"):k19.index("#ifndef O2V_LS_HOST")] + k19[k19.index("// ---- runs:"):k19.index("// ---- kernels")] +
            k25[k25.index("constexpr uint32_t kEuCols"):k25.index("#ifndef O2V_EU_HOST")] + k25[k25.index("// ---- windows:"):k25.index("// ---- kernels")])
    tmp = tmp_path_factory.mktemp("host_eu")

    def build(defines=()):
        name = "eu_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_EU % text)
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = C.CDLL(str(tmp / (name + ".so")))
        L.eu_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.eu_slots.restype = L.eu_increments_of.restype = C.c_uint32

        def run(g, n, use_table=1):
            g = np.ascontiguousarray(g)
            assert g.dtype in (np.int32, np.uint8)
            nz, ny, nx = g.shape
            table = np.full((n + 1, R.COLUMNS), -7, np.int64)
            ctr = np.zeros(5, np.uint64)
            L.eu_host(g.ctypes.data, 0 if g.dtype == np.int32 else 1, (C.c_uint32 * 3)(nx, ny, nz), n, use_table, table.ctypes.data, ctr.ctypes.data)
            counters = dict(to_lds=int(ctr[1]), to_global=int(ctr[2]), joined=int(ctr[3]), mismatches=int(ctr[4]))
            assert counters["mismatches"] == 0, "eu_columns is not the sum of eu_increments over the windows"
            return table, int(ctr[0]), counters
        run.slots = int(L.eu_slots())
        run.increments_of = L.eu_increments_of
        return run
    return build


def test_the_increments_of_every_configuration_on_the_host(host_eu):
    run = host_eu()
    for config in range(256):
        want = [0] * R.COLUMNS
        for col, mask in R.WINDOW_CELLS:
            want[col] += (config & mask) != 0
            if col in R.INNER_OF:
                want[R.INNER_OF[col]] += (config & mask) == mask
        packed = run.increments_of(config)
        assert [(packed >> (4 * k)) & 15 for k in range(R.COLUMNS)] == want, config
    assert [(run.increments_of(255) >> (4 * k)) & 15 for k in range(R.COLUMNS)] == R.ONE_WINDOW


def test_every_row_length_on_the_host(host_eu):
    run = host_eu()
    rng = np.random.default_rng(250)
    n_cases = 0
    for nx in list(range(1, 40)) + [63, 64, 65, 255, 256, 257]:
        ny, nz = 1 + n_cases % 3, 1 + n_cases // 3 % 3
        n = (0, 1, 7, 255)[n_cases % 4]
        g = R.blobs(rng, (nx, ny, nz), n, 0.05)
        if n_cases % 5 == 4:
            g = rng.integers(-1, n + 2, g.shape).astype(np.int32)   # pure noise
        u = np.where((g < 0) | (g > n), (n + 1) & 255, g).astype(np.uint8)
        for use_table in (1, 0):
            got = run(g, n, use_table)
            same(got[:2], R.euler_stats(g, n), (nx, ny, nz, n, "int32", use_table))
            assert got[2]["to_global" if use_table else "to_lds"] == 0 and (got[2]["to_lds" if use_table else "to_global"] > 0) == bool(got[0].any())
            same(run(u, n, use_table)[:2], R.euler_stats(u, n), (nx, ny, nz, n, "uint8", use_table))
        n_cases += 1
    assert n_cases == 45
    # every (ny, nz) in 1 ... 3 at one width that ends a chunk and one that does not
    for nx in (16, 21):
        for ny in (1, 2, 3):
            for nz in (1, 2, 3):
                g = R.blobs(rng, (nx, ny, nz), 3)
                same(run(g, 3)[:2], R.euler_stats(g, 3), (nx, ny, nz))
                same(run(g.astype(np.uint8), 3)[:2], R.euler_stats(g.astype(np.uint8), 3), (nx, ny, nz, "uint8"))
    # all-distinct labels: the row ends - the window at vx = nx sees nothing of the next row
    for nx in (5, 17):
        g = np.arange(1, nx * 3 * 2 + 1, dtype=np.int32).reshape(2, 3, nx)
        t, outside, _ = run(g, g.size)
        assert outside == 0 and not t[0].any() and (t[1:] == np.array(R.SINGLE_VOXEL)).all()
    # one label for whole wavefronts: the box's closed form, with joined runs, with and without the table
    for dtype in (np.int32, np.uint8):
        for use_table in (1, 0):
            t, outside, counters = run(np.full((3, 4, 300), 2, dtype), 2, use_table)
            assert t[2].tolist() == R.box_row(300, 4, 3) and not t[:2].any() and outside == 0 and counters["joined"] > 0
    # known answers through the kernel's algebra
    t, _, _ = run(R.hollow_box().astype(np.uint8), 1)
    assert t.tolist() == [[512, 1728, 1944, 729, 1344, 1176, 343], [488, 1956, 2454, 988, 972, 486, 0]]
    assert run(R.checkerboard().astype(np.int32), 1)[0][1].tolist() == [32, 192, 276, 121, 0, 0, 0]


def test_a_full_slot_table_on_the_host(host_eu):
    run = host_eu(("O2V_EU_SLOT_BITS=2",))
    assert run.slots == 4
    rng = np.random.default_rng(253)
    g = rng.integers(0, 40, (4, 6, 50)).astype(np.int32)
    got = run(g, 39)
    same(got[:2], R.euler_stats(g, 39), "four slots")
    assert got[2]["to_lds"] > 0 and got[2]["to_global"] > 0
    g = R.blobs(rng, (70, 9, 5), 30, 0.1)
    same(run(g, 30)[:2], R.euler_stats(g, 30), "four slots, blobs")


def test_the_row_end_mutation_is_caught_on_the_host(host_eu):
    """With the window at vx = nx taking the element behind its rows (O2V_EU_MUTATE_WRAP_ROW_END) - in linear memory the next
    row's first voxel - a row's last window sees a label that the definition does not put there.  A 1-wide grid here is a grid of
    one voxel or of one row: behind its only row there is no next row, and nothing changes."""
    run = host_eu(("O2V_EU_MUTATE_WRAP_ROW_END",))
    g = np.arange(1, 5 * 3 * 2 + 1, dtype=np.int32).reshape(2, 3, 5)
    got, want = run(g, g.size)[0], R.euler_stats(g, g.size)[0]
    assert not np.array_equal(got, want) and (want[1:] == np.array(R.SINGLE_VOXEL)).all()
    assert got[6].tolist() != R.SINGLE_VOXEL and got[6, R.VERTICES] > 8   # (label 6, the first voxel of the second row, is seen from the first row's end)
    one = np.array([[[3]]], np.int32)
    same(run(one, 3)[:2], R.euler_stats(one, 3), "one voxel")
    line = np.arange(1, 20, dtype=np.int32).reshape(1, 1, 19)
    same(run(line, 19)[:2], R.euler_stats(line, 19), "one row")


# ---- dense.* against a stub ----------------------------------------------------------------------------------------------------------

class EuStub(LsStub):
    """euler_stats fills the table with the reference's; label_stats is LsStub's, and components_dense with CC_INVERT honoured."""

    def components_dense(self, grid_ptr, fmt, strides, dims, level, connectivity, flags, labels_ptr, label_strides):
        assert fmt == hip.GRID_U8
        solid = _strided(grid_ptr, C.c_uint8, tuple(dims), tuple(strides)) != 0
        labels, n = CR.label(~solid if flags & hip.CC_INVERT else solid, connectivity)
        _strided(labels_ptr, C.c_int32, tuple(dims), tuple(label_strides))[...] = labels
        return n

    def euler_stats(self, labels_ptr, fmt, strides, dims, n_labels, table_ptr):
        self.calls.append(dict(labels=labels_ptr, fmt=fmt, strides=tuple(strides), dims=tuple(dims), n=n_labels, table=table_ptr))
        g = _strided(labels_ptr, C.c_int32 if fmt == hip.LABELS_I32 else C.c_uint8, tuple(dims), tuple(strides))
        table, outside = R.euler_stats(g, n_labels)
        np.ctypeslib.as_array(C.cast(table_ptr, C.POINTER(C.c_int64)), shape=(table.size,))[:] = table.reshape(-1)
        return outside


FIELDS = ("voxels", "faces", "edges", "vertices", "inner_faces", "inner_edges", "inner_vertices")


def test_euler_stats_formats_strides_and_n():
    dv = EuStub()
    rng = np.random.default_rng(254)
    g = torch.from_numpy(R.blobs(rng, (7, 6, 5), 9))
    g[0, 0, :3] = -2   # (below every row; n=None is the grid's maximum)
    st = dense.euler_stats(dv, g)
    c = dv.calls[-1]
    assert (c["labels"], c["fmt"], c["strides"], c["dims"]) == (g.data_ptr(), hip.LABELS_I32, (1, 7, 42), (7, 6, 5))
    assert c["n"] == int(g.max()) == st.n and isinstance(st, dense.EulerStats) and dense.EulerStats is topology.EulerStats
    want, outside = R.euler_stats(g.numpy(), st.n)
    assert st.outside == outside > 0
    for k, f in enumerate(FIELDS):
        assert getattr(st, f).dtype == torch.int64 and np.array_equal(getattr(st, f).numpy(), want[:, k]), f
    with pytest.raises(dataclasses.FrozenInstanceError):
        st.n = 3
    # n=None per dtype; an int32 grid of negative values only has row 0
    assert dense.euler_stats(dv, g.to(torch.uint8)).n == 255 and dv.calls[-1]["fmt"] == hip.LABELS_U8
    st = dense.euler_stats(dv, g > 3)
    assert st.n == 1 and dv.calls[-1]["fmt"] == hip.LABELS_U8 and dv.calls[-1]["n"] == 1 and int(st.voxels.sum()) == g.numel()
    neg = dense.euler_stats(dv, torch.full((2, 2, 2), -5, dtype=torch.int32))
    assert neg.n == 0 and neg.outside == 8 and int(neg.vertices[0]) == 0
    assert dense.euler_stats(dv, g, 3).outside == int(((g < 0) | (g > 3)).sum())
    # any view: a slice of a batch with x and z swapped; a sliced view
    batch = torch.from_numpy(R.blobs(rng, (4, 6, 10), 5)).reshape(2, 5, 6, 4)
    view = batch[1].permute(2, 1, 0)
    st = dense.euler_stats(dv, view, 5)
    assert dv.calls[-1]["strides"] == (24, 4, 1) and dv.calls[-1]["dims"] == (5, 6, 4)
    assert np.array_equal(st.edges.numpy(), R.euler_stats(view.numpy(), 5)[0][:, 2])
    sliced = torch.from_numpy(R.blobs(rng, (12, 6, 4), 5))[:, ::2, 1::3]
    st = dense.euler_stats(dv, sliced, 5)
    assert dv.calls[-1]["strides"] == (3, 24, 72) and dv.calls[-1]["dims"] == (4, 3, 4)
    assert np.array_equal(st.inner_faces.numpy(), R.euler_stats(sliced.numpy(), 5)[0][:, 4])


def test_the_wait_comes_before_the_library_call(monkeypatch):
    dv = EuStub()
    order = []
    monkeypatch.setattr(dense, "_sync", lambda device: order.append("sync"))
    monkeypatch.setattr(dv, "euler_stats", lambda *a, **kw: order.append("euler_stats") or 0)
    dense.euler_stats(dv, torch.zeros((4, 4, 4), dtype=torch.uint8), 2)
    assert order == ["sync", "euler_stats"]


def test_euler_numbers_and_intrinsic_volumes():
    dv = EuStub()
    rng = np.random.default_rng(255)
    g = R.blobs(rng, (9, 8, 7), 6)
    st = dense.euler_stats(dv, torch.from_numpy(g), 6)
    want, _ = R.euler_stats(g, 6)
    x26, x6, v = dense.euler_numbers(st), dense.euler_numbers(st, connectivity=6), dense.intrinsic_volumes(st)
    assert x26.dtype == x6.dtype == v.dtype == torch.int64 and tuple(x26.shape) == (7,) and tuple(v.shape) == (7, 4)
    assert np.array_equal(x26.numpy(), R.euler_numbers(want, 26)) and np.array_equal(x6.numpy(), R.euler_numbers(want, 6))
    assert np.array_equal(v.numpy(), R.intrinsic_volumes(want)) and torch.equal(v[:, 0], x26) and torch.equal(v[:, 3], st.voxels)
    st = dense.euler_stats(dv, torch.ones((4, 3, 2), dtype=torch.bool))
    assert dense.intrinsic_volumes(st)[1].tolist() == [1, 9, 26, 24] and dense.euler_numbers(st, 6).tolist() == [0, 1]
    assert int(6 * st.voxels[1] - 2 * st.inner_faces[1]) == 2 * 26
    with pytest.raises(ValueError, match="no cell complex of this kind models 18-connectivity"):
        dense.euler_numbers(st, 18)
    for bad in (8, True, "26", None, 26.5):
        with pytest.raises(ValueError):
            dense.euler_numbers(st, bad)
    for fn in (dense.euler_numbers, dense.intrinsic_volumes):
        with pytest.raises(TypeError):
            fn((1, 2))


def test_betti_numbers_known_shapes():
    dv = EuStub()
    t = lambda m: torch.from_numpy(np.ascontiguousarray(m))   # noqa: E731
    assert dense.betti_numbers(dv, t(R.ball())) == (1, 0, 0)
    assert dense.betti_numbers(dv, t(R.square_ring())) == (1, 1, 0) == dense.betti_numbers(dv, t(R.square_ring()), connectivity=6)
    assert dense.betti_numbers(dv, t(R.plate_with_two_holes())) == (1, 2, 0)
    assert dense.betti_numbers(dv, t(R.hollow_box())) == (1, 0, 1) == dense.betti_numbers(dv, t(R.hollow_box()), connectivity=6)
    assert dense.betti_numbers(dv, t(R.edge_pair()), connectivity=6) == (2, 0, 0) and dense.betti_numbers(dv, t(R.edge_pair()), connectivity=26) == (1, 0, 0)
    assert all(isinstance(b, int) for b in dense.betti_numbers(dv, t(R.ball())))
    # the complement of the hollow box inside a margin: the cavity's air is a component, the outer air a hollow box with a cavity
    padded = np.pad(R.hollow_box(), 1)
    assert dense.betti_numbers(dv, t(padded), background=True) == (2, 0, 1)
    assert dense.betti_numbers(dv, t(padded.astype(np.uint8))) == (1, 0, 1)
    # two rings that share nothing, and nothing at all
    two = np.zeros((3, 5, 11), bool)
    two[1:2, :, :5] = R.square_ring()
    two[1:2, :, 6:] = R.square_ring()
    assert dense.betti_numbers(dv, t(two)) == (2, 2, 0) == R.betti_numbers(two)
    assert dense.betti_numbers(dv, torch.zeros((3, 3, 3), dtype=torch.bool)) == (0, 0, 0)
    # against the numpy twin on random grids, both connectivities
    rng = np.random.default_rng(256)
    for p in (0.2, 0.5, 0.8):
        m = rng.random((6, 7, 8)) < p
        for conn in (6, 26):
            assert dense.betti_numbers(dv, t(m), connectivity=conn) == R.betti_numbers(m, conn), (p, conn)


_U8 = torch.zeros((4, 4, 4), dtype=torch.uint8)
_I32 = torch.zeros((4, 4, 4), dtype=torch.int32)


@pytest.mark.parametrize("args, exc", [
    ((torch.zeros((4, 4, 4), dtype=torch.int64),), TypeError),
    ((torch.zeros((4, 4, 4)),), TypeError),
    ((torch.zeros((4, 4), dtype=torch.uint8),), ValueError),
    ((np.zeros((4, 4, 4), np.uint8),), ValueError),
    ((torch.zeros((4, 0, 4), dtype=torch.uint8),), ValueError),
    ((torch.zeros((4, 4, 4), device="meta", dtype=torch.uint8),), ValueError),
    ((torch.zeros((1, 1, 65537), dtype=torch.uint8),), ValueError),
    ((torch.zeros((1, 1, 1), dtype=torch.uint8).expand(2048, 1024, 1024),), ValueError),      # 2^31 voxels
    ((_U8, 256), ValueError),
    ((_U8, -1), ValueError),
    ((_U8, 1.0), ValueError),
    ((_U8, True), ValueError),
    ((_U8 != 0, 2), ValueError),
    ((_I32, 2 ** 31 - 1), ValueError),
])
def test_euler_stats_rejects_before_any_device_call(args, exc):
    dv = EuStub()
    with pytest.raises(exc):
        dense.euler_stats(dv, *args)
    assert not dv.calls


@pytest.mark.parametrize("args, kw, exc, match", [
    ((_U8,), dict(connectivity=18), ValueError, "no cell complex of this kind models 18-connectivity"),
    ((_U8,), dict(connectivity=8), ValueError, "6 or 26"),
    ((_U8,), dict(connectivity=True), ValueError, "6 or 26"),
    ((_U8,), dict(background=1), ValueError, "background"),
    ((torch.zeros((4, 4, 4)),), {}, ValueError, "level"),
    ((torch.zeros((4, 4), dtype=torch.uint8),), {}, ValueError, "3-D"),
    ((torch.zeros((4, 0, 4), dtype=torch.uint8),), {}, ValueError, "empty"),
])
def test_betti_numbers_rejects_before_any_device_call(args, kw, exc, match):
    dv = EuStub()
    with pytest.raises(exc, match=match):
        dense.betti_numbers(dv, *args, **kw)
    assert not dv.calls


def test_the_docstrings_and_constants():
    assert "section 29" in dense.__doc__ and "o2v_hip_euler_stats" in dense.__doc__ and "section 29" in dense.euler_stats.__doc__
    assert hip.EULER_COLUMNS == R.COLUMNS == 7
    header = open(os.path.join(os.path.dirname(SRC), "..", "include", "o2v_hip.h")).read()
    assert "O2V_HIP_EULER_COLUMNS = %d" % hip.EULER_COLUMNS in header and "int o2v_hip_euler_stats(" in header and "int o2v_hip_euler_stats_times(" in header
    for name in ("euler_stats", "euler_stats_times"):
        assert callable(getattr(hip.DeviceVoxelizer, name))
    for name in ("EulerStats", "euler_stats", "euler_numbers", "intrinsic_volumes", "betti_numbers"):
        assert getattr(dense, name) is getattr(topology, name)


# ---- the code object ---------------------------------------------------------------------------------------------------------------

K25_KERNELS = ["k_eulerILj%dELb%dEE" % (f, vec) for f in (0, 1) for vec in (0, 1)] + ["k_eu_initE"]
EULER_LDS = 256 * 4 + 256 * 7 * 8   # a workgroup's table: 256 keys and their rows of seven int64 (the kernel's comment)


@pytest.mark.parametrize("kernel", K25_KERNELS)
def test_k25_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    """From the code object's metadata only: wave64, 256 threads, no private segment, and the 15 KiB of LDS of the pass alone."""
    meta = device_asm[device_asm.index("amdhsa.kernels:"):]
    entry = [e for e in meta.split("\n  - ") if re.search(r"\.name: +_ZN\S*" + kernel + r"\S*\n", e)]
    assert len(entry) == 1, kernel + " is not in the gfx950 code object"
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
    assert int(re.search(r"\.wavefront_size: +(\d+)", entry[0]).group(1)) == 64 and int(re.search(r"\.max_flat_workgroup_size: +(\d+)", entry[0]).group(1)) == 256
    lds = int(re.search(r"\.group_segment_fixed_size: +(\d+)", entry[0]).group(1))
    assert lds == (EULER_LDS if "euler" in kernel else 0) and EULER_LDS == 15360
