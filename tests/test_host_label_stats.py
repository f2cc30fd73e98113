"""Per-label statistics without a GPU: the numpy reference (tests/label_stats_ref.py) against the
definition as a scalar loop, known answers, the overflow bound in Python ints, the plain C++ of o2v_dev_k19_label_stats.hpp
compiled for the host and run wavefront by wavefront against the reference (and one mutation seen to fail), obj2voxel_amd.dense's
label_stats, component_stats, centroids, covariances, mass_properties, keep_largest and crop against a stub of the device call
that computes the table with the reference, and the K19 kernels in the gfx950 code object."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import components_ref as CR
from tests import label_stats_ref as R

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_components import mesh_sets, two_cubes  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401

K19 = os.path.join(SRC, "o2v_dev_k19_label_stats.hpp")
WHICH = (R.ALL, 0, R.BOX, R.SUMS, R.MOMENTS, R.FACES, R.BOX | R.MOMENTS)


# ---- the reference ----------------------------------------------------------------------------------------------------------------

def test_reference_against_a_scalar_loop():
    rng = np.random.default_rng(19)
    cases = 0
    for dims in ((1, 1, 1), (1, 4, 3), (5, 1, 2), (4, 3, 1), (2, 2, 2), (3, 3, 3), (7, 3, 2), (9, 5, 4)):
        for n in (0, 1, 7, 255):
            for origin in ((0, 0, 0), (3, 0, 11), tuple(int(v) for v in rng.integers(0, 60000, 3))):
                for outside in (0.0, 0.2):
                    g = R.blobs(rng, dims, n, outside)
                    if cases % 3 == 0:
                        g = rng.integers(-1 if outside else 0, n + 2 if outside else n + 1, g.shape).astype(np.int32)   # no coherence at all
                    which = WHICH[cases % len(WHICH)]
                    a, oa = R.label_stats(g, n, origin, which)
                    b, ob = R.label_stats_loop(g, n, origin, which)
                    assert a.dtype == np.int64 and np.array_equal(a, b) and oa == ob, (dims, n, origin, outside, which)
                    assert int(a[:, 0].sum()) + oa == g.size
                    cases += 1
    assert cases == 192
    # uint8 and bool grids, as the device takes them
    for n in (0, 1, 7, 255):
        g = rng.integers(0, 256, (3, 4, 5)).astype(np.uint8)
        a, oa = R.label_stats(g, n, (1, 2, 3))
        b, ob = R.label_stats_loop(g, n, (1, 2, 3))
        assert np.array_equal(a, b) and oa == ob and (n < 255) == (oa > 0)
    g = rng.random((4, 4, 4)) < 0.5
    assert np.array_equal(R.label_stats(g, 1)[0], R.label_stats_loop(g, 1)[0])


# ---- known answers ---------------------------------------------------------------------------------------------------------------

def stats_of(g, n, origin=(0, 0, 0), **which):
    """dense.label_stats on the CPU through the stub."""
    return dense.label_stats(LsStub(), torch.from_numpy(np.ascontiguousarray(g)), n, origin=origin, **which)


def test_known_answer_solid_box():
    a, b, c = 6, 4, 3
    ox, oy, oz = 10, 20, 30
    g = np.ones((c, b, a), np.uint8)
    t, outside = R.label_stats(g, 1, (ox, oy, oz))
    assert outside == 0 and not t[0, 0] and t[0, 1:7].tolist() == [R.EMPTY_MIN] * 3 + [-1] * 3
    assert t[1].tolist() == R.box_row((a, b, c), (ox, oy, oz))
    assert t[1, 0] == a * b * c and t[1, 1:7].tolist() == [ox, oy, oz, ox + a - 1, oy + b - 1, oz + c - 1]
    assert t[1, 7] == b * c * (a * ox + a * (a - 1) // 2)
    st = stats_of(g, 1, (ox, oy, oz), moments=True, faces=True)
    assert st.lo[1].tolist() == [ox, oy, oz] and st.hi[1].tolist() == [ox + a, oy + b, oz + c] and st.lo[0].tolist() == st.hi[0].tolist() == [0, 0, 0]
    cen, cov = dense.centroids(st), dense.covariances(st)
    assert cen[1].tolist() == [ox + a / 2, oy + b / 2, oz + c / 2] and bool(torch.isnan(cen[0]).all()) and bool(torch.isnan(cov[0]).all())
    assert torch.allclose(cov[1], torch.diag(torch.tensor([a * a / 12, b * b / 12, c * c / 12], dtype=torch.float64)), rtol=0, atol=1e-9)
    assert int(st.faces[1]) == 2 * (a * b + b * c + a * c)


def test_known_answer_hollow_box_and_two_cubes():
    H = np.ones((10, 10, 10), bool)
    H[1:-1, 1:-1, 1:-1] = False
    t, _ = R.label_stats(H, 1)
    assert t[1, 16] == 984 and t[1, 0] == 488 and t[0, 16] == 6 * 64        # (the README's hollow box; the cavity's own six walls)
    surface, _ = mesh_sets(two_cubes(), 40)
    filled = CR.solidify(surface)
    t, outside = R.label_stats(filled, 2)
    assert outside == 0 and t[2, 0] == 33636 and t[1, 0] == surface.sum() and t[1, 0] + t[2, 0] == (filled != 0).sum()
    st = stats_of(filled, 2, moments=True)
    volume, centre, inertia = dense.mass_properties(st, (1, 2))
    assert volume == 33636 + int(surface.sum())
    z, y, x = np.nonzero(filled)
    p = np.stack([x, y, z], 1) + 0.5
    assert np.allclose(centre.numpy(), p.mean(0), rtol=0, atol=1e-9)
    d = p - p.mean(0)
    second = d.T @ d + np.eye(3) * len(p) / 12
    assert np.allclose(inertia.numpy(), np.eye(3) * np.trace(second) - second, rtol=1e-12)


def test_the_overflow_bound():
    top = R.largest_sum()
    assert top == (2 ** 32 - 131071) * (2 ** 31 - 1) and top < 2 ** 63
    assert (R.MAX_EXTENT - 1) ** 2 == 2 ** 32 - 131071
    # one more voxel, or one more step of the extent, is not covered
    assert (2 * R.MAX_EXTENT - 1) ** 2 * R.MAX_VOXELS >= 2 ** 63 and (R.MAX_EXTENT - 1) ** 2 * 2 ** 31 >= 2 ** 63 - 2 ** 49
    # a full row at the far corner: the closed forms stay exact in int64
    row = R.box_row((2047, 1024, 1024), (65536 - 2047, 65536 - 1024, 65536 - 1024))
    assert row[0] == 2146435072 and max(row) < top and np.array(row, dtype=np.int64).tolist() == row


# ---- the kernel's own algebra on the host ------------------------------------------------------------------------------------------

HOST_LS = r"""
#include <cstdint>
#include <stddef.h>
#include <vector>
#define O2V_LS_HOST
#define O2V_LS_FN static inline
%s
// k_label_stats' steps for one workgroup that takes the whole grid (contiguous, [z][y][x]), a wavefront of 64 chunks at a time.
template <uint32_t Format, typename T>
static void ls_host_t(const T *grid, const uint32_t *dims, const uint32_t *origin, uint32_t n_labels, uint32_t which, uint32_t use_table,
                      int64_t *table, uint64_t *outside)
{
    constexpr uint32_t K = ls_lane<Format>();
    const uint32_t nx = dims[0], ny = dims[1], nz = dims[2], cpr = (nx + K - 1u) / K;
    const uint64_t chunks = (uint64_t) cpr * ny * nz;
    std::vector<int32_t> keys(kLsSlots, kLsEmptyKey);
    std::vector<long long> tab(kLsSlots * kLsCols);
    for (uint32_t i = 0; i < kLsSlots * kLsCols; ++i) tab[i] = ls_init_value(i %% kLsCols, which);
    for (uint64_t i = 0; i < ((uint64_t) n_labels + 1u) * kLsCols; ++i) table[i] = ls_init_value((uint32_t) (i %% kLsCols), which);
    *outside = 0;
    auto chunk = [&](uint32_t x0, uint32_t n, uint32_t y, uint32_t z) {
        LsVec v{{0u, 0u, 0u, 0u}};
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t e = (uint32_t) grid[((size_t) z * ny + y) * nx + x0 + i];
            if (Format == kLsI32) v.w[i] = e;
            else v.w[i >> 2] |= (e & 0xffu) << (8u * (i & 3u));
        }
        return v;
    };
    auto add_run = [&](long long *row, uint64_t X0, uint64_t len, uint64_t Y, uint64_t Z, uint64_t faces) {
        ls_apply_run(which, X0, len, Y, Z, faces, [&](uint32_t c, uint64_t v) { row[c] += (long long) v; },
                     [&](uint32_t c, uint64_t v) { if ((long long) v < row[c]) row[c] = (long long) v; },
                     [&](uint32_t c, uint64_t v) { if ((long long) v > row[c]) row[c] = (long long) v; });
    };
    for (uint64_t base = 0; base < chunks; base += 64u) {
        bool active[64], joined[64], single[64], head[64];
        uint32_t row[64], x0[64], y[64], z[64], n[64], starts[64], sv[64], diff[64][6];
        int32_t first_label[64], last_label[64];
        LsVec v[64];
        for (uint32_t l = 0; l < 64u; ++l) {
            active[l] = base + l < chunks;
            row[l] = x0[l] = y[l] = z[l] = n[l] = starts[l] = sv[l] = 0;
            first_label[l] = last_label[l] = 0;
            if (!active[l]) continue;
            const uint32_t c = (uint32_t) (base + l);
            row[l] = c / cpr, x0[l] = (c - row[l] * cpr) * K, z[l] = row[l] / ny, y[l] = row[l] - z[l] * ny;
            n[l] = nx - x0[l] < K ? nx - x0[l] : K;
            v[l] = chunk(x0[l], n[l], y[l], z[l]);
            const uint32_t all = (1u << n[l]) - 1u;
            const bool before = x0[l] > 0u, behind = x0[l] + n[l] < nx;
            const uint32_t d = ls_diff<Format>(v[l], ls_shift_up<Format>(v[l], before ? (int32_t) grid[((size_t) z[l] * ny + y[l]) * nx + x0[l] - 1u] : 0));
            diff[l][0] = (before ? d : d | 1u) & all;
            const bool end_differs = !behind || (int32_t) grid[((size_t) z[l] * ny + y[l]) * nx + x0[l] + n[l]] != ls_value<Format>(v[l], n[l] - 1u);
            diff[l][1] = ((d >> 1) & (all >> 1)) | (uint32_t) end_differs << (n[l] - 1u);
            diff[l][2] = y[l] > 0u ? ls_diff<Format>(v[l], chunk(x0[l], n[l], y[l] - 1u, z[l])) & all : all;
            diff[l][3] = y[l] + 1u < ny ? ls_diff<Format>(v[l], chunk(x0[l], n[l], y[l] + 1u, z[l])) & all : all;
            diff[l][4] = z[l] > 0u ? ls_diff<Format>(v[l], chunk(x0[l], n[l], y[l], z[l] - 1u)) & all : all;
            diff[l][5] = z[l] + 1u < nz ? ls_diff<Format>(v[l], chunk(x0[l], n[l], y[l], z[l] + 1u)) & all : all;
            starts[l] = ls_starts<Format>(v[l], n[l]);
            const uint32_t last = 31u - (uint32_t) __builtin_clz(starts[l]);
            first_label[l] = ls_value<Format>(v[l], 0u), last_label[l] = ls_value<Format>(v[l], last);
            uint32_t f = 0;
            for (uint32_t k = 0; k < 6u; ++k) f += (uint32_t) __builtin_popcount(diff[l][k] & all & ~((1u << last) - 1u));
            sv[l] = ls_pack(n[l] - last, f);
        }
        for (uint32_t l = 0; l < 64u; ++l) {
            joined[l] = active[l] && l > 0u && ls_joins(last_label[l - 1u], row[l - 1u], first_label[l], row[l]);
            single[l] = starts[l] == 1u;
            head[l] = !(single[l] && joined[l]);
        }
        for (uint32_t d = 1u; d < 64u; d <<= 1) {   // (all lanes at once: from the values before the step)
            uint32_t pv[64];
            bool ph[64];
            for (uint32_t l = 0; l < 64u; ++l) pv[l] = sv[l], ph[l] = head[l];
            for (uint32_t l = d; l < 64u; ++l) ls_scan_step(sv[l], head[l], pv[l - d], ph[l - d]);
        }
        for (uint32_t l = 0; l < 64u; ++l) {
            if (!active[l]) continue;
            const uint32_t before = l ? sv[l - 1u] : 0u;
            const bool goes_on = l < 63u && joined[l + 1u];
            for (uint32_t m = starts[l]; m;) {
                const uint32_t s = (uint32_t) __builtin_ctz(m);
                m &= m - 1u;
                const uint32_t e = m ? (uint32_t) __builtin_ctz(m) : n[l];
                if (!m && goes_on) break;
                uint32_t len = e - s, faces = 0;
                for (uint32_t k = 0; k < 6u; ++k) faces += (uint32_t) __builtin_popcount(diff[l][k] & ((1u << e) - 1u) & ~((1u << s) - 1u));
                if (s == 0u && single[l]) len = ls_len(sv[l]), faces = ls_faces(sv[l]);
                else if (s == 0u && joined[l]) len += ls_len(before), faces += ls_faces(before);
                const int32_t label = ls_value<Format>(v[l], s);
                if (label < 0 || (uint32_t) label > n_labels) {
                    *outside += len;
                    continue;
                }
                const uint32_t slot = use_table ? ls_find_slot(keys.data(), label, [](int32_t *p, int32_t expected, int32_t desired) {
                    const int32_t was = *p;
                    if (was == expected) *p = desired;
                    return was;
                }) : kLsNoSlot;
                long long *dst = slot != kLsNoSlot ? tab.data() + slot * kLsCols : reinterpret_cast<long long *>(table) + (size_t) label * kLsCols;
                add_run(dst, (uint64_t) origin[0] + x0[l] + e - len, len, (uint64_t) origin[1] + y[l], (uint64_t) origin[2] + z[l], faces);
            }
        }
    }
    uint32_t used = 0;
    for (uint32_t slot = 0; slot < kLsSlots; ++slot) {
        if (keys[slot] == kLsEmptyKey) continue;
        ++used;
        for (uint32_t c = 0; c < kLsCols; ++c) {
            long long *dst = reinterpret_cast<long long *>(table) + (size_t) keys[slot] * kLsCols + c;
            const long long val = tab[slot * kLsCols + c];
            if (c >= kLsMin && c < kLsMax) *dst = val < *dst ? val : *dst;
            else if (c >= kLsMax && c < kLsSum) *dst = val > *dst ? val : *dst;
            else *dst += val;
        }
    }
    outside[1] = used;
}
extern "C" void ls_host(const void *grid, uint32_t format, const uint32_t *dims, const uint32_t *origin, uint32_t n_labels, uint32_t which,
                        uint32_t use_table, int64_t *table, uint64_t *outside)
{
    if (format == kLsI32) ls_host_t<kLsI32>(static_cast<const int32_t *>(grid), dims, origin, n_labels, which, use_table, table, outside);
    else ls_host_t<kLsU8>(static_cast<const uint8_t *>(grid), dims, origin, n_labels, which, use_table, table, outside);
}
extern "C" uint32_t ls_slots(void) { return kLsSlots; }
"""


@pytest.fixture(scope="module")
def host_ls(tmp_path_factory):
    """build(defines) -> run(grid, n, origin, which, use_table) -> (table, outside, slots in use): the plain C++ part of
    o2v_dev_k19_label_stats.hpp, compiled for the host."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    k19 = open(K19).read()
    text = k19[k19.index("constexpr uint32_t kLsI32"):k19.index("#ifndef O2V_LS_HOST")] + k19[k19.index("// ---- runs:"):k19.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_ls")

    def build(defines=()):
        name = "ls_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_LS % text)
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = C.CDLL(str(tmp / (name + ".so")))
        L.ls_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.ls_host.restype = None
        L.ls_slots.restype = C.c_uint32

        def run(g, n, origin=(0, 0, 0), which=R.ALL, use_table=1):
            g = np.ascontiguousarray(g)
            assert g.dtype in (np.int32, np.uint8)
            nz, ny, nx = g.shape
            table = np.full((n + 1, R.COLUMNS), -7, np.int64)
            out = (C.c_uint64 * 2)()
            L.ls_host(g.ctypes.data, 0 if g.dtype == np.int32 else 1, (C.c_uint32 * 3)(nx, ny, nz), (C.c_uint32 * 3)(*origin), n, which, use_table,
                      table.ctypes.data, out)
            return table, int(out[0]), int(out[1])
        run.slots = int(L.ls_slots())
        return run
    return build


def same(got, want, what):
    assert got[1] == want[1], (what, "outside", got[1], want[1])
    bad = np.argwhere(got[0] != want[0])
    assert not len(bad), (what, len(bad), "elements differ, the first at", bad[0].tolist(), got[0][tuple(bad[0])], want[0][tuple(bad[0])])


def test_every_row_length_on_the_host(host_ls):
    run = host_ls()
    rng = np.random.default_rng(190)
    n_cases = 0
    for nx in list(range(1, 71)) + [255, 256, 257]:
        for n in (1, 7):
            g = R.blobs(rng, (nx, 3, 2), n, 0.05)
            origin = (int(rng.integers(0, 65536 - nx)), 5, 65533)
            for which in (R.ALL, R.BOX | R.SUMS, 0):
                same(run(g, n, origin, which), R.label_stats(g, n, origin, which), (nx, n, "int32", which))
            u = np.where((g < 0) | (g > n), n + 1, g).astype(np.uint8)
            for use_table in (1, 0):
                same(run(u, n, origin, R.ALL, use_table), R.label_stats(u, n, origin), (nx, n, "uint8", use_table))
            n_cases += 1
    assert n_cases == 146
    # one label everywhere: chains over whole wavefronts, and the closed forms
    for dims in ((257, 3, 2), (1024, 2, 1), (1030, 1, 1), (1, 70, 3), (4, 1, 1)):
        for dtype in (np.int32, np.uint8):
            t, outside, _ = run(np.full(dims[::-1], 3, dtype), 3, (65536 - dims[0], 1, 2))
            assert outside == 0 and t[3].tolist() == R.box_row(dims, (65536 - dims[0], 1, 2)) and not t[:3, 0].any()
    # every voxel its own label, a two-label checkerboard, random labels
    g = np.arange(40 * 6 * 4, dtype=np.int32).reshape(4, 6, 40)
    same(run(g, g.size - 1), R.label_stats(g, g.size - 1), "own labels")
    z, y, x = np.indices((5, 6, 37))
    same(run(((x + y + z) & 1).astype(np.uint8), 1), R.label_stats((x + y + z) & 1, 1), "checkerboard")
    g = rng.integers(0, 5000, (6, 8, 50)).astype(np.int32)
    same(run(g, 4999, (1, 2, 3)), R.label_stats(g, 4999, (1, 2, 3)), "random labels")
    same(run(g, 4999, (1, 2, 3), use_table=0), R.label_stats(g, 4999, (1, 2, 3)), "random labels, no table")


def test_a_full_slot_table_on_the_host(host_ls):
    run = host_ls()
    slots = run.slots
    # more labels than slots, each in two runs far apart: the second run of a label finds its slot again or goes around the table
    n = 4 * slots
    g = np.concatenate([np.arange(n), np.arange(n)[::-1]]).astype(np.int32).reshape(2, 4, slots)
    for which in (R.ALL, R.BOX):
        t, outside, used = run(g, n - 1, (7, 8, 9), which)
        same((t, outside), R.label_stats(g, n - 1, (7, 8, 9), which), ("full table", which))
        assert used > slots // 2 and (t[:, 0] == 2).all()
    assert run(g, n - 1, use_table=0)[2] == 0
    # labels that all hash to one slot's neighbourhood cannot take more than the probes allow; the rest goes past the table
    g = rng_same_hash(slots)
    t, outside, used = run(g, int(g.max()))
    same((t, outside), R.label_stats(g, int(g.max())), "one hash")
    assert used < len(np.unique(g))


def rng_same_hash(slots):
    """int32 [1, 1, 64]: 64 labels whose hash (the kernel's ls_hash) is the same slot."""
    bits = slots.bit_length() - 1
    labels = [v for v in range(1, 200000) if ((v * 0x9e3779b1) & 0xffffffff) >> (32 - bits) == 5][:64]
    assert len(labels) == 64
    return np.array(labels, np.int32).reshape(1, 1, 64)


def test_the_squares_term_mutation_is_caught_on_the_host(host_ls):
    """Without the run's own sum of squares, len (len - 1) (2 len - 1) / 6 (O2V_LS_MUTATE_NO_SQUARES_TERM), the xx column of every
    run longer than one voxel is too small; runs of one voxel, and every other column, are the same."""
    run = host_ls(("O2V_LS_MUTATE_NO_SQUARES_TERM",))
    g = np.full((2, 3, 10), 1, np.int32)
    got, want = run(g, 1, (4, 5, 6))[0], R.label_stats(g, 1, (4, 5, 6))[0]
    assert got[1, 10] < want[1, 10] and want[1, 10] - got[1, 10] == 6 * (9 * 10 * 19 // 6)
    cols = [c for c in range(R.COLUMNS) if c != 10]
    assert np.array_equal(got[:, cols], want[:, cols])
    z, y, x = np.indices((3, 4, 9))
    board = ((x + y + z) & 1).astype(np.int32)
    same(run(board, 1, (4, 5, 6)), R.label_stats(board, 1, (4, 5, 6)), "runs of one voxel")


# ---- dense.* against a stub ----------------------------------------------------------------------------------------------------------

def _strided(ptr, ctype, dims, strides):
    """The numpy view [z, y, x] of the grid at the address ptr (host memory here), element strides (x, y, z)."""
    reach = 1 + sum((d - 1) * s for d, s in zip(dims, strides))
    flat = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(reach,))
    size = flat.itemsize
    return np.lib.stride_tricks.as_strided(flat, shape=dims[::-1], strides=tuple(s * size for s in strides[::-1]))


class LsStub(StubVoxelizer):
    """label_stats fills the table with the reference's; components_dense labels with the reference's."""

    def label_stats(self, labels_ptr, fmt, strides, dims, origin, n_labels, which, table_ptr):
        self.calls.append(dict(labels=labels_ptr, fmt=fmt, strides=tuple(strides), dims=tuple(dims), origin=tuple(origin), n=n_labels, which=which,
                               table=table_ptr))
        g = _strided(labels_ptr, C.c_int32 if fmt == hip.LABELS_I32 else C.c_uint8, tuple(dims), tuple(strides))
        table, outside = R.label_stats(g, n_labels, origin, which)
        np.ctypeslib.as_array(C.cast(table_ptr, C.POINTER(C.c_int64)), shape=(table.size,))[:] = table.reshape(-1)
        return outside

    def components_dense(self, grid_ptr, fmt, strides, dims, level, connectivity, flags, labels_ptr, label_strides):
        assert fmt == hip.GRID_U8
        labels, n = CR.label(_strided(grid_ptr, C.c_uint8, tuple(dims), tuple(strides)) != 0, connectivity)
        _strided(labels_ptr, C.c_int32, tuple(dims), tuple(label_strides))[...] = labels
        return n


def test_label_stats_formats_strides_and_n():
    dv = LsStub()
    rng = np.random.default_rng(191)
    g = torch.from_numpy(R.blobs(rng, (7, 6, 5), 9))
    st = dense.label_stats(dv, g, origin=(1, 2, 3), moments=True, faces=True)
    c = dv.calls[-1]
    assert (c["labels"], c["fmt"], c["strides"], c["dims"], c["origin"]) == (g.data_ptr(), hip.LABELS_I32, (1, 7, 42), (7, 6, 5), (1, 2, 3))
    assert c["n"] == int(g.max()) and c["which"] == 15 and st.n == c["n"] and st.origin == (1, 2, 3) and st.outside == 0
    want, _ = R.label_stats(g.numpy(), st.n, (1, 2, 3))
    assert st.count.dtype == torch.int64 and np.array_equal(st.count.numpy(), want[:, 0]) and tuple(st.lo.shape) == (st.n + 1, 3)
    assert np.array_equal(st.sum.numpy(), want[:, 7:10]) and np.array_equal(st.moment.numpy(), want[:, 10:16]) and np.array_equal(st.faces.numpy(), want[:, 16])
    some = want[:, 0] > 0
    assert np.array_equal(st.lo.numpy()[some], want[some, 1:4]) and np.array_equal(st.hi.numpy()[some], want[some, 4:7] + 1)
    assert not st.lo.numpy()[~some].any() and not st.hi.numpy()[~some].any()
    # n=None per dtype; an int32 grid of negative values only counts row 0
    assert dense.label_stats(dv, g.to(torch.uint8)).n == 255 and dv.calls[-1]["fmt"] == hip.LABELS_U8
    assert dense.label_stats(dv, g > 3).n == 1 and dv.calls[-1]["fmt"] == hip.LABELS_U8 and dv.calls[-1]["n"] == 1
    neg = dense.label_stats(dv, torch.full((2, 2, 2), -5, dtype=torch.int32))
    assert neg.n == 0 and neg.outside == 8 and int(neg.count[0]) == 0
    # what is not asked for is None, and the bits say so
    st = dense.label_stats(dv, g, 3, box=False, sums=False)
    assert dv.calls[-1]["which"] == 0 and st.lo is st.hi is st.sum is st.moment is st.faces is None and st.outside == int((g > 3).sum())
    st = dense.label_stats(dv, g, 3, sums=False, faces=True)
    assert dv.calls[-1]["which"] == hip.STATS_BOX | hip.STATS_FACES and st.sum is None and st.faces is not None
    # any view: a slice of a batch with x and z swapped
    batch = torch.from_numpy(R.blobs(rng, (4, 6, 10), 5)).reshape(2, 5, 6, 4)
    view = batch[1].permute(2, 1, 0)
    st = dense.label_stats(dv, view, 5)
    assert dv.calls[-1]["strides"] == (24, 4, 1) and dv.calls[-1]["dims"] == (5, 6, 4) and dv.calls[-1]["labels"] == view.data_ptr()
    assert np.array_equal(st.count.numpy(), R.label_stats(view.numpy(), 5)[0][:, 0])


def test_the_wait_comes_before_the_library_call(monkeypatch):
    dv = LsStub()
    order = []
    monkeypatch.setattr(dense, "_sync", lambda device: order.append("sync"))
    monkeypatch.setattr(dv, "label_stats", lambda *a, **kw: order.append("label_stats") or 0)
    dense.label_stats(dv, torch.zeros((4, 4, 4), dtype=torch.uint8), 2)
    assert order == ["sync", "label_stats"]


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
    ((_U8,), dict(origin=(0, 0)), ValueError),
    ((_U8,), dict(origin=(0, -1, 0)), ValueError),
    ((_U8,), dict(origin=(65533, 0, 0)), ValueError),
    ((_U8,), dict(origin=(0, 0, 65536)), ValueError),
    ((_U8,), dict(box=1), ValueError),
    ((_U8,), dict(moments=None), ValueError),
    ((_U8,), dict(faces="yes"), ValueError),
])
def test_rejects_before_any_device_call(args, kw, exc):
    dv = LsStub()
    with pytest.raises(exc):
        dense.label_stats(dv, *args, **kw)
    assert not dv.calls


def test_derived_quantities_need_their_columns():
    st = stats_of(np.ones((2, 2, 2), np.uint8), 1, box=False, sums=False)
    for fn in (dense.centroids, dense.covariances, lambda s: dense.mass_properties(s, (1,)), lambda s: dense.crop(_U8, s, 1)):
        with pytest.raises(ValueError):
            fn(st)
    with pytest.raises(TypeError):
        dense.centroids((1, 2))
    full = stats_of(np.ones((2, 2, 2), np.uint8), 1, moments=True)
    for rows in ((), (2,), (1, 1), (-1,)):
        with pytest.raises(ValueError):
            dense.mass_properties(full, rows)
    with pytest.raises(ValueError):
        dense.mass_properties(full, (1,), transform=[1.0] * 11)
    with pytest.raises(ValueError):
        dense.mass_properties(full, (1,), supersampling=3)
    for label in (2, -1, True, 1.0):
        with pytest.raises(ValueError):
            dense.crop(_U8, full, label)
    with pytest.raises(ValueError):
        dense.crop(torch.zeros((1, 1, 1)), full, 1)


def test_mass_properties_against_closed_forms():
    a, b, c = 8, 5, 3
    ox, oy, oz = 2, 7, 11
    g = np.zeros((20, 20, 20), np.uint8)
    g[oz:oz + c, oy:oy + b, ox:ox + a] = 2
    g[oz, oy:oy + b, ox:ox + a] = 1                                        # a surface layer and an interior: rows 1 + 2 are the box
    st = stats_of(g, 2, (100, 200, 300), moments=True)
    volume, centre, inertia = dense.mass_properties(st, (1, 2))
    assert volume == a * b * c and centre.tolist() == [100 + ox + a / 2, 200 + oy + b / 2, 300 + oz + c / 2]
    m = a * b * c
    want = torch.diag(torch.tensor([m * (b * b + c * c) / 12, m * (a * a + c * c) / 12, m * (a * a + b * b) / 12], dtype=torch.float64))
    assert torch.allclose(inertia, want, rtol=1e-12, atol=1e-6)
    # a row without voxels: volume 0, the rest NaN
    empty = dense.mass_properties(stats_of(g, 3, moments=True), (3,))
    assert empty[0] == 0.0 and bool(torch.isnan(empty[1]).all()) and bool(torch.isnan(empty[2]).all())
    # model space: voxel = A model + t at supersampling 2, so model = A^-1 (2 p - t): a scale of 1/4 per voxel after a rotation
    s, angle = 8.0, 0.3
    rot = np.array([[np.cos(angle), -np.sin(angle), 0], [np.sin(angle), np.cos(angle), 0], [0, 0, 1]])
    A, t = s * rot, np.array([5.0, -3.0, 2.0])
    vol_m, centre_m, inertia_m = dense.mass_properties(st, (1, 2), transform=list(A.reshape(-1)) + list(t), supersampling=2)
    k = 2.0 / s                                                             # model units per voxel
    assert abs(vol_m - volume * k ** 3) < 1e-9
    assert np.allclose(centre_m.numpy(), np.linalg.inv(A) @ (2 * centre.numpy() - t), rtol=0, atol=1e-9)
    assert np.allclose(inertia_m.numpy(), k ** 5 * (rot.T @ inertia.numpy() @ rot), rtol=1e-12, atol=1e-9)


def test_component_stats_keep_largest_and_crop():
    g = np.zeros((6, 8, 12), np.uint8)
    g[0, 0, 0:3] = 1            # component 1: 3 voxels
    g[2, 2:4, 2:4] = 1          # component 2: 4 voxels
    g[4, 0, 8:12] = 1           # component 3: 4 voxels (a tie with 2)
    g[5, 7, 0] = 1              # component 4: 1 voxel
    t = torch.from_numpy(g)
    dv = LsStub()
    labels, n, st = dense.component_stats(dv, t, connectivity=6, origin=(10, 20, 30), moments=True)
    assert n == 4 and st.count.tolist() == [g.size - 12, 3, 4, 4, 1] and st.moment is not None and st.origin == (10, 20, 30)
    assert dense.centroids(st)[2].tolist() == [13.0, 23.0, 32.5]
    for k, want in ((1, [2]), (2, [2, 3]), (3, [2, 3, 1]), (4, [2, 3, 1, 4]), (9, [2, 3, 1, 4])):
        kept = dense.keep_largest(dv, t, k, connectivity=6)
        assert kept.dtype == torch.bool and np.array_equal(kept.numpy(), np.isin(labels.numpy(), want)), k
    assert not dense.keep_largest(dv, torch.zeros((3, 3, 3), dtype=torch.uint8)).any()
    for bad in (0, -1, 1.0, True):
        with pytest.raises(ValueError):
            dense.keep_largest(dv, t, bad)
    for L in range(1, 5):
        view, o = dense.crop(labels, st, L)
        lo = st.lo[L].tolist()
        assert o == tuple(lo) and view.data_ptr() == labels[lo[2] - 30, lo[1] - 20, lo[0] - 10:].data_ptr()
        assert bool((view == L).all()) and int((labels == L).sum()) == view.numel()
    st5 = dense.label_stats(dv, labels, 5)
    view, o = dense.crop(labels, st5, 5)
    assert view.numel() == 0 and o == (0, 0, 0)
    with pytest.raises(ValueError):
        dense.crop(labels[:2], st, 3)      # the grid does not reach the box


def test_the_docstrings_name_the_units():
    assert "+ 0.5" in dense.centroids.__doc__ and "1/12" in dense.covariances.__doc__ and "|det|" in " ".join(dense.mass_properties.__doc__.split())
    assert "section 22" in dense.__doc__ and "o2v_hip_label_stats" in dense.__doc__


# ---- the kernels in the code object ------------------------------------------------------------------------------------------------

K19_KERNELS = ["k_ls_init"] + ["k_label_statsILj%dELb%dELb%dE" % (f, v, faces) for f in (0, 1) for v in (0, 1) for faces in (0, 1)]


@pytest.mark.parametrize("kernel", K19_KERNELS)
def test_k19_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    scratch = re.findall(r"; ScratchSize: (\d+)", device_asm[m.end():m.end() + 4000])
    assert scratch and scratch[0] == "0", scratch[:1]
