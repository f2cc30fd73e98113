"""Sky visibility without a GPU: the numpy reference (tests/openness_ref.py) against a scalar walk in Python
ints and against a Python restatement of the block skip, against the closed forms of the definition and a symmetry of the lattice;
the plain C++ of o2v_dev_k27_openness.hpp - the step, the skip, the short division - compiled for the host and run against the
reference, the division on every dividend below 2^25 for every divisor 1 ... 127, one mutation seen to fail; obj2voxel_amd.dense's
openness against a stub of the device call that computes with the reference; direction_set and shade_colors on CPU tensors against
Python ints; the Python-side refusals; the K27 kernels' metadata in the gfx950 code object."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import openness_ref as R

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip, visibility  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401
from tests.test_host_label_stats import _strided  # noqa: E402

K27 = os.path.join(SRC, "o2v_dev_k27_openness.hpp")
CUSTOM = [(127, 1, 0), (0, 0, -1), (3, -5, 7), (-2, -2, 1), (1, 126, -127)]


# ---- the reference ----------------------------------------------------------------------------------------------------------------

def test_direction_sets():
    for n, r in ((6, 1), (26, 1), (98, 2), (290, 3)):
        d = R.direction_set(n)
        assert d.shape == (n, 3) and d.dtype == np.int32 and np.abs(d).max() == r and len({tuple(v) for v in d.tolist()}) == n
        keys = [(v[2], v[1], v[0]) for v in d.tolist()]
        assert keys == sorted(keys)
        assert np.array_equal(np.sort(d, axis=0), np.sort(-d, axis=0))   # with d also -d
        assert torch.equal(dense.direction_set(n), torch.from_numpy(d)) and dense.direction_set(n).dtype == torch.int32
    assert R.direction_set(6).tolist() == [[0, 0, -1], [0, -1, 0], [-1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert [2, 0, 0] not in R.direction_set(98).tolist() and [2, 1, 0] in R.direction_set(98).tolist() and [2, 2, 1] in R.direction_set(98).tolist()
    for bad in (0, 7, 27, True, 26.0, "26", None):
        with pytest.raises(ValueError):
            dense.direction_set(bad)


def test_the_reference_against_the_scalar_walk_and_the_skip():
    """Three constructions of one answer: the vectorised fine walk, the scalar fine walk, the walk that skips empty blocks of two
    levels (and of the kernel's three), on random sparse grids with random directions and cut-offs."""
    rng = np.random.default_rng(310)
    rays = 0
    for dims, density, levels in (((37, 19, 21), 0.0005, (2, 4)), ((40, 40, 40), 0.005, (2, 4)), ((25, 33, 18), 0.05, (1, 3)), ((70, 9, 66), 0.002, (2, 4, 6)),
                                  ((5, 6, 7), 0.3, (2, 4, 6))):
        g = R.blobs(rng, dims, density)
        pyr = R.pyramid(g, levels)
        dirs = rng.integers(-5, 6, (40, 3))
        dirs = dirs[np.abs(dirs).max(1) > 0][:24]
        for md2 in (0, int(rng.integers(1, 400))):
            tg = rng.random(g.shape) < min(1.0, 60.0 / g.size)
            tg[0, 0, 0] = tg[-1, -1, -1] = True
            want = R.open_rays(g, dirs, tg, md2)
            cells = np.argwhere(tg)[:, ::-1].tolist()
            for t, c0 in enumerate(cells):
                for i, d in enumerate(dirs.tolist()):
                    assert R.scalar_open(g, c0, d, md2) == want[t, i], (dims, c0, d, md2)
                    assert R.skip_open(g, pyr, c0, d, md2) == want[t, i], (dims, c0, d, md2, "skip")
                    rays += 1
    assert rays > 5000


def test_closed_forms_of_the_definition():
    box = R.box_in(12, 1, 11)
    for n, face, edge, corner in ((6, 1, 2, 3), (26, 9, 15, 19), (98, 25, 45, 61), (290, 65, 121, 169)):
        got = R.open_counts(box, n)
        assert (got[10, 5, 5], got[10, 1, 5], got[10, 1, 1]) == (face, edge, corner), n
        assert got[5, 5, 5] == -1 and (got >= 0).sum() == 10 ** 3 - 8 ** 3
    hollow = R.box_in(12, 1, 11, hollow=True)
    inner = np.zeros_like(hollow)
    inner[2:10, 2:10, 2:10] = True
    for n in (26, 98):
        got = R.open_counts(hollow, n, "empty")
        assert (got[inner] == 0).all() and (got[~inner & ~hollow] > 0).all()
    for depth, want in ((1, (9, 25, 65)), (2, (1, 1, 9)), (3, (1, 1, 1))):
        g, floor = R.shaft(depth)
        assert not g[floor[2], floor[1], floor[0]] and g[floor[2] - 1, floor[1], floor[0]]
        assert tuple(int(R.open_counts(g, n, "empty")[floor[2], floor[1], floor[0]]) for n in (26, 98, 290)) == want, depth
    ball = R.ball()
    assert ball[30, 16, 16] and not ball[31, 16, 16]
    assert tuple(int(R.open_counts(ball, n)[30, 16, 16]) for n in (26, 98, 290)) == (17, 57, 161)
    lone = np.zeros((5, 5, 5), bool)
    lone[2, 2, 2] = True
    for n in (6, 26, 98, 290):
        assert R.open_counts(lone, n)[2, 2, 2] == n
    count, mask = R.openness(lone, 26, mask=True)
    assert count[2, 2, 2] == 26 and mask[2, 2, 2] == 2 ** 26 - 1 and (count == 255).sum() == 124 and not mask[count == 255].any()
    # the lowest-axis-first rule of the ray caster would give the roof's centre 1 of 26: the tie rule is what gives 9
    assert R.open_counts(box, 26)[10, 5, 5] == 9
    # the cut-off: from the centre of an empty 9^3 every direction is open without one and with any; a wall two voxels away blocks
    # +x unless the cut-off comes first (k^2 = 1 > floor(r^2) needs r < 1: never), and the order is outside, cut-off, solid
    wall = np.zeros((9, 9, 9), bool)
    wall[:, :, 6] = True
    c = np.zeros_like(wall)
    c[4, 4, 4] = True
    plus_x = [(1, 0, 0)]
    assert not R.open_rays(wall, plus_x, c)[0, 0] and not R.open_rays(wall, plus_x, c, 4)[0, 0] and R.open_rays(wall, plus_x, c, 3)[0, 0]
    assert R.max_distance2(None) == 0 and R.max_distance2(1) == 1 and R.max_distance2(2.5) == 6 and R.max_distance2(16) == 256


def test_the_result_commutes_with_a_symmetry_of_the_lattice():
    """A mirror in x combined with a swap of y and z, applied to the grid and the direction set together."""
    rng = np.random.default_rng(311)
    g = rng.random((9, 9, 9)) < 0.2
    dirs = R.direction_set(98)
    t = lambda a: a[:, :, ::-1].transpose(1, 0, 2)   # noqa: E731  ([z, y, x] -> mirrored in x, y and z swapped)
    dirs_t = np.stack([-dirs[:, 0], dirs[:, 2], dirs[:, 1]], 1)
    assert {tuple(v) for v in dirs_t.tolist()} == {tuple(v) for v in dirs.tolist()}
    for mode in ("surface", "empty"):
        for md2 in (0, 9):
            assert np.array_equal(R.open_counts(t(g), dirs_t, mode, md2), t(R.open_counts(g, dirs, mode, md2))), (mode, md2)
            assert np.array_equal(R.open_counts(t(g), dirs, mode, md2), t(R.open_counts(g, dirs, mode, md2))), (mode, md2)


# ---- the plain C++ of the header on the host --------------------------------------------------------------------------------------

HOST_OPEN = r"""
#include <cstdint>
#include <vector>
#define O2V_OPEN_HOST
#define O2V_OPEN_FN static inline
#define O2V_OPEN_HD static inline
static inline uint32_t open_mulhi(uint32_t a, uint32_t b) { return (uint32_t) (((uint64_t) a * b) >> 32); }
%s
extern "C" {

// the dividends n_begin <= n < n_end for which open_div differs from n / d, over every divisor d = 1 ... 127; *first: the first
// such n * 128 + d
uint64_t open_host_div_errors(uint32_t n_begin, uint32_t n_end, uint64_t *first)
{
    uint64_t bad = 0;
    for (uint32_t d = 1; d <= 127u; ++d) {
        const uint32_t r = open_recip(d);
        uint32_t q = n_begin / d, t = n_begin %% d;   // n = q d + t
        for (uint32_t n = n_begin; n < n_end; ++n) {
            if (open_div(n, r) != q) {
                if (!bad) *first = (uint64_t) n * 128u + d;
                ++bad;
            }
            if (++t == d) t = 0, ++q;
        }
    }
    return bad;
}

// the walk of the header from every cell of `cells` (x, y, z) along every direction, on masks built here from the byte grid
// [z][y][x]: counts[cell] = open directions, bits[cell] = bit i for direction i < 64
void open_host_counts(const uint8_t *grid, const int32_t *dims, const int32_t *dirs, uint32_t n_dirs, const int32_t *cells, uint64_t n_cells,
                      uint32_t md2, int skip, uint32_t *counts, uint64_t *bits)
{
    OpenGrid g{};
    std::vector<unsigned long long> m[3];
    for (int l = 0; l < 3; ++l) {
        uint32_t *b = l == 0 ? g.b0 : l == 1 ? g.b1 : g.b2;
        uint64_t words = 1;
        for (int a = 0; a < 3; ++a) b[a] = (uint32_t) ((dims[a] + (4 << 2 * l) - 1) / (4 << 2 * l)), words *= b[a];
        m[l].assign(words, 0ull);
    }
    for (int a = 0; a < 3; ++a) g.dim[a] = dims[a];
    for (int32_t z = 0; z < dims[2]; ++z)
        for (int32_t y = 0; y < dims[1]; ++y)
            for (int32_t x = 0; x < dims[0]; ++x)
                if (grid[((uint64_t) z * dims[1] + y) * dims[0] + x]) {
                    m[0][((uint64_t) (z >> 2) * g.b0[1] + (y >> 2)) * g.b0[0] + (x >> 2)] |= 1ull << open_bit(x, y, z);
                    m[1][((uint64_t) (z >> 4) * g.b1[1] + (y >> 4)) * g.b1[0] + (x >> 4)] |= 1ull << open_bit(x >> 2, y >> 2, z >> 2);
                    m[2][((uint64_t) (z >> 6) * g.b2[1] + (y >> 6)) * g.b2[0] + (x >> 6)] |= 1ull << open_bit(x >> 4, y >> 4, z >> 4);
                }
    g.m0 = m[0].data(), g.m1 = m[1].data(), g.m2 = m[2].data();
    for (uint64_t t = 0; t < n_cells; ++t) {
        counts[t] = 0, bits[t] = 0;
        for (uint32_t i = 0; i < n_dirs; ++i) {
            OpenDir d{};
            for (int a = 0; a < 3; ++a) {
                const int32_t v = dirs[3 * i + a];
                d.s[a] = v > 0 ? 1 : v < 0 ? -1 : 0, d.m[a] = (uint32_t) (v < 0 ? -v : v), d.r[a] = open_recip(d.m[a]);
            }
            const bool open = skip ? open_walk<true>(g, cells + 3 * t, d, md2) : open_walk<false>(g, cells + 3 * t, d, md2);
            if (open) ++counts[t], bits[t] |= i < 64u ? 1ull << i : 0ull;
        }
    }
}

}
"""


@pytest.fixture(scope="module")
def host_open(tmp_path_factory):
    """build(defines) -> the library of the plain C++ part of o2v_dev_k27_openness.hpp, compiled for the host."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    k = open(K27).read()
    text = k[k.index("constexpr uint32_t kOpenSurface"):k.index("#ifndef O2V_OPEN_HOST")] + k[k.index("// ---- the step, the skip"):k.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_open")

    def build(defines=()):
        name = "open_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_OPEN % text)
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = C.CDLL(str(tmp / (name + ".so")))
        L.open_host_div_errors.restype = C.c_uint64
        L.open_host_div_errors.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.open_host_counts.restype = None
        L.open_host_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        return L
    return build


def host_counts(L, g, dirs, mode, md2, skip):
    """(count uint8 [z, y, x], mask int64) as openness_ref.openness gives them, from the header's walk on the host"""
    g8 = np.ascontiguousarray(g, np.uint8)
    tg = R.targets(g, mode)
    cells = np.ascontiguousarray(np.argwhere(tg)[:, ::-1], np.int32)
    dirs = np.ascontiguousarray(dirs, np.int32)
    dims = np.array(g.shape[::-1], np.int32)
    counts, bits = np.zeros(len(cells), np.uint32), np.zeros(len(cells), np.uint64)
    L.open_host_counts(g8.ctypes.data, dims.ctypes.data, dirs.ctypes.data, len(dirs), cells.ctypes.data, len(cells), md2, int(skip), counts.ctypes.data,
                       bits.ctypes.data)
    dst, mk = np.full(g.shape, 255, np.uint8), np.zeros(g.shape, np.int64)
    dst[tg], mk[tg] = counts.astype(np.uint8), bits.view(np.int64)
    return dst, mk


def test_the_short_division_on_every_dividend(host_open):
    """floor(n / d) for every n < 2^25 and every d = 1 ... 127, the range DESIGN.md section 31 proves the form exact on - and one
    window past it where it no longer is (d = 127: 2^32 - 127 r = 16, so n + 1 > 2^28 fails at the multiples of 127): the form
    has no bits to spare beyond what the proof needs."""
    L = host_open()
    first = C.c_uint64(0)
    assert L.open_host_div_errors(0, 1 << 25, C.byref(first)) == 0, divmod(first.value, 128)
    assert L.open_host_div_errors(1 << 28, (1 << 28) + 4096, C.byref(first)) > 0


def test_the_walk_of_the_header_on_the_host(host_open):
    L = host_open()
    rng = np.random.default_rng(312)
    dirs = np.concatenate([R.direction_set(26), np.array(CUSTOM, np.int32), rng.integers(-5, 6, (12, 3)).astype(np.int32)])
    dirs = dirs[np.abs(dirs).max(1) > 0]
    n = 0
    for dims, density in (((1, 1, 1), 1.0), ((5, 6, 7), 0.3), ((17, 4, 3), 0.05), ((65, 9, 4), 0.05), ((70, 67, 66), 0.001), ((40, 40, 40), 0.02), ((130, 20, 18), 0.001)):
        g = R.blobs(rng, dims, density)
        for mode in ("surface", "empty"):
            if g.size > 3000:   # (a sample of the voxels of either kind)
                mode = R.targets(g, mode) & (rng.random(g.shape) < 600.0 / g.size)
            for md2 in (0, 6, 256):
                want = R.openness(g, dirs, mode, md2, mask=True)
                for skip in (True, False):
                    got = host_counts(L, g, dirs, mode, md2, skip)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (dims, md2, skip)
                    n += 1
    assert n == 84
    # the closed forms through the header's walk; the 290 set in two halves
    box, d290 = R.box_in(12, 1, 11), R.direction_set(290)
    halves = [host_counts(L, box, d290[a:a + 145], "surface", 0, True)[0].astype(int) for a in (0, 145)]
    both = halves[0] + halves[1]
    assert (both[10, 5, 5], both[10, 1, 5], both[10, 1, 1]) == (65, 121, 169)


def test_the_magnitudes_on_the_host(host_open):
    """An extent of 65 536 along x with m = 127: (2 K - 1) * m reaches its bound in the skip, and the cut-off's sum of squares
    passes 2^32.  The rays along x are too long for the reference to walk: a closed form stands in for it there."""
    L = host_open()
    g = np.zeros((2, 2, 65536), bool)
    g[1, 1, 40000] = g[0, 0, 3] = True
    short = np.array([(127, 1, 0), (-127, 0, 1), (-126, 1, 1), (0, 0, 1), (127, -1, -1), (5, 0, -1)], np.int32)
    along = np.array([(1, 0, 0), (-1, 0, 0), (127, 0, 0), (-127, 0, 0)], np.int32)
    tg = np.zeros_like(g)
    for x in (0, 1, 2, 3, 4, 39999, 40001, 65535, 32768):
        tg[:, :, x] = True
    for md2 in (0, 2 ** 32 - 1, 65535 ** 2, 39996 ** 2, 39995 ** 2):
        want = R.openness(g, short, tg, md2, mask=True)
        want_x = np.stack([R.open_along_x(g, tg, int(np.sign(d[0])), md2) for d in along], 1)
        for skip in (True, False):
            got = host_counts(L, g, short, tg, md2, skip)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (md2, skip)
            got = host_counts(L, g, along, tg, md2, skip)[1]
            assert np.array_equal((got[tg][:, None] >> np.arange(4)) & 1, want_x), (md2, skip)
    # x = 4 at y = z = 1 sees voxel 40 000 at distance 39 996 unless the cut-off comes first
    assert want_x[np.argwhere(tg).tolist().index([1, 1, 4])].tolist() == [True, True, True, True]
    assert R.open_along_x(g, tg, 1, 39996 ** 2)[np.argwhere(tg).tolist().index([1, 1, 4])] == False   # noqa: E712


def test_the_tie_mutation_is_caught_on_the_host(host_open):
    """With the `<=` of the tie turned into `<` (O2V_OPEN_MUTATE_TIE_LESS) only the lowest axis of equal events crosses: the centre of
    a flat roof sees 1 of the 26 directions instead of 9.  Along the axes, where no two events tie, nothing changes."""
    L = host_open(("O2V_OPEN_MUTATE_TIE_LESS",))
    box = R.box_in(12, 1, 11)
    for skip in (True, False):
        got = host_counts(L, box, R.direction_set(26), "surface", 0, skip)[0]
        assert got[10, 5, 5] == 1 and R.openness(box, 26)[0][10, 5, 5] == 9
        assert not np.array_equal(got, R.openness(box, 26)[0])
        assert np.array_equal(host_counts(L, box, R.direction_set(6), "surface", 0, skip)[0], R.openness(box, 6)[0])
    assert np.array_equal(host_counts(host_open(), box, R.direction_set(26), "surface", 0, True)[0], R.openness(box, 26)[0])


# ---- dense.openness against a stub ---------------------------------------------------------------------------------------------------

class OpenStub(StubVoxelizer):
    """The openness call, computed with the reference on the host memory behind the pointers."""

    def openness(self, grid_ptr, fmt, strides, dims, level, directions, target_mode, target_ptr, target_strides, max_distance2, dst_ptr, dst_strides,
                 mask_ptr=None, mask_strides=None, flags=0):
        self.calls.append(dict(grid=grid_ptr, fmt=fmt, strides=tuple(strides), dims=tuple(dims), level=level, directions=list(directions), mode=target_mode,
                               target=target_ptr, target_strides=target_strides, md2=max_distance2, dst=dst_ptr, dst_strides=tuple(dst_strides), mask=mask_ptr,
                               flags=flags))
        dims = tuple(dims)
        if fmt == hip.GRID_F32_BELOW:
            g = _strided(grid_ptr, C.c_float, dims, tuple(strides)) < level
        else:
            assert fmt == hip.GRID_U8
            g = _strided(grid_ptr, C.c_uint8, dims, tuple(strides)) != 0
        mode = {hip.OPEN_SURFACE: "surface", hip.OPEN_SOLID: "solid", hip.OPEN_EMPTY: "empty"}.get(target_mode)
        if mode is None:
            assert target_mode == hip.OPEN_GRID
            mode = _strided(target_ptr, C.c_uint8, dims, tuple(target_strides)) != 0
        dst, mk = R.openness(g, np.array(directions), mode, max_distance2, mask=mask_ptr is not None)
        _strided(dst_ptr, C.c_uint8, dims, tuple(dst_strides))[...] = dst
        if mask_ptr is not None:
            _strided(mask_ptr, C.c_int64, dims, tuple(mask_strides))[...] = mk
        return int((dst != 255).sum())


def test_openness_through_the_stub(on_cpu):  # noqa: F811
    dv = OpenStub()
    rng = np.random.default_rng(313)
    g = R.blobs(rng, (11, 6, 5), 0.2)
    for kind in ("bool", "uint8", "float32", "sliced"):
        t = {"bool": torch.from_numpy(g), "uint8": torch.from_numpy(g.astype(np.uint8) * 7), "float32": torch.from_numpy(np.where(g, -1.0, 1.0).astype(np.float32)),
             "sliced": torch.from_numpy(np.repeat(g, 2, axis=2).copy())[:, :, ::2]}[kind]
        level = 0.0 if kind == "float32" else None
        got = dense.openness(dv, t, level=level)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), R.openness(g, 26)[0])
        c = dv.calls[-1]
        assert (c["grid"], c["dims"], c["mode"], c["md2"], c["mask"], c["target"]) == (t.data_ptr(), (11, 6, 5), hip.OPEN_SURFACE, 0, None, None)
        assert c["strides"] == (t.stride(2), t.stride(1), t.stride(0)) and c["directions"] == [tuple(v) for v in R.direction_set(26).tolist()]
        for targets in ("solid", "empty"):
            for r, md2 in ((None, 0), (1, 1), (2.5, 6), (16, 256)):
                got, mk = dense.openness(dv, t, level=level, directions=torch.tensor(CUSTOM), targets=targets, max_distance=r, mask=True)
                want = R.openness(g, CUSTOM, targets, md2, mask=True)
                assert dv.calls[-1]["md2"] == md2 and mk.dtype == torch.int64 and np.array_equal(got.numpy(), want[0]) and np.array_equal(mk.numpy(), want[1])
    tg = torch.from_numpy(rng.random(g.shape) < 0.3)
    wide = torch.full((5, 6, 22), 77, dtype=torch.uint8)
    out = dense.openness(dv, torch.from_numpy(g), directions=98, targets=tg[:, :, :], out=wide[:, :, ::2])
    assert out.data_ptr() == wide.data_ptr() and dv.calls[-1]["dst_strides"] == (2, 22, 132) and dv.calls[-1]["mode"] == hip.OPEN_GRID
    assert np.array_equal(out.numpy(), R.openness(g, 98, tg.numpy())[0]) and bool((wide[:, :, 1::2] == 77).all())
    # a sun shadow
    shadow = dense.openness(dv, torch.from_numpy(g), directions=[(1, 2, 3)]) == 0
    assert np.array_equal(shadow.numpy(), R.openness(g, [(1, 2, 3)])[0] == 0)


def test_the_wait_comes_before_the_library_call(monkeypatch):
    dv = OpenStub()
    order = []
    monkeypatch.setattr(dense, "_device", lambda dv: torch.device("cpu"))
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: True)
    monkeypatch.setattr(dense, "_sync", lambda device: order.append("sync"))
    monkeypatch.setattr(dv, "openness", (lambda real: lambda *a, **kw: order.append("openness") or real(*a, **kw))(dv.openness))
    dense.openness(dv, torch.ones((4, 4, 4), dtype=torch.bool))
    assert order == ["sync", "openness"]


_B = torch.zeros((4, 4, 4), dtype=torch.bool)


@pytest.mark.parametrize("args, kw, exc", [
    ((np.zeros((4, 4, 4), bool),), {}, ValueError),
    ((torch.zeros((4, 4)),), {}, ValueError),
    ((torch.zeros((4, 4, 4), dtype=torch.int64),), {}, TypeError),
    ((torch.zeros((4, 4, 4)),), {}, ValueError),                                   # float32 without a level
    ((_B,), dict(level=0.5), ValueError),
    ((torch.zeros((4, 0, 4), dtype=torch.bool),), {}, ValueError),
    ((torch.zeros((4, 4, 4), device="meta", dtype=torch.bool),), {}, ValueError),
    ((torch.zeros((1, 1, 1), dtype=torch.bool).expand(1, 1, 65537),), {}, ValueError),
    ((torch.zeros((1, 1, 1), dtype=torch.bool).expand(2048, 1024, 1024),), {}, ValueError),   # 2^31 voxels
    ((_B,), dict(directions=27), ValueError),
    ((_B,), dict(directions=290), ValueError),                                     # above 254: a count is one byte
    ((_B,), dict(directions=True), ValueError),
    ((_B,), dict(directions=[]), ValueError),
    ((_B,), dict(directions=[(0, 0, 0)]), ValueError),
    ((_B,), dict(directions=[(128, 0, 0)]), ValueError),
    ((_B,), dict(directions=[(0, -128, 1)]), ValueError),
    ((_B,), dict(directions=[(1, 2)]), ValueError),
    ((_B,), dict(directions=[(1.0, 0, 0)]), ValueError),
    ((_B,), dict(directions=torch.zeros((3, 2), dtype=torch.int32)), ValueError),
    ((_B,), dict(directions=torch.ones((3, 3))), TypeError),
    ((_B,), dict(directions=[(1, 0, 0)] * 255), ValueError),
    ((_B,), dict(directions=98, mask=True), ValueError),                           # a mask holds 64
    ((_B,), dict(mask=1), ValueError),
    ((_B,), dict(targets="inside"), ValueError),
    ((_B,), dict(targets=torch.zeros((4, 4, 5), dtype=torch.bool)), ValueError),
    ((_B,), dict(targets=torch.zeros((4, 4, 4), dtype=torch.uint8)), TypeError),
    ((_B,), dict(targets=np.zeros((4, 4, 4), bool)), ValueError),
    ((_B,), dict(max_distance=0), ValueError),
    ((_B,), dict(max_distance=0.5), ValueError),
    ((_B,), dict(max_distance=-3), ValueError),
    ((_B,), dict(max_distance=float("nan")), ValueError),
    ((_B,), dict(max_distance=65536), ValueError),
    ((_B,), dict(max_distance=True), ValueError),
    ((_B,), dict(out=torch.zeros((4, 4, 5), dtype=torch.uint8)), ValueError),
    ((_B,), dict(out=torch.zeros((4, 4, 4), dtype=torch.bool)), TypeError),
    ((_B,), dict(out=np.zeros((4, 4, 4), np.uint8)), ValueError),
])
def test_openness_rejects_before_any_device_call(on_cpu, args, kw, exc):  # noqa: F811
    dv = OpenStub()
    with pytest.raises(exc):
        dense.openness(dv, *args, **kw)
    assert not dv.calls


# ---- shade_colors ---------------------------------------------------------------------------------------------------------------------

def shade_int(argb, count, D, ambient, hemisphere):
    """One voxel in Python ints."""
    v = argb & 0xffffffff
    if count == 255:
        return v
    f = min(2 * count, D) if hemisphere else count
    out = v & 0xff000000
    for shift in (16, 8, 0):
        out |= (((v >> shift) & 0xff) * (ambient * D + (256 - ambient) * f) + 128 * D) // (256 * D) << shift
    return out


def test_shade_colors_against_python_ints():
    rng = np.random.default_rng(314)
    for D in (1, 6, 26, 98, 254):
        count = rng.integers(0, D + 1, (3, 4, 5)).astype(np.uint8)
        count[rng.random(count.shape) < 0.3] = 255
        count[0, 0, 0], count[0, 0, 1], count[0, 0, 2] = 0, D, 255
        argb = rng.integers(0, 2 ** 32, count.shape, dtype=np.uint64).astype(np.uint32).view(np.int32)
        argb[0, 0, 0] = argb[0, 0, 1] = -1
        for ambient in (0, 64, 256):
            for hemisphere in (True, False):
                got = dense.shade_colors(torch.from_numpy(argb), torch.from_numpy(count), D, ambient=ambient, hemisphere=hemisphere)
                want = [shade_int(int(a), int(c), D, ambient, hemisphere) for a, c in zip(argb.reshape(-1), count.reshape(-1))]
                assert got.dtype == torch.int32 and got.numpy().view(np.uint32).reshape(-1).tolist() == want, (D, ambient, hemisphere)
                # alpha is kept, voxels that are no targets are unchanged, an open voxel keeps its colour, a closed one has ambient / 256
                assert np.array_equal(got.numpy().view(np.uint32) >> 24, argb.view(np.uint32) >> 24) and np.array_equal(got.numpy()[count == 255], argb[count == 255])
                assert got[0, 0, 1] == -1 and (got[0, 0, 0].item() & 0xff) == (255 * ambient + 128) // 256
    c8, a32 = torch.from_numpy(count), torch.from_numpy(argb)
    out = torch.zeros_like(a32)
    assert dense.shade_colors(a32, c8, 254, out=out) is out and torch.equal(out, dense.shade_colors(a32, c8, 254))
    assert dense.shade_colors is visibility.shade_colors and dense.openness is visibility.openness and dense.direction_set is visibility.direction_set
    for args, kw, exc in (((a32.long(), c8, 26), {}, TypeError), ((a32, c8.int(), 26), {}, TypeError), ((a32, c8[:2], 26), {}, ValueError), ((a32, c8, 0), {}, ValueError),
                          ((a32, c8, 255), {}, ValueError), ((a32, c8, 26.0), {}, ValueError), ((a32, c8, 26), dict(ambient=257), ValueError),
                          ((a32, c8, 26), dict(ambient=-1), ValueError), ((a32, c8, 26), dict(hemisphere=1), ValueError), ((a32, c8, 26), dict(out=out[:2]), ValueError),
                          ((a32.numpy(), c8, 26), {}, TypeError)):
        with pytest.raises(exc):
            dense.shade_colors(*args, **kw)


def test_the_docstrings_and_constants():
    assert "section 31" in dense.__doc__ and "o2v_hip_openness" in dense.__doc__ and "section 31" in dense.openness.__doc__
    header = open(os.path.join(os.path.dirname(SRC), "..", "include", "o2v_hip.h")).read()
    for name in ("SURFACE", "SOLID", "EMPTY", "GRID"):
        assert "O2V_HIP_OPEN_%s = %d" % (name, getattr(hip, "OPEN_" + name)) in header
    assert "O2V_HIP_OPEN_MAX_DIRECTIONS = %d" % hip.OPEN_MAX_DIRECTIONS in header and "O2V_HIP_OPEN_MAX_COMPONENT = %d" % hip.OPEN_MAX_COMPONENT in header
    for name in ("openness(", "openness_times(", "openness_scratch_bytes("):
        assert "o2v_hip_" + name in header, name
    assert callable(hip.DeviceVoxelizer.openness) and callable(hip.DeviceVoxelizer.openness_times)
    device = open(os.path.join(SRC, "o2v_device.hip")).read()
    assert 'env_on("O2V_OPEN_NO_SKIP")' in device and 'env_on("O2V_RAY_NO_SKIP")' in device
    # the scratch question needs no device: the masks and a list entry per voxel
    assert hip.openness_scratch_bytes((0, 4, 4)) == 0
    assert hip.openness_scratch_bytes((64, 64, 64)) == 8 * (16 ** 3 + 4 ** 3 + 1) + 8 + 36 * 254 + 4 * 64 ** 3


# ---- the code object -----------------------------------------------------------------------------------------------------------------

K27_KERNELS = ["k_open_targetsILj0ELb0E", "k_open_targetsILj0ELb1E", "k_open_targetsILj3ELb1E", "k_open_walkILb0ELb0E", "k_open_walkILb1ELb0E", "k_open_walkILb1ELb1E"]
DIR_LDS = 254 * 9 * 4   # k_open_walk's direction table: the only LDS of K27


@pytest.mark.parametrize("kernel", K27_KERNELS)
def test_k27_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    """From the code object's metadata only: wave64, 256 threads, no private segment, no LDS but the walk's direction table."""
    meta = device_asm[device_asm.index("amdhsa.kernels:"):]
    entry = [e for e in meta.split("\n  - ") if re.search(r"\.name: +_ZN\S*" + kernel + r"\S*\n", e)]
    assert len(entry) == 1, kernel + " is not in the gfx950 code object"
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
    assert int(re.search(r"\.wavefront_size: +(\d+)", entry[0]).group(1)) == 64
    assert int(re.search(r"\.max_flat_workgroup_size: +(\d+)", entry[0]).group(1)) == 256
    assert int(re.search(r"\.group_segment_fixed_size: +(\d+)", entry[0]).group(1)) == (DIR_LDS if "walk" in kernel else 0)
