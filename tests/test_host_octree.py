"""Sparse voxel octrees without a GPU: the numpy reference (tests/octree_ref.py) against the closed forms of
the definition and against a second construction, a scalar breadth-first build; to_dense(build(g)) == g in the reference; the plain
C++ of o2v_dev_k26_octree.hpp compiled for the host behind the bit grid's and run against the reference - the cells of every level,
the mask of a 2^3 block from bit words where blocks straddle bit pairs and words, the descent, one mutation seen to fail;
obj2voxel_amd.dense's build_octree, octree_lookup and octree_to_dense against a stub of the device calls that computes with the
reference; octree_depth and octree_level on CPU tensors; the K26 kernels' metadata in the gfx950 code object."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import bits_host
from tests import octree_ref as R

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip, octree  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401
from tests.test_host_label_stats import _strided  # noqa: E402

K26 = os.path.join(SRC, "o2v_dev_k26_octree.hpp")


def counts(g, **kw):
    return R.build(g, **kw)["level_counts"]


# ---- the reference ----------------------------------------------------------------------------------------------------------------

def test_closed_forms_of_the_definition():
    t = R.build(np.zeros((4, 4, 4), bool))
    assert t["level_counts"] == [1, 0] and t["valid"].tolist() == [0] and t["full"].tolist() == [0] and t["first_child"].tolist() == [-1]
    cube = np.ones((8, 8, 8), bool)
    assert counts(cube, collapse=False) == [1, 8, 64] and R.build(cube, collapse=False)["voxels_listed"] == 512
    t = R.build(cube)
    assert t["level_counts"] == [1, 0, 0] and t["valid"].tolist() == [255] and t["full"].tolist() == [255] and t["voxels_listed"] == 0
    one = np.zeros((16, 16, 16), bool)
    one[3, 9, 14] = True
    for collapse in (True, False):
        t = R.build(one, collapse=collapse)
        assert t["level_counts"] == [1, 1, 1, 1] and t["voxels_listed"] == 1 and t["coords"].tolist() == [[0, 0, 0], [8, 8, 0], [12, 8, 0], [14, 8, 2]]
    t = R.build(R.checkerboard(16))
    assert t["level_counts"] == [1, 8, 64, 512] and t["depth"] == 4 and set(t["valid"][-512:].tolist()) == {0x69} and t["voxels_listed"] == 2048
    box = R.box((5, 6, 7))
    assert counts(box, origin=(1, 3, 5), depth=4) == [1, 4, 12, 36] and counts(box, origin=(1, 3, 5), depth=4, collapse=False) == [1, 4, 12, 48]
    ball = R.ball()
    assert int(ball.sum()) == 33552 and R.depth_of((0, 0, 0), (64, 64, 64)) == 6
    assert counts(ball) == [1, 8, 32, 104, 336, 936] and counts(ball, collapse=False) == [1, 8, 32, 136, 696, 4680]
    # a tree of depth 1: the root is the last level, its first_child the voxel index 0
    t = R.build(np.ones((1, 1, 1), bool))
    assert (t["depth"], t["level_counts"], t["valid"].tolist(), t["first_child"].tolist(), t["voxels_listed"]) == (1, [1], [1], [0], 1)


def test_solid_box_counts_in_python_ints():
    for origin, dims in (((1, 3, 5), (5, 6, 7)), ((0, 0, 0), (8, 8, 8)), ((0, 0, 0), (9, 4, 3)), ((63, 7, 8), (65, 5, 4)), ((0, 0, 0), (1, 1, 1))):
        for extra in (0, 2):
            for collapse in (True, False):
                D = R.depth_of(origin, dims) + extra
                t = R.build(R.box(dims), origin, D, collapse)
                assert (t["level_counts"], t["voxels_listed"]) == R.solid_box_counts(origin, dims, D, collapse), (origin, dims, extra, collapse)


def test_reference_against_the_recursive_build():
    rng = np.random.default_rng(30)
    n = 0
    for dims, origin in (((5, 6, 7), (1, 3, 5)), ((9, 3, 4), (0, 0, 0)), ((13, 9, 10), (7, 7, 8)), ((1, 1, 1), (0, 0, 0)), ((2, 2, 2), (0, 0, 0)),
                         ((1, 1, 1), (1, 1, 1)), ((17, 2, 3), (63, 0, 1)), ((16, 16, 16), (0, 0, 0)), ((8, 8, 8), (8, 16, 24))):
        for collapse in (True, False):
            for extra in (0, 2):
                for p in (0.02, 0.6, 0.98):
                    g = R.blobs(rng, dims, p)
                    D = R.depth_of(origin, dims) + extra
                    a = R.build(g, origin, D, collapse)
                    R.same(a, R.build_recursive(g, origin, D, collapse), (dims, origin, collapse, extra, p))
                    assert np.array_equal(R.to_dense(a, g.shape, origin), g)
                    # the children of a node are contiguous and every level is in Morton order
                    off = np.concatenate([[0], np.cumsum(a["level_counts"])])
                    for l in range(D):   # noqa: E741
                        c = a["coords"][off[l]:off[l + 1]].astype(np.int64)
                        assert (np.diff(R.morton(c[:, 0], c[:, 1], c[:, 2]).astype(np.int64)) > 0).all()
                    n += 1
    assert n == 108


def test_to_dense_of_a_padded_box_and_outside_the_cube():
    rng = np.random.default_rng(31)
    g = R.blobs(rng, (11, 6, 5), 0.5)
    for collapse in (True, False):
        t = R.build(g, (3, 1, 2), None, collapse)
        assert t["depth"] == 4
        got = R.to_dense(t, (12, 13, 20), (1, 0, 0))   # sticks out of [0, 16)^3 along x
        want = np.zeros((12, 13, 20), bool)
        want[2:7, 1:7, 2:13] = g
        assert np.array_equal(got, want)
    assert R.lookup_one(t, -1, 0, 0) == (0, -1, -1, -1) and R.lookup_one(t, 0, 16, 0) == (0, -1, -1, -1)


# ---- the kernel's plain C++ on the host ---------------------------------------------------------------------------------------------

HOST_OCT = r"""
#include <cstdint>
#include <stddef.h>
%s
#define O2V_OCT_HOST
#define O2V_OCT_FN static inline
#define O2V_OCT_HD static inline
static inline uint32_t oct_popc(uint32_t v) { return (uint32_t) __builtin_popcount(v); }
%s
static BitGrid grid_of(const uint32_t *dims)
{
    const uint32_t W = (dims[0] + 63u) / 64u;
    return BitGrid{dims[0], dims[1], dims[2], W, (uint64_t) W * dims[1] * dims[2]};
}
// the levels as the host side plans them, then k_oct_leaves and k_oct_up cell by cell; info: per level c0[3], n[3], first
extern "C" uint64_t oct_host_pyramid(const unsigned long long *bits, const uint32_t *dims, const uint32_t *origin, uint32_t D, uint16_t *pyr, uint64_t *info)
{
    const BitGrid g = grid_of(dims);
    OctLevel lv[16];
    uint64_t cells = 0;
    for (uint32_t l = 0; l < D; ++l) {
        lv[l].cells = 1;
        for (int a = 0; a < 3; ++a) {
            lv[l].c0[a] = oct_cell_lo(origin[a], D - l), lv[l].n[a] = oct_cell_n(origin[a], dims[a], D - l);
            lv[l].cells *= lv[l].n[a];
            info[7u * l + a] = lv[l].c0[a], info[7u * l + 3u + a] = lv[l].n[a];
        }
        lv[l].first = cells, info[7u * l + 6u] = cells;
        cells += lv[l].cells;
    }
    if (!pyr) return cells;
    for (uint32_t l = D; l-- > 0u;) {
        const OctLevel &L = lv[l];
        for (uint64_t c = 0; c < L.cells; ++c) {
            uint32_t i, j, k;
            oct_cell_at(L, (uint32_t) c, i, j, k);
            if (l + 1u == D) {
                const uint32_t mask = oct_block_mask(g, bits, origin[0], origin[1], origin[2], L.c0[0] + i, L.c0[1] + j, L.c0[2] + k);
                pyr[L.first + c] = (uint16_t) (mask | mask << 8);
                continue;
            }
            const OctLevel &Lc = lv[l + 1u];
            uint32_t child[8];
            for (uint32_t o = 0; o < 8u; ++o) {
                const uint32_t ci = 2u * (L.c0[0] + i) + (o & 1u) - Lc.c0[0], cj = 2u * (L.c0[1] + j) + ((o >> 1) & 1u) - Lc.c0[1],
                               ck = 2u * (L.c0[2] + k) + (o >> 2) - Lc.c0[2];
                child[o] = ci < Lc.n[0] && cj < Lc.n[1] && ck < Lc.n[2] ? pyr[Lc.first + ((uint64_t) ck * Lc.n[1] + cj) * Lc.n[0] + ci] : 0u;
            }
            pyr[L.first + c] = (uint16_t) oct_merge(child);
        }
    }
    return cells;
}
extern "C" uint32_t oct_host_pair(const unsigned long long *bits, const uint32_t *dims, int32_t x0, uint32_t y, uint32_t z)
{
    return oct_row_pair(grid_of(dims), bits, x0, y, z);
}
extern "C" void oct_host_lookup(const uint8_t *valid, const uint8_t *full, const int32_t *first_child, uint32_t n_nodes, uint32_t depth, uint32_t collapsed,
                                const int32_t *points, uint64_t n, int32_t *out)
{
    const OctTree t{valid, full, first_child, n_nodes, depth, collapsed};
    for (uint64_t p = 0; p < n; ++p) oct_descend(t, points[3u * p], points[3u * p + 1u], points[3u * p + 2u], out + 4u * p);
}
extern "C" void oct_host_blocks(const uint8_t *valid, const uint8_t *full, const int32_t *first_child, uint32_t n_nodes, uint32_t depth, uint32_t collapsed,
                                const uint32_t *blocks, uint64_t n, uint32_t *out)
{
    const OctTree t{valid, full, first_child, n_nodes, depth, collapsed};
    for (uint64_t p = 0; p < n; ++p) out[p] = oct_block(t, blocks[3u * p], blocks[3u * p + 1u], blocks[3u * p + 2u]);
}
"""


def pack(g):
    """the bit grid of g [z, y, x]: uint64 words [z][y][W], padding bits 0"""
    nz, ny, nx = g.shape
    W = -(-nx // 64)
    padded = np.zeros((nz, ny, W * 64), np.uint8)
    padded[:, :, :nx] = g
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view("<u8").reshape(-1).copy()


def u32(*v):
    return (C.c_uint32 * len(v))(*v)


@pytest.fixture(scope="module")
def host_oct(tmp_path_factory):
    """build(defines) -> the library of the plain C++ part of o2v_dev_k26_octree.hpp, compiled for the host behind the bit grid's."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    k = open(K26).read()
    text = k[k.index("constexpr uint32_t kOctMaxDepth"):k.index("#ifndef O2V_OCT_HOST")] + k[k.index("// ---- cells, bit pairs"):k.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_oct")

    def build(defines=()):
        name = "oct_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_OCT % (bits_host.plain_part(), text))
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = C.CDLL(str(tmp / (name + ".so")))
        L.oct_host_pyramid.restype = C.c_uint64
        L.oct_host_pyramid.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.oct_host_pair.restype = C.c_uint32
        L.oct_host_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32]
        tree = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        L.oct_host_lookup.argtypes = L.oct_host_blocks.argtypes = tree + [C.c_void_p, C.c_uint64, C.c_void_p]
        L.oct_host_lookup.restype = L.oct_host_blocks.restype = None
        return L
    return build


def host_pyramid(L, g, origin, D):
    """per level (valid [kz, ky, kx], full, lo (z, y, x)) from oct_host_pyramid"""
    nz, ny, nx = g.shape
    bits, info = pack(g), np.zeros(7 * D, np.uint64)
    cells = L.oct_host_pyramid(bits.ctypes.data, u32(nx, ny, nz), u32(*origin), D, None, info.ctypes.data)
    pyr = np.full(cells, 0xdead, np.uint16)
    assert L.oct_host_pyramid(bits.ctypes.data, u32(nx, ny, nz), u32(*origin), D, pyr.ctypes.data, info.ctypes.data) == cells
    out = []
    for l in range(D):   # noqa: E741
        c0, n, first = info[7 * l:7 * l + 3].astype(np.int64), info[7 * l + 3:7 * l + 6].astype(np.int64), int(info[7 * l + 6])
        e = pyr[first:first + int(n.prod())].reshape(n[2], n[1], n[0])
        out.append(((e & 0xff).astype(np.uint8), (e >> 8).astype(np.uint8), c0[::-1]))
    return out


def test_the_cells_of_every_level_on_the_host(host_oct):
    """Origins x = 0, 1, 63 and nx = 1, 63, 64, 65, 129: blocks that straddle bit pairs (odd origin) and words (x = 63 | 64)."""
    L = host_oct()
    rng = np.random.default_rng(32)
    n = 0
    for ox in (0, 1, 63):
        for nx in (1, 63, 64, 65, 129):
            ny, nz, oy, oz = 1 + n % 3, 1 + n // 3 % 3, n % 2, n // 2 % 2 * 3
            g = R.blobs(rng, (nx, ny, nz), (0.5, 0.9, 0.1)[n % 3], noise=0.1)
            for extra in (0, 2):
                D = R.depth_of((ox, oy, oz), (nx, ny, nz)) + extra
                got, want = host_pyramid(L, g, (ox, oy, oz), D), R.pyramid(g, (ox, oy, oz), D)
                for l in range(D):   # noqa: E741
                    assert np.array_equal(got[l][2], want[l]["lo"]) and got[l][0].shape == want[l]["valid"].shape, (ox, nx, D, l)
                    assert np.array_equal(got[l][0], want[l]["valid"]) and np.array_equal(got[l][1], want[l]["full"]), (ox, nx, D, l)
            n += 1
    assert n == 15
    # all solid: full cells exactly where a cell lies in the box
    g = R.box((129, 4, 6))
    got, want = host_pyramid(L, g, (63, 2, 2), 8), R.pyramid(g, (63, 2, 2), 8)
    assert all(np.array_equal(a[1], b["full"]) for a, b in zip(got, want)) and got[7][1].any() and got[6][1].any() and not got[5][1].any()


def test_the_pair_of_a_row_from_bit_words(host_oct):
    L = host_oct()
    rng = np.random.default_rng(33)
    for nx in (1, 2, 63, 64, 65, 128, 129):
        g = rng.random((2, 3, nx)) < 0.5
        bits = pack(g)
        for z in range(2):
            for y in range(3):
                row = np.concatenate([[False], g[z, y], [False]])   # row[x + 1] = voxel x
                for x0 in range(-1, nx):
                    assert L.oct_host_pair(bits.ctypes.data, u32(nx, 3, 2), x0, y, z) == int(row[x0 + 1]) | int(row[x0 + 2]) << 1, (nx, x0, y, z)
        assert L.oct_host_pair(bits.ctypes.data, u32(nx, 3, 2), -2, 0, 0) == 0 == L.oct_host_pair(bits.ctypes.data, u32(nx, 3, 2), nx, 0, 0)


def run_lookup(L, t, points):
    points = np.ascontiguousarray(points, np.int32).reshape(-1, 3)
    out = np.full((len(points), 4), -9, np.int32)
    L.oct_host_lookup(t["valid"].ctypes.data, t["full"].ctypes.data, t["first_child"].ctypes.data, len(t["valid"]), t["depth"], int(t["collapsed"]),
                      points.ctypes.data, len(points), out.ctypes.data)
    return out


def box_points(lo, hi):
    z, y, x = np.meshgrid(*(np.arange(lo, hi),) * 3, indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3)


def test_the_descent_on_the_host(host_oct):
    L = host_oct()
    rng = np.random.default_rng(34)
    for dims, origin, extra in (((11, 6, 5), (3, 1, 2), 0), ((16, 16, 16), (0, 0, 0), 0), ((5, 6, 7), (1, 3, 5), 1), ((1, 1, 1), (0, 0, 0), 0)):
        g = R.blobs(rng, dims, 0.6)
        for collapse in (True, False):
            t = R.build(g, origin, R.depth_of(origin, dims) + extra, collapse)
            side = 2 ** t["depth"]
            pts = box_points(-2, side + 2)
            got = run_lookup(L, t, pts)
            assert np.array_equal(got, R.lookup(t, pts)), (dims, collapse)
            inside = ((pts >= 0) & (pts < side)).all(1)
            assert (got[~inside] == (0, -1, -1, -1)).all() and got[inside, 0].sum() == g.sum()
            # a voxel's slot: the solid voxels with a slot have the slots 0 ... voxels_listed - 1, each once
            slots = got[got[:, 3] >= 0, 3]
            assert np.array_equal(np.sort(slots), np.arange(t["voxels_listed"]))
            # a block at a time: the eight voxels of every aligned 2^3 block of the cube
            b = box_points(0, side // 2) * 2
            b32 = np.ascontiguousarray(b, np.uint32)
            masks = np.zeros(len(b), np.uint32)
            L.oct_host_blocks(t["valid"].ctypes.data, t["full"].ctypes.data, t["first_child"].ctypes.data, len(t["valid"]), t["depth"], int(collapse),
                              b32.ctypes.data, len(b), masks.ctypes.data)
            for o in range(8):
                d = np.array([o & 1, (o >> 1) & 1, o >> 2])
                assert np.array_equal((masks >> o) & 1, R.lookup(t, b + d)[:, 0]), (dims, collapse, o)
    assert run_lookup(L, t, [[-2 ** 31, 0, 0], [0, 2 ** 31 - 1, 0]]).tolist() == [[0, -1, -1, -1]] * 2


def test_a_corrupt_tree_ends_the_descent_on_the_host(host_oct):
    L = host_oct()
    g = R.blobs(np.random.default_rng(35), (16, 16, 16), 0.5, noise=0.1)
    for collapse in (True, False):
        t = R.build(g, collapse=collapse)
        pts = box_points(0, 16)
        for bad in (len(t["valid"]), 2 ** 31 - 1, -1, -2 ** 31):
            broken = dict(t, first_child=np.where(np.arange(len(t["valid"])) < t["level_counts"][0] + t["level_counts"][1], bad, t["first_child"]).astype(np.int32))
            got = run_lookup(L, broken, pts)
            assert np.array_equal(got, R.lookup(broken, pts)) and (got[:, 1] == -2).any() and (got[got[:, 1] == -2] == (0, -2, -1, -1)).all(), (collapse, bad)


def test_the_swapped_octant_mutation_is_caught_on_the_host(host_oct):
    """With the octant bits of y and z exchanged (O2V_OCT_MUTATE_SWAP_YZ) the descent of a grid that is not symmetric in y and z
    takes other children; a grid that is symmetric in them does not notice."""
    L = host_oct(("O2V_OCT_MUTATE_SWAP_YZ",))
    g = np.zeros((8, 8, 8), bool)
    g[6, 1, 2] = True   # (x, y, z) = (2, 1, 6)
    t = R.build(g)
    pts = box_points(0, 8)
    got, want = run_lookup(L, t, pts), R.lookup(t, pts)
    assert not np.array_equal(got, want) and got[:, 0].sum() == 1 and pts[got[:, 0] == 1].tolist() == [[2, 6, 1]]
    sym = g | g.transpose(1, 0, 2)
    t = R.build(sym)
    assert np.array_equal(run_lookup(L, t, pts)[:, 0], R.lookup(t, pts)[:, 0])
    assert np.array_equal(run_lookup(host_oct(), R.build(g), pts), want)


# ---- dense.* against a stub ----------------------------------------------------------------------------------------------------------

def _array(ptr, ctype, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,))


class OctStub(StubVoxelizer):
    """The four octree calls, computed with the reference on the host memory behind the pointers."""

    def octree_build(self, grid_ptr, fmt, strides, dims, level, origin, depth=0, flags=hip.OCT_COLLAPSE):
        self.calls.append(dict(call="build", grid=grid_ptr, fmt=fmt, strides=tuple(strides), dims=tuple(dims), level=level, origin=tuple(origin),
                               depth=depth, flags=flags))
        if fmt == hip.GRID_F32_BELOW:
            g = _strided(grid_ptr, C.c_float, tuple(dims), tuple(strides)) < level
        else:
            assert fmt == hip.GRID_U8
            g = _strided(grid_ptr, C.c_uint8, tuple(dims), tuple(strides)) != 0
        self.tree = t = R.build(g, tuple(origin), depth or None, bool(flags & hip.OCT_COLLAPSE))
        return t["depth"], tuple(t["level_counts"]), len(t["valid"]), t["voxels_listed"]

    def octree_write(self, valid_ptr, full_ptr, first_child_ptr, coords_ptr=None):
        self.calls.append(dict(call="write", coords=coords_ptr))
        t, n = self.tree, len(self.tree["valid"])
        _array(valid_ptr, C.c_uint8, n)[:] = t["valid"]
        _array(full_ptr, C.c_uint8, n)[:] = t["full"]
        _array(first_child_ptr, C.c_int32, n)[:] = t["first_child"]
        if coords_ptr is not None:
            _array(coords_ptr, C.c_int32, 3 * n)[:] = t["coords"].reshape(-1)

    def _tree(self, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags):
        return dict(valid=_array(valid_ptr, C.c_uint8, n_nodes), full=_array(full_ptr, C.c_uint8, n_nodes), first_child=_array(first_child_ptr, C.c_int32, n_nodes),
                    depth=depth, collapsed=bool(flags & hip.OCT_COLLAPSE))

    def octree_lookup(self, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags, points_ptr, n, out_ptr):
        self.calls.append(dict(call="lookup", n_nodes=n_nodes, depth=depth, flags=flags, n=n))
        t = self._tree(valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags)
        _array(out_ptr, C.c_int32, 4 * n)[:] = R.lookup(t, _array(points_ptr, C.c_int32, 3 * n).reshape(-1, 3)).reshape(-1)

    def octree_to_dense(self, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags, origin, dims, out_ptr, out_strides):
        self.calls.append(dict(call="to_dense", origin=tuple(origin), dims=tuple(dims), strides=tuple(out_strides), flags=flags))
        t = self._tree(valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags)
        _strided(out_ptr, C.c_uint8, tuple(dims), tuple(out_strides))[...] = R.to_dense(t, tuple(dims)[::-1], tuple(origin))


def as_ref(tree):
    """an Octree as the reference's dict"""
    offs = tree.level_offsets
    return dict(valid=tree.valid.numpy(), full=tree.full.numpy(), first_child=tree.first_child.numpy(),
                coords=None if tree.coords is None else tree.coords.numpy(), level_counts=[b - a for a, b in zip(offs, offs[1:])],
                voxels_listed=tree.voxels_listed, depth=tree.depth, collapsed=tree.collapsed)


def test_build_octree_through_the_stub(on_cpu):  # noqa: F811
    dv = OctStub()
    rng = np.random.default_rng(36)
    g = R.blobs(rng, (11, 6, 5), 0.6)
    for kind in ("bool", "uint8", "float32", "sliced"):
        for collapse in (True, False):
            t = {"bool": torch.from_numpy(g), "uint8": torch.from_numpy(g.astype(np.uint8) * 7), "float32": torch.from_numpy(np.where(g, -1.0, 1.0).astype(np.float32)),
                 "sliced": torch.from_numpy(np.repeat(g, 2, axis=2).copy())[:, :, ::2]}[kind]
            tree = dense.build_octree(dv, t, level=0.0 if kind == "float32" else None, origin=(3, 1, 2), collapse=collapse, coords=True)
            assert isinstance(tree, dense.Octree) and dense.Octree is octree.Octree
            R.same(as_ref(tree), R.build(g, (3, 1, 2), None, collapse), (kind, collapse))
            b = dv.calls[-2]
            assert (b["call"], b["grid"], b["dims"], b["origin"], b["depth"], b["flags"]) == ("build", t.data_ptr(), (11, 6, 5), (3, 1, 2), 0, hip.OCT_COLLAPSE * collapse)
            assert b["strides"] == (t.stride(2), t.stride(1), t.stride(0)) and dv.calls[-1]["call"] == "write" and dv.calls[-1]["coords"] == tree.coords.data_ptr()
            assert tree.collapsed is collapse and tree.depth == 4 and len(tree.level_offsets) == 5 and all(type(v) is int for v in tree.level_offsets)
            assert tree.valid.dtype == tree.full.dtype == torch.uint8 and tree.first_child.dtype == tree.coords.dtype == torch.int32
    tree = dense.build_octree(dv, torch.from_numpy(g), depth=6)
    assert tree.coords is None and dv.calls[-1]["coords"] is None and dv.calls[-2]["depth"] == 6 and tree.depth == 6 and tree.collapsed is True
    with pytest.raises(dataclasses.FrozenInstanceError):
        tree.depth = 3


def test_lookup_and_to_dense_through_the_stub(on_cpu):  # noqa: F811
    dv = OctStub()
    rng = np.random.default_rng(37)
    g = R.blobs(rng, (11, 6, 5), 0.6)
    for collapse in (True, False):
        tree = dense.build_octree(dv, torch.from_numpy(g), origin=(3, 1, 2), collapse=collapse)
        ref = R.build(g, (3, 1, 2), None, collapse)
        pts = torch.from_numpy(box_points(-1, 17).astype(np.int32))
        got = dense.octree_lookup(dv, tree, pts)
        assert got.dtype == torch.int32 and tuple(got.shape) == (len(pts), 4) and np.array_equal(got.numpy(), R.lookup(ref, pts.numpy()))
        assert dv.calls[-1]["flags"] == hip.OCT_COLLAPSE * collapse and dv.calls[-1]["n_nodes"] == len(ref["valid"])
        # any leading shape, any strides
        cube = pts.reshape(18, 18, 18, 3)[1:17:2, :, 3:]
        assert torch.equal(dense.octree_lookup(dv, tree, cube), got.reshape(18, 18, 18, 4)[1:17:2, :, 3:])
        n_calls = len(dv.calls)
        assert tuple(dense.octree_lookup(dv, tree, pts[:0]).shape) == (0, 4) and len(dv.calls) == n_calls   # nothing to look up: no call
        back = dense.octree_to_dense(dv, tree, g.shape, origin=(3, 1, 2))
        assert back.dtype == torch.bool and np.array_equal(back.numpy(), g)
        wide = torch.zeros((12, 13, 40), dtype=torch.uint8)
        out = dense.octree_to_dense(dv, tree, (12, 13, 20), origin=(1, 0, 0), out=wide[:, :, ::2])
        assert out.data_ptr() == wide.data_ptr() and dv.calls[-1]["strides"] == (2, 40, 520) and dv.calls[-1]["dims"] == (20, 13, 12)
        assert np.array_equal(out.numpy() != 0, R.to_dense(ref, (12, 13, 20), (1, 0, 0))) and not wide[:, :, 1::2].any()


def test_the_wait_comes_before_every_library_call(monkeypatch):
    dv = OctStub()
    order = []
    monkeypatch.setattr(dense, "_device", lambda dv: torch.device("cpu"))
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: True)
    monkeypatch.setattr(dense, "_sync", lambda device: order.append("sync"))
    for name in ("octree_build", "octree_write", "octree_lookup", "octree_to_dense"):
        monkeypatch.setattr(dv, name, (lambda real, name: lambda *a, **kw: order.append(name) or real(*a, **kw))(getattr(dv, name), name))
    tree = dense.build_octree(dv, torch.ones((4, 4, 4), dtype=torch.bool), collapse=False)
    assert order == ["sync", "octree_build", "octree_write"]
    del order[:]
    dense.octree_lookup(dv, tree, torch.zeros((5, 3), dtype=torch.int32))
    dense.octree_to_dense(dv, tree, (4, 4, 4))
    assert order == ["sync", "octree_lookup", "sync", "octree_to_dense"]


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
    ((_B,), dict(origin=(0, 0)), ValueError),
    ((_B,), dict(origin=(0, -1, 0)), ValueError),
    ((_B,), dict(origin=(65533, 0, 0)), ValueError),                               # origin + extent above 65 536
    ((_B,), dict(depth=0), ValueError),
    ((_B,), dict(depth=17), ValueError),
    ((_B,), dict(depth=True), ValueError),
    ((_B,), dict(depth=2.0), ValueError),
    ((_B,), dict(depth=1), ValueError),                                            # 4 voxels do not fit 2^1
    ((_B,), dict(origin=(1, 0, 0), depth=2), ValueError),
    ((_B,), dict(collapse=1), ValueError),
    ((_B,), dict(coords=None), ValueError),
])
def test_build_octree_rejects_before_any_device_call(on_cpu, args, kw, exc):  # noqa: F811
    dv = OctStub()
    with pytest.raises(exc):
        dense.build_octree(dv, *args, **kw)
    assert not dv.calls


def test_the_queries_reject_before_any_device_call(on_cpu):  # noqa: F811
    dv = OctStub()
    tree = dense.build_octree(dv, torch.ones((4, 4, 4), dtype=torch.bool), collapse=False)
    del dv.calls[:]
    pts = torch.zeros((5, 3), dtype=torch.int32)
    r = dataclasses.replace
    for bad_tree, exc in ((as_ref(tree), TypeError), (r(tree, valid=tree.valid[:-1]), ValueError), (r(tree, valid=tree.valid.to(torch.int32)), TypeError),
                          (r(tree, first_child=tree.first_child.to(torch.int64)), TypeError), (r(tree, full=tree.full.numpy()), TypeError),
                          (r(tree, valid=tree.valid.repeat_interleave(2)[::2]), TypeError), (r(tree, depth=0), ValueError), (r(tree, depth=17), ValueError),
                          (r(tree, depth=True), ValueError), (r(tree, collapsed=0), ValueError), (r(tree, valid=tree.valid.to("meta")), ValueError),
                          (r(tree, valid=tree.valid[:0], full=tree.full[:0], first_child=tree.first_child[:0]), ValueError)):
        with pytest.raises(exc):
            dense.octree_lookup(dv, bad_tree, pts)
        with pytest.raises(exc):
            dense.octree_to_dense(dv, bad_tree, (4, 4, 4))
    for bad, exc in ((pts.to(torch.int64), TypeError), (pts.float(), TypeError), (pts.numpy(), ValueError), (torch.zeros((5, 4), dtype=torch.int32), ValueError),
                     (torch.zeros((), dtype=torch.int32), ValueError), (pts.to("meta"), ValueError)):
        with pytest.raises(exc):
            dense.octree_lookup(dv, tree, bad)
    for args, kw, exc in ((((4, 4),), {}, ValueError), (((4, 0, 4),), {}, ValueError), (((4, 4, 4),), dict(origin=(0, -1, 0)), ValueError),
                          (((1, 1, 65537),), {}, ValueError), (((2048, 1024, 1024),), {}, ValueError), (((4, 4, 4),), dict(origin=(2 ** 32 - 3, 0, 0)), ValueError),
                          (((4, 4, 4),), dict(out=torch.zeros((4, 4, 5), dtype=torch.bool)), ValueError), (((4, 4, 4),), dict(out=torch.zeros((4, 4, 4))), TypeError),
                          (((4, 4, 4),), dict(out=np.zeros((4, 4, 4), bool)), ValueError), (((4, 4, 4),), dict(out=torch.zeros((4, 4, 4), dtype=torch.bool, device="meta")), ValueError)):
        with pytest.raises(exc):
            dense.octree_to_dense(dv, tree, *args, **kw)
    assert not dv.calls


def test_octree_depth_and_octree_level_on_cpu_tensors(on_cpu):  # noqa: F811
    assert dense.octree_depth((0, 0, 0), (1, 1, 1)) == 1 and dense.octree_depth((0, 0, 0), (2, 2, 2)) == 1 and dense.octree_depth((0, 0, 0), (1, 3, 2)) == 2
    assert dense.octree_depth((1, 3, 5), (7, 6, 5)) == 4 and dense.octree_depth((63, 7, 8), (10, 9, 129)) == 8 and dense.octree_depth((0, 0, 65535), (1, 1, 1)) == 16
    assert dense.octree_depth((0, 0, 0), (1, 65536, 1)) == 16 and dense.octree_depth((1, 1, 1), (1, 1, 1)) == 1 and dense.octree_depth((2, 0, 0), (1, 1, 1)) == 2
    for origin, shape in (((1, 0, 0), (1, 1, 65536)), ((0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1)), ((0, 0, 0), (1, 0, 1)), ((-1, 0, 0), (1, 1, 1))):
        with pytest.raises(ValueError):
            dense.octree_depth(origin, shape)
    for origin, dims in (((0, 0, 0), (1, 1, 1)), ((1, 3, 5), (5, 6, 7)), ((63, 7, 8), (129, 9, 10)), ((0, 0, 0), (64, 64, 64)), ((0, 0, 0), (65, 1, 1))):
        assert dense.octree_depth(origin, dims[::-1]) == R.depth_of(origin, dims)
    dv = OctStub()
    g = R.ball(16, 7.5, 30)
    tree = dense.build_octree(dv, torch.from_numpy(g), collapse=False, coords=True)
    ref = R.build(g, collapse=False)
    off = np.concatenate([[0], np.cumsum(ref["level_counts"])])
    for l in range(tree.depth):   # noqa: E741
        valid, full, first, coords = dense.octree_level(tree, l)
        assert np.array_equal(valid.numpy(), ref["valid"][off[l]:off[l + 1]]) and np.array_equal(full.numpy(), ref["full"][off[l]:off[l + 1]])
        assert np.array_equal(first.numpy(), ref["first_child"][off[l]:off[l + 1]]) and np.array_equal(coords.numpy(), ref["coords"][off[l]:off[l + 1]])
        # the level as occupancy at 1 / 2^(D - l): the cells of the nodes are the non-empty cells
        s = 2 ** (tree.depth - l)
        occ = np.zeros((16 // s,) * 3, bool)
        c = coords.numpy() // s
        occ[c[:, 2], c[:, 1], c[:, 0]] = True
        assert np.array_equal(occ, g.reshape(16 // s, s, 16 // s, s, 16 // s, s).any(axis=(1, 3, 5)))
    assert dense.octree_level(dense.build_octree(dv, torch.from_numpy(g)), 0)[3] is None
    for bad in (-1, tree.depth, True, 1.0, None):
        with pytest.raises(ValueError):
            dense.octree_level(tree, bad)
    with pytest.raises(TypeError):
        dense.octree_level(ref, 0)


def test_the_docstrings_and_constants():
    assert "section 30" in dense.__doc__ and "o2v_hip_octree_build" in dense.__doc__ and "section 30" in dense.build_octree.__doc__
    header = open(os.path.join(os.path.dirname(SRC), "..", "include", "o2v_hip.h")).read()
    assert "O2V_HIP_OCT_COLLAPSE = %du" % hip.OCT_COLLAPSE in header and "O2V_HIP_OCT_MAX_DEPTH = %d" % hip.OCT_MAX_DEPTH in header
    for name in ("build", "write", "lookup", "to_dense", "times", "scratch_bytes", "depth"):
        assert "o2v_hip_octree_%s(" % name in header, name
    for name in ("octree_build", "octree_write", "octree_lookup", "octree_to_dense", "octree_times"):
        assert callable(getattr(hip.DeviceVoxelizer, name))
    for name in ("Octree", "build_octree", "octree_lookup", "octree_to_dense", "octree_level", "octree_depth"):
        assert getattr(dense, name) is getattr(octree, name)
    # the scratch question and the depth need no device
    assert hip.octree_depth((1, 3, 5), (5, 6, 7)) == 4 and hip.octree_depth((0, 0, 0), (0, 1, 1)) == 0 and hip.octree_depth((65535, 0, 0), (2, 1, 1)) == 0
    small, deep = hip.octree_scratch_bytes((64, 64, 64)), hip.octree_scratch_bytes((64, 64, 64), (0, 0, 0), 8)
    assert 0 < small < deep < small + 64 and hip.octree_scratch_bytes((64, 64, 64), (0, 0, 0), 5) == 0 == hip.octree_scratch_bytes((64, 64, 64), (0, 0, 0), 17)
    # a 1024 x 400 x 300 box does not pay for 1024^3: the pyramid stays below 3/8 byte per voxel
    plan = hip.octree_scratch_bytes((1024, 400, 300))
    assert plan < (1 / 8 + 2 / 7 * 1.02 + 18 / 7 * 1.02) * 1024 * 400 * 300 + 4096


# ---- the code object ---------------------------------------------------------------------------------------------------------------

K26_KERNELS = ["k_oct_leavesE", "k_oct_upE", "k_oct_rootE", "k_oct_countE", "k_oct_childrenE", "k_oct_lookupE", "k_oct_denseE"]
SCAN_LDS = 4 * 8   # fill_block_exscan64's word per wavefront: the only LDS of K26 (the kernel's comment)


@pytest.mark.parametrize("kernel", K26_KERNELS)
def test_k26_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    """From the code object's metadata only: wave64, at most 256 threads, no private segment, no LDS but the block scan's."""
    meta = device_asm[device_asm.index("amdhsa.kernels:"):]
    entry = [e for e in meta.split("\n  - ") if re.search(r"\.name: +_ZN\S*" + kernel + r"\S*\n", e)]
    assert len(entry) == 1, kernel + " is not in the gfx950 code object"
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
    assert int(re.search(r"\.wavefront_size: +(\d+)", entry[0]).group(1)) == 64
    assert int(re.search(r"\.max_flat_workgroup_size: +(\d+)", entry[0]).group(1)) == (1024 if "root" in kernel else 256)
    lds = int(re.search(r"\.group_segment_fixed_size: +(\d+)", entry[0]).group(1))
    assert lds == (SCAN_LDS if "count" in kernel else 0)
