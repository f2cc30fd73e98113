"""Downsampling without a GPU: the vectorised numpy reference against the definition as a scalar loop, known answers, the plain
C++ of o2v_dev_k17_downsample.hpp compiled for the host and run against the reference (and one mutation seen to fail), the
argument checks and the call of obj2voxel_amd.dense.downsample with the device call stubbed, the K17 kernels in the gfx950 code
object, and the link between downsampling and supersampling on the CPU oracle."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests import downsample_ref as D

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip, meshes  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401

K17 = os.path.join(SRC, "o2v_dev_k17_downsample.hpp")


def random_case(rng, dims, density):
    shape = dims[::-1]
    g = np.where(rng.random(shape) < density, rng.choice(np.array([1, 2, 255], np.uint8), shape), 0).astype(np.uint8)
    return g, rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)


def assert_same(a, b, what):
    assert a["corigin"] == b["corigin"], what
    for k in ("count", "solid", "values", "argb"):
        if k in a or k in b:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


# ---- the reference ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f", range(2, 9))
def test_reference_against_a_scalar_loop(f):
    rng = np.random.default_rng(f)
    n = 0
    for dims in ((1, 1, 1), (3, 2, 1), (5, 4, 3), (2 * f + 1, f, f - 1)):
        for density in (0.0, 0.3, 1.0):
            g, c = random_case(rng, dims, density)
            for origin in ((0, 0, 0), (f - 1, 1, 2 * f + 1), tuple(int(v) for v in rng.integers(0, 20, 3))):
                for mc, mode in ((1, D.MIN), (D.majority(f), D.MAX), (f ** 3, D.MIN)):
                    assert_same(D.downsample(g != 0, f, origin, mc, g, mode, c), D.downsample_loop(g != 0, f, origin, mc, g, mode, c),
                                (f, dims, density, origin, mc))
                    n += 1
    assert n == 108


def test_box():
    assert D.box((3, 3, 3), (10, 10, 10), 4) == ((0, 0, 0), (4, 4, 4))
    assert D.box((8, 9, 15), (8, 1, 2), 8) == ((1, 1, 1), (1, 1, 2))
    assert D.box((2 ** 32 - 5, 0, 7), (5, 1, 1), 3) == (((2 ** 32 - 5) // 3, 0, 2), (3, 1, 1))
    L = hip._bind()
    rng = np.random.default_rng(1)
    for _ in range(200):
        f = int(rng.integers(2, 9))
        origin = tuple(int(v) for v in rng.integers(0, 100, 3))
        dims = tuple(int(v) for v in rng.integers(1, 50, 3))
        assert hip.downsample_box(origin, dims, f) == D.box(origin, dims, f)
        corigin, cshape = dense.downsample_box(origin, dims[::-1], f)
        assert (corigin, cshape[::-1]) == D.box(origin, dims, f)
    assert hip.downsample_box((2 ** 32 - 5, 0, 7), (5, 1, 1), 3) == D.box((2 ** 32 - 5, 0, 7), (5, 1, 1), 3)
    u3 = lambda v: (C.c_uint32 * 3)(*v)   # noqa: E731
    out = u3((9, 9, 9)), u3((9, 9, 9))
    for origin, dims, f, code in (((0, 0, 0), (1, 1, 1), 1, 3), ((0, 0, 0), (1, 1, 1), 9, 3), ((0, 0, 0), (1, 0, 1), 2, 3),
                                  ((2 ** 32 - 1, 0, 0), (2, 1, 1), 2, 5)):
        assert L.o2v_hip_downsample_box(u3(origin), u3(dims), f, *out) == code
        assert list(out[0]) == [9, 9, 9] and list(out[1]) == [9, 9, 9]
    assert L.o2v_hip_downsample_box(None, u3((1, 1, 1)), 2, *out) == 3
    for bad in (dict(factor=1), dict(factor=9), dict(factor=2.0), dict(factor=True), dict(shape=(1, 0, 1)), dict(shape=(1, 1)), dict(origin=(0, -1, 0)),
                dict(origin=(2 ** 32 - 1, 0, 0), shape=(1, 1, 2))):
        kw = dict(origin=(0, 0, 0), shape=(4, 4, 4), factor=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            dense.downsample_box(**kw)


def test_known_answer_solid_box():
    """A solid 10^3 box at (3, 3, 3), f = 4: per axis the blocks hold 1, 4, 4 and 1 of its voxels."""
    g = np.ones((10, 10, 10), np.uint8)
    r = D.downsample(g != 0, 4, (3, 3, 3))
    per_axis = np.array([1, 4, 4, 1])
    assert r["corigin"] == (0, 0, 0) and r["count"].shape == (4, 4, 4)
    assert np.array_equal(r["count"], per_axis[:, None, None] * per_axis[None, :, None] * per_axis[None, None, :])
    assert int(r["count"].sum()) == 1000
    assert int(r["solid"].sum()) == 64
    assert int(D.downsample(g != 0, 4, (3, 3, 3), D.majority(4))["solid"].sum()) == 8 and D.majority(4) == 32
    assert int(D.downsample(g != 0, 4, (3, 3, 3), 64)["solid"].sum()) == 8
    assert [D.majority(f) for f in range(2, 9)] == [4, 14, 32, 63, 108, 172, 256]


def test_known_answers_of_the_mean():
    assert D.mean_half_up([0, 1]) == 1 and D.mean_half_up([0, 0, 1]) == 0 and D.mean_half_up([255] * 512) == 255
    assert D.mean_half_up([1, 2, 2]) == 2 and D.mean_half_up([254, 255]) == 255 and D.mean_half_up([0] * 511 + [1]) == 0
    # ... and through the reference, a channel each
    g = np.zeros((2, 2, 2), np.uint8)
    g.reshape(-1)[:3] = 1
    c = np.full((2, 2, 2), 0xffffffff, np.uint32)                        # (garbage where the grid is empty)
    c.reshape(-1)[:3] = [0x00000001, 0x01000100, 0x01010000]
    r = D.downsample(g != 0, 2, colors=c)
    assert r["count"].item() == 3 and r["argb"].item() == 0x01000000      # sums 1, 1, 1 and 2 of three: 0, 0, 0 and 1
    g8 = np.ones((8, 8, 8), np.uint8)
    assert D.downsample(g8 != 0, 8, colors=np.full((8, 8, 8), 0xff80ff01, np.uint32))["argb"].item() == 0xff80ff01
    # values: the smallest / largest non-zero byte, 0 where not solid
    g = np.array([0, 2, 1, 255, 0, 0, 0, 0], np.uint8).reshape(2, 2, 2)
    assert D.downsample(g != 0, 2, grid_u8=g, value_mode=D.MIN)["values"].item() == 1
    assert D.downsample(g != 0, 2, grid_u8=g, value_mode=D.MAX)["values"].item() == 255
    assert D.downsample(g != 0, 2, min_count=4, grid_u8=g, value_mode=D.MAX)["values"].item() == 0


# ---- the kernel's own algebra on the host ------------------------------------------------------------------------------------------

HOST_DS = r"""
#include <cstdint>
#include <stddef.h>
#include <vector>
#define O2V_DS_HOST
#define O2V_DS_FN static inline
static inline uint32_t ds_popc(uint32_t v) { return (uint32_t) __builtin_popcount(v); }
%s
// The box as the harness reads it: a voxel outside it is solid with the byte 255 and a white colour, so that a range that is not
// clipped to the box shows.
struct Box {
    const uint8_t *g;
    const uint32_t *colors;
    uint32_t nx, ny, nz;
    bool in(int64_t x, int64_t y, int64_t z) const { return x >= 0 && y >= 0 && z >= 0 && x < nx && y < ny && z < nz; }
    uint8_t byte(int64_t x, int64_t y, int64_t z) const { return in(x, y, z) ? g[(z * ny + y) * nx + x] : 255; }
    uint32_t color(int64_t x, int64_t y, int64_t z) const { return in(x, y, z) ? colors[(z * ny + y) * nx + x] : 0xffffffffu; }
};
// k_downsample's steps for spans of `span` coarse voxels: the rows of a coarse row as 16-bit chunks from chunk c0 on with a zero
// chunk behind them, then per coarse voxel the clipped range, the fields, their popcounts, the values and the mean colour.
extern "C" void ds_host(const uint8_t *grid, const uint32_t *colors, const uint32_t *dims, const uint32_t *origin, uint32_t f, uint32_t min_count,
                        uint32_t mode, uint32_t span, int16_t *count, uint8_t *solid, uint8_t *values, uint32_t *argb)
{
    const Box b{grid, colors, dims[0], dims[1], dims[2]};
    uint32_t cn[3];
    for (int a = 0; a < 3; ++a) cn[a] = ds_cdim(origin[a], dims[a], f);
    for (uint32_t Z = 0; Z < cn[2]; ++Z)
        for (uint32_t Y = 0; Y < cn[1]; ++Y)
            for (uint32_t X0 = 0; X0 < cn[0]; X0 += span) {
                const uint32_t nX = cn[0] - X0 < span ? cn[0] - X0 : span;
                uint32_t ylo, yhi, zlo, zhi, flo, fhi, unused;
                ds_block_range(origin[1], dims[1], f, Y, ylo, yhi);
                ds_block_range(origin[2], dims[2], f, Z, zlo, zhi);
                ds_block_range(origin[0], dims[0], f, X0, flo, unused);
                ds_block_range(origin[0], dims[0], f, X0 + nX - 1u, unused, fhi);
                const uint32_t c0 = flo >> 4, nc = ((fhi + 15u) >> 4) - c0;
                const uint32_t nry = yhi - ylo, nr = nry * (zhi - zlo);
                std::vector<uint16_t> rows((size_t) nr * (nc + 1u), 0);
                for (uint32_t r = 0; r < nr; ++r)
                    for (uint32_t c = 0; c < nc; ++c) {
                        uint32_t bits = 0;
                        for (uint32_t i = 0; i < 16u; ++i) bits |= (uint32_t) (b.byte((c0 + c) * 16u + i, ylo + r %% nry, zlo + r / nry) != 0) << i;
                        rows[(size_t) r * (nc + 1u) + c] = (uint16_t) bits;
                    }
                for (uint32_t X = X0; X < X0 + nX; ++X) {
                    uint32_t lo, hi;
                    ds_block_range(origin[0], dims[0], f, X, lo, hi);
                    const uint32_t off = lo - c0 * 16u, width = hi - lo;
                    uint32_t cnt = 0, lowest = 255u, highest = 0u, sum[4] = {0u, 0u, 0u, 0u};
                    for (uint32_t r = 0; r < nr; ++r) {
                        const uint32_t m = ds_field(rows.data() + (size_t) r * (nc + 1u), off, width);
                        cnt += ds_popc(m);
                        for (uint32_t i = 0; i < width; ++i)
                            if (m >> i & 1u) {
                                const uint32_t v = b.byte(lo + i, ylo + r %% nry, zlo + r / nry);
                                lowest = v < lowest ? v : lowest, highest = v > highest ? v : highest;
                                ds_add_argb(sum, b.color(lo + i, ylo + r %% nry, zlo + r / nry));
                            }
                    }
                    const size_t at = ((size_t) Z * cn[1] + Y) * cn[0] + X;
                    const bool is = cnt >= min_count;
                    count[at] = (int16_t) cnt;
                    solid[at] = is;
                    values[at] = (uint8_t) (is ? (mode == kDsValueMin ? lowest : highest) : 0u);
                    argb[at] = is ? ds_mean_argb(sum, cnt) : 0u;
                }
            }
}
"""


@pytest.fixture(scope="module")
def host_ds(tmp_path_factory):
    """build(defines) -> run(grid, colors, origin, f, min_count, mode, span) -> the reference's dict: the plain C++ part of
    o2v_dev_k17_downsample.hpp, compiled for the host."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    k17 = open(K17).read()
    text = k17[k17.index("constexpr uint32_t kDsMinFactor"):k17.index("#ifndef O2V_DS_HOST")] + k17[k17.index("// ---- the coarse box"):k17.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_ds")

    def build(defines=()):
        name = "ds_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_DS % text)
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = C.CDLL(str(tmp / (name + ".so")))
        L.ds_host.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 4 + [C.c_void_p] * 4
        L.ds_host.restype = None

        def run(g, c, origin, f, min_count, mode, span=256):
            nz, ny, nx = g.shape
            corigin, cdims = D.box(origin, (nx, ny, nz), f)
            cshape = cdims[::-1]
            out = dict(count=np.full(cshape, -3, np.int16), solid=np.full(cshape, 7, np.uint8), values=np.full(cshape, 9, np.uint8),
                       argb=np.full(cshape, 5, np.uint32), corigin=corigin)
            g, c = np.ascontiguousarray(g), np.ascontiguousarray(c)
            L.ds_host(g.ctypes.data, c.ctypes.data, (C.c_uint32 * 3)(nx, ny, nz), (C.c_uint32 * 3)(*origin), f, min_count, mode, span,
                      *[out[k].ctypes.data for k in ("count", "solid", "values", "argb")])
            return out
        return run
    return build


def test_every_factor_and_origin_residue_on_the_host(host_ds):
    run = host_ds()
    rng = np.random.default_rng(17)
    n = 0
    for f in range(2, 9):
        g, c = random_case(rng, (2 * f + 3, f + 1, 3), 0.5)
        for oz in range(f):
            for oy in range(f):
                for ox in range(f):
                    origin = (ox + 3 * f, oy, oz + f)
                    mc, mode = 1 + (ox + 2 * oy + 3 * oz) % f ** 3, (ox + oy) % 2
                    assert_same(run(g, c, origin, f, mc, mode, span=3), D.downsample(g != 0, f, origin, mc, g, mode, c), (f, origin))
                    n += 1
        # long rows: fields that straddle chunks, spans that begin anywhere within a chunk, a box narrower than a block
        for dims, origin in (((300, 2, 2), (f + 5, 1, 0)), ((1, 1, 1), (f - 1, f - 1, f - 1)), ((f - 1, 1, 1), (1, 0, 0)), ((77, 3, f + 2), (2 ** 32 - 77, 5, 1))):
            g2, c2 = random_case(rng, dims, 0.6)
            for span in (256, 7):
                assert_same(run(g2, c2, origin, f, 2, D.MAX, span=span), D.downsample(g2 != 0, f, origin, 2, g2, D.MAX, c2), (f, dims, span))
    assert n == sum(f ** 3 for f in range(2, 9))
    # the known answers through the C++
    ones = np.ones((10, 10, 10), np.uint8)
    r = run(ones, np.zeros(ones.shape, np.uint32), (3, 3, 3), 4, 32, D.MIN)
    assert int(r["count"].sum()) == 1000 and int(r["solid"].sum()) == 8
    g = np.ones((8, 8, 8), np.uint8)
    assert run(g, np.full(g.shape, 0xff80ff01, np.uint32), (0, 0, 0), 8, 512, D.MIN)["argb"].item() == 0xff80ff01


def test_the_end_clip_mutation_is_caught_on_the_host(host_ds):
    """Without the clip of a block's end to the box (O2V_DS_MUTATE_NO_END_CLIP) the last block of an axis whose box does not end
    on the lattice reaches past the box; a box that ends on the lattice is the same."""
    run = host_ds(("O2V_DS_MUTATE_NO_END_CLIP",))
    g = np.ones((5, 5, 5), np.uint8)
    c = np.zeros(g.shape, np.uint32)
    want = D.downsample(g != 0, 2, (0, 0, 0), 1, g, D.MIN, c)
    got = run(g, c, (0, 0, 0), 2, 1, D.MIN)
    assert int(want["count"].sum()) == 125 and int(got["count"].sum()) > 125
    assert not np.array_equal(got["count"], want["count"]) and np.array_equal(got["count"][:2, :2, :2], want["count"][:2, :2, :2])
    g = np.ones((4, 6, 8), np.uint8)
    c = np.zeros(g.shape, np.uint32)
    assert_same(run(g, c, (2, 4, 6), 2, 1, D.MIN), D.downsample(g != 0, 2, (2, 4, 6), 1, g, D.MIN, c), "ends on the lattice")


# ---- dense.downsample against a stub ------------------------------------------------------------------------------------------------

class DownStub(StubVoxelizer):
    def downsample(self, grid_ptr, fmt, strides, dims, level, origin, factor, min_count, value_mode=hip.DOWN_VALUE_MIN, colors_ptr=None,
                   color_strides=None, count_ptr=None, count_strides=None, solid_ptr=None, solid_strides=None, values_ptr=None,
                   value_strides=None, argb_ptr=None, argb_strides=None):
        t = lambda v: None if v is None else tuple(v)   # noqa: E731
        self.calls.append(dict(grid=grid_ptr, fmt=fmt, strides=tuple(strides), dims=tuple(dims), level=level, origin=tuple(origin), factor=factor,
                               min_count=min_count, value_mode=value_mode, colors=colors_ptr, color_strides=t(color_strides), count=count_ptr,
                               count_strides=t(count_strides), solid=solid_ptr, solid_strides=t(solid_strides), values=values_ptr,
                               value_strides=t(value_strides), argb=argb_ptr, argb_strides=t(argb_strides)))


def test_downsample_formats_strides_and_the_returned_tuple():
    dv = DownStub()
    lab = torch.zeros((2, 5, 6, 7), dtype=torch.uint8)
    got = dense.downsample(dv, lab[1], 2, origin=(1, 0, 3))
    c = dv.calls[-1]
    assert len(got) == 2 and got[1] == (0, 0, 1) and got[0].dtype == torch.bool and tuple(got[0].shape) == (3, 3, 4) and got[0].is_contiguous()
    assert (c["grid"], c["fmt"], c["strides"], c["dims"], c["origin"], c["factor"], c["min_count"]) == (lab[1].data_ptr(), hip.GRID_U8, (1, 7, 42), (7, 6, 5),
                                                                                                     (1, 0, 3), 2, 1)
    assert c["solid"] == got[0].data_ptr() and c["solid_strides"] == (1, 4, 12)
    assert c["count"] is None and c["values"] is None and c["argb"] is None and c["colors"] is None and c["level"] == 0.0
    # every output, in the fixed order
    colors = torch.zeros((5, 6, 14), dtype=torch.int32)[:, :, ::2]
    solid, n, val, argb, corigin = dense.downsample(dv, lab[0].to(torch.bool), 3, count=True, values="max", colors=colors, reduce="majority")
    c = dv.calls[-1]
    assert (solid.dtype, n.dtype, val.dtype, argb.dtype) == (torch.bool, torch.int16, torch.uint8, torch.int32) and corigin == (0, 0, 0)
    assert all(tuple(t.shape) == (2, 2, 3) for t in (solid, n, val, argb))
    assert (c["solid"], c["count"], c["values"], c["argb"]) == (solid.data_ptr(), n.data_ptr(), val.data_ptr(), argb.data_ptr())
    assert c["value_mode"] == hip.DOWN_VALUE_MAX and c["min_count"] == 14 and c["colors"] == colors.data_ptr() and c["color_strides"] == (2, 14, 84)
    assert c["count_strides"] == c["value_strides"] == c["argb_strides"] == (1, 3, 6)
    # subsets keep the order
    solid, val, corigin = dense.downsample(dv, lab[0], 2, values="min")
    assert val.dtype == torch.uint8 and dv.calls[-1]["value_mode"] == hip.DOWN_VALUE_MIN and dv.calls[-1]["count"] is None
    solid, n, argb, corigin = dense.downsample(dv, lab[0], 2, count=True, colors=torch.zeros((5, 6, 7), dtype=torch.int32))
    assert n.dtype == torch.int16 and argb.dtype == torch.int32 and dv.calls[-1]["values"] is None
    # bits: 32 voxels per word along x; float32 with a level; permuted and sliced outputs; out_count alone asks for the count
    bits = torch.zeros((5, 6, 2), dtype=torch.int32)
    solid, corigin = dense.downsample(dv, bits, 8)
    assert tuple(solid.shape) == (1, 1, 8) and dv.calls[-1]["fmt"] == hip.GRID_BITS and dv.calls[-1]["dims"] == (64, 6, 5)
    obuf, cbuf = torch.zeros((4, 3, 3), dtype=torch.uint8), torch.zeros((2, 3, 3, 4), dtype=torch.int16)
    solid, n, corigin = dense.downsample(dv, torch.zeros((5, 6, 7)), 2, level=0.5, out=obuf.permute(1, 2, 0), out_count=cbuf[1])
    c = dv.calls[-1]
    assert solid.data_ptr() == obuf.data_ptr() and n.data_ptr() == cbuf[1].data_ptr()
    assert (c["fmt"], c["level"], c["solid_strides"], c["count_strides"]) == (hip.GRID_F32_BELOW, 0.5, (9, 1, 3), (1, 4, 12))
    out = torch.zeros((3, 3, 4), dtype=torch.bool)
    assert dense.downsample(dv, lab[0], 2, out=out)[0] is out


@pytest.mark.parametrize("f", range(2, 9))
def test_reduce_becomes_min_count(f):
    dv = DownStub()
    grid = torch.zeros((4, 4, 4), dtype=torch.uint8)
    for reduce, want in (("any", 1), ("majority", -(-f ** 3 // 2)), ("all", f ** 3), (1, 1), (f ** 3, f ** 3), (5, 5)):
        dense.downsample(dv, grid, f, reduce=reduce)
        assert dv.calls[-1]["min_count"] == want and dv.calls[-1]["factor"] == f
    for bad in (0, f ** 3 + 1, "most", 1.0, True, None):
        with pytest.raises(ValueError):
            dense.downsample(dv, grid, f, reduce=bad)
    assert len(dv.calls) == 6


def test_the_wait_comes_before_the_library_call(monkeypatch):
    dv = DownStub()
    order = []
    monkeypatch.setattr(dense, "_sync", lambda device: order.append("sync"))
    monkeypatch.setattr(dv, "downsample", lambda *a, **kw: order.append("downsample"))
    dense.downsample(dv, torch.zeros((4, 4, 4), dtype=torch.uint8), 2, count=True)
    assert order == ["sync", "downsample"]


_U8 = torch.zeros((4, 4, 4), dtype=torch.uint8)
_I32 = torch.zeros((4, 4, 4), dtype=torch.int32)


@pytest.mark.parametrize("args, kw, exc", [
    ((torch.zeros((4, 4, 4), dtype=torch.int64), 2), {}, TypeError),
    ((torch.zeros((4, 4), dtype=torch.uint8), 2), {}, ValueError),
    ((torch.zeros((4, 0, 4), dtype=torch.uint8), 2), {}, ValueError),
    ((torch.zeros((4, 4, 4), device="meta", dtype=torch.uint8), 2), {}, ValueError),
    ((torch.zeros((4, 4, 4)), 2), {}, ValueError),                                        # float32 without a level
    ((_U8, 2), dict(level=0.0), ValueError),
    ((torch.zeros((1, 1, 65537), dtype=torch.uint8), 2), {}, ValueError),
    ((_U8, 1), {}, ValueError),
    ((_U8, 9), {}, ValueError),
    ((_U8, 2.0), {}, ValueError),
    ((_U8, True), {}, ValueError),
    ((_U8, 2), dict(origin=(0, 0)), ValueError),
    ((_U8, 2), dict(origin=(0, -1, 0)), ValueError),
    ((_U8, 2), dict(origin=(2 ** 32 - 3, 0, 0)), ValueError),
    ((_U8, 2), dict(values="mean"), ValueError),
    ((_I32, 2), dict(values="min"), ValueError),                                           # bits have no bytes
    ((torch.zeros((4, 4, 4)), 2), dict(level=0.0, values="max"), ValueError),
    ((_U8, 2), dict(count=1), ValueError),
    ((_U8, 2), dict(colors=torch.zeros((4, 4, 4))), TypeError),
    ((_U8, 2), dict(colors=torch.zeros((4, 4, 5), dtype=torch.int32)), ValueError),
    ((_U8, 2), dict(colors=torch.zeros((4, 4, 4), device="meta", dtype=torch.int32)), ValueError),
    ((_U8, 2), dict(out_colors=torch.zeros((2, 2, 2), dtype=torch.int32)), ValueError),   # without colors
    ((_U8, 2), dict(out_values=torch.zeros((2, 2, 2), dtype=torch.uint8)), ValueError),   # without values
    ((_U8, 2), dict(out=torch.zeros((2, 2, 2))), TypeError),
    ((_U8, 2), dict(out=torch.zeros((2, 2, 3), dtype=torch.bool)), ValueError),
    ((_U8, 2), dict(out=torch.zeros((4, 4, 4), dtype=torch.bool)), ValueError),            # the fine shape
    ((_U8, 2), dict(origin=(1, 0, 0), out=torch.zeros((2, 2, 2), dtype=torch.bool)), ValueError),   # the coarse box is 3 wide
    ((_U8, 2), dict(out_count=torch.zeros((2, 2, 2), dtype=torch.int32)), TypeError),
    ((_U8, 2), dict(out_count=torch.zeros((2, 2), dtype=torch.int16)), ValueError),
    ((_U8, 2), dict(values="min", out_values=torch.zeros((2, 2, 2), dtype=torch.bool)), TypeError),
    ((_U8, 2), dict(colors=_I32, out_colors=torch.zeros((2, 2, 2), dtype=torch.uint8)), TypeError),
    ((_U8, 2), dict(colors=_I32, out_colors=torch.zeros((2, 2, 2), device="meta", dtype=torch.int32)), ValueError),
])
def test_rejects_before_any_device_call(args, kw, exc):
    dv = DownStub()
    with pytest.raises(exc):
        dense.downsample(dv, *args, **kw)
    assert not dv.calls


def test_the_docstring_names_the_coverage_and_the_chain():
    doc = " ".join(dense.downsample.__doc__.split())
    assert "count.float() / factor ** 3" in doc and "any of any" in doc and "mean of means, not the mean" in doc


# ---- the kernels in the code object ------------------------------------------------------------------------------------------------

K17_KERNELS = ["k_downsampleILj0ELb0E", "k_downsampleILj0ELb1E", "k_downsampleILj1ELb0E", "k_downsampleILj2ELb0E", "k_downsampleILj2ELb1E"]


@pytest.mark.parametrize("kernel", K17_KERNELS)
def test_k17_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    name, body = m.group(1), m.group(2)
    entry = [e for e in device_asm[device_asm.index("amdhsa.kernels:"):].split("\n  - ") if re.search(r"\.name: +" + re.escape(name) + r"\n", e)]
    assert len(entry) == 1
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
    assert "scratch_" not in body and "atomic" not in body
    if kernel.endswith("Lb1E"):
        assert "global_load_dwordx4" in body   # the 16-byte loads of the aligned rows


# ---- downsampling and supersampling on the CPU oracle --------------------------------------------------------------------------------

@pytest.mark.parametrize("R, voxels, fine_voxels", [(16, 1160, 4664), (21, 1994, 8024)])
def test_supersampling_2_is_the_block_any_of_twice_the_resolution(R, voxels, fine_voxels):
    verts = meshes.uv_sphere(12)

    def occupancy(res, ss):
        vox = oracle.voxelize(verts, res, supersampling=ss)
        xyz = np.asarray(vox)[:, :3].astype(np.int64)
        occ = np.zeros((res, res, res), bool)
        occ[xyz[:, 2], xyz[:, 1], xyz[:, 0]] = True
        return occ

    coarse, fine = occupancy(R, 2), occupancy(2 * R, 1)
    assert int(coarse.sum()) == voxels and int(fine.sum()) == fine_voxels
    assert np.array_equal(D.downsample(fine, 2)["solid"] != 0, coarse)
    # ... and from the fine grid's own box, put back by the coarse origin
    z, y, x = np.nonzero(fine)
    o = (int(x.min()), int(y.min()), int(z.min()))
    tight = fine[o[2]:z.max() + 1, o[1]:y.max() + 1, o[0]:x.max() + 1]
    r = D.downsample(tight, 2, o)
    assert np.array_equal(D.place(r["solid"] != 0, r["corigin"], (R, R, R), False), coarse)
