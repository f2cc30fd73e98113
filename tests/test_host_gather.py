"""Dense grids as voxel lists without a GPU: the numpy reference against a scalar restatement of the
header, the argument checks and range arithmetic of dense.to_voxels / count_voxels / save_voxels with the device calls stubbed,
from_voxels on CPU tensors, the slot -> block -> word -> bit mapping of o2v_dev_k13_gather.hpp compiled for the host, and a static
check of the K13 kernels in the gfx950 code object."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import gather_ref as GR

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401

K13 = os.path.join(SRC, "o2v_dev_k13_gather.hpp")
CPU = torch.device("cpu")


# ---- the reference against the header, restated with loops -------------------------------------------------------------------------

def small_grids():
    rng = np.random.default_rng(4)
    for dims in ((5, 4, 3), (33, 2, 2), (1, 7, 1), (64, 1, 2)):
        shape = dims[::-1]
        solid = rng.random(shape) < 0.4
        yield "u8", np.where(solid, rng.integers(1, 256, shape), 0).astype(np.uint8), GR.U8, None
        yield "bool", solid, GR.U8, None
        yield "bits", rng.integers(-2 ** 31, 2 ** 31, (shape[0], shape[1], -(-shape[2] // 32)), dtype=np.int64).astype(np.int32), GR.BITS, None
        f = rng.normal(size=shape).astype(np.float32)
        f[rng.random(shape) < 0.2] = np.nan
        f[rng.random(shape) < 0.1] = -np.inf
        f[rng.random(shape) < 0.1] = 0.5
        yield "f32", f, GR.F32_BELOW, 0.5


def test_reference_against_a_scalar_loop():
    rng = np.random.default_rng(9)
    palette = rng.integers(0, 2 ** 32, 256, dtype=np.uint64)
    n = 0
    for name, grid, fmt, level in small_grids():
        shape = GR.solid(grid, fmt, level).shape
        colors = rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
        for kw in (dict(argb=0x01020304), dict(colors=colors), dict(palette=palette)):
            if "palette" in kw and fmt != GR.U8:
                continue
            got = GR.records(grid, fmt, level, (7, 2 ** 31, 0), **kw)
            want = GR.records_scalar(grid, fmt, level, (7, 2 ** 31, 0), **kw)
            assert got.dtype == np.uint32 and np.array_equal(got, want), (name, list(kw))
            n += 1
        z, y, x = np.nonzero(GR.solid(grid, fmt, level))     # the order of numpy.nonzero on [z, y, x]
        assert np.array_equal(GR.records(grid, fmt, level)[:, :3], np.stack([x, y, z], axis=1).astype(np.uint32))
    assert n == 4 * 8 + 2 * 4
    # a NaN and the level itself are not below the level; -inf is
    f = np.array([[[np.nan, 0.5, -np.inf, 0.49999997, np.inf]]], np.float32)
    assert GR.records(f, GR.F32_BELOW, 0.5)[:, 0].tolist() == [2, 3]
    i = np.array([0, 2047, 2048, 2 ** 22 - 1, 2 ** 22, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 2 ** 22 - 1], np.uint64)
    assert GR.closed_form_expanded_row(i, 2048, 2048)[:, :3].tolist() == [[0, 0, 0], [2047, 0, 0], [0, 1, 0], [2047, 2047, 0], [0, 0, 1],
                                                                           [2047, 2047, 1023], [0, 0, 1024], [2047, 2047, 1024]]


def test_parsers_round_trip():
    rec = np.array([[1, 2, 3, 0xFF102030], [70000, 0, 5, 0xFFFFFFFF], [0, 0, 0, 0xFF000000]], np.uint32)
    assert np.array_equal(GR.parse_vl32(rec.astype(">u4").tobytes()), rec)
    header = ("ply\nformat binary_big_endian 1.0\nelement vertex 3\n").ljust(289) + "end_header\n"
    assert np.array_equal(GR.parse_ply(header.encode() + rec.astype(">u4").tobytes()), rec)
    text = "".join("%d %d %d %d %d %d\n" % (x, y, z, c >> 16 & 255, c >> 8 & 255, c & 255) for x, y, z, c in rec.tolist())
    assert np.array_equal(GR.parse_xyzrgb(text.encode()), rec)
    assert np.array_equal(GR.as_set(rec)[:, :3], [[0, 0, 0], [1, 2, 3], [70000, 0, 5]])


# ---- dense.to_voxels / count_voxels / save_voxels against a stub -------------------------------------------------------------------

class GatherStub(StubVoxelizer):
    """gather_count returns len(records); gather_write copies records[first : first + n] to the address it is given."""

    def __init__(self, records):
        super().__init__()
        self.records = np.ascontiguousarray(records, np.uint32).reshape(-1, 4)

    def gather_count(self, *args):
        self.calls.append(("count", args))
        return len(self.records)

    def gather_write(self, *args):
        self.calls.append(("write", args))
        first, n, ptr = args[-3:]
        assert n > 0 and ptr
        np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint32)), (n, 4))[:] = self.records[first:first + n]

    def gather_save(self, *args):
        self.calls.append(("save", args))
        return len(self.records)


def test_to_voxels_passes_the_grid_as_it_is():
    rng = np.random.default_rng(2)
    labels = np.where(rng.random((4, 5, 6)) < 0.5, 2, 0).astype(np.uint8)
    rec = GR.records(labels, GR.U8, origin=(1, 2, 3), argb=0x80000001)
    dv = GatherStub(rec)
    wide = torch.zeros((4, 5, 12), dtype=torch.uint8)
    wide[:, :, ::2] = torch.from_numpy(labels)
    out = dense.to_voxels(dv, wide[:, :, ::2], origin=(1, 2, 3), argb=0x80000001)
    assert out.dtype == torch.int32 and tuple(out.shape) == (len(rec), 4) and np.array_equal(out.numpy().view(np.uint32), rec)
    (kind, count_args), (_, write_args) = dv.calls
    assert kind == "count" and count_args == (wide.data_ptr(), hip.GRID_U8, (2, 12, 60), (6, 5, 4), 0.0)
    assert write_args[:5] == count_args                                             # the same grid, so that the count matches
    assert write_args[5:11] == ((1, 2, 3), hip.GATHER_COLOR_CONSTANT, 0x80000001, None, None, None)
    assert write_args[11:13] == (0, len(rec)) and write_args[13] == out.data_ptr()
    # an int32 grid is bits: 32 voxels per word along x; a float32 grid takes its level as a float32
    dv = GatherStub(rec)
    dense.to_voxels(dv, torch.zeros((2, 3, 2), dtype=torch.int32))
    assert dv.calls[0][1][1:4] == (hip.GRID_BITS, (1, 2, 6), (64, 3, 2))
    dv = GatherStub(rec)
    dense.to_voxels(dv, torch.zeros((2, 3, 2)), level=0.1)
    assert dv.calls[0][1][1] == hip.GRID_F32_BELOW and dv.calls[0][1][4] == float(np.float32(0.1))
    # colours: a strided int32 grid of the voxel shape; a palette as a list or a tensor
    dv = GatherStub(rec)
    cgrid = torch.zeros((4, 5, 12), dtype=torch.int32)[:, :, 1::2]
    dense.to_voxels(dv, torch.from_numpy(labels), colors=cgrid)
    assert dv.calls[1][1][6:10] == (hip.GATHER_COLOR_GRID, 0xFFFFFFFF, cgrid.data_ptr(), (2, 12, 60))
    for palette in (list(range(256)), torch.arange(256), torch.arange(256, dtype=torch.int32) - 128):
        dv = GatherStub(rec)
        dense.to_voxels(dv, torch.from_numpy(labels), palette=palette)
        assert dv.calls[1][1][6] == hip.GATHER_COLOR_PALETTE and dv.calls[1][1][10] == [int(v) for v in palette]


def test_to_voxels_ranges():
    rec = np.arange(40, dtype=np.uint32).reshape(10, 4)
    grid = torch.ones((1, 2, 5), dtype=torch.bool)
    for first, count, want in ((0, None, rec), (3, None, rec[3:]), (3, 4, rec[3:7]), (0, 10, rec), (9, 1, rec[9:]), (10, None, rec[:0]),
                               (10, 0, rec[:0]), (4, 0, rec[:0])):
        dv = GatherStub(rec)
        out = dense.to_voxels(dv, grid, first=first, count=count)
        assert np.array_equal(out.numpy().view(np.uint32), want), (first, count)
        assert [c[0] for c in dv.calls] == (["count", "write"] if len(want) else ["count"])    # n = 0: no write call
    for first, count in ((11, None), (0, 11), (10, 1), (5, 6)):
        with pytest.raises(ValueError, match="reach past"):
            dense.to_voxels(GatherStub(rec), grid, first=first, count=count)
    assert dense.count_voxels(GatherStub(rec), grid) == 10
    dv = GatherStub(rec[:0])
    out = dense.to_voxels(dv, grid)
    assert tuple(out.shape) == (0, 4) and out.dtype == torch.int32 and [c[0] for c in dv.calls] == ["count"]


U8 = torch.zeros((2, 3, 4), dtype=torch.uint8)


@pytest.mark.parametrize("args, kw, exc", [
    ((np.zeros((2, 3, 4), np.uint8),), {}, ValueError),                              # not a tensor
    ((torch.zeros((3, 4), dtype=torch.uint8),), {}, ValueError),                     # not 3-D
    ((torch.zeros((2, 3, 4), dtype=torch.int64),), {}, TypeError),                   # no grid dtype
    ((torch.zeros((2, 3, 4)),), {}, ValueError),                                     # float32 without a level
    ((torch.zeros((2, 3, 4)),), {"level": float("nan")}, ValueError),
    ((U8,), {"level": 0.0}, ValueError),                                             # a level with a uint8 grid
    ((torch.zeros((2, 0, 4), dtype=torch.uint8),), {}, ValueError),                  # an empty dimension
    ((torch.zeros((2, 3, 8), dtype=torch.int32)[:, :, ::2],), {}, ValueError),       # bits with an x stride of 2
    ((U8.expand(2, 3, 4)[:, :, :1].expand(2, 3, 65537),), {}, ValueError),           # above 65 536 along an axis
    ((U8,), {"origin": (0, -1, 0)}, ValueError),
    ((U8,), {"origin": (0, 0)}, ValueError),
    ((U8,), {"origin": (2 ** 32 - 3, 0, 0)}, ValueError),                            # origin + extent above 2^32
    ((U8,), {"argb": 2 ** 32}, ValueError),
    ((U8,), {"argb": 1.5}, ValueError),
    ((U8,), {"colors": torch.zeros((2, 3, 4), dtype=torch.int32), "palette": list(range(256))}, ValueError),   # both
    ((U8,), {"colors": torch.zeros((2, 3, 5), dtype=torch.int32)}, ValueError),      # another shape
    ((U8,), {"colors": torch.zeros((2, 3, 4), dtype=torch.int64)}, TypeError),
    ((U8,), {"colors": np.zeros((2, 3, 4), np.int32)}, ValueError),
    ((U8,), {"palette": list(range(255))}, ValueError),
    ((U8,), {"palette": [2 ** 32] * 256}, ValueError),
    ((torch.zeros((2, 3, 4)),), {"level": 0.0, "palette": list(range(256))}, ValueError),   # a palette needs a uint8 / bool grid
    ((torch.zeros((2, 3, 1), dtype=torch.int32),), {"palette": list(range(256))}, ValueError),
    ((U8,), {"first": -1}, ValueError),
    ((U8,), {"count": 1.0}, ValueError),
    ((U8,), {"first": True}, ValueError),
])
def test_to_voxels_rejects(args, kw, exc):
    dv = GatherStub(np.zeros((3, 4), np.uint32))
    with pytest.raises(exc):
        dense.to_voxels(dv, *args, **kw)
    assert not dv.calls                                                              # refused before any device call


def test_the_word_limit_replaces_the_voxel_limit():
    # 2048 x 2048 x 1025 voxels are above 2^31 - 1 voxels (components refuses them) and 2^26 + 2^16 words
    big = torch.zeros(2048, dtype=torch.uint8)[None, None, :].expand(1025, 2048, 2048)
    with pytest.raises(ValueError, match="voxels in all"):
        dense.components(GatherStub(np.zeros((0, 4))), big)
    assert dense.count_voxels(GatherStub(np.zeros((5, 4))), big) == 5
    too_many = torch.zeros(1, dtype=torch.uint8)[None, None, :].expand(32768, 65536, 1)      # 2^31 words of one voxel
    with pytest.raises(ValueError, match="words of 64 voxels"):
        dense.count_voxels(GatherStub(np.zeros((5, 4))), too_many)


def test_save_voxels_arguments(tmp_path):
    rec = np.zeros((7, 4), np.uint32)
    dv = GatherStub(rec)
    grid = torch.zeros((4, 5, 6), dtype=torch.uint8)
    path = tmp_path / "a.vox"
    assert dense.save_voxels(dv, grid, path, origin=(10, 0, 1), palette=list(range(256))) == 7
    (kind, a), = dv.calls
    assert kind == "save" and a[:5] == (grid.data_ptr(), hip.GRID_U8, (1, 6, 30), (6, 5, 4), 0.0)
    assert a[5:7] == ((10, 0, 1), hip.GATHER_COLOR_PALETTE) and a[10] == list(range(256))
    assert a[11:] == (path, None, 16)                                                # resolution: max(origin + extent)
    dv = GatherStub(rec)
    dense.save_voxels(dv, grid, str(path), fmt="vl32", resolution=256, argb=-1)
    assert dv.calls[0][1][7] == -1 and dv.calls[0][1][11:] == (str(path), "vl32", 256)
    for kw, exc in (({"resolution": 5}, ValueError), ({"resolution": 15, "origin": (10, 0, 0)}, ValueError), ({"resolution": 2 ** 32}, ValueError),
                    ({"resolution": 16.0}, ValueError), ({"fmt": 3}, TypeError), ({"colors": grid}, TypeError),
                    ({"colors": torch.zeros((4, 5, 6), dtype=torch.int32), "palette": [0] * 256}, ValueError)):
        dv = GatherStub(rec)
        with pytest.raises(exc):
            dense.save_voxels(dv, grid, path, **kw)
        assert not dv.calls


def test_a_failed_save_raises_the_library_message():
    class Failing(GatherStub):
        def gather_save(self, *args):
            raise hip.DeviceError("o2v_hip_gather_save failed with code 6: o2v_hip_gather_save: cannot open \"/nowhere/a.vl32\" for writing")
    with pytest.raises(hip.DeviceError, match="code 6.*cannot open"):
        dense.save_voxels(Failing(np.zeros((1, 4))), U8, "/nowhere/a.vl32")
    assert hip.ERR_IO == 6 and (hip.GATHER_COLOR_CONSTANT, hip.GATHER_COLOR_GRID, hip.GATHER_COLOR_PALETTE) == (0, 1, 2)


def test_the_bindings_name_the_library_symbols():
    L = hip._bind()
    for name in ("o2v_hip_gather_count", "o2v_hip_gather_write", "o2v_hip_gather_save", "o2v_hip_gather_scratch_bytes", "o2v_hip_gather_times"):
        assert hasattr(L, name), name
    # 12 bytes per word, 8 per block of 256 words and the count, the palette and a counter
    assert hip.gather_scratch_bytes((64, 1, 1)) == 12 + 8 * 2 + 1032
    assert hip.gather_scratch_bytes((65, 40, 40)) == 12 * 3200 + 8 * 14 + 1032
    assert hip.gather_scratch_bytes((2048, 2048, 1025)) == 12 * 67174400 + 8 * 262401 + 1032
    assert hip.gather_scratch_bytes((0, 4, 4)) == 0


# ---- from_voxels -------------------------------------------------------------------------------------------------------------------

def test_from_voxels_round_trips():
    rng = np.random.default_rng(6)
    for dims, origin in (((9, 7, 5), (0, 0, 0)), ((33, 2, 3), (5, 6, 7)), ((1, 1, 1), (2 ** 31, 0, 2 ** 32 - 1))):
        shape = dims[::-1]
        solid = rng.random(shape) < 0.4
        colors = rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
        rec = GR.records(solid, GR.U8, origin=origin, colors=colors)
        for records in (torch.from_numpy(rec.view(np.int32)), torch.from_numpy(rec.astype(np.int64))):
            got = dense.from_voxels(records, shape, origin=origin)
            assert got.dtype == torch.bool and np.array_equal(got.numpy(), solid)
            got = dense.from_voxels(records, shape, origin=origin, fmt="labels")
            assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), solid.astype(np.uint8))
            got = dense.from_voxels(records, shape, origin=origin, fmt="argb")
            assert got.dtype == torch.int32 and np.array_equal(got.numpy(), np.where(solid, colors, 0))
        # through the stub: from_voxels(to_voxels(g), g.shape) == (g != 0)
        g = torch.from_numpy(solid.astype(np.uint8) * 9)
        back = dense.from_voxels(dense.to_voxels(GatherStub(GR.records(g.numpy(), GR.U8)), g), g.shape)
        assert bool((back == (g != 0)).all())
    empty = dense.from_voxels(torch.zeros((0, 4), dtype=torch.int32), (2, 3, 4))
    assert tuple(empty.shape) == (2, 3, 4) and not bool(empty.any())


@pytest.mark.parametrize("rec, shape, origin", [
    ([[4, 0, 0, 1]], (2, 3, 4), (0, 0, 0)),          # x = nx
    ([[0, 3, 0, 1]], (2, 3, 4), (0, 0, 0)),
    ([[0, 0, 2, 1]], (2, 3, 4), (0, 0, 0)),
    ([[0, 0, 0, 1]], (2, 3, 4), (1, 0, 0)),          # below the origin
    ([[1, 1, 1, 1], [5, 6, 9, 1]], (2, 3, 4), (1, 1, 1)),
    ([[-1, 0, 0, 1]], (2, 3, 4), (0, 0, 0)),         # int32 bits of 2^32 - 1
])
def test_from_voxels_refuses_records_outside_the_box(rec, shape, origin):
    with pytest.raises(ValueError, match="outside the box"):
        dense.from_voxels(torch.tensor(rec, dtype=torch.int32), shape, origin=origin)


def test_from_voxels_rejects():
    ok = torch.zeros((1, 4), dtype=torch.int32)
    for records, shape, kw in ((ok, (2, 3, 4), {"fmt": "bits"}), (ok.reshape(4), (2, 3, 4), {}), (ok.to(torch.float32), (2, 3, 4), {}),
                               (ok, (2, 3), {}), (ok, (2, 0, 4), {}), (ok, (2, 3, 4), {"origin": (0, -1, 0)}), (np.zeros((1, 4), np.int32), (2, 3, 4), {})):
        with pytest.raises(ValueError):
            dense.from_voxels(records, shape, **kw)


# ---- the kernel's own mapping on the host ------------------------------------------------------------------------------------------

HOST_GA = r"""
#include <cstdint>
#define O2V_GA_HOST
#define O2V_GA_FN static inline
static inline uint32_t ga_popc64(uint64_t v) { return (uint32_t) __builtin_popcountll(v); }
constexpr uint32_t kBlock = 256;
%s
// The passes in the kernels' order, a "lane" at a time.  local / boff as k_gather_count and k_fill_scan_blocks leave them; then
// for every slot of [first, first + n): the block by the rounds of k_gather_find, the word and the bit as k_gather_write finds
// them -> out[2 * i] = word, out[2 * i + 1] = bit.  Returns the rounds of the last search.
extern "C" uint32_t ga_host(const uint64_t *bits, uint64_t words, uint64_t first, uint64_t n, uint32_t *local, unsigned long long *boff, uint64_t *out)
{
    const uint64_t n_blocks = (words + kBlock - 1) / kBlock;
    uint64_t run = 0;
    for (uint64_t b = 0; b < n_blocks; ++b) {
        boff[b] = run;
        uint32_t in_block = 0;
        for (uint64_t wi = b * kBlock; wi < words && wi < (b + 1) * kBlock; ++wi) {
            local[wi] = in_block;
            in_block += ga_popc64(bits[wi]);
        }
        run += in_block;
    }
    boff[n_blocks] = run;
    uint32_t rounds = 0;
    for (uint64_t slot = first; slot < first + n; ++slot) {
        uint64_t lo = 0, hi = n_blocks;
        rounds = 0;
        while (hi - lo > 1u) {
            const uint64_t step = ga_step(lo, hi);
            uint32_t c = 0;
            for (uint32_t t = 0; t < kGaFan; ++t) c += ga_probe_hit(boff, lo, hi, step, t, slot) ? 1u : 0u;
            ga_narrow(lo, hi, step, c);
            ++rounds;
        }
        // (k_gather_write walks on from the block of `first`: a block ends where the next begins)
        uint64_t b = lo;
        while (boff[b + 1] <= slot && b + 1 < n_blocks) ++b;
        const uint32_t cnt = (uint32_t) (boff[b + 1] - boff[b]);
        uint32_t pref[kBlock];
        for (uint32_t l = 0; l < kBlock; ++l) pref[l] = b * kBlock + l < words ? local[b * kBlock + l] : cnt;
        const uint32_t s = (uint32_t) (slot - boff[b]);
        const uint32_t l = ga_find_word(pref, s);
        out[2 * (slot - first)] = b * kBlock + l;
        out[2 * (slot - first) + 1] = ga_select(bits[b * kBlock + l], s - pref[l]);
    }
    return rounds;
}
"""


@pytest.fixture(scope="module")
def host_ga(tmp_path_factory):
    """build(defines) -> slots(words, first, n) -> ((word, bit) int64 [n, 2], rounds): the part of o2v_dev_k13_gather.hpp between
    "slot -> block -> word -> bit" and "kernels", compiled for the host."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    text = open(K13).read()
    head = text[text.index("constexpr uint32_t kGaFan"):text.index("#ifndef O2V_GA_HOST")]
    part = text[text.index("// ---- slot -> block -> word -> bit"):text.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_ga")

    def build(defines=()):
        name = "ga_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_GA % (head + part))
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = C.CDLL(str(tmp / (name + ".so")))
        L.ga_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ga_host.restype = C.c_uint32

        def slots(words, first=0, n=None):
            words = np.ascontiguousarray(words, np.uint64)
            total = int(sum(bin(int(w)).count("1") for w in words))
            n = total - first if n is None else n
            local = np.zeros(len(words), np.uint32)
            boff = np.zeros(-(-len(words) // 256) + 1, np.uint64)
            out = np.zeros((n, 2), np.uint64)
            rounds = L.ga_host(words.ctypes.data, len(words), first, n, local.ctypes.data, boff.ctypes.data, out.ctypes.data)
            assert int(boff[-1]) == total
            return out.astype(np.int64), rounds
        return slots
    return build


def host_words():
    rng = np.random.default_rng(13)
    full, one = np.uint64(2 ** 64 - 1), np.uint64(1)
    yield "random", rng.integers(0, 2 ** 64, 1000, dtype=np.uint64) & rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    yield "words of 0, 1 and 64 bits", rng.choice(np.array([0, 1, 2 ** 63, 2 ** 64 - 1, 1 << 17], np.uint64), 700)
    yield "full", np.full(513, full)
    yield "one word", np.array([0x8000000000000001], np.uint64)
    yield "empty blocks", np.concatenate([np.full(256, full), np.zeros(1024, np.uint64), [one << np.uint64(63)], np.zeros(300, np.uint64), [one]])
    yield "a record at each end of a block", np.concatenate([[one], np.zeros(254, np.uint64), [one << np.uint64(63)]] * 3)
    yield "sparse", np.where(rng.random(70000) < 0.001, one << rng.integers(0, 64, 70000).astype(np.uint64), 0).astype(np.uint64)   # 274 blocks: two rounds


def test_slot_to_word_to_bit_on_the_host(host_ga):
    slots = host_ga()
    for name, words in host_words():
        want = GR.slots_of_words(words)
        got, rounds = slots(words)
        assert np.array_equal(got, want), (name, int((got != want).any(axis=1).sum()), "slots differ")
        assert rounds <= (0 if len(words) <= 256 else 1 if len(words) <= 65536 else 2), (name, rounds)
        # ranges that begin on, before and behind every block boundary
        ends = np.cumsum([bin(int(w)).count("1") for w in words])[255::256]
        for first in sorted({int(f) for e in ends for f in (e - 1, e, e + 1) if 0 <= f < len(want)}):
            got, _ = slots(words, first, min(3, len(want) - first))
            assert np.array_equal(got, want[first:first + 3]), (name, first)


def test_the_search_mutation_is_caught_on_the_host(host_ga):
    """The search taken with slot + 1 (O2V_GA_MUTATE_SEARCH) loses a range that begins at the last record of a block."""
    slots = host_ga(("O2V_GA_MUTATE_SEARCH",))
    words = np.full(513, np.uint64(2 ** 64 - 1))
    want = GR.slots_of_words(words)
    got, _ = slots(words, 256 * 64 - 1, 1)
    assert not np.array_equal(got, want[256 * 64 - 1:256 * 64])
    got, _ = slots(words, 256 * 64, 1)           # (and only there)
    assert np.array_equal(got, want[256 * 64:256 * 64 + 1])


# ---- the kernels in the code object ------------------------------------------------------------------------------------------------

K13_KERNELS = ["k_gather_countE", "k_gather_findE", "k_gather_writeILj0E", "k_gather_writeILj1E", "k_gather_writeILj2E"]


@pytest.mark.parametrize("kernel", K13_KERNELS)
def test_k13_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    name = m.group(1)
    entry = [e for e in device_asm[device_asm.index("amdhsa.kernels:"):].split("\n  - ") if re.search(r"\.name: +" + re.escape(name) + r"\n", e)]
    assert len(entry) == 1
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
