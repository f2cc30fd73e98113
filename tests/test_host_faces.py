"""Blocky meshes without a GPU: the numpy reference against a scalar restatement of the header, known
answers and invariants of the contract, the mask algebra, run-length walk and corner layout of o2v_dev_k14_faces.hpp compiled for
the host, dense.voxel_faces / count_faces with the device calls stubbed, the mesh files of dense.save_mesh, and a static check of
the K14 kernels in the gfx950 code object."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import bits_host
from tests import faces_ref as FR
from tests import fill_ref
from tests import gather_ref as GR

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401

K14 = os.path.join(SRC, "o2v_dev_k14_faces.hpp")
F = np.float32


# ---- the reference against the header, restated with loops -------------------------------------------------------------------------

def small_grids():
    """(name, grid, format, level): the four tensor formats over four shapes, with NaN, -inf and values equal to the level."""
    rng = np.random.default_rng(14)
    for dims in ((5, 4, 3), (33, 2, 2), (1, 7, 1), (64, 1, 2)):
        shape = dims[::-1]
        solid = rng.random(shape) < 0.55
        yield "u8", np.where(solid, rng.integers(1, 4, shape), 0).astype(np.uint8), FR.U8, None
        yield "bool", solid, FR.U8, None
        yield "bits", rng.integers(-2 ** 31, 2 ** 31, (shape[0], shape[1], -(-shape[2] // 32)), dtype=np.int64).astype(np.int32), FR.BITS, None
        f = rng.normal(size=shape).astype(F)
        f[rng.random(shape) < 0.2] = np.nan
        f[rng.random(shape) < 0.1] = -np.inf
        f[rng.random(shape) < 0.1] = 0.5
        yield "f32", f, FR.F32_BELOW, 0.5


def color_modes(rng, grid, fmt, level):
    shape = FR.solid(grid, fmt, level).shape
    yield dict(argb=0x01020304)
    yield dict(colors=rng.integers(-1, 2, shape, dtype=np.int64).astype(np.int32))          # three colours: runs and cuts
    if fmt == FR.U8:
        yield dict(palette=[0, 7, 7, 9] + [int(v) for v in rng.integers(0, 2 ** 32, 252, dtype=np.uint64)])   # 1 and 2 share a colour


def test_reference_against_a_scalar_loop():
    rng = np.random.default_rng(9)
    n = 0
    for name, grid, fmt, level in small_grids():
        for kw in color_modes(rng, grid, fmt, level):
            for merge in (FR.NONE, FR.RUNS):
                got = FR.quads(grid, fmt, level, (7, 65000, 0), merge, **kw)
                want = FR.quads_scalar(grid, fmt, level, (7, 65000, 0), merge, **kw)
                assert got[0].dtype == F and got[1].dtype == np.int32 and got[2].dtype == np.uint32
                for g, w in zip(got, want):
                    assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (name, list(kw), merge)
                n += 1
    assert n == 2 * (8 * 3 + 8 * 2)
    # a NaN and the level itself are not below the level; -inf is
    f = np.array([[[np.nan, 0.5, -np.inf, 0.49999997, np.inf]]], F)
    assert FR.solid(f, FR.F32_BELOW, 0.5).tolist() == [[[False, False, True, True, False]]]
    assert FR.count(f, FR.F32_BELOW, 0.5, FR.NONE) == 10 and FR.count(f, FR.F32_BELOW, 0.5, FR.RUNS) == 6


def ball():
    z, y, x = np.indices((24, 24, 24))
    return (x - 11.5) ** 2 + (y - 11.5) ** 2 + (z - 11.5) ** 2 <= 10.5 ** 2, x


def test_known_answers():
    for (a, b, c), none, runs in (((5, 3, 2), 62, 14), ((65, 2, 3), 662, 16), ((1, 1, 1), 6, 6), ((130, 3, 1), 1046, 10)):
        box = np.ones((c, b, a), np.uint8)
        assert none == 2 * (a * b + b * c + c * a) and runs == 2 * b + 4 * c
        assert FR.count(box, FR.U8, merge=FR.NONE) == none and FR.count(box, FR.U8, merge=FR.RUNS) == runs, (a, b, c)
    z, y, x = np.indices((5, 6, 7))
    checker = (x + y + z) % 2 == 0
    assert FR.count(checker, FR.U8, merge=FR.NONE) == FR.count(checker, FR.U8, merge=FR.RUNS) == 6 * checker.sum()
    B, x = ball()
    assert B.sum() == 4776
    assert FR.count(B, FR.U8, merge=FR.NONE) == 1992 and FR.count(B, FR.U8, merge=FR.RUNS) == 1104
    assert FR.count(B, FR.U8, merge=FR.RUNS, colors=(x >= 12).astype(np.int32)) == 1184
    # colours, not labels: two palette entries with the same word merge
    labels = np.array([[[1, 2, 3, 3]]], np.uint8)
    assert FR.count(labels, FR.U8, merge=FR.RUNS, palette=[0, 5, 5, 6] + [0] * 252) == 2 + 4 * 2
    assert FR.count(labels, FR.U8, merge=FR.RUNS, palette=[0, 5, 6, 7] + [0] * 252) == 2 + 4 * 3


def check_invariants(grid, fmt, level, origin, kw):
    S = FR.solid(grid, fmt, level)
    Cv = FR.voxel_colors(grid, fmt, S, **{k: v for k, v in kw.items()})
    nz, ny, nx = S.shape
    want = FR.unit_faces(S, Cv)
    for merge in (FR.NONE, FR.RUNS):
        p, f, c = FR.quads(grid, fmt, level, origin, merge, **kw)
        assert np.array_equal(FR.rasterize(p, c, origin), want)                       # every exposed face, each exactly once
        assert (np.diff(FR.order_keys(p, (nx, ny, nz), origin)) > 0).all()            # the order key ascends strictly
        d, lo, hi, normals = FR.quad_boxes(p)
        area = (hi - lo + (np.arange(3) == (d >> 1)[:, None])).prod(axis=1)
        axis = np.zeros((len(d), 3))
        axis[np.arange(len(d)), d >> 1] = np.where(d & 1, 1, -1)
        assert np.array_equal(normals[:, 0], axis * area[:, None]) and np.array_equal(normals[:, 1], axis * area[:, None])
        assert np.array_equal(f.reshape(-1, 6), 4 * np.arange(len(d))[:, None] + [0, 1, 2, 0, 2, 3])
        if merge == FR.RUNS:
            # no two quads of one direction and colour are adjacent along the run axis
            run = np.where(d >= 2, 0, 1)
            end = lo.copy()
            end[np.arange(len(d)), run] = hi[np.arange(len(d)), run]
            begins = {(int(k), int(col)) + tuple(v) for k, col, v in zip(d, c, lo.tolist())}
            assert not any((int(k), int(col)) + tuple(v) in begins for k, col, v in zip(d, c, end.tolist()))
        # the mesh is closed: its parity set is the solid set (centres at half-integers, faces at integers)
        G = max(o + n for o, n in zip(origin, (nx, ny, nz)))
        z, y, x = np.nonzero(S)
        keys = np.sort(((x + origin[0]).astype(np.int64) * G + y + origin[1]) * G + z + origin[2])
        assert np.array_equal(fill_ref.parity_keys(p[f], G, 1), keys)


def test_invariants_on_every_grid():
    rng = np.random.default_rng(3)
    for name, grid, fmt, level in small_grids():
        for kw in color_modes(rng, grid, fmt, level):
            check_invariants(grid, fmt, level, (2, 0, 1), kw)
    B, x = ball()
    check_invariants(B, FR.U8, None, (0, 0, 0), dict(colors=(x >= 12).astype(np.int32)))


# ---- the kernel's own algebra on the host ------------------------------------------------------------------------------------------

HOST_FA = r"""
#include <cstdint>
#define O2V_FA_HOST
#define O2V_FA_FN static inline
static inline uint32_t fa_ctz64(uint64_t v) { return (uint32_t) __builtin_ctzll(v); }
%s
// The passes in the kernels' order, an item at a time: starts[item] as k_faces_count and k_faces_write compute them; then for
// every set bit in ascending (item, bit) the run length and the corners as k_faces_write finds them -> pos[12 q ..].  Returns Q.
extern "C" uint64_t fa_host(const unsigned long long *solid, const unsigned long long *same_x, const unsigned long long *same_y, uint32_t nx, uint32_t ny,
                            uint32_t nz, uint32_t merge, uint32_t colored, uint32_t ox, uint32_t oy, uint32_t oz, uint64_t *starts, float *pos,
                            uint64_t capacity)
{
    FaGrid g{};
    g.nx = nx, g.ny = ny, g.nz = nz, g.W = (nx + 63u) / 64u, g.merge = merge, g.colored = colored;
    g.words = (uint64_t) g.W * ny * nz, g.items = 6u * g.words;
    const FaBits b{solid, same_x, same_y};
    uint64_t q = 0;
    for (uint64_t item = 0; item < g.items; ++item) {
        uint32_t d, wx, y, z;
        fa_item_at(g, item, d, wx, y, z);
        const uint64_t s = starts[item] = fa_starts(b, g, d, wx, y, z);
        for (uint32_t bit = 0; bit < 64u; ++bit) {
            if (!(s >> bit & 1u)) continue;
            if (q < capacity) fa_quad(d, ox + wx * 64u + bit, oy + y, oz + z, fa_run_length(b, g, d, wx, y, z, bit), 1u, pos + 12u * q);
            ++q;
        }
    }
    return q;
}
"""


@pytest.fixture(scope="module")
def host_fa(tmp_path_factory):
    """build(defines) -> run(S, Cv, merge, origin) -> (starts uint64 [6 * words], positions float32 [4Q, 3]): the plain C++ part of
    o2v_dev_k14_faces.hpp, compiled for the host behind the plain part of o2v_dev_bits.hpp."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    text = open(K14).read()
    head = text[text.index("constexpr uint32_t kFaMergeNone"):text.index("#ifndef O2V_FA_HOST")]
    part = text[text.index("// ---- words -> exposed faces"):text.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_fa")

    def build(defines=()):
        name = "fa_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_FA % (bits_host.plain_part() + head + part))
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = C.CDLL(str(tmp / (name + ".so")))
        L.fa_host.argtypes = [C.c_void_p] * 3 + [C.c_uint32] * 8 + [C.c_void_p, C.c_void_p, C.c_uint64]
        L.fa_host.restype = C.c_uint64

        def run(S, Cv, merge, origin=(0, 0, 0)):
            nz, ny, nx = S.shape
            solid = GR.words64(S)
            colored = Cv is not None and merge == FR.RUNS
            sx = sy = None
            if colored:
                sx = GR.words64(S & FR.shifted(S, 0, False) & (Cv == FR.shifted(Cv, 0, 0)))
                sy = GR.words64(S & FR.shifted(S, 2, False) & (Cv == FR.shifted(Cv, 2, 0)))
            starts = np.zeros(6 * len(solid), np.uint64)
            args = (solid.ctypes.data, sx.ctypes.data if colored else None, sy.ctypes.data if colored else None, nx, ny, nz, merge, int(colored)) + \
                tuple(origin)
            Q = L.fa_host(*args, starts.ctypes.data, None, 0)
            pos = np.zeros((4 * Q, 3), F)
            assert L.fa_host(*args, starts.ctypes.data, pos.ctypes.data, Q) == Q
            return starts, pos
        return run
    return build


def host_cases():
    """(name, solid [z, y, x], colours or None)"""
    rng = np.random.default_rng(21)
    S = rng.random((3, 4, 200)) < 0.7
    yield "random words", S, None
    yield "random words, random colours", S, rng.integers(0, 2, S.shape).astype(np.uint32)
    yield "full words", np.ones((2, 3, 192), bool), None
    yield "full words, one colour as a grid", np.ones((2, 3, 192), bool), np.full((2, 3, 192), 5, np.uint32)
    S = np.zeros((2, 2, 200), bool)
    S[:, :, 63:129] = True                                                # from bit 63 of word 0 to bit 0 of word 2
    S[1, 1, 127:193] = True                                               # from bit 63 of word 1 to bit 0 of word 3
    yield "runs that begin at bit 63 and end at bit 0", S, None
    Cv = (np.arange(200) >= 64).astype(np.uint32) + (np.arange(200) >= 128) + np.zeros((2, 2, 200), np.uint32)
    yield "a colour change exactly at a word boundary", np.ones((2, 2, 200), bool), Cv
    yield "a row of 1 024 full words", np.ones((1, 1, 65536), bool), None
    yield "tall", rng.random((2, 70, 3)) < 0.8, rng.integers(0, 2, (2, 70, 3)).astype(np.uint32)


def test_masks_runs_and_corners_on_the_host(host_fa):
    run = host_fa()
    for name, S, Cv in host_cases():
        Cr = np.zeros(S.shape, np.uint32) if Cv is None else Cv
        nz, ny, nx = S.shape
        W = -(-nx // 64)
        for merge in (FR.NONE, FR.RUNS):
            q = FR.runs(S, Cr, merge)
            # the six start masks per (row, direction) from the reference's first faces
            want = np.zeros((nz, ny, 6, W * 64), bool)
            want[q[:, 2], q[:, 1], q[:, 3], q[:, 0]] = True
            want = (want.reshape(-1, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
            starts, pos = run(S, Cv, merge, (3, 2, 1))
            assert np.array_equal(starts, want), (name, merge, "start masks differ")
            assert np.array_equal(pos.view(np.uint32), FR.geometry(q, (3, 2, 1))[0].view(np.uint32)), (name, merge)
    full = np.ones((1, 1, 65536), bool)
    assert len(run(full, None, FR.RUNS)[1]) == 4 * 6                      # the x runs cross 1 024 words uncut


def test_the_carry_mutation_is_caught_on_the_host(host_fa):
    """Without the carry from the word before (O2V_FA_MUTATE_NO_CARRY) runs along x are cut at multiples of 64 - and nothing else."""
    run = host_fa(("O2V_FA_MUTATE_NO_CARRY",))
    S = np.ones((1, 2, 130), bool)
    _, pos = run(S, None, FR.RUNS)
    assert len(pos) // 4 == 2 + 6 * 3 and FR.count(S, FR.U8, merge=FR.RUNS) == 2 + 6           # six x runs, in three pieces each
    assert np.array_equal(FR.rasterize(pos, np.zeros(len(pos) // 4, np.uint32)), FR.unit_faces(S, np.zeros(S.shape, np.uint32)))
    S = np.ones((2, 2, 64), bool)                                           # (within one word: the same)
    assert np.array_equal(run(S, None, FR.RUNS)[1], FR.quads(S, FR.U8)[0])


# ---- dense.voxel_faces / count_faces against a stub --------------------------------------------------------------------------------

class FacesStub(StubVoxelizer):
    """faces_count returns the number of quads of `mesh` (positions, faces, argb); faces_write copies them to the addresses it is
    given (the stub's "device" is the host)."""

    def __init__(self, mesh=None, n=None):
        super().__init__()
        self.mesh, self.n_quads = mesh, len(mesh[2]) if n is None else n

    def faces_count(self, *args):
        self.calls.append(("count", args))
        return self.n_quads

    def faces_write(self, *args):
        self.calls.append(("write", args))
        pos, fac, col, cap = args[-4:]
        assert cap == self.n_quads and pos and fac and col
        np.ctypeslib.as_array(C.cast(pos, C.POINTER(C.c_float)), (cap * 4, 3))[:] = self.mesh[0]
        np.ctypeslib.as_array(C.cast(fac, C.POINTER(C.c_int32)), (cap * 2, 3))[:] = self.mesh[1]
        np.ctypeslib.as_array(C.cast(col, C.POINTER(C.c_uint32)), (cap,))[:] = self.mesh[2]


def test_voxel_faces_passes_the_grid_as_it_is():
    rng = np.random.default_rng(2)
    labels = np.where(rng.random((4, 5, 6)) < 0.5, 2, 0).astype(np.uint8)
    mesh = FR.quads(labels, FR.U8, origin=(1, 2, 3), argb=0x80000001)
    dv = FacesStub(mesh)
    wide = torch.zeros((4, 5, 12), dtype=torch.uint8)
    wide[:, :, ::2] = torch.from_numpy(labels)
    p, f, c = dense.voxel_faces(dv, wide[:, :, ::2], origin=(1, 2, 3), argb=0x80000001)
    Q = len(mesh[2])
    assert p.dtype == torch.float32 and tuple(p.shape) == (4 * Q, 3) and p.is_contiguous() and np.array_equal(p.numpy(), mesh[0])
    assert f.dtype == torch.int32 and tuple(f.shape) == (2 * Q, 3) and np.array_equal(f.numpy(), mesh[1])
    assert c.dtype == torch.int32 and tuple(c.shape) == (Q,) and np.array_equal(c.numpy().view(np.uint32), mesh[2])
    (kind, count_args), (_, write_args) = dv.calls
    assert kind == "count" and count_args == (wide.data_ptr(), hip.GRID_U8, (2, 12, 60), (6, 5, 4), 0.0, hip.FACES_MERGE_RUNS,
                                              hip.GATHER_COLOR_CONSTANT, 0x80000001, None, None, None)
    assert write_args[:11] == count_args                                            # the same arguments, so that the count matches
    assert write_args[11:] == ((1, 2, 3), p.data_ptr(), f.data_ptr(), c.data_ptr(), Q)
    # merge; bits and float32 grids; colours as a strided grid, a palette as a list or tensor
    dv = FacesStub(mesh)
    dense.voxel_faces(dv, torch.zeros((2, 3, 2), dtype=torch.int32), merge="none")
    assert dv.calls[0][1][1:6] == (hip.GRID_BITS, (1, 2, 6), (64, 3, 2), 0.0, hip.FACES_MERGE_NONE)
    dv = FacesStub(mesh)
    dense.voxel_faces(dv, torch.zeros((2, 3, 2)), level=0.1)
    assert dv.calls[0][1][1] == hip.GRID_F32_BELOW and dv.calls[0][1][4] == float(F(0.1))
    dv = FacesStub(mesh)
    cgrid = torch.zeros((4, 5, 12), dtype=torch.int32)[:, :, 1::2]
    dense.voxel_faces(dv, torch.from_numpy(labels), colors=cgrid)
    assert dv.calls[1][1][6:10] == (hip.GATHER_COLOR_GRID, 0xFFFFFFFF, cgrid.data_ptr(), (2, 12, 60))
    for palette in (list(range(256)), torch.arange(256), torch.arange(256, dtype=torch.int32) - 128):
        dv = FacesStub(mesh)
        dense.voxel_faces(dv, torch.from_numpy(labels), palette=palette)
        assert dv.calls[1][1][6] == hip.GATHER_COLOR_PALETTE and dv.calls[1][1][10] == [int(v) for v in palette]
    # count_faces: merge "none" unless told otherwise, no write
    dv = FacesStub(mesh)
    assert dense.count_faces(dv, torch.from_numpy(labels)) == Q and dense.count_faces(dv, torch.from_numpy(labels), merge="runs", argb=5) == Q
    assert [k for k, _ in dv.calls] == ["count", "count"] and dv.calls[0][1][5] == hip.FACES_MERGE_NONE
    assert dv.calls[1][1][5:8] == (hip.FACES_MERGE_RUNS, hip.GATHER_COLOR_CONSTANT, 5)
    # no quads: no write call
    dv = FacesStub(n=0)
    p, f, c = dense.voxel_faces(dv, torch.zeros((2, 2, 2), dtype=torch.bool))
    assert (tuple(p.shape), tuple(f.shape), tuple(c.shape)) == ((0, 3), (0, 3), (0,)) and [k for k, _ in dv.calls] == ["count"]
    assert (p.dtype, f.dtype, c.dtype) == (torch.float32, torch.int32, torch.int32)


def test_voxel_faces_transform_maps_back_to_model_space():
    box = np.ones((2, 3, 4), np.uint8)
    mesh = FR.quads(box, FR.U8, origin=(5, 6, 7))
    xf = np.array([3.5, 0.25, 0, 0, -2.0, 0.5, 1.0, 0, 4.0, 10.0, -3.0, 0.75], F)
    model, _, _ = dense.voxel_faces(FacesStub(mesh), torch.from_numpy(box), origin=(5, 6, 7), transform=xf)
    a, t = xf[:9].reshape(3, 3).astype(np.float64), xf[9:].astype(np.float64)
    forward = model.numpy().astype(np.float64) @ a.T + t
    assert model.dtype == torch.float32 and model.is_contiguous() and np.abs(forward - mesh[0]).max() < 1e-4
    with pytest.raises(ValueError, match="12 numbers"):
        dense.voxel_faces(FacesStub(mesh), torch.from_numpy(box), transform=xf[:9])


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
    ((torch.zeros(1, dtype=torch.uint8)[None, None, :].expand(32768, 65536, 1),), {}, ValueError),   # 2^31 words
    ((U8,), {"origin": (0, -1, 0)}, ValueError),
    ((U8,), {"origin": (0, 0)}, ValueError),
    ((U8,), {"origin": (65533, 0, 0)}, ValueError),                                  # origin + extent above 65 536
    ((U8,), {"origin": (0, 0, 65535)}, ValueError),
    ((U8,), {"merge": "greedy"}, ValueError),
    ((U8,), {"merge": 1}, ValueError),
    ((U8,), {"argb": 2 ** 32}, ValueError),
    ((U8,), {"argb": 1.5}, ValueError),
    ((U8,), {"colors": torch.zeros((2, 3, 4), dtype=torch.int32), "palette": list(range(256))}, ValueError),   # both
    ((U8,), {"colors": torch.zeros((2, 3, 5), dtype=torch.int32)}, ValueError),      # another shape
    ((U8,), {"colors": torch.zeros((2, 3, 4), dtype=torch.int64)}, TypeError),
    ((U8,), {"colors": np.zeros((2, 3, 4), np.int32)}, ValueError),
    ((U8,), {"palette": list(range(255))}, ValueError),
    ((U8,), {"palette": [2 ** 32] * 256}, ValueError),
    ((torch.zeros((2, 3, 4)),), {"level": 0.0, "palette": list(range(256))}, ValueError),   # a palette needs a uint8 / bool grid
    ((U8,), {"transform": [1.0] * 9}, ValueError),
])
def test_voxel_faces_rejects(args, kw, exc):
    dv = FacesStub(n=3)
    with pytest.raises(exc):
        dense.voxel_faces(dv, *args, **kw)
    if "origin" not in kw and "transform" not in kw:
        with pytest.raises(exc):
            dense.count_faces(dv, *args, **kw)
    assert not dv.calls                                                              # refused before any device call
    dense.voxel_faces(FacesStub(n=0), U8, origin=(65532, 65533, 65534))              # (origin + extent of exactly 65 536 is taken)


def test_the_index_limit():
    """4 Q must fit an int32: 2^29 - 1 quads are taken (the stub is never asked to write them), 2^29 are refused by name."""
    dv = FacesStub(n=2 ** 29)
    with pytest.raises(ValueError, match="536870912 quads"):
        dense.voxel_faces(dv, U8)
    assert [k for k, _ in dv.calls] == ["count"]
    assert dense.count_faces(FacesStub(n=6442450944), U8) == 6442450944               # (the count itself has no limit)


def test_the_bindings_name_the_library_symbols():
    L = hip._bind()
    for name in ("o2v_hip_faces_count", "o2v_hip_faces_write", "o2v_hip_faces_scratch_bytes", "o2v_hip_faces_times"):
        assert hasattr(L, name), name
    assert (hip.FACES_MERGE_NONE, hip.FACES_MERGE_RUNS, hip.ERR_LIMIT) == (0, 1, 5)
    # 8 bytes per word (24 with a colour grid or palette), 8 per block of 256 items and the count, the palette
    assert hip.faces_scratch_bytes((64, 1, 1)) == 8 + 8 * 2 + 1024
    assert hip.faces_scratch_bytes((65, 40, 40), hip.GATHER_COLOR_GRID) == 24 * 3200 + 8 * 76 + 1024
    assert hip.faces_scratch_bytes((2048, 1024, 1024), hip.GATHER_COLOR_PALETTE) == 24 * 2 ** 25 + 8 * (6 * 2 ** 17 + 1) + 1024
    assert hip.faces_scratch_bytes((0, 4, 4)) == 0


# ---- dense.save_mesh ---------------------------------------------------------------------------------------------------------------

def colored_mesh():
    rng = np.random.default_rng(8)
    labels = np.where(rng.random((3, 4, 5)) < 0.6, rng.integers(1, 4, (3, 4, 5)), 0).astype(np.uint8)
    palette = [0, 0xFF102030, 0x80FFFFFF, 0xFF0000FE] + [0] * 252
    return FR.quads(labels, FR.U8, origin=(2, 0, 1), palette=palette)


def shared_mesh():
    """an extract_surface-shaped mesh: shared vertices, positions that are no integers"""
    p = np.array([[0, 0, 0], [1.25, 0, 0], [0, 1.5, 0], [0, 0, 0.1], [1, 1, 1]], F) * F(1 / 3)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3], [1, 2, 2]], np.int32)            # (the last one is degenerate)
    return p, f


def test_save_mesh_stl(tmp_path):
    for k, (p, f) in enumerate((colored_mesh()[:2], shared_mesh())):
        path = tmp_path / ("m%d.stl" % k)
        dense.save_mesh(path, torch.from_numpy(p), torch.from_numpy(f), argb=None)
        normals, v = FR.parse_stl(path.read_bytes())
        assert np.array_equal(v.view(np.uint32), p[f].view(np.uint32))
        n = np.cross(p[f][:, 1] - p[f][:, 0], p[f][:, 2] - p[f][:, 0]).astype(F)
        length = np.sqrt((n * n).sum(axis=1, dtype=F))
        assert np.allclose(normals[length > 0], n[length > 0] / length[length > 0, None], atol=1e-6) and (normals[length == 0] == 0).all()
        back, _, _ = hip.load_mesh_file(str(path))
        assert np.array_equal(back.view(np.uint32), p[f].reshape(-1, 9).view(np.uint32))       # bit for bit
    assert (FR.parse_stl((tmp_path / "m1.stl").read_bytes())[0][-1] == 0).all()


def test_save_mesh_obj_and_mtl(tmp_path):
    p, f, c = colored_mesh()
    path = tmp_path / "m.obj"
    dense.save_mesh(str(path), torch.from_numpy(p), torch.from_numpy(f), argb=torch.from_numpy(c.view(np.int32)))
    tri = np.repeat(c, 2)
    _, first = np.unique(tri, return_index=True)
    order = np.argsort(np.searchsorted(np.sort(first), first[np.searchsorted(np.unique(tri), tri)]), kind="stable")   # by first appearance
    pp, ff, names, kd = FR.parse_obj(path.read_text(), (tmp_path / "m.mtl").read_text())
    assert np.array_equal(pp.view(np.uint32), p.view(np.uint32)) and np.array_equal(ff, f[order])
    assert names == ["c_%08X" % v for v in tri[order]] and len(kd) == len(np.unique(c)) == 3
    assert [n for i, n in enumerate(names) if i == 0 or names[i - 1] != n] == ["c_%08X" % tri[i] for i in np.sort(first)]
    back, mat, _ = hip.load_mesh_file(str(path))
    assert np.array_equal(back.view(np.uint32), p[f[order]].reshape(-1, 9).view(np.uint32))
    want = np.array([kd[n] for n in names], F)
    assert np.array_equal(mat["colors"], want)                                                 # the Kd written
    rgb = np.stack([tri[order] >> 16 & 255, tri[order] >> 8 & 255, tri[order] & 255], axis=1)
    assert np.abs(want.astype(np.float64) - rgb / 255).max() < 1e-7                             # (nine digits of channel / 255)
    # without colours: no material file; per-vertex colours are refused
    p, f = shared_mesh()
    dense.save_mesh(tmp_path / "s.obj", p, f)
    assert not (tmp_path / "s.mtl").exists()
    back, _, _ = hip.load_mesh_file(str(tmp_path / "s.obj"))
    assert np.array_equal(back.view(np.uint32), p[f].reshape(-1, 9).view(np.uint32))
    with pytest.raises(ValueError, match="per-vertex"):
        dense.save_mesh(tmp_path / "v.obj", p, f[:4], argb=np.arange(5))


def test_save_mesh_ply(tmp_path):
    p, f, c = colored_mesh()
    rgba = np.stack([c >> 16 & 255, c >> 8 & 255, c & 255, c >> 24], axis=1).astype(np.uint8)
    path = tmp_path / "m.ply"
    dense.save_mesh(path, p, f, argb=c)                                                         # per quad
    pp, cc, ff = FR.parse_ply(path.read_bytes())
    assert np.array_equal(pp.view(np.uint32), p.view(np.uint32)) and np.array_equal(ff, f) and np.array_equal(cc, np.repeat(rgba, 4, axis=0))
    dense.save_mesh(path, p, f, argb=np.repeat(c, 2))                                           # per triangle: the same file
    assert np.array_equal(FR.parse_ply(path.read_bytes())[1], cc)
    dense.save_mesh(path, p, f, argb=np.repeat(c, 4).view(np.int32))                            # per vertex
    assert np.array_equal(FR.parse_ply(path.read_bytes())[1], cc)
    dense.save_mesh(tmp_path / "plain.xyz", p, f, fmt="PLY")
    pp, cc, ff = FR.parse_ply((tmp_path / "plain.xyz").read_bytes())
    assert cc is None and np.array_equal(pp, p) and np.array_equal(ff, f)
    # shared vertices: per-vertex colours as they are; triangles of two colours at one vertex get corners of their own
    p, f = shared_mesh()
    dense.save_mesh(path, p, f[:4], argb=np.array([1, 2, 3, 4, 5]) << 8)
    pp, cc, ff = FR.parse_ply(path.read_bytes())
    assert np.array_equal(pp, p) and np.array_equal(ff, f[:4]) and cc[:, 1].tolist() == [1, 2, 3, 4, 5]
    dense.save_mesh(path, p, f[:4], argb=np.array([7, 7, 8, 8]))
    pp, cc, ff = FR.parse_ply(path.read_bytes())
    assert np.array_equal(pp[ff], p[f[:4]]) and cc[ff][:, :, 2].tolist() == [[7] * 3, [7] * 3, [8] * 3, [8] * 3]


def test_save_mesh_rejects(tmp_path):
    p, f = shared_mesh()
    for path, kw, exc in ((tmp_path / "a.vox", {}, ValueError), (tmp_path / "a", {}, ValueError), (tmp_path / "a.stl", {"fmt": "gltf"}, ValueError),
                          (tmp_path / "a.stl", {"fmt": 3}, TypeError), (tmp_path / "a.ply", {"argb": np.zeros(7, np.int32)}, ValueError),
                          (tmp_path / "a.ply", {"argb": np.zeros(5)}, ValueError)):
        with pytest.raises(exc):
            dense.save_mesh(path, p, f, **kw)
        assert not path.exists()
    for bad_p, bad_f in ((p[:, :2], f), (p.astype(np.int32), f), (p, f.astype(F)), (p, f + 3), (p, f[:, :2])):
        with pytest.raises(ValueError):
            dense.save_mesh(tmp_path / "b.stl", bad_p, bad_f)
    dense.save_mesh(tmp_path / "empty.stl", np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    assert len((tmp_path / "empty.stl").read_bytes()) == 84


# ---- the kernels in the code object ------------------------------------------------------------------------------------------------

K14_KERNELS = ["k_faces_sameILj1E", "k_faces_sameILj2E", "k_faces_countE", "k_faces_writeILj0E", "k_faces_writeILj1E", "k_faces_writeILj2E"]


@pytest.mark.parametrize("kernel", K14_KERNELS)
def test_k14_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    name = m.group(1)
    entry = [e for e in device_asm[device_asm.index("amdhsa.kernels:"):].split("\n  - ") if re.search(r"\.name: +" + re.escape(name) + r"\n", e)]
    assert len(entry) == 1
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
