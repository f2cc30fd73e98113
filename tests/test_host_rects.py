"""Rectangles of blocky meshes without a GPU: the numpy reference of O2V_HIP_FACES_MERGE_RECTS against a
scalar restatement of the header, known answers and invariants of the contract, the plain C++ of o2v_dev_k16_rects.hpp (the
stacked test, the height walk, the corners over two extents) compiled for the host behind K14's, one mutation of it,
dense.voxel_faces / count_faces with merge="rects" against a stub, the scratch bound, and a static check of the K16 kernels in
the gfx950 code object."""
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
from tests import rects_ref as RR

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, device_asm, on_cpu  # noqa: E402,F401
from tests.test_host_faces import FacesStub, ball, color_modes, small_grids  # noqa: E402

K14 = os.path.join(SRC, "o2v_dev_k14_faces.hpp")
K16 = os.path.join(SRC, "o2v_dev_k16_rects.hpp")
F = np.float32


# ---- the reference against the header, restated with loops -------------------------------------------------------------------------

def test_reference_against_a_scalar_loop():
    rng = np.random.default_rng(16)
    n = 0
    for name, grid, fmt, level in small_grids():
        for kw in color_modes(rng, grid, fmt, level):
            got = RR.quads(grid, fmt, level, (7, 65000, 0), **kw)
            want = RR.quads_scalar(grid, fmt, level, (7, 65000, 0), **kw)
            assert got[0].dtype == F and got[1].dtype == np.int32 and got[2].dtype == np.uint32
            for g, w in zip(got, want):
                assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (name, list(kw))
            assert RR.count(grid, fmt, level, **kw) == len(want[2])
            n += 1
    assert n == 8 * 3 + 8 * 2
    # walls, where runs do stack: the scalar loop on the grids of the known answers that are small enough for it
    for S, Cv in (wall_grids()[k] for k in ("plate with a hole", "plate of two colours", "L plate", "stairs")):
        kw = {} if Cv is None else dict(colors=Cv.astype(np.int32))
        for g, w in zip(RR.quads(S, FR.U8, None, (1, 2, 3), **kw), RR.quads_scalar(S, FR.U8, None, (1, 2, 3), **kw)):
            assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
    # the other merge modes pass through to faces_ref
    S = wall_grids()["stairs"][0]
    assert RR.count(S, FR.U8, merge=RR.RUNS) == FR.count(S, FR.U8, merge=FR.RUNS) and RR.count(S, FR.U8, merge=RR.NONE) == 328


def wall_grids():
    """name -> (solid [z, y, x], colours or None): the grids of the known answers that have walls."""
    out = {}
    z, y, x = np.indices((8, 8, 8))
    out["stairs"] = (x + z < 8, None)
    P = np.ones((1, 5, 5), bool)
    P[0, 2, 2] = False
    out["plate with a hole"] = (P, None)
    Cv = np.zeros((1, 3, 4), np.uint32)
    Cv[0, 2] = 9
    out["plate of two colours"] = (np.ones((1, 3, 4), bool), Cv)
    H = np.ones((10, 10, 10), bool)
    H[1:-1, 1:-1, 1:-1] = False
    out["hollow box"] = (H, None)
    L = np.zeros((1, 2, 4), bool)
    L[0, 0], L[0, 1, :2] = True, True
    out["L plate"] = (L, None)
    S = np.ones((1, 2, 130), bool)
    S[0, 1, 129] = False
    out["(130, 2, 1) less a voxel"] = (S, None)
    return out


def counts(S, Cv=None):
    kw = {} if Cv is None else dict(colors=Cv.astype(np.int32))
    return tuple(RR.count(S, FR.U8, merge=m, **kw) for m in (RR.NONE, RR.RUNS, RR.RECTS))


def test_known_answers():
    for a, b, c in ((5, 3, 2), (65, 2, 3), (1, 1, 1), (130, 3, 1)):
        assert RR.count(np.ones((c, b, a), np.uint8), FR.U8) == 6, (a, b, c)
    z, y, x = np.indices((5, 6, 7))
    assert counts((x + y + z) % 2 == 0) == (630, 630, 630)
    B, _ = ball()
    z, y, x = np.indices(B.shape)
    assert B.sum() == 4776 and counts(B) == (1992, 1104, 726)
    assert [counts(B, (a >= 12).astype(np.uint32))[2] for a in (x, y, z)] == [786, 778, 770]
    W = wall_grids()
    assert counts(*W["stairs"]) == (328, 104, 34)
    assert counts(*W["plate with a hole"]) == (72, 20, 16)
    assert counts(*W["plate of two colours"]) == (38, 12, 10)
    assert counts(*W["hollow box"]) == (984, 108, 12)
    assert counts(*W["L plate"]) == (24, 10, 10)                     # the +z runs [0, 4) and [0, 2) begin together, and do not stack
    assert counts(*W["(130, 2, 1) less a voxel"]) == (782, 10, 10)   # the rows agree over two words and differ in the third
    # the L plate's +z and -z faces stay a quad per row
    r = RR.rects(*[W["L plate"][0], np.zeros((1, 2, 4), np.uint32)])
    assert sorted(r[r[:, 3] == 5][:, [0, 1, 4, 5]].tolist()) == [[0, 0, 4, 1], [0, 1, 2, 1]]
    # colours, not labels: two palette entries with one word stack, two different words do not
    labels = np.array([[[1, 1, 1], [2, 2, 2]]], np.uint8)
    assert RR.count(labels, FR.U8, palette=[0, 5, 5] + [0] * 253) == 6
    assert RR.count(labels, FR.U8, palette=[0, 5, 6] + [0] * 253) == 10   # +-z and +-x twice, +-y once each
    # nothing is joined across the last row of a layer
    bars = two_bars()
    assert RR.count(bars, FR.U8) == 12


def two_bars():
    """(x 0..3, y = ny - 1, z = 0) and (x 0..3, y = 0, z = 1): neighbours in memory, not in space."""
    S = np.zeros((2, 3, 4), bool)
    S[0, 2, :] = True
    S[1, 0, :] = True
    return S


def check_invariants(grid, fmt, level, origin, kw):
    S = FR.solid(grid, fmt, level)
    Cv = FR.voxel_colors(grid, fmt, S, **kw)
    nz, ny, nx = S.shape
    want = FR.unit_faces(S, Cv)
    p, f, c = RR.quads(grid, fmt, level, origin, **kw)
    pr, _, cr = FR.quads(grid, fmt, level, origin, FR.RUNS, **kw)
    # every exposed face exactly once, with its colour - as the runs cover them
    assert np.array_equal(FR.rasterize(p, c, origin), want) and np.array_equal(FR.rasterize(pr, cr, origin), want)
    # a rectangle is a union of whole runs: no run has faces in two rectangles
    by_rect = FR.rasterize(p, np.arange(len(c)), origin)
    by_run = FR.rasterize(pr, np.arange(len(cr)), origin)
    assert np.array_equal(by_rect[:, :4], by_run[:, :4])
    pairs = np.unique(np.stack([by_run[:, 4], by_rect[:, 4]], axis=1), axis=0)
    assert len(pairs) == len(cr) and len(c) <= len(cr)
    assert (np.diff(FR.order_keys(p, (nx, ny, nz), origin)) > 0).all()                  # the order key ascends strictly
    d, lo, hi, normals = FR.quad_boxes(p)
    area = (hi - lo + (np.arange(3) == (d >> 1)[:, None])).prod(axis=1)
    axis = np.zeros((len(d), 3))
    axis[np.arange(len(d)), d >> 1] = np.where(d & 1, 1, -1)
    assert np.array_equal(normals[:, 0], axis * area[:, None]) and np.array_equal(normals[:, 1], axis * area[:, None])
    assert np.array_equal(f.reshape(-1, 6), 4 * np.arange(len(d))[:, None] + [0, 1, 2, 0, 2, 3])
    # no two rectangles of one direction, plane, colour and extent along the run axis are neighbours along the stack axis
    k = np.arange(len(d))
    above = lo.copy()
    stack = RR.stack_axis(d)
    above[k, stack] = hi[k, stack]
    run = np.where(d >= 2, 0, 1)
    begins = {(int(a), int(col), int(n)) + tuple(v) for a, col, n, v in zip(d, c, (hi - lo)[k, run], lo.tolist())}
    assert not any((int(a), int(col), int(n)) + tuple(v) in begins for a, col, n, v in zip(d, c, (hi - lo)[k, run], above.tolist()))
    # the mesh is closed: its parity set is the solid set
    G = max(o + n for o, n in zip(origin, (nx, ny, nz)))
    z, y, x = np.nonzero(S)
    keys = np.sort(((x + origin[0]).astype(np.int64) * G + y + origin[1]) * G + z + origin[2])
    assert np.array_equal(fill_ref.parity_keys(p[f], G, 1), keys)


def test_invariants_on_every_grid():
    rng = np.random.default_rng(5)
    for name, grid, fmt, level in small_grids():
        for kw in color_modes(rng, grid, fmt, level):
            check_invariants(grid, fmt, level, (2, 0, 1), kw)
    B, _ = ball()
    z, y, x = np.indices(B.shape)
    for a in (x, y, z):
        check_invariants(B, FR.U8, None, (0, 0, 0), dict(colors=(a >= 12).astype(np.int32)))
    for S, Cv in list(wall_grids().values()) + [(two_bars(), None)]:
        check_invariants(S, FR.U8, None, (3, 1, 2), {} if Cv is None else dict(colors=Cv.astype(np.int32)))
    n = 0
    for dims in ((1, 1, 1), (2, 1, 3), (4, 4, 4), (7, 3, 5), (12, 11, 10)):
        for density in (0.3, 0.7, 0.95):
            for n_colors in (1, 2, 4):
                S = rng.random(dims[::-1]) < density
                # colours in slabs, so that runs of one colour stack
                Cv = rng.integers(0, n_colors, dims[::-1]) if n % 2 else rng.integers(0, n_colors, (dims[2], 1, 1)) + np.zeros(dims[::-1], np.int64)
                check_invariants(S, FR.U8, None, (0, 5, 0), dict(colors=Cv.astype(np.int32)))
                n += 1
    assert n == 45


# ---- the kernel's own algebra on the host ------------------------------------------------------------------------------------------

HOST_RC = r"""
#include <cstdint>
#define O2V_FA_HOST
#define O2V_FA_FN static inline
static inline uint32_t fa_ctz64(uint64_t v) { return (uint32_t) __builtin_ctzll(v); }
%s
// The passes in the kernels' order: rstarts[item] as k_rects_count keeps them, for all items first; then for every set bit in
// ascending (item, bit) the run length, the height and the corners as k_rects_write finds them from the kept masks.  Returns Q.
extern "C" uint64_t rc_host(const unsigned long long *solid, const unsigned long long *same_x, const unsigned long long *same_y,
                            const unsigned long long *same_z, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t colored, uint32_t ox, uint32_t oy,
                            uint32_t oz, unsigned long long *rstarts, float *pos, uint32_t *extents, uint64_t capacity)
{
    FaGrid g{};
    g.nx = nx, g.ny = ny, g.nz = nz, g.W = (nx + 63u) / 64u, g.merge = kFaMergeRects, g.colored = colored;
    g.words = (uint64_t) g.W * ny * nz, g.items = 6u * g.words;
    const FaBits b{solid, same_x, same_y};
    for (uint64_t item = 0; item < g.items; ++item) {
        uint32_t d, wx, y, z;
        fa_item_at(g, item, d, wx, y, z);
        rstarts[item] = rc_rect_starts(b, same_z, g, d, wx, y, z);
    }
    uint64_t q = 0;
    for (uint64_t item = 0; item < g.items; ++item) {
        uint32_t d, wx, y, z;
        fa_item_at(g, item, d, wx, y, z);
        for (uint32_t bit = 0; bit < 64u; ++bit) {
            if (!(rstarts[item] >> bit & 1u)) continue;
            if (q < capacity) {
                const uint32_t len = fa_run_length(b, g, d, wx, y, z, bit), height = rc_height(b, g, rstarts, d, wx, y, z, bit);
                extents[2u * q] = len, extents[2u * q + 1u] = height;
                fa_quad(d, ox + wx * 64u + bit, oy + y, oz + z, len, height, pos + 12u * q);
            }
            ++q;
        }
    }
    return q;
}
"""


@pytest.fixture(scope="module")
def host_rc(tmp_path_factory):
    """build(defines) -> run(S, Cv, origin) -> (rstarts uint64 [6 * words], positions float32 [4Q, 3], (length, height) [Q, 2]):
    the plain C++ parts of o2v_dev_bits.hpp, o2v_dev_k14_faces.hpp and o2v_dev_k16_rects.hpp, compiled for the host."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    k14, k16 = open(K14).read(), open(K16).read()
    text = (bits_host.plain_part() + k14[k14.index("constexpr uint32_t kFaMergeNone"):k14.index("#ifndef O2V_FA_HOST")] +
            k14[k14.index("// ---- words -> exposed faces"):k14.index("// ---- kernels")] +
            k16[k16.index("// ---- stacked runs"):k16.index("// ---- kernels")])
    tmp = tmp_path_factory.mktemp("host_rc")

    def build(defines=()):
        name = "rc_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_RC % text)
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = C.CDLL(str(tmp / (name + ".so")))
        L.rc_host.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 7 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.rc_host.restype = C.c_uint64

        def run(S, Cv, origin=(0, 0, 0)):
            nz, ny, nx = S.shape
            solid = GR.words64(S)
            same = [None, None, None]
            if Cv is not None:
                same = [GR.words64(S & FR.shifted(S, back, False) & (Cv == FR.shifted(Cv, back, 0))) for back in (0, 2, 4)]
            rstarts = np.zeros(6 * len(solid), np.uint64)
            args = (solid.ctypes.data,) + tuple(None if a is None else a.ctypes.data for a in same) + (nx, ny, nz, int(Cv is not None)) + tuple(origin)
            Q = L.rc_host(*args, rstarts.ctypes.data, None, None, 0)
            pos, ext = np.zeros((4 * Q, 3), F), np.zeros((Q, 2), np.uint32)
            assert L.rc_host(*args, rstarts.ctypes.data, pos.ctypes.data, ext.ctypes.data, Q) == Q
            return rstarts, pos, ext
        return run
    return build


def host_cases():
    """(name, solid [z, y, x], colours or None)"""
    rng = np.random.default_rng(22)
    for density in (0.7, 0.97):
        S = rng.random((3, 4, 200)) < density
        yield "random words at %.2f" % density, S, None
        yield "random words at %.2f, random colours" % density, S, rng.integers(0, 2, S.shape).astype(np.uint32)
    row = rng.random((1, 1, 200)) < 0.8
    S = np.broadcast_to(row, (3, 4, 200)).copy()
    S[1, 2, 150] ^= True                                                   # equal rows, but for one bit
    yield "equal rows", S, None
    yield "equal rows, colours in slabs", S, (np.arange(200) // 37 % 2 + np.zeros((3, 4, 200))).astype(np.uint32)
    yield "full words", np.ones((2, 3, 192), bool), None
    yield "full words, one colour as a grid", np.ones((2, 3, 192), bool), np.full((2, 3, 192), 5, np.uint32)
    S = np.ones((2, 2, 192), bool)
    S[:, :, 129:] = False
    S[0, 1, 128] = S[1, 0, 128] = False                                    # equal for 128 bits, different exactly at bit 0 of word 2
    yield "rows that differ at bit 0 of the third word", S, None
    S = np.ones((1, 2, 130), bool)
    S[0, 1, 129] = False
    yield "(130, 2, 1) less a voxel", S, None
    Cv = (np.arange(200) >= 64).astype(np.uint32) + (np.arange(200) >= 128) + np.zeros((2, 2, 200), np.uint32)
    yield "a colour change exactly at a word boundary", np.ones((2, 2, 200), bool), Cv
    Cv = Cv.copy()
    Cv[1, 1, 128:] = 1                                                     # ... and in one row not at the second one
    yield "a colour change at a word boundary in all rows but one", np.ones((2, 2, 200), bool), Cv
    S = np.zeros((2, 2, 200), bool)
    S[:, :, 63:129] = True                                                # from bit 63 of word 0 to bit 0 of word 2
    S[1, 1, 127:193] = True                                               # from bit 63 of word 1 to bit 0 of word 3
    yield "runs that begin at bit 63 and end at bit 0", S, None
    yield "1 024 full words over 3 rows of y", np.ones((1, 3, 65536), bool), None
    yield "1 024 full words over 3 rows of z", np.ones((3, 1, 65536), bool), None
    S = np.ones((3, 1, 65536), bool)
    S[1, 0, 65535] = False
    yield "1 024 words that differ in the last bit", S, None
    yield "tall", rng.random((3, 70, 3)) < 0.8, rng.integers(0, 2, (3, 70, 3)).astype(np.uint32)
    col = rng.random((1, 70, 3)) < 0.8
    S = np.broadcast_to(col, (3, 70, 3)).copy()
    S[2, 40, 1] ^= True
    yield "tall, equal layers", S, None
    yield "tall, equal layers, colours in slabs", S, (np.arange(70)[None, :, None] // 9 % 2 + np.zeros((3, 70, 3))).astype(np.uint32)
    yield "two bars across y = ny - 1", two_bars(), None
    for name, (S, Cv) in wall_grids().items():
        yield name, S, Cv


def want_masks(r, shape):
    nz, ny, nx = shape
    W = -(-nx // 64)
    want = np.zeros((nz, ny, 6, W * 64), bool)
    want[r[:, 2], r[:, 1], r[:, 3], r[:, 0]] = True
    return (want.reshape(-1, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def test_stacks_heights_and_corners_on_the_host(host_rc):
    run = host_rc()
    stacked = 0
    for name, S, Cv in host_cases():
        r = RR.rects(S, np.zeros(S.shape, np.uint32) if Cv is None else Cv)
        rstarts, pos, ext = run(S, Cv, (3, 2, 1))
        assert np.array_equal(rstarts, want_masks(r, S.shape)), (name, "rectangle-start masks differ")
        assert np.array_equal(ext, r[:, 4:6]), (name, "lengths or heights differ")
        assert np.array_equal(pos.view(np.uint32), RR.geometry(r, (3, 2, 1))[0].view(np.uint32)), name
        stacked += int((r[:, 5] > 1).sum())
    assert stacked > 500                                                   # (the cases do stack)
    assert len(run(np.ones((1, 3, 65536), bool), None)[1]) == 4 * 6        # 1 024 words a row, three rows: six quads
    assert len(run(two_bars(), None)[1]) == 4 * 12


def test_the_length_mutation_is_caught_on_the_host(host_rc):
    """With an equality that ignores the length (O2V_RC_MUTATE_NO_LENGTH) the L plate's +z and -z runs [0, 4) and [0, 2) stack:
    fewer than 10 quads, over faces that are not there."""
    run = host_rc(("O2V_RC_MUTATE_NO_LENGTH",))
    S, _ = wall_grids()["L plate"]
    _, pos, _ = run(S, None)
    assert RR.count(S, FR.U8) == 10 and len(pos) // 4 < 10
    assert not np.array_equal(FR.rasterize(pos, np.zeros(len(pos) // 4, np.uint32)), FR.unit_faces(S, np.zeros(S.shape, np.uint32)))
    box = np.ones((2, 3, 70), bool)                                        # (equal lengths everywhere: the same)
    assert np.array_equal(run(box, None)[1], RR.quads(box, FR.U8)[0])


# ---- dense.voxel_faces / count_faces against a stub --------------------------------------------------------------------------------

def test_voxel_faces_passes_merge_rects():
    rng = np.random.default_rng(4)
    labels = np.where(rng.random((4, 5, 6)) < 0.8, 2, 0).astype(np.uint8)
    mesh = RR.quads(labels, FR.U8, origin=(1, 2, 3), argb=0x80000001)
    Q = len(mesh[2])
    dv = FacesStub(mesh)
    p, f, c = dense.voxel_faces(dv, torch.from_numpy(labels), origin=(1, 2, 3), merge="rects", argb=0x80000001)
    assert np.array_equal(p.numpy(), mesh[0]) and np.array_equal(f.numpy(), mesh[1]) and np.array_equal(c.numpy().view(np.uint32), mesh[2])
    (kind, count_args), (_, write_args) = dv.calls
    assert kind == "count" and count_args[5:8] == (hip.FACES_MERGE_RECTS, hip.GATHER_COLOR_CONSTANT, 0x80000001) and hip.FACES_MERGE_RECTS == 3
    assert write_args[:11] == count_args and write_args[11:] == ((1, 2, 3), p.data_ptr(), f.data_ptr(), c.data_ptr(), Q)
    # the colour arguments
    cgrid = torch.zeros((4, 5, 12), dtype=torch.int32)[:, :, 1::2]
    dv = FacesStub(mesh)
    dense.voxel_faces(dv, torch.from_numpy(labels), merge="rects", colors=cgrid)
    assert dv.calls[1][1][5:10] == (hip.FACES_MERGE_RECTS, hip.GATHER_COLOR_GRID, 0xFFFFFFFF, cgrid.data_ptr(), (2, 12, 60))
    dv = FacesStub(mesh)
    dense.voxel_faces(dv, torch.from_numpy(labels), merge="rects", palette=list(range(256)))
    assert dv.calls[1][1][5:7] == (hip.FACES_MERGE_RECTS, hip.GATHER_COLOR_PALETTE) and dv.calls[1][1][10] == list(range(256))
    # count_faces; the defaults stay "none" and "runs"
    dv = FacesStub(mesh)
    assert dense.count_faces(dv, torch.from_numpy(labels), merge="rects", argb=5) == Q
    assert [k for k, _ in dv.calls] == ["count"] and dv.calls[0][1][5:8] == (hip.FACES_MERGE_RECTS, hip.GATHER_COLOR_CONSTANT, 5)
    dv = FacesStub(mesh)
    dense.count_faces(dv, torch.from_numpy(labels))
    dense.voxel_faces(dv, torch.from_numpy(labels))
    assert [a[5] for _, a in dv.calls] == [hip.FACES_MERGE_NONE, hip.FACES_MERGE_RUNS, hip.FACES_MERGE_RUNS]
    # no quads: no write call
    dv = FacesStub(n=0)
    p, f, c = dense.voxel_faces(dv, torch.zeros((2, 2, 2), dtype=torch.bool), merge="rects")
    assert (tuple(p.shape), tuple(f.shape), tuple(c.shape)) == ((0, 3), (0, 3), (0,)) and [k for k, _ in dv.calls] == ["count"]
    for bad in ("greedy", 3, 1, None):
        with pytest.raises(ValueError):
            dense.voxel_faces(FacesStub(n=0), torch.zeros((2, 2, 2), dtype=torch.bool), merge=bad)


def test_the_scratch_bound():
    L = hip._bind()
    assert hasattr(L, "o2v_hip_faces_scratch_bytes_merge")
    C_, G, P = hip.GATHER_COLOR_CONSTANT, hip.GATHER_COLOR_GRID, hip.GATHER_COLOR_PALETTE
    for dims in ((64, 1, 1), (65, 40, 40), (2048, 1024, 1024), (1, 1, 1)):
        words = -(-dims[0] // 64) * dims[1] * dims[2]
        for mode in (C_, G, P):
            old = hip.faces_scratch_bytes(dims, mode)
            assert old == (8 if mode == C_ else 24) * words + 8 * (-(-6 * words // 256) + 1) + 1024
            assert hip.faces_scratch_bytes(dims, mode, hip.FACES_MERGE_NONE) == hip.faces_scratch_bytes(dims, mode, hip.FACES_MERGE_RUNS) == old
            # the header's formula: the kept masks, 48 bytes a word, and the z comparison, 8 bytes a word with colours
            assert hip.faces_scratch_bytes(dims, mode, hip.FACES_MERGE_RECTS) == old + 48 * words + (0 if mode == C_ else 8 * words)
    assert hip.faces_scratch_bytes((65, 40, 40), G, hip.FACES_MERGE_RECTS) == 80 * 3200 + 8 * 76 + 1024
    for merge in (None, 0, 1, 3):
        assert hip.faces_scratch_bytes((0, 4, 4), merge=merge) == 0 and hip.faces_scratch_bytes((4, 4, 0), G, merge) == 0
    assert hip.DeviceVoxelizer.faces_scratch_bytes(None, (64, 1, 1), C_, 3) == 8 + 48 + 8 * 2 + 1024


# ---- the kernels in the code object ------------------------------------------------------------------------------------------------

K16_KERNELS = ["k_rects_same_zILj1E", "k_rects_same_zILj2E", "k_rects_countE", "k_rects_writeILj0E", "k_rects_writeILj1E", "k_rects_writeILj2E"]


@pytest.mark.parametrize("kernel", K16_KERNELS)
def test_k16_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    name = m.group(1)
    entry = [e for e in device_asm[device_asm.index("amdhsa.kernels:"):].split("\n  - ") if re.search(r"\.name: +" + re.escape(name) + r"\n", e)]
    assert len(entry) == 1
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
