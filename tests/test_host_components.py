"""Connected components and flood fill without a GPU: the numpy reference (tests/components_ref.py) against
a scalar breadth-first restatement of the header's words and against scipy.ndimage.label where scipy is present; analytic counts;
the property that motivates dense.solidify, from the oracle and tests/fill_ref.py; the kernel's own union-find, tile pass and seam
pass compiled for the host and run tile by tile, with two deliberate changes that must be caught; the torch layer against a stub;
the K12 kernels in the gfx950 code object."""
import collections
import itertools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import bits_host
from tests import components_ref as CR

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401

K12 = os.path.join(SRC, "o2v_dev_k12_components.hpp")


# ---- the header's words, voxel by voxel ---------------------------------------------------------------------------------------

def scalar_label(S, connectivity):
    """Breadth-first search from every voxel of S in linear order: two voxels are adjacent if they differ by at most 1 on every
    axis and on at most 1, 2 or 3 axes; components are numbered in the order their smallest linear index is met."""
    nz, ny, nx = S.shape
    axes = {6: 1, 18: 2, 26: 3}[connectivity]
    steps = [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(map(abs, d)) <= axes]
    labels = np.zeros(S.shape, np.int32)
    n = 0
    for z, y, x in itertools.product(range(nz), range(ny), range(nx)):
        if not S[z, y, x] or labels[z, y, x]:
            continue
        n += 1
        labels[z, y, x] = n
        queue = collections.deque([(z, y, x)])
        while queue:
            cz, cy, cx = queue.popleft()
            for dz, dy, dx in steps:
                Z, Y, X = cz + dz, cy + dy, cx + dx
                if 0 <= Z < nz and 0 <= Y < ny and 0 <= X < nx and S[Z, Y, X] and not labels[Z, Y, X]:
                    labels[Z, Y, X] = n
                    queue.append((Z, Y, X))
    return labels, n


def scalar_flood(S, connectivity, seeds, border, values):
    nz, ny, nx = S.shape
    labels, n = scalar_label(S, connectivity)
    seeded = set()
    for x, y, z in seeds:
        if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and S[z, y, x]:
            seeded.add(labels[z, y, x])
    out = np.empty(S.shape, np.uint8)
    for z, y, x in itertools.product(range(nz), range(ny), range(nx)):
        if border and S[z, y, x] and (x in (0, nx - 1) or y in (0, ny - 1) or z in (0, nz - 1)):
            seeded.add(labels[z, y, x])
    reached = 0
    for z, y, x in itertools.product(range(nz), range(ny), range(nx)):
        hit = S[z, y, x] and labels[z, y, x] in seeded
        reached += int(hit)
        out[z, y, x] = values[0] if hit else values[1] if S[z, y, x] else values[2]
    return out, reached


SMALL_DIMS = [(1, 1, 1), (1, 1, 9), (7, 1, 1), (1, 6, 1), (2, 2, 2), (5, 4, 3), (3, 7, 2), (9, 2, 5), (4, 4, 4), (6, 5, 1)]


@pytest.mark.parametrize("connectivity", CR.CONNECTIVITIES)
def test_reference_equals_the_scalar_restatement(connectivity):
    rng = np.random.default_rng(connectivity)
    n = 0
    for dims in SMALL_DIMS:
        for density in (0.0, 0.15, 0.3, 0.5, 0.7, 1.0):
            for _ in range(2):
                solid = CR.random_grid(rng, dims, density)
                for S in (solid, ~solid):                       # both polarities
                    got, want = CR.label(S, connectivity), scalar_label(S, connectivity)
                    assert got[1] == want[1] and got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), (dims, density)
                    n += 1
    assert n >= 200


@pytest.mark.parametrize("connectivity", CR.CONNECTIVITIES)
def test_reference_flood_equals_the_scalar_restatement(connectivity):
    rng = np.random.default_rng(10 + connectivity)
    for dims in SMALL_DIMS:
        for density in (0.2, 0.5, 0.8):
            S = CR.random_grid(rng, dims, density)
            seeds = rng.integers(-1, max(dims) + 1, (4, 3))
            for border, values in ((False, (1, 0, 0)), (True, (0, 2, 1)), (True, (7, 8, 9)), (False, (255, 3, 0))):
                got = CR.flood(S, connectivity, seeds, border, values)
                want = scalar_flood(S, connectivity, seeds.tolist(), border, values)
                assert got[1] == want[1] and got[0].dtype == np.uint8 and np.array_equal(got[0], want[0]), (dims, density, border)


@pytest.mark.parametrize("connectivity, rank", [(6, 1), (18, 2), (26, 3)])
def test_reference_equals_scipy(connectivity, rank):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(rank)
    structure = ndimage.generate_binary_structure(3, rank)
    for dims, density in (((70, 50, 40), 0.1), ((70, 50, 40), 0.35), ((70, 50, 40), 0.6), ((33, 1, 65), 0.5), ((64, 64, 64), 0.3)):
        S = CR.random_grid(rng, dims, density)
        want, n = ndimage.label(S, structure)
        got = CR.label(S, connectivity)
        assert got[1] == n and np.array_equal(got[0], want)        # identical arrays, not up to renumbering
    S = CR.serpentine((40, 30, 20))
    assert np.array_equal(CR.label(S, connectivity)[0], ndimage.label(S, structure)[0])


# ---- analytic counts ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 4, 3), (8, 8, 8), (65, 9, 9), (3, 2, 7)])
def test_checkerboard_counts(dims):
    S = CR.checkerboard(dims)
    n = math.prod(dims)
    assert S.sum() == -(-n // 2)
    assert CR.label(S, 6)[1] == -(-n // 2) and CR.label(S, 18)[1] == 1 and CR.label(S, 26)[1] == 1


@pytest.mark.parametrize("dims", [(20, 11, 7), (64, 16, 16), (5, 5, 5), (130, 9, 4)])
def test_serpentine_spiral_and_comb_are_one_component(dims):
    for S in (CR.serpentine(dims), CR.spiral(dims), CR.comb(dims)):
        assert S.sum() >= dims[0]
        for connectivity in CR.CONNECTIVITIES:
            assert CR.label(S, connectivity)[1] == 1


@pytest.mark.parametrize("kind, counts", [("edge", (2, 1, 1)), ("corner", (2, 2, 1))])
def test_touching_pairs(kind, counts):
    for corner in ((8, 8, 8), (64, 8, 8), (64, 16, 8), (5, 9, 13)):
        S = CR.touching_pair((80, 24, 24), corner, kind)
        assert tuple(CR.label(S, c)[1] for c in CR.CONNECTIVITIES) == counts


# ---- what solidify is for: the parity fill and the flood fill ----------------------------------------------------------------

def mesh_sets(verts, res):
    """(surface, parity) bool [z, y, x] of a mesh at `res`: the oracle's surface voxels and the parity set of the solid fill
    (tests/fill_ref.py), under the transform the voxelizer takes from the mesh's own bounds."""
    from oracle import oracle
    from tests import fill_ref
    verts = np.asarray(verts, np.float32).reshape(-1, 9)
    v = verts.reshape(-1, 3)
    xf = oracle.mesh_transform(np.concatenate([v.min(0), v.max(0)]), res)
    keys = fill_ref.parity_keys(fill_ref.sample_vertices(verts, xf), res, 1)
    parity = np.zeros((res, res, res), bool)
    parity[keys % res, keys // res % res, keys // (res * res)] = True
    rec = oracle.voxelize(verts, res).astype(np.int64)
    surface = np.zeros((res, res, res), bool)
    surface[rec[:, 2], rec[:, 1], rec[:, 0]] = True
    return surface, parity


def two_cubes():
    from obj2voxel_amd import meshes
    c = meshes.unit_cube().reshape(-1, 9)
    return np.concatenate([c * 16 + 4.03, c * 16 + 10.07]).astype(np.float32)


@pytest.mark.parametrize("mesh, res", [("cube", 32), ("sphere", 32), ("sphere", 48), ("sphere", 64)])
def test_on_one_closed_body_flood_and_parity_agree(mesh, res):
    from obj2voxel_amd import meshes
    from tests import fill_ref
    surface, parity = mesh_sets(meshes.unit_cube() if mesh == "cube" else fill_ref.weld(meshes.uv_sphere(14)), res)
    filled = CR.solidify(surface)
    assert np.array_equal(filled == 1, surface) and (filled == 2).sum() > 10000
    assert np.array_equal(filled == 2, parity & ~surface)


def test_on_two_overlapping_cubes_the_flood_holds_the_overlap():
    surface, parity = mesh_sets(two_cubes(), 40)
    inside, hollowed = CR.solidify(surface) == 2, parity & ~surface
    assert hollowed.sum() == 29540 and inside.sum() == 33636
    assert not (hollowed & ~inside).any() and (inside & ~hollowed).sum() == 4096
    z, y, x = np.nonzero(inside & ~hollowed)                 # exactly the overlap: a 16^3 block
    assert (x.max() - x.min(), y.max() - y.min(), z.max() - z.min()) == (15, 15, 15)
    assert inside[15, 15, 15] and not hollowed[15, 15, 15]


# ---- the kernel's own logic on the host ------------------------------------------------------------------------------------------

HOST_CC = r"""
#include <cstdint>
#include <cstring>
#define O2V_CC_HOST
#define O2V_CC_FN static inline
static inline uint32_t cc_load(const uint32_t *p) { return *p; }
static inline void cc_store(uint32_t *p, uint32_t v) { *p = v; }
static inline uint32_t cc_min(uint32_t *p, uint32_t v) { const uint32_t o = *p; if (v < o) *p = v; return o; }
static inline uint32_t cc_max(uint32_t *p, uint32_t v) { const uint32_t o = *p; if (v > o) *p = v; return o; }
static inline uint32_t cc_clz64(uint64_t v) { return (uint32_t) __builtin_clzll(v); }
constexpr uint32_t kCcTileRows = 64u, kCcTileVoxels = 4096u;
%s
// The passes in the kernels' order, a "lane" at a time; P[i] for i in S ends as the root of i.  out2: unions, retries of the seams.
extern "C" void cc_host(const uint64_t *bits, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t conn, int no_tiles, uint32_t *P, uint64_t *out2)
{
    CcGrid g;
    g.nx = nx, g.ny = ny, g.nz = nz, g.W = (nx + 63u) / 64u, g.tiles_y = (ny + 7u) / 8u, g.tiles_z = (nz + 7u) / 8u, g.conn = conn;
    g.words = (uint64_t) g.W * ny * nz;
    static uint64_t s_w[kCcTileRows];
    static uint32_t s_lab[kCcTileVoxels];
    if (no_tiles) {
        for (uint64_t wi = 0; wi < g.words; ++wi)
            for (uint32_t x = 0; x < 64u; ++x)
                if ((bits[wi] >> x) & 1ull) {
                    const uint32_t i = (uint32_t) (wi / g.W) * nx + (uint32_t) (wi %% g.W) * 64u + x;
                    P[i] = i;
                }
    } else {
        for (uint32_t tz = 0; tz < g.tiles_z; ++tz)
            for (uint32_t ty = 0; ty < g.tiles_y; ++ty)
                for (uint32_t tx = 0; tx < g.W; ++tx) {
                    for (uint32_t row = 0; row < kCcTileRows; ++row) {
                        const uint32_t y = ty * 8u + (row & 7u), z = tz * 8u + (row >> 3);
                        s_w[row] = y < ny && z < nz ? bits[((uint64_t) z * ny + y) * g.W + tx] : 0ull;
                    }
                    std::memset(s_lab, 0xff, sizeof s_lab);
                    for (uint32_t row = 0; row < kCcTileRows; ++row)
                        for (uint32_t x = 0; x < 64u; ++x) cc_tile_init(s_w, s_lab, row, x);
                    for (uint32_t row = 0; row < kCcTileRows; ++row)
                        for (uint32_t x = 0; x < 64u; ++x) cc_tile_merge(conn, s_w, s_lab, row, x);
                    for (uint32_t row = 0; row < kCcTileRows; ++row)
                        for (uint32_t x = 0; x < 64u; ++x) cc_tile_out(g, s_w, s_lab, P, tx * 64u, ty * 8u, tz * 8u, row, x);
                }
    }
    out2[0] = out2[1] = 0;
    for (uint64_t wi = 0; wi < g.words; ++wi) {
        const uint32_t wx = (uint32_t) (wi %% g.W), y = (uint32_t) (wi / g.W %% ny), z = (uint32_t) (wi / g.W / ny);
        for (uint32_t x = 0; x < 64u; ++x) {
            const CcCount n = no_tiles ? cc_seam<true>(g, bits, P, wx, y, z, x) : cc_seam<false>(g, bits, P, wx, y, z, x);
            out2[0] += n.unions, out2[1] += n.retries;
        }
    }
    for (uint64_t wi = 0; wi < g.words; ++wi)
        for (uint32_t x = 0; x < 64u; ++x)
            if ((bits[wi] >> x) & 1ull) {
                const uint32_t i = (uint32_t) (wi / g.W) * nx + (uint32_t) (wi %% g.W) * 64u + x;
                P[i] = cc_root(P, i);
            }
}
"""


def words64(S):
    """The set's bits as the kernels keep them: uint64 [z, y, ceil(nx / 64)], padding bits 0."""
    nz, ny, nx = S.shape
    W = -(-nx // 64)
    pad = np.zeros((nz, ny, W * 64), bool)
    pad[:, :, :nx] = S
    return np.ascontiguousarray((pad.reshape(nz, ny, W, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=3, dtype=np.uint64))


@pytest.fixture(scope="module")
def host_cc(tmp_path_factory):
    """build(defines) -> label(S, connectivity, no_tiles) -> (labels, n, roots, (unions, retries)): the part of
    o2v_dev_k12_components.hpp between "the union-find and the adjacency" and "kernels", compiled for the host behind the plain part
    of o2v_dev_bits.hpp."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    text = open(K12).read()
    part = text[text.index("// ---- the union-find and the adjacency"):text.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_cc")

    def build(defines=()):
        name = "cc_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_CC % (bits_host.plain_part() + part))
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = hip.C.CDLL(str(tmp / (name + ".so")))

        def label(S, connectivity, no_tiles=False):
            C = hip.C
            S = np.asarray(S, bool)
            nz, ny, nx = S.shape
            bits = words64(S)
            P = np.full(S.size, 0xFFFFFFFF, np.uint32)
            out2 = np.zeros(2, np.uint64)
            L.cc_host(C.c_void_p(bits.ctypes.data), nx, ny, nz, connectivity, int(no_tiles), C.c_void_p(P.ctypes.data), C.c_void_p(out2.ctypes.data))
            P = P.reshape(S.shape)
            assert (P[~S] == 0xFFFFFFFF).all()                       # nothing outside S is written
            roots = np.where(S, P.astype(np.int64), -1)
            ids = np.unique(roots[S])
            labels = np.zeros(S.shape, np.int32)
            labels[S] = np.searchsorted(ids, roots[S]) + 1
            return labels, len(ids), roots, tuple(int(v) for v in out2)
        return label
    return build


def host_cases():
    rng = np.random.default_rng(12)
    for dims in ((70, 50, 40), (64, 8, 8), (65, 9, 9), (1, 30, 30), (130, 1, 17), (200, 3, 1), (63, 17, 25)):
        for density in (0.1, 0.4, 0.7):
            yield f"random {dims} {density}", CR.random_grid(rng, dims, density)
    yield "serpentine", CR.serpentine((70, 21, 19))
    yield "spiral", CR.spiral((131, 40, 9))
    yield "comb", CR.comb((200, 30, 20))
    yield "checkerboard", CR.checkerboard((66, 10, 9))
    yield "full", np.ones((9, 17, 129), bool)
    yield "empty", np.zeros((9, 17, 129), bool)
    for kind in ("edge", "corner"):
        for corner in ((64, 8, 8), (64, 16, 8), (128, 8, 16), (5, 9, 13), (63, 7, 7)):
            yield f"{kind} {corner}", CR.touching_pair((140, 24, 24), corner, kind)


@pytest.mark.parametrize("no_tiles", [False, True])
def test_the_kernels_passes_on_the_host_equal_the_reference(host_cc, no_tiles):
    label = host_cc()
    n = 0
    for name, S in host_cases():
        for connectivity in CR.CONNECTIVITIES:
            for T in (S, ~S):
                want, count = CR.label(T, connectivity)
                got, got_count, roots, _ = label(T, connectivity, no_tiles)
                assert got_count == count and np.array_equal(got, want), (name, connectivity, no_tiles)
                assert np.array_equal(roots, CR.roots(T, connectivity)[0]), (name, "a root is not its component's smallest index")
                n += 1
    assert n > 200


def test_the_tile_pass_leaves_the_seams_little(host_cc):
    label = host_cc()
    S = CR.random_grid(np.random.default_rng(3), (128, 32, 32), 0.5)
    tiled, every = label(S, 26)[3][0], label(S, 26, True)[3][0]
    assert 0 < tiled < every / 2


@pytest.mark.parametrize("define, connectivities", [("O2V_CC_MUTATE_HOOK_LARGER", (6, 18, 26)), ("O2V_CC_MUTATE_DROP_DIAGONAL", (26,))])
def test_a_changed_rule_is_caught(host_cc, define, connectivities):
    """DESIGN.md section 15, mutations: the smaller root hooked under the larger (the roots are no longer the smallest indexes,
    so the numbering changes); the offset (+1, +1, -1) left out at 26 (components that touch only there stay apart)."""
    label = host_cc([define])
    S = CR.random_grid(np.random.default_rng(8), (70, 50, 40), 0.12)
    for connectivity in CR.CONNECTIVITIES:
        for no_tiles in (False, True):
            same = np.array_equal(label(S, connectivity, no_tiles)[0], CR.label(S, connectivity)[0])
            assert same == (connectivity not in connectivities), (define, connectivity, no_tiles)


# ---- the torch layer against a stub ----------------------------------------------------------------------------------------------

class CcStub(StubVoxelizer):
    def components_dense(self, grid_ptr, fmt, strides, dims, level, connectivity, flags, labels_ptr, label_strides):
        self.calls.append(("components", grid_ptr, fmt, tuple(strides), tuple(dims), level, connectivity, flags, labels_ptr, tuple(label_strides)))
        return 3

    def flood_dense(self, grid_ptr, fmt, strides, dims, level, connectivity, flags, seeds_ptr, n_seeds, values, out_ptr, out_strides):
        self.calls.append(("flood", grid_ptr, fmt, tuple(strides), tuple(dims), level, connectivity, flags, seeds_ptr, n_seeds, tuple(values),
                           out_ptr, tuple(out_strides)))
        return 5


@pytest.mark.parametrize("dtype, fmt, level", [(torch.bool, hip.GRID_U8, None), (torch.uint8, hip.GRID_U8, None), (torch.int32, hip.GRID_BITS, None),
                                               (torch.float32, hip.GRID_F32_BELOW, 0.1)])
def test_components_formats_and_strides(dtype, fmt, level):
    dv = CcStub()
    grid = torch.zeros((6, 7, 8), dtype=dtype)
    labels, n = dense.components(dv, grid, level=level, connectivity=18, background=True)
    nx = 8 * 32 if fmt == hip.GRID_BITS else 8
    assert n == 3 and labels.dtype == torch.int32 and tuple(labels.shape) == (6, 7, nx) and labels.is_contiguous()
    assert dv.calls == [("components", grid.data_ptr(), fmt, (1, 8, 56), (nx, 7, 6), 0.0 if level is None else float(np.float32(level)), 18,
                         hip.CC_INVERT, labels.data_ptr(), (1, nx, 7 * nx))]
    assert (hip.GRID_U8, hip.GRID_BITS, hip.GRID_F32_BELOW) == (hip.RAY_GRID_U8, hip.RAY_GRID_BITS, hip.RAY_GRID_F32_BELOW)
    if fmt != hip.GRID_BITS:
        batch = torch.zeros((2, 6, 7, 5), dtype=dtype)
        view = batch[1].permute(1, 0, 2)[:, ::2]                       # [z = 7, y = 3, x = 5]
        out = torch.zeros((7, 3, 10), dtype=torch.int32)[:, :, ::2]
        got, _ = dense.components(dv, view, level=level, out=out)
        assert got is out and dv.calls[-1][1:5] == (batch[1].data_ptr(), fmt, (1, 70, 5), (5, 3, 7)) and dv.calls[-1][6:] == (6, 0, out.data_ptr(), (2, 10, 30))
        flat = torch.zeros((1, 7, 5), dtype=dtype).expand(9, -1, -1)
        dense.components(dv, flat, level=level)
        assert dv.calls[-1][3] == (1, 5, 0)


def test_flood_and_what_is_built_on_it():
    dv = CcStub()
    grid = torch.zeros((4, 5, 6), dtype=torch.uint8)
    out = dense.flood(dv, grid, seeds=[(1, 2, 3), (9, 9, 9)], values=(7, 8, 9), connectivity=26)
    c = dv.calls[-1]
    assert out.dtype == torch.uint8 and tuple(out.shape) == (4, 5, 6) and c[0] == "flood" and c[2:8] == (hip.GRID_U8, (1, 6, 30), (6, 5, 4), 0.0, 26, 0)
    assert c[9:11] == (2, (7, 8, 9)) and c[8] is not None and c[11:] == (out.data_ptr(), (1, 6, 30))
    seeds = torch.tensor([[0, 0, 0], [2 ** 40, 0, 0]], dtype=torch.int64)
    dense.flood(dv, grid, seeds=seeds, border=True, background=True)
    assert dv.calls[-1][7] == hip.CC_INVERT | hip.CC_SEED_BORDER and dv.calls[-1][9] == 2
    dense.flood(dv, grid)                                               # no seeds: the pointer is not passed
    assert dv.calls[-1][8] is None and dv.calls[-1][9] == 0
    dense.flood(dv, grid, seeds=torch.zeros((0, 3), dtype=torch.int32))
    assert dv.calls[-1][8] is None and dv.calls[-1][9] == 0
    mask = torch.zeros((4, 5, 6), dtype=torch.bool)
    assert dense.flood(dv, grid, border=True, out=mask) is mask
    ext = dense.exterior(dv, grid, connectivity=18)
    assert ext.dtype == torch.bool and dv.calls[-1][6:8] == (18, hip.CC_INVERT | hip.CC_SEED_BORDER) and dv.calls[-1][10] == (1, 0, 0)
    sol = dense.solidify(dv, torch.zeros((4, 5, 6)), level=0.0)
    assert sol.dtype == torch.uint8 and dv.calls[-1][2] == hip.GRID_F32_BELOW and dv.calls[-1][6:8] == (6, hip.CC_INVERT | hip.CC_SEED_BORDER)
    assert dv.calls[-1][10] == (0, 2, 1)
    for text in ("leak", "hole one voxel wide", "pocket"):
        assert text in " ".join(dense.solidify.__doc__.split())


def test_component_sizes_and_remove_small():
    labels = torch.tensor([[[0, 1, 1], [2, 0, 3]], [[3, 3, 0], [0, 0, 1]]], dtype=torch.int32)
    sizes = dense.component_sizes(labels, 4)
    assert sizes.dtype == torch.int64 and sizes.tolist() == [5, 3, 1, 3, 0]

    class Fixed(CcStub):
        def components_dense(self, *args):
            super().components_dense(*args)
            np.ctypeslib.as_array(hip.C.cast(args[7], hip.C.POINTER(hip.C.c_int32)), (12,))[:] = labels.reshape(-1).numpy()
            return 3
    dv = Fixed()
    keep = dense.remove_small(dv, labels != 0, 2)
    assert keep.dtype == torch.bool and torch.equal(keep, (labels == 1) | (labels == 3)) and dv.calls[-1][6] == 26
    assert torch.equal(dense.remove_small(dv, labels != 0, 0, connectivity=6), labels != 0) and dv.calls[-1][6] == 6
    assert not dense.remove_small(dv, labels != 0, 4).any()


U8 = torch.zeros((4, 4, 4), dtype=torch.uint8)


@pytest.mark.parametrize("fn, kw, exc", [
    (dense.components, dict(grid=torch.zeros((4, 4, 4), dtype=torch.float64)), TypeError), (dense.components, dict(grid=torch.zeros((4, 4))), ValueError),
    (dense.components, dict(grid=np.zeros((4, 4, 4), np.uint8)), ValueError), (dense.components, dict(grid=torch.zeros((4, 4, 4))), ValueError),
    (dense.components, dict(grid=torch.zeros((4, 4, 4)), level=float("nan")), ValueError), (dense.components, dict(grid=torch.zeros((4, 4, 4)), level=1e39), ValueError),
    (dense.components, dict(level=0.0), ValueError), (dense.components, dict(grid=torch.zeros((4, 4, 8), dtype=torch.int32)[:, :, ::2]), ValueError),
    (dense.components, dict(grid=torch.zeros((4, 0, 4), dtype=torch.uint8)), ValueError),
    (dense.components, dict(grid=torch.zeros((4, 4, 4), dtype=torch.uint8, device="meta")), ValueError),
    (dense.components, dict(connectivity=8), ValueError), (dense.components, dict(connectivity=True), ValueError), (dense.components, dict(connectivity="6"), ValueError),
    (dense.components, dict(grid=torch.zeros((1, 1, 1), dtype=torch.uint8).expand(1, 1, 65537)), ValueError),
    (dense.components, dict(grid=torch.zeros((1, 1, 1), dtype=torch.uint8).expand(2048, 1024, 1024)), ValueError),
    (dense.components, dict(out=torch.zeros((4, 4, 4), dtype=torch.int64)), TypeError), (dense.components, dict(out=torch.zeros((4, 4, 5), dtype=torch.int32)), ValueError),
    (dense.components, dict(out=torch.zeros((4, 4, 4), dtype=torch.int32, device="meta")), ValueError),
    (dense.flood, dict(values=(1, 0)), ValueError), (dense.flood, dict(values=(256, 0, 0)), ValueError), (dense.flood, dict(values=(1.0, 0, 0)), ValueError),
    (dense.flood, dict(values=(True, 0, 0)), ValueError), (dense.flood, dict(seeds=torch.zeros((2, 3))), TypeError),
    (dense.flood, dict(seeds=torch.zeros((2, 4), dtype=torch.int32)), ValueError), (dense.flood, dict(seeds=torch.zeros((2, 3), dtype=torch.int32, device="meta")), ValueError),
    (dense.flood, dict(out=torch.zeros((4, 4, 4), dtype=torch.int32)), TypeError), (dense.flood, dict(out=torch.zeros((4, 4, 4), dtype=torch.bool), values=(2, 0, 0)), ValueError),
    (dense.flood, dict(out=torch.zeros((4, 4, 3), dtype=torch.uint8)), ValueError), (dense.flood, dict(connectivity=7), ValueError),
    (dense.exterior, dict(grid=torch.zeros((4, 4, 4), dtype=torch.int64)), TypeError), (dense.solidify, dict(out=torch.zeros((4, 4, 4), dtype=torch.int8)), TypeError),
    (dense.solidify, dict(connectivity=0), ValueError),
])
def test_the_new_functions_reject(fn, kw, exc):
    dv = CcStub()
    args = dict(grid=U8)
    args.update(kw)
    with pytest.raises(exc):
        fn(dv, args.pop("grid"), **args)
    assert not dv.calls


@pytest.mark.parametrize("min_voxels", [-1, 1.5, True, "3"])
def test_remove_small_rejects(min_voxels):
    dv = CcStub()
    with pytest.raises(ValueError):
        dense.remove_small(dv, U8, min_voxels)
    assert not dv.calls


def test_components_accept_the_limits():
    dv = CcStub()
    dense.flood(dv, torch.zeros((1, 1, 1), dtype=torch.uint8).expand(1, 1, 65536))
    dense.flood(dv, torch.zeros((1, 1, 1), dtype=torch.uint8).expand(2047, 1024, 1024), out=torch.zeros((1, 1, 1), dtype=torch.uint8).expand(2047, 1024, 1024))
    assert dv.calls[-1][4] == (1024, 1024, 2047)


def test_refused_when_the_library_came_first(monkeypatch):
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: False)
    for fn in (dense.components, dense.flood, dense.exterior, dense.solidify):
        with pytest.raises(RuntimeError, match="before torch"):
            fn(CcStub(), U8)


@pytest.mark.parametrize("kw, exc", [
    (dict(grid=torch.zeros((4, 4, 4), dtype=torch.float64)), TypeError), (dict(grid=torch.zeros((4, 4, 4), dtype=torch.int64)), TypeError),
    (dict(grid=torch.zeros((4, 4))), ValueError), (dict(grid=torch.zeros((4, 4, 4))), ValueError), (dict(grid=torch.zeros((4, 4, 4)), level=float("inf")), ValueError),
    (dict(grid=torch.zeros((4, 4, 4)), level=True), ValueError), (dict(grid=torch.zeros((4, 4, 4), dtype=torch.bool), level=0.0), ValueError),
    (dict(grid=torch.zeros((4, 4, 8), dtype=torch.int32)[:, :, ::2]), ValueError), (dict(grid=torch.zeros((4, 4, 4), dtype=torch.float64, device="meta")), TypeError),
    (dict(grid=torch.zeros((4, 4, 4), device="meta")), ValueError), (dict(origin=(0, -1, 0)), ValueError),
])
def test_raycaster_still_raises_what_it_raised(kw, exc):
    from tests.test_host_raycast import RayStub
    dv = RayStub()
    args = dict(grid=U8)
    args.update(kw)
    with pytest.raises(exc):
        dense.RayCaster(dv, args.pop("grid"), **args)
    assert not dv.calls
    dense.RayCaster(dv, torch.zeros((4, 4, 4)), level=0.25)
    assert dv.calls[-1][2] == hip.RAY_GRID_F32_BELOW and dv.calls[-1][5] == 0.25


# ---- the scratch formula and the code object -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(1, 1, 1), (64, 8, 8), (65, 9, 9), (1024, 1024, 1024), (65536, 1, 7), (1000, 999, 17)])
def test_scratch_bytes_formula(dims):
    words, voxels = -(-dims[0] // 64) * dims[1] * dims[2], math.prod(dims)
    labels = 20 * words + 8 * (-(-words // 256) + 1) + 32
    assert hip.components_scratch_bytes(dims, hip.CC_SCRATCH_LABELS) == labels
    assert hip.components_scratch_bytes(dims, hip.CC_SCRATCH_LABELS_STRIDED) == labels + 4 * voxels
    assert hip.components_scratch_bytes(dims, hip.CC_SCRATCH_FLOOD) == 16 * words + 4 * voxels + 32
    assert hip.components_scratch_bytes((4, 0, 4)) == 0 and hip.components_scratch_bytes(dims, 3) == 0
    assert hip.DeviceVoxelizer.components_scratch_bytes(None, dims) == labels


K12_KERNELS = ["k_cc_classifyILj0ELb0E", "k_cc_classifyILj0ELb1E", "k_cc_classifyILj1ELb0E", "k_cc_classifyILj2ELb0E", "k_cc_classifyILj2ELb1E",
               "k_cc_tilesE", "k_cc_initE", "k_cc_seamsILb0ELb0E", "k_cc_seamsILb0ELb1E", "k_cc_seamsILb1ELb0E", "k_cc_seamsILb1ELb1E", "k_cc_flattenE",
               "k_cc_countE", "k_cc_labelsE", "k_cc_seed_listE", "k_cc_seed_borderE", "k_cc_flood_outE"]
TILE_LDS = 64 * 8 + 4096 * 4 + 8     # the row words, the labels, the "not empty" word (and its padding): DESIGN.md section 15


@pytest.mark.parametrize("kernel", K12_KERNELS)
def test_k12_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    name, body = m.group(1), m.group(2)
    scratch = re.findall(r"; ScratchSize: (\d+)", device_asm[m.end():m.end() + 4000])
    assert scratch and scratch[0] == "0", scratch[:1]
    assert "scratch_" not in body
    entry = [e for e in device_asm[device_asm.index("amdhsa.kernels:"):].split("\n  - ") if re.search(r"\.name: +" + re.escape(name) + r"\n", e)]
    assert len(entry) == 1
    lds = int(re.search(r"\.group_segment_fixed_size: +(\d+)", entry[0]).group(1))
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
    atomics = set(re.findall(r"^\s*(\S*atomic\S*)", body, re.M))
    if kernel == "k_cc_tilesE":
        assert not atomics, atomics                                     # no global (or flat) atomics: the unions are in LDS
        assert "ds_min_rtn_u32" in body and lds == TILE_LDS
    elif kernel in ("k_cc_seamsILb0ELb0E", "k_cc_seamsILb1ELb0E"):
        assert atomics and all(re.fullmatch(r"global_atomic_\w*min\w*", a) for a in atomics), atomics
        assert "cmpswap" not in body
    elif "k_cc_seams" in kernel:
        assert atomics == {"global_atomic_umin", "global_atomic_add_x2"}, atomics   # ... and the two counters, once per wavefront
    if kernel in ("k_cc_classifyILj0ELb1E", "k_cc_classifyILj2ELb1E"):
        assert "global_load_dwordx4" in body


def test_the_new_source_has_none_of_the_barred_instructions():
    text = open(K12).read().lower()
    barred = ["s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_dcache_" + "wb", "s_dcache_" + "discard",
              "debug_hip_" + "force_graph_queues", "roc" + "gdb", "asm volatile", "__asm"]
    assert not [w for w in barred if w in text]
