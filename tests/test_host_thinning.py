"""Topological thinning without a GPU: the numpy reference (tests/thinning_ref.py) against
scipy.ndimage.label on the 3^3 block and on whole grids (components of the set and of the background unchanged); the pinned
skeletons of the definition; the kernel header's plain part - the simple test, the masks from row words, the border word, "which
tiles see this voxel" and the rule for when a tile runs - compiled for the host, counted over all 2^26 masks and run tile by tile
in a shuffled order and as whole-grid sweeps against the reference, with the wrong tile rule that the lines must catch; the torch
layer against a stub; the scratch formula; the K22 kernels in the gfx950 code object."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import bits_host
from tests import thinning_ref as TR
from tests import thinning_sets as TS

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_components import words64  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401

K22 = os.path.join(SRC, "o2v_dev_k22_thinning.hpp")
SIMPLE_MASKS = 25985144


def sampled_masks():
    """20 000 random masks, the all-set and all-clear masks and all 2^6 face patterns (alone, and with every other bit set)."""
    rng = np.random.default_rng(22)
    m = rng.integers(0, 1 << 27, 20000, dtype=np.uint32) & np.uint32(TR.ALL26)
    faces = [k for k in range(27) if (TR.FACES >> k) & 1]
    pats = np.array([sum(1 << k for i, k in enumerate(faces) if (p >> i) & 1) for p in range(64)], np.uint32)
    return np.concatenate([m, [TR.ALL26, 0], pats, pats | np.uint32(TR.ALL26 & ~TR.FACES)]).astype(np.uint32)


# ---- the reference against the definition --------------------------------------------------------------------------------------

def test_reference_is_simple_equals_scipy_label():
    ndimage = pytest.importorskip("scipy.ndimage")
    m = sampled_masks()
    got26, got6 = TR.c26(m), TR.c6(m)
    six = ndimage.generate_binary_structure(3, 1)
    n18 = np.array([(TR.N18 >> k) & 1 for k in range(27)], bool).reshape(3, 3, 3)
    face = np.array([(TR.FACES >> k) & 1 for k in range(27)], bool).reshape(3, 3, 3)
    for i, v in enumerate(m):
        block = np.array([(int(v) >> k) & 1 for k in range(27)], bool).reshape(3, 3, 3)     # [dz, dy, dx]: bit k = 9 dz + 3 dy + dx
        assert ndimage.label(block, np.ones((3, 3, 3)))[1] == got26[i], hex(v)
        lab, _ = ndimage.label(~block & n18, six)
        assert len(set(lab[face & (lab > 0)].tolist())) == got6[i], hex(v)
    assert (got26[20000], got6[20000], got26[20001], got6[20001]) == (1, 0, 0, 1)
    assert not TR.is_simple(m[20000:20002]).any()
    assert 0.2 < TR.is_simple(m[:20000]).mean() < 0.6


def components(S):
    """(26-components of S, 6-components of the background of the padded grid)."""
    ndimage = pytest.importorskip("scipy.ndimage")
    P = np.pad(np.asarray(S, bool), 1)
    return ndimage.label(P, np.ones((3, 3, 3)))[1], ndimage.label(~P, ndimage.generate_binary_structure(3, 1))[1]


def shapes():
    rng = np.random.default_rng(25)
    yield "box", TR.box()
    yield "ball", TR.ball()
    yield "shell", TR.shell()
    yield "torus", TR.torus()
    yield "cross", TR.cross()
    yield "line", TR.line("x", 130)
    yield "staircase", TR.staircase()
    for density in (0.3, 0.6):
        yield f"random {density}", TR.random_grid(rng, (24, 24, 24), density)


@pytest.mark.parametrize("mode", [TR.ULTIMATE, TR.CURVE])
def test_topology_is_kept(mode):
    rng = np.random.default_rng(3)
    for name, S in shapes():
        keep = rng.random(S.shape) < 0.01
        for kp in (None, keep):
            K, iterations, removed = TR.thin(S, mode, kp)
            assert components(K) == components(S), (name, mode)
            assert not (K & ~S).any() and removed == int(S.sum()) - int(K.sum()), name
            if kp is not None:
                assert (K[kp & S]).all(), name
            again = TR.thin(K, mode, kp)
            assert np.array_equal(again[0], K) and again[1:] == (1, 0), name                # a second call removes nothing


def test_pinned_results():
    K, it, _ = TR.thin(TR.box(), TR.ULTIMATE)
    assert (int(K.sum()), it) == (1, 5)
    K, it, _ = TR.thin(TR.box(), TR.CURVE)
    assert int(K.sum()) == 25 and int((TR.degree(K) == 2).sum()) == 8
    K, it, _ = TR.thin(TR.ball(), TR.ULTIMATE)
    assert (int(K.sum()), it) == (1, 13)
    for mode in (TR.ULTIMATE, TR.CURVE):
        K, it, _ = TR.thin(TR.shell(), mode)
        assert (int(K.sum()), it) == (1142, 3) and components(K)[1] == 2
    K, it, _ = TR.thin(TR.torus(), TR.ULTIMATE)
    assert int(K.sum()) == 56 and (TR.degree(K)[K] == 3).all() and components(K) == (1, 1)
    for S in (TR.line("x", 130), TR.line("x", 130, 1)):
        K, it, _ = TR.thin(S, TR.ULTIMATE)
        assert np.argwhere(K).tolist() == [[1, 1, 65]] and it == 34
    K, it, removed = TR.thin(TR.line("x", 130), TR.CURVE)
    assert np.array_equal(K, TR.line("x", 130)) and (it, removed) == (1, 0)
    for axis, at in (("y", [1, 10, 1]), ("z", [10, 1, 1])):
        K, it, _ = TR.thin(TR.line(axis, 20), TR.ULTIMATE)
        assert np.argwhere(K).tolist() == [at] and it == 6
    K, it, _ = TR.thin(TR.staircase(), TR.ULTIMATE)
    assert np.argwhere(K).tolist() == [[9, 9, 65]] and it == 34
    # an unpadded box equals the padded one: voxels outside the box are background
    S = np.ones((5, 5, 21), bool)
    for mode in (TR.ULTIMATE, TR.CURVE):
        a, b = TR.thin(S, mode), TR.thin(np.pad(S, 2), mode)
        assert np.array_equal(a[0], b[0][2:-2, 2:-2, 2:-2]) and a[1:] == b[1:]


def test_degree_and_nodes():
    K = TR.thin(TR.cross(), TR.CURVE)[0]
    deg = TR.degree(K)
    ends, junctions = TR.nodes(deg)
    assert deg.dtype == np.uint8 and (deg[~K] == 0).all() and deg[K].min() >= 2
    # the documented limit: the end-point rule keeps a spur at each of the four corners of a bar's square end
    assert len(ends) == 6 * 4 and components(K) == (1, 1) and [16, 16, 16] in junctions.tolist()
    assert all(sorted(abs(c - 16) for c in e) == [1, 1, 13] for e in ends.tolist())


# ---- the kernel header's plain part on the host ----------------------------------------------------------------------------------

HOST_THIN = r"""
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>
#define O2V_THIN_HOST
#define O2V_THIN_FN static inline
static inline uint64_t thin_load(const unsigned long long *p) { return *p; }
constexpr uint32_t kCcTileRows = 64u;
%s
extern "C" uint64_t thin_count_simple()
{
    uint64_t n = 0;
    for (uint32_t i = 0; i < (1u << 26); ++i) n += thin_is_simple((i & 0x1fffu) | (i >> 13) << 14) ? 1u : 0u;
    return n;
}

extern "C" void thin_classify(const uint32_t *m, uint64_t n, uint8_t *c26, uint8_t *c6, uint8_t *simple, uint8_t *removes2)
{
    for (uint64_t i = 0; i < n; ++i)
        c26[i] = (uint8_t) thin_c26(m[i]), c6[i] = (uint8_t) thin_c6(m[i]), simple[i] = thin_is_simple(m[i]),
        removes2[i] = (uint8_t) ((thin_removes(m[i], kThinUltimate) ? 1 : 0) | (thin_removes(m[i], kThinCurve) ? 2 : 0));
}

// The passes in the kernels' order, a "lane" at a time, in place on bits.  Tiles: the tiles of a sub-step in an order shuffled by
// `shuffle`, each reading what the tiles before it have stored, a tile left out where thin_tile_runs lets it.  out4: iterations,
// launches, tile turns, voxels removed.
extern "C" void thin_host(unsigned long long *bits, const unsigned long long *keep, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t mode,
                          uint32_t max_iterations, int no_tiles, uint32_t shuffle, uint64_t *out4)
{
    ThinGrid g;
    g.nx = nx, g.ny = ny, g.nz = nz, g.W = (nx + 63u) / 64u, g.words = (uint64_t) g.W * ny * nz;
    g.tiles_y = (ny + 7u) / 8u, g.tiles_z = (nz + 7u) / 8u, g.mode = mode;
    const uint32_t tiles = g.W * g.tiles_y * g.tiles_z;
    std::vector<unsigned long long> border(g.words, 0ull);
    std::vector<uint32_t> stamps(2u * tiles, 0u), order(tiles);
    for (uint32_t t = 0; t < tiles; ++t) order[t] = t;
    std::mt19937 rng(shuffle);
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    static uint64_t s_rows[kThinHaloRows * kThinRowWords], s_cand[64];
    for (uint32_t it = 1;; ++it) {
        const uint64_t before = out4[3];
        for (uint64_t wi = 0; wi < g.words; ++wi) {
            const BitWord at = bits_word_at(g, wi);
            const uint32_t tile = ((at.z >> 3) * g.tiles_y + (at.y >> 3)) * g.W + at.wx;
            if (!no_tiles && !thin_tile_runs(stamps[((it - 1u) & 1u) * tiles + tile], stamps[(it & 1u) * tiles + tile], it)) continue;
            border[wi] = thin_border_at(g, bits, at.wx, at.y, at.z);
        }
        for (uint32_t sub = 0; sub < 8u; ++sub) {
            if (no_tiles) {
                for (uint64_t wi = 0; wi < g.words; ++wi) {
                    const BitWord at = bits_word_at(g, wi);
                    const uint64_t w = bits[wi], cand = border[wi] & w & ~(keep ? keep[wi] : 0ull) & thin_subfield_word(sub, at.y, at.z);
                    uint64_t all = 0;
                    for (uint32_t lane = 0; lane < 64u; ++lane)
                        if (((cand >> lane) & 1ull) && thin_removes(thin_mask_grid(g, bits, at.wx * 64u + lane, at.y, at.z), mode)) all |= 1ull << lane;
                    bits[wi] = w & ~all;
                    out4[3] += (uint64_t) __builtin_popcountll(all);
                }
                continue;
            }
            std::shuffle(order.begin(), order.end(), rng);
            const uint32_t px = sub & 1u, py = (sub >> 1) & 1u, pz = (sub >> 2) & 1u;
            for (const uint32_t tile : order) {
                if (!thin_tile_runs(stamps[((it - 1u) & 1u) * tiles + tile], stamps[(it & 1u) * tiles + tile], it)) continue;
                uint32_t tx, ty, tz;
                bits_tile_at(g, g.tiles_y, tile, tx, ty, tz);
                const uint32_t y0 = ty * 8u, z0 = tz * 8u;
                for (uint32_t i = 0; i < kThinHaloRows * kThinRowWords; ++i) {
                    const uint32_t row = i / kThinRowWords, c = i - row * kThinRowWords;
                    s_rows[i] = thin_word(g, bits, tx + c - 1u, y0 + row %% 10u - 1u, z0 + row / 10u - 1u);
                }
                bool any = false;
                for (uint32_t r = 0; r < 64u; ++r) {
                    const uint32_t y = y0 + (r & 7u), z = z0 + (r >> 3);
                    uint64_t c = 0;
                    if (y < ny && z < nz) {
                        const uint64_t wi = bits_word_index(g, tx, y, z);
                        c = border[wi] & bits[wi] & ~(keep ? keep[wi] : 0ull) & thin_subfield_word(sub, y, z);
                    }
                    s_cand[r] = c, any |= c != 0ull;
                }
                if (!any) continue;
                ++out4[2];
                uint32_t see = 0;
                for (uint32_t c = 0; c < 16u; ++c) {
                    const uint32_t y = 2u * (c & 3u) + py, z = 2u * (c >> 2) + pz, row = z * 8u + y;
                    uint64_t *const own = s_rows + ((z + 1u) * 10u + (y + 1u)) * kThinRowWords;
                    uint32_t mine = 0;
                    for (uint32_t l = 0; l < 32u; ++l) {
                        const uint32_t x = 2u * l + px;
                        if (((s_cand[row] >> x) & 1ull) && thin_removes(thin_mask_rows(own, 1, 10, x), mode)) mine |= 1u << l, see |= thin_see_mask(x, y, z);
                    }
                    if (!mine) continue;
                    own[1] &= ~(thin_spread(mine) << px);
                    bits[bits_word_index(g, tx, y0 + y, z0 + z)] = own[1];
                    out4[3] += (uint64_t) __builtin_popcount(mine);
                }
                for (int k = 0; k < 27; ++k) {
                    if (!((see >> k) & 1u)) continue;
                    const uint32_t X = tx + (uint32_t) thin_d(0, k), Y = ty + (uint32_t) thin_d(1, k), Z = tz + (uint32_t) thin_d(2, k);
                    if (X < g.W && Y < g.tiles_y && Z < g.tiles_z) stamps[(it & 1u) * tiles + (Z * g.tiles_y + Y) * g.W + X] = it;
                }
            }
        }
        ++out4[0], out4[1] += 9u;
        if (no_tiles) out4[2] += 8u * tiles;
        if (out4[3] == before || (max_iterations && it == max_iterations)) return;
    }
}
"""


@pytest.fixture(scope="module")
def host_thin(tmp_path_factory):
    """build(defines) -> a library with thin_count_simple, thin_classify and thin_host: the part of o2v_dev_k22_thinning.hpp between
    "the simple test" and "kernels", compiled for the host behind its constants and the plain part of o2v_dev_bits.hpp."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    text = open(K22).read()
    consts = text[text.index("constexpr uint32_t kThinUltimate"):text.index("#ifndef O2V_THIN_HOST")]
    part = text[text.index("// ---- the simple test, the masks"):text.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_thin")
    built = {}

    def build(defines=()):
        if defines not in built:
            name = "thin_%d" % len(built)
            (tmp / (name + ".cpp")).write_text(HOST_THIN % (bits_host.plain_part() + consts + part))
            subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                           [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
            L = hip.C.CDLL(str(tmp / (name + ".so")))
            L.thin_count_simple.restype = hip.C.c_uint64
            built[defines] = L
        return built[defines]
    return build


def from_words(bits, shape):
    nz, ny, nx = shape
    b = (bits.reshape(nz, ny, -1, 1) >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return b.reshape(nz, ny, -1)[:, :, :nx].astype(bool)


def host_thin_run(L, S, mode, keep=None, max_iterations=0, no_tiles=False, shuffle=0):
    """(skeleton, (iterations, launches, tile turns, removed)) of the host build."""
    C = hip.C
    S = np.asarray(S, bool)
    nz, ny, nx = S.shape
    bits = words64(S)
    kb = None if keep is None else words64(np.asarray(keep) != 0)
    out4 = np.zeros(4, np.uint64)
    L.thin_host(C.c_void_p(bits.ctypes.data), None if kb is None else C.c_void_p(kb.ctypes.data), nx, ny, nz, mode, max_iterations, int(no_tiles), shuffle,
                C.c_void_p(out4.ctypes.data))
    return from_words(bits, S.shape), tuple(int(v) for v in out4)


def test_the_simple_masks_counted_over_all_2_26(host_thin):
    assert host_thin().thin_count_simple() == SIMPLE_MASKS


def test_the_header_equals_the_reference_on_sampled_masks(host_thin):
    C = hip.C
    m = np.ascontiguousarray(sampled_masks())
    out = [np.zeros(len(m), np.uint8) for _ in range(4)]
    host_thin().thin_classify(C.c_void_p(m.ctypes.data), len(m), *[C.c_void_p(o.ctypes.data) for o in out])
    c26, c6 = TR.c26(m), TR.c6(m)
    assert np.array_equal(out[0], c26) and np.array_equal(out[1], c6) and np.array_equal(out[2] != 0, (c26 == 1) & (c6 == 1))
    one = (m != 0) & ((m & (m - np.uint32(1))) == 0)
    assert np.array_equal(out[3] & 1, out[2]) and np.array_equal(out[3] >> 1, out[2] & ~one)
    assert (c26[-130:-128].tolist(), c6[-130:-128].tolist()) == ([1, 0], [0, 1])             # all set, all clear


LINES = [("line 130", TR.line("x", 130)), ("line 129", TR.line("x", 130, 1)), ("line y", TR.line("y", 20)), ("line z", TR.line("z", 20)),
         ("staircase", TR.staircase())]


def tile_cases():
    rng = np.random.default_rng(7)
    yield from LINES
    for density in (0.3, 0.45, 0.6, 0.8):
        yield f"random {density}", TR.random_grid(rng, (130, 19, 17), density)
    yield "ball", TR.ball()
    yield "wide box", np.ones((9, 17, 129), bool)


@pytest.mark.parametrize("no_tiles", [False, True])
def test_the_kernels_passes_on_the_host_equal_the_reference(host_thin, no_tiles):
    L = host_thin()
    rng = np.random.default_rng(9)
    for name, S in tile_cases():
        for mode in (TR.ULTIMATE, TR.CURVE):
            keep = (rng.random(S.shape) < 0.02) if "random" in name else None
            want = TR.thin(S, mode, keep)
            for shuffle in ((0,) if no_tiles else (1, 2)):
                got, (iterations, launches, turns, removed) = host_thin_run(L, S, mode, keep, no_tiles=no_tiles, shuffle=shuffle)
                assert np.array_equal(got, want[0]) and (iterations, removed) == want[1:] and launches == 9 * iterations, (name, mode, no_tiles)
        capped = TR.thin(S, TR.ULTIMATE, None, 2)
        got, counts = host_thin_run(L, S, TR.ULTIMATE, None, 2, no_tiles, 3)
        assert np.array_equal(got, capped[0]) and (counts[0], counts[3]) == capped[1:], name


def test_tiles_that_see_no_change_are_left_out(host_thin):
    """The line ends in one tile long before the others would notice: most tile turns are saved, the bits are the same."""
    L = host_thin()
    S = TR.staircase()
    tiled, whole = host_thin_run(L, S, TR.ULTIMATE, shuffle=1), host_thin_run(L, S, TR.ULTIMATE, no_tiles=True)
    assert np.array_equal(tiled[0], whole[0]) and tiled[1][0] == whole[1][0] == 34
    assert tiled[1][2] < whole[1][2] // 4


def test_the_wrong_tile_rule_is_caught_by_the_lines(host_thin):
    """DESIGN.md section 25, the trap: a tile woken by a removal in a neighbour tile earlier in the same iteration must run in that
    iteration.  -DO2V_THIN_MUTATE_STALE_LIST takes "or during iteration i so far" out of the rule: the lines across a tile border
    end elsewhere."""
    L = host_thin(("O2V_THIN_MUTATE_STALE_LIST",))
    caught = 0
    for name, S in LINES:
        want = TR.thin(S, TR.ULTIMATE)[0]
        for shuffle in (1, 2):
            caught += not np.array_equal(host_thin_run(L, S, TR.ULTIMATE, shuffle=shuffle)[0], want)
    assert caught >= 2
    got = host_thin_run(L, TR.line("x", 130), TR.ULTIMATE, shuffle=1)[0]
    assert not np.array_equal(got, TR.thin(TR.line("x", 130), TR.ULTIMATE)[0]) and got.sum() >= 1


def test_the_see_mask_and_the_spread(host_thin):
    text = open(K22).read()
    assert "thin_see_mask" in text and "thin_spread" in text
    # through the tile pass: a single voxel on a tile's corner is seen by eight tiles, and thinning a 2-voxel pair across the
    # corner (both ends are end points in CURVE; ULTIMATE removes one) gives the reference's bits
    L = host_thin()
    S = np.zeros((16, 16, 128), bool)
    S[7, 7, 63] = S[8, 8, 64] = True
    for mode in (TR.ULTIMATE, TR.CURVE):
        for shuffle in (1, 2, 3):
            assert np.array_equal(host_thin_run(L, S, mode, shuffle=shuffle)[0], TR.thin(S, mode)[0])


# ---- sets of isolated objects: the lemma, the shapes and the sets of the large device cases ----------------------------------------

def lemma_objects():
    """Four random objects of 13 x 11 x 9 at density 0.7 (one at an odd offset on every axis, two with keep), and a pair of
    small ones with exactly two empty voxels between them, in a box of 70 x 64 x 40."""
    rng = np.random.default_rng(2200)
    objects = []
    for i, origin in enumerate([(2, 4, 2), (41, 3, 5), (20, 30, 20), (48, 40, 24)]):
        A = rng.random((9, 11, 13)) < 0.7
        objects.append((origin, A, (rng.random(A.shape) < 0.05) if i in (1, 2) else None))
    left, right = np.ones((5, 4, 6), bool), rng.random((5, 4, 6)) < 0.8
    right[:, :, 0] = True                                      # (the facing sides are full: the gap is two voxels, no more)
    objects += [((4, 52, 30), left, None), ((4 + 6 + 2, 52, 30), right, None)]
    return (70, 64, 40), objects


@pytest.mark.parametrize("mode", [TR.ULTIMATE, TR.CURVE])
def test_the_locality_lemma(mode):
    """tests/thinning_sets.py: objects two empty voxels apart thin as they do alone, in crops that keep the parities."""
    dims, objects = lemma_objects()
    assert TS.separation_holds(dims, objects) and all(o & 1 for o in objects[1][0])
    assert not TS.separation_holds(dims, objects[:5] + [((11, 52, 30), objects[5][1], None)])          # (one empty voxel is too few)
    S, keep = TS.grid_of(dims, TS.set_of(objects)), TS.grid_of(dims, TS.keep_of(objects))
    assert keep.any() and (keep & S).any()
    want, iterations, removed = TR.thin(S, mode, keep)
    placements, skeleton, it, n = TS.isolated_objects(objects, mode)
    assert np.array_equal(TS.grid_of(dims, skeleton), want)
    alone = [TS.thin_alone(o, A, k, mode) for o, A, k in objects]
    assert (it, n) == (iterations, removed) == (max(a[1] for a in alone), sum(a[2] for a in alone))
    assert len({a[1] for a in alone}) > 1                                                               # (the maximum is of unequal counts)
    assert all(K[k & A].all() for (_, A, k, K) in placements if k is not None)
    print(f"mode {mode}: {int(S.sum())} -> {int(want.sum())} voxels in {iterations} = max{tuple(a[1] for a in alone)} iterations, {removed} removed")


def test_a_crop_must_keep_the_parities():
    """The object at the odd offset, thinned in a crop whose origin is odd (the object two voxels in, as if its own origin were
    even): other bits than it has in the box."""
    dims, objects = lemma_objects()
    origin, A, keep = objects[1]
    differs = 0
    for mode in (TR.ULTIMATE, TR.CURVE):
        right = TS.thin_alone(origin, A, keep, mode)[0]
        wrong = TR.thin(np.pad(A, 2), mode, np.pad(keep, 2))[0][2:-2, 2:-2, 2:-2]
        whole = TR.thin(TS.grid_of(dims, [(origin, A)]), mode, TS.grid_of(dims, [(origin, keep)]))[0]
        assert np.array_equal(TS.grid_of(dims, [(origin, right)]), whole)
        differs += not np.array_equal(wrong, right)
    assert differs == 2


CUS = (256, 304, 64)
CHUNK_GRIDS = {"a": (3, 3), "b": (3, 70), "c": (32, 3)}        # tile_chunks' grids: (the chunk value wanted, nx)


@pytest.mark.parametrize("cus", CUS)
def test_the_shapes_hit_what_they_claim(cus):
    """The host's choice restated (o2v_hip_thin_dense: chunk = clamp(tiles / (16 CUs), 1, 32), chunks = ceil(tiles / chunk), grid
    = min(chunks, 2^20)): the boxes of tile_chunks and grid_turns get the chunk values they are built for, with ragged lists, and
    the kernel's tile = thread * chunks + chunk over the grid's turns takes every tile once."""
    text = open(os.path.join(SRC, "o2v_dev_host_k22_thinning.hpp")).read()
    assert "tiles / ((uint64_t) ctx->num_cus * 16u), 1u), kThinChunk)" in text and "(tiles + chunk - 1u) / chunk, kCcMaxGrid)" in text
    assert "constexpr uint32_t kThinChunk = 32u;" in open(K22).read() and "threadIdx.x * chunks + chunk" in open(K22).read()
    assert "kCcMaxGrid = 1ull << 20;" in open(os.path.join(SRC, "o2v_dev_host_k12_components.hpp")).read()
    for name, (want, nx) in CHUNK_GRIDS.items():
        dims = TS.dims_for_chunk(cus, want, nx)
        tiles = TS.tile_count(dims)
        chunk, chunks, grid = TS.plan(tiles, cus)
        assert chunk == want and tiles % chunk and grid == chunks <= TS.MAX_GRID and dims[0] == nx and dims[1] % 8 and dims[2] % 8, (name, dims)
        seen, later = TS.visits(tiles, cus)
        assert (seen == 1).all() and not len(later), name
        assert max(dims) <= 65536 and dims[0] * dims[1] * dims[2] < 2 ** 31
    assert TS.dims_for_chunk(256, 3, 3) == (3, 893, 895) and TS.dims_for_chunk(256, 32, 3) == (3, 2893, 2903)
    # grid_turns: the same box on every device with 32 tiles per workgroup; a side less, and the chunks fit one turn
    dims = TS.GRID_TURNS_DIMS
    tiles = TS.tile_count(dims)
    assert dims[1] * dims[2] == 2147395600 < 2 ** 31 <= 46341 ** 2 and tiles == 5793 ** 2 == 33558849
    assert TS.plan(tiles, cus) == (32, 1048715, 1 << 20)
    assert TS.plan(TS.tile_count((1, 46340, 46332)), cus)[1] <= 1 << 20 and TS.plan(5792 * 5793, cus)[1] <= 1 << 20
    seen, later = TS.visits(tiles, cus)
    assert (seen == 1).all() and len(later) == 139 and later[0] == 1 << 20 and later[-1] == 1048714
    assert tiles % 32 == 1                                                                              # (the last chunk's list: one tile)


@pytest.mark.parametrize("name, cus", [("a", 256), ("a", 64), ("b", 64), ("c", 64)])
def test_the_sets_of_tile_chunks(name, cus):
    """Objects separated as the lemma needs, inside the box; a candidate in every tile; every lattice object loses a voxel in
    ULTIMATE; the palette's ten shapes all occur; the tiles of three workgroups' lists hold random objects."""
    want, nx = CHUNK_GRIDS[name]
    dims = TS.dims_for_chunk(cus, want, nx)
    objects, what = TS.tile_chunks_objects(dims, cus, 7, with_keep=name == "a")
    for origin, A, _ in objects:
        b = TS.box_of(origin, A)
        assert min(b[:3]) >= 0 and b[3] <= dims[0] and b[4] <= dims[1] and b[5] <= dims[2]
    assert TS.separation_holds(dims, objects)
    S = TS.grid_of(dims, TS.set_of(objects))
    assert int(S.sum()) == sum(int(A.sum()) for _, A, _ in objects)
    assert TS.tiles_with_candidates(dims, S).all()
    lattice = objects[what["random"]:]
    assert what["random"] >= 200 and what["lattice"] == len(lattice) > what["tiles"] // 2 and what["list_tiles"] == what["list_tiles_hit"] >= 2 * what["chunk"]
    assert len({id(A) for _, A, _ in lattice}) == len(TS.PALETTE) >= 8
    for origin, A, keep in lattice:
        assert 2 <= origin[1] % 8 and origin[1] % 8 + 3 <= 6 and 2 <= origin[2] % 8 and origin[2] % 8 + 3 <= 6
        assert dims[0] == 3 or (2 <= origin[0] % 64 and (origin[0] % 64 + 3 <= 62 or origin[0] + 3 > dims[0] - 3))
        assert TS.thin_alone(origin, A, None, TR.ULTIMATE)[2] >= 1
    assert (name == "a") == any(k is not None for _, _, k in lattice)
    # consecutive entries of a workgroup's list differ in content: no two tiles t * chunks + c, (t + 1) * chunks + c of the first
    # lists share a palette entry more often than chance (a tenth)
    same = sum(TS._hash(t * what["chunks"] + c) % 10 == TS._hash((t + 1) * what["chunks"] + c) % 10 for c in range(200) for t in range(what["chunk"] - 1))
    assert same < 0.2 * 200 * (what["chunk"] - 1)


def test_the_set_of_grid_turns():
    dims = TS.GRID_TURNS_DIMS
    objects, required, what = TS.grid_turns_objects()
    assert what["second_turn"] == 139 and what["required"] == 2 + 139 * 32 - 31 and what["random"] >= 200   # (chunk 1 048 714 has one tile)
    placed = TS.set_of(objects)
    hit = TS.tiles_hit(dims, placed)
    assert set(required) <= hit and {0, what["tiles"] - 1} <= hit
    z, y, x = TS.coords(placed)
    assert x.max() == 0 and y.min() >= 0 and z.min() >= 0 and y.max() == dims[1] - 1 and z.max() == dims[2] - 1
    assert bool(((y == dims[1] - 1) & (z == dims[2] - 1)).any())                                         # the last row and column
    # separation, on the voxels: sorted keys, and no voxel of another object within two steps
    owner = np.concatenate([np.full(int(A.sum()), i) for i, (_, A) in enumerate(placed)])
    zz, yy, _ = (np.concatenate(v) for v in zip(*[TS.coords([p]) for p in placed]))
    key = zz * dims[1] + yy
    order = np.argsort(key)
    key, owner, zz, yy = key[order], owner[order], zz[order], yy[order]
    assert len(np.unique(key)) == len(key)
    for dz in range(-2, 3):
        for dy in range(-2, 3):
            ok = (yy + dy >= 0) & (yy + dy < dims[1])
            at = np.searchsorted(key, key + dz * dims[1] + dy)
            found = ok & (at < len(key)) & (key[np.minimum(at, len(key) - 1)] == key + dz * dims[1] + dy)
            assert (owner[np.minimum(at, len(key) - 1)][found] == owner[found]).all()
    # objects cross tile borders: all but those pulled in at the box's end lie across a tile's corner, in four tiles
    assert sum(o[1] % 8 == 5 and o[2] % 8 == 5 for o, _, _ in objects) >= 0.95 * len(objects)
    for mode in (TR.ULTIMATE, TR.CURVE):
        _, skeleton, iterations, removed = TS.isolated_objects(objects, mode)
        assert iterations >= 3 and removed > 10 * len(objects)


@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_the_longest_axis_on_the_host_build(host_thin, axis):
    """65 536 voxels along an axis, segments at both of its ends: thin_word's "-1 wraps to above any dim" and "one past the last"
    with the largest dim there is, tile by tile and as whole-grid sweeps."""
    S = TS.long_axis_set(axis)
    K, iterations, removed = TR.thin(S, TR.ULTIMATE)
    assert (np.argwhere(K)[:, {"x": 2, "y": 1, "z": 0}[axis]].tolist(), iterations, removed) == ([20, 32767, 65472, 65516], 11, 134)
    for no_tiles in (False, True):
        got, counts = host_thin_run(host_thin(), S, TR.ULTIMATE, no_tiles=no_tiles, shuffle=1)
        assert np.array_equal(got, K) and (counts[0], counts[3]) == (iterations, removed), (axis, no_tiles)


# ---- the torch layer against a stub ----------------------------------------------------------------------------------------------

class ThinStub(StubVoxelizer):
    """Computes with the reference, on the tensors' own memory (CPU)."""

    def thin_dense(self, grid_ptr, fmt, strides, dims, level, flags, mode, max_iterations, keep_ptr, keep_strides, dst_ptr, dst_strides, dst_format):
        self.calls.append(("thin", grid_ptr, fmt, tuple(strides), tuple(dims), level, flags, mode, max_iterations, keep_ptr,
                           None if keep_strides is None else tuple(keep_strides), dst_ptr, tuple(dst_strides), dst_format))
        C = hip.C
        assert fmt == hip.GRID_U8
        nx, ny, nz = dims

        def view(ptr, st):
            span = sum((d - 1) * s for d, s in zip(dims, st)) + 1
            raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (span,))
            return np.lib.stride_tricks.as_strided(raw, (nz, ny, nx), (st[2], st[1], st[0]))
        S = view(grid_ptr, strides) != 0
        if flags & hip.CC_INVERT:
            S = ~S
        K = TR.thin(S, mode, None if keep_ptr is None else view(keep_ptr, keep_strides) != 0, max_iterations)[0]
        view(dst_ptr, dst_strides)[...] = TR.degree(K) if dst_format == hip.THIN_DST_DEGREE else K


def test_skeletonize_arguments(on_cpu):  # noqa: F811
    dv = ThinStub()
    S = TR.cross()
    grid = torch.from_numpy(S)
    K = dense.skeletonize(dv, grid)
    c = dv.calls[-1]
    assert c[2:11] == (hip.GRID_U8, (1, 33, 1089), (33, 33, 33), 0.0, 0, hip.THIN_CURVE, 0, None, None) and c[12:] == ((1, 33, 1089), hip.THIN_DST_MASK)
    assert K.dtype == torch.bool and K.is_contiguous() and np.array_equal(K.numpy(), TR.thin(S, TR.CURVE)[0])
    deg = dense.skeletonize(dv, grid, fmt="degree")
    assert deg.dtype == torch.uint8 and dv.calls[-1][13] == hip.THIN_DST_DEGREE and np.array_equal(deg.numpy(), TR.degree(K.numpy()))
    ends, junctions = dense.skeleton_nodes(deg)
    want = TR.nodes(deg.numpy())
    assert ends.dtype == junctions.dtype == torch.int32 and np.array_equal(ends.numpy(), want[0]) and np.array_equal(junctions.numpy(), want[1])
    assert len(ends) == 24
    # ultimate with a cap: an erosion that breaks nothing; the background; keep
    one = dense.skeletonize(dv, grid, mode="ultimate", max_iterations=1)
    assert dv.calls[-1][7:9] == (hip.THIN_ULTIMATE, 1) and np.array_equal(one.numpy(), TR.thin(S, TR.ULTIMATE, None, 1)[0])
    bg = dense.skeletonize(dv, grid, background=True, mode="ultimate")
    assert dv.calls[-1][6] == hip.CC_INVERT and np.array_equal(bg.numpy(), TR.thin(~S, TR.ULTIMATE)[0])
    keep = torch.zeros((33, 33, 66), dtype=torch.uint8)
    keep[16, 16, 8] = 1
    kept = dense.skeletonize(dv, grid, mode="ultimate", keep=keep[:, :, ::2])
    assert dv.calls[-1][10] == (2, 66, 2178) and dv.calls[-1][9] == keep.data_ptr() and bool(kept[16, 16, 4]) and int(kept.sum()) == 1
    assert not bool(dense.skeletonize(dv, grid, mode="ultimate")[16, 16, 4])                # the anchor decides where the one voxel is
    # out= is written as it is; a uint8 grid thins in place
    wide = torch.full((33, 33, 66), 7, dtype=torch.uint8)
    got = dense.skeletonize(dv, grid, fmt="degree", out=wide[:, :, 1::2])
    assert got.data_ptr() == wide[:, :, 1::2].data_ptr() and dv.calls[-1][12] == (2, 66, 2178) and bool((wide[:, :, ::2] == 7).all())
    assert np.array_equal(wide[:, :, 1::2].numpy(), deg.numpy())
    own = torch.from_numpy(S.astype(np.uint8))
    assert dense.skeletonize(dv, own, out=own) is own and np.array_equal(own.numpy() != 0, K.numpy())
    for text in ("section 25", "end points", "parity"):
        assert text in " ".join(dense.skeletonize.__doc__.split())


U8 = torch.zeros((4, 4, 4), dtype=torch.uint8)


@pytest.mark.parametrize("kw, exc", [
    (dict(grid=torch.zeros((4, 4, 4), dtype=torch.float64)), TypeError), (dict(grid=torch.zeros((4, 4))), ValueError), (dict(grid=torch.zeros((4, 4, 4))), ValueError),
    (dict(grid=torch.zeros((4, 0, 4), dtype=torch.uint8)), ValueError), (dict(grid=torch.zeros((1, 1, 1), dtype=torch.uint8).expand(1, 1, 65537)), ValueError),
    (dict(grid=torch.zeros((1, 1, 1), dtype=torch.uint8).expand(2048, 1024, 1024)), ValueError),
    (dict(mode="surface"), ValueError), (dict(mode=1), ValueError), (dict(fmt="labels"), ValueError),
    (dict(max_iterations=0), ValueError), (dict(max_iterations=-1), ValueError), (dict(max_iterations=1.0), ValueError), (dict(max_iterations=True), ValueError),
    (dict(max_iterations=2 ** 32), ValueError),
    (dict(keep=np.zeros((4, 4, 4), np.uint8)), TypeError), (dict(keep=torch.zeros((4, 4, 4))), TypeError), (dict(keep=torch.zeros((4, 4, 5), dtype=torch.uint8)), ValueError),
    (dict(keep=torch.zeros((4, 4, 4), dtype=torch.uint8, device="meta")), ValueError),
    (dict(out=torch.zeros((4, 4, 4), dtype=torch.int32)), TypeError), (dict(out=torch.zeros((4, 4, 5), dtype=torch.bool)), ValueError),
    (dict(out=torch.zeros((4, 4, 4), dtype=torch.bool), fmt="degree"), TypeError), (dict(out=U8.transpose(0, 2)), ValueError),
    (dict(out=torch.zeros((4, 4, 4), dtype=torch.bool, device="meta")), ValueError),
])
def test_skeletonize_rejects(on_cpu, kw, exc):  # noqa: F811
    dv = ThinStub()
    args = dict(grid=U8)
    args.update(kw)
    with pytest.raises(exc):
        dense.skeletonize(dv, args.pop("grid"), **args)
    assert not dv.calls
    with pytest.raises(ValueError):
        dense.skeleton_nodes(torch.zeros((4, 4, 4), dtype=torch.int32))


def test_refused_when_the_library_came_first(monkeypatch):
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: False)
    with pytest.raises(RuntimeError, match="before torch"):
        dense.skeletonize(ThinStub(), U8)


def test_a_wait_comes_before_the_library(monkeypatch):
    dv = ThinStub()
    own = torch.device("cpu")
    monkeypatch.setattr(dense, "_device", lambda v: own)
    monkeypatch.setattr(dense, "_sync", lambda device: dv.calls.append(("sync", device)))
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: True)
    dense.skeletonize(dv, U8 + 1)
    names = [c[0] for c in dv.calls]
    assert "thin" in names and "sync" in names[:names.index("thin")] and all(c[1] is own for c in dv.calls if c[0] == "sync")


# ---- the scratch formula and the code object -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(1, 1, 1), (64, 8, 8), (65, 9, 9), (1024, 1024, 1024), (65536, 1, 7), (1000, 999, 17)])
def test_scratch_bytes_formula(dims):
    words = -(-dims[0] // 64) * dims[1] * dims[2]
    tiles = -(-dims[0] // 64) * -(-dims[1] // 8) * -(-dims[2] // 8)
    assert hip.thin_scratch_bytes(dims) == hip.thin_scratch_bytes(dims, False) == 16 * words + 8 * tiles + 64
    assert hip.thin_scratch_bytes(dims, True) == 24 * words + 8 * tiles + 64
    assert hip.thin_scratch_bytes((4, 0, 4)) == 0 and hip.DeviceVoxelizer.thin_scratch_bytes(None, dims, True) == 24 * words + 8 * tiles + 64


K22_KERNELS = ["k_thin_borderILb0EE", "k_thin_borderILb1EE", "k_thin_substepILb0EE", "k_thin_substepILb1EE", "k_thin_sweepE", "k_thin_writeILb0EE",
               "k_thin_writeILb1EE"]
# 10 x 10 rows of (left, own, right) words, the 64 candidate words, the list of a chunk's 32 tiles, three words of counts and flags
# (padded to 16 bytes) and the 256 bytes that the workgroup reduction of __syncthreads_or takes: DESIGN.md section 25
SUBSTEP_LDS = 100 * 3 * 8 + 64 * 8 + 32 * 4 + 16 + 256


@pytest.mark.parametrize("kernel", K22_KERNELS)
def test_k22_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
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
    if "k_thin_substep" in kernel:
        assert lds == SUBSTEP_LDS and "ds_read" in body                     # the masks come from LDS
        assert any(re.fullmatch(r"global_atomic_\w*max\w*", a) for a in atomics), atomics     # the stamps
        assert not any("and" in a or "_or" in a for a in atomics if a.startswith("global")), atomics   # a word has one writer: no atomic on the bits
    elif "k_thin_write" in kernel or "k_thin_border" in kernel:
        assert not atomics and lds == 0


def test_the_new_source_has_no_waiting_loop():
    """No kernel of K22 waits for another workgroup, lane or flag: nothing in the source polls or sleeps."""
    text = open(K22).read()
    kernels = text[text.index("// ---- kernels"):]
    assert "s_sleep" not in kernels and "while (" not in kernels and "__builtin_amdgcn_s_sleep" not in kernels
