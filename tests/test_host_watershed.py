"""Watershed parts without a GPU: the numpy reference (tests/watershed_ref.py) against what follows from the
definition - persistences against threshold floods with scipy.ndimage.label, nesting, the surviving peak - and against the pinned
results; the kernel header's plain part - the key, the offsets, the ascent step, the tile-local follow, the insert into the pair
table (o2v_dev_pair_table.hpp, through tests/pair_table_host.py) and the merge - compiled for the host and run tile by tile in a shuffled order against the reference, with the change that must be caught; the
torch layer against a stand-in that computes with the reference; the scratch formula; the K23 kernels' metadata in the gfx950 code
object."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import bits_host, pair_table_host
from tests import watershed_ref as WR

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from obj2voxel_amd import watershed as WS  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401

K23 = os.path.join(SRC, "o2v_dev_k23_watershed.hpp")
CONNECTIVITIES = (6, 18, 26)


# ---- the reference against what follows from the definition --------------------------------------------------------------------------

def flood_persistence(H, connectivity):
    """Per peak (ascending index) H[p] - t*, t* the highest level t at which the component of {H >= t} that holds p also holds a
    voxel of greater key; INF where there is no such level."""
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    K = WR.packed_keys(H)
    w = WR.Watershed(H, connectivity)
    pers = [WR.INF] * len(w.peaks)
    for t in range(int(H.max()), 0, -1):
        lab, n = ndimage.label(H >= t, structure)
        top = ndimage.maximum(K, lab, np.arange(1, n + 1)) if n else []
        for r, p in enumerate(w.peaks):
            at = np.unravel_index(p, H.shape)
            if pers[r] == WR.INF and H[at] >= t and top[lab[at] - 1] > K[at]:
                pers[r] = int(H[at]) - t
    return w, pers


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_persistence_equals_threshold_floods(connectivity):
    rng = np.random.default_rng(60 + connectivity)
    for _ in range(6):
        H = rng.integers(0, 6, (6, 7, 9)).astype(np.int32)
        w, want = flood_persistence(H, connectivity)
        assert list(w.pers) == want
        assert sum(p == WR.INF for p in want) == pytest.importorskip("scipy.ndimage").label(
            H > 0, pytest.importorskip("scipy.ndimage").generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity]))[1]


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_partitions_nest_and_the_survivor_is_the_greatest_key(connectivity):
    H = np.random.default_rng(9).integers(0, 9, (9, 11, 40)).astype(np.int32)
    w = WR.Watershed(H, connectivity)
    K = WR.packed_keys(H)
    finer, counts = None, []
    for h in (0, 1, 2, 3, 4, 9):
        L, n = w.labels(h)
        counts.append(n)
        assert np.array_equal(L > 0, H > 0) and sorted(np.unique(L[L > 0]).tolist()) == list(range(1, n + 1))
        if finer is not None:   # every finer part lies in one coarser part
            pairs = np.unique(np.stack([finer[finer > 0], L[finer > 0]], 1), axis=0)
            assert len(pairs) == len(np.unique(pairs[:, 0]))
        finer = L
        # the surviving peak is the part's voxel of greatest key, and the parts are numbered by it
        xyz, heights = WR.part_peaks(L, H, n)
        flat = (xyz[:, 2].astype(np.int64) * H.shape[1] + xyz[:, 1]) * H.shape[2] + xyz[:, 0]
        fin = w.final(h)
        assert np.array_equal(flat, w.peaks[np.flatnonzero(fin == np.arange(len(fin)))]) and np.array_equal(heights, H.ravel()[flat])
        assert (np.diff(flat) > 0).all() and all(K.ravel()[flat[i]] == K[L == i + 1].max() for i in range(0, n, max(1, n // 7)))
    assert counts == sorted(counts, reverse=True) and counts[0] == len(w.peaks) and counts[0] > counts[-1]
    assert np.array_equal(w.labels(0)[0].ravel()[w.basin >= 0], 1 + np.searchsorted(w.peaks, w.basin[w.basin >= 0]))   # h = 0: the ascent basins


def test_pinned_results():
    S = WR.dumbbell()
    H = WR.squared_edt(S)
    assert int(S.sum()) == 7827 and np.array_equal(H > 0, S)
    w = WR.Watershed(H, 26)
    assert (len(w.peaks), len(w.a), w.seen, sorted(w.pers)) == (2, 1, 1413, [49, WR.INF])
    for h in (0, 1, 49):
        L, n = w.labels(h)
        assert n == 2 and np.bincount(L.ravel())[1:].tolist() == [3833, 3994]
    assert w.labels(50)[1] == 1
    w = WR.Watershed(H, 6)
    assert len(w.peaks) == 6 and sorted(w.pers)[:5] == [0, 0, 0, 0, 49]
    for h in (1, 49):
        L, n = w.labels(h)
        assert n == 2 and np.bincount(L.ravel())[1:].tolist() == [3832, 3995]
    assert [WR.watershed(WR.flat_u(), h, 26)[1] for h in (0, 1)] == [2, 1]
    R = WR.random_relief()
    assert R.shape == (17, 19, 70)
    w = WR.Watershed(R, 6)
    assert (len(w.peaks), len(w.a)) == (3183, 13042) and [w.labels(h)[1] for h in (1, 2, 3, 6)] == [2554, 852, 111, 1]
    assert len(WR.Watershed(R, 18).peaks) == 897 and len(WR.Watershed(R, 26).peaks) == 523
    B = np.full((3, 4, 5), 7, np.int32)
    L, n = WR.watershed(B)
    xyz, heights = WR.part_peaks(L, B, n)
    assert n == 1 and (L == 1).all() and xyz.tolist() == [[4, 3, 2]] and heights.tolist() == [7]          # a flat box: its last voxel
    L, n = WR.watershed(np.zeros((3, 4, 5), np.int32), 3)
    assert n == 0 and not L.any()
    assert WR.watershed(np.array([[[5]]], np.int32), 2)[0].tolist() == [[[1]]]
    neg = np.array([[[-5, 3, -(2 ** 31), 2 ** 31 - 1, 0, 1]]], np.int32)
    assert WR.watershed(neg, 0)[0].tolist() == [[[0, 1, 0, 2, 0, 3]]]


# ---- the kernel header's plain part on the host ------------------------------------------------------------------------------------

HOST_WS = r"""
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>
#define O2V_WS_HOST
#define O2V_WS_FN static inline
static inline uint32_t ws_load(const uint32_t *p) { return *p; }
static inline void ws_store(uint32_t *p, uint32_t v) { *p = v; }
static inline uint64_t cas64(unsigned long long *p, uint64_t expect, uint64_t v) { const uint64_t old = *p; if (old == expect) *p = v; return old; }
static inline void ws_max32(uint32_t *p, uint32_t v) { if (*p < v) *p = v; }
constexpr uint32_t kCcTileRows = 64u, kCcTileVoxels = 4096u;
%s
extern "C" uint64_t ws_host_key(int32_t h, uint32_t i) { return ws_key(h, i); }
extern "C" void ws_host_offsets(uint32_t conn, int32_t *out /* [27][4]: on, dx, dy, dz */)
{
    for (int k = 0; k < 27; ++k) out[4 * k] = ws_offset_on(conn, k), out[4 * k + 1] = ws_dx(k), out[4 * k + 2] = ws_dy(k), out[4 * k + 3] = ws_dz(k);
}

// keys / values into a table of 2^log2 slots in the given order; out: per insert ws_table_insert's result.  Then the table's content.
extern "C" void ws_host_table(uint32_t log2, const unsigned long long *k, const uint32_t *v, uint64_t n, int32_t *out, unsigned long long *keys, uint32_t *vals)
{
    for (uint64_t s = 0; s < (1ull << log2); ++s) keys[s] = kPtEmpty, vals[s] = 0u;
    for (uint64_t e = 0; e < n; ++e) out[e] = ws_table_insert(keys, vals, log2, k[e], v[e], cas64);
}

extern "C" uint32_t ws_host_merge(uint32_t n, const uint32_t *index, const int32_t *h, uint64_t m, const unsigned long long *keys, const uint32_t *vals,
                                  uint32_t min_depth, int32_t *label_of_rank)
{
    return ws_merge(n, index, h, m, keys, vals, min_depth, label_of_rank);
}

// The stages in the kernels' order on a contiguous relief, a "lane" at a time: the ascent tile by tile in an order shuffled by
// `shuffle` (no_tiles: voxel by voxel, P = the parent), the flatten voxel by voxel in a shuffled order, the peaks by rank, the pairs
// through the table (doubled while a probe run overflows), the merge, the labels.  out6: the counters of the C-ABI.
extern "C" int ws_host(const int32_t *H, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t conn, uint32_t min_depth, int no_tiles, uint32_t shuffle,
                       uint32_t table_log2, int32_t *labels, uint64_t *out6)
{
    BitGrid g;
    g.nx = nx, g.ny = ny, g.nz = nz, g.W = (nx + 63u) / 64u, g.words = (uint64_t) g.W * ny * nz;
    const uint32_t tiles_y = (ny + 7u) / 8u, tiles_z = (nz + 7u) / 8u, tiles = g.W * tiles_y * tiles_z, sy = nx, sz = nx * ny, voxels = nx * ny * nz;
    std::mt19937 rng(shuffle);
    std::vector<uint32_t> P(voxels, 0x12345678u), order(tiles);
    const auto at = [&](uint32_t x, uint32_t y, uint32_t z) { return x < nx && y < ny && z < nz ? H[(z * ny + y) * nx + x] : 0; };
    if (no_tiles) {
        for (uint32_t i = 0; i < voxels; ++i) {
            const uint32_t x = i %% nx, y = i / nx %% ny, z = i / sz;
            if (H[i] <= 0) { P[i] = kWsOutside; continue; }
            const int k = ws_ascent_step(conn, H[i], i, sy, sz, [&](int n) { return at(x + (uint32_t) ws_dx(n), y + (uint32_t) ws_dy(n), z + (uint32_t) ws_dz(n)); });
            P[i] = k < 0 ? i : ws_neighbour(i, k, sy, sz);
        }
    } else {
        for (uint32_t t = 0; t < tiles; ++t) order[t] = t;
        std::shuffle(order.begin(), order.end(), rng);
        static int32_t s_h[kWsHalo];
        static uint32_t s_q[kCcTileVoxels];
        for (const uint32_t tile : order) {
            uint32_t tx, ty, tz;
            bits_tile_at(g, tiles_y, tile, tx, ty, tz);
            const uint32_t x0 = tx * 64u, y0 = ty * 8u, z0 = tz * 8u;
            for (uint32_t e = 0; e < kWsHalo; ++e) {
                const uint32_t r = e / kWsHaloX, hx = e - r * kWsHaloX, hz = r / kWsHaloY, hy = r - hz * kWsHaloY;
                const int32_t v = at(x0 + hx - 1u, y0 + hy - 1u, z0 + hz - 1u);
                s_h[e] = v > 0 ? v : 0;
            }
            std::memset(s_q, 0x5a, sizeof s_q);
            for (int pass = 0; pass < 2; ++pass)
                for (uint32_t l = 0; l < kCcTileVoxels; ++l) {
                    const uint32_t lx = l & 63u, ly = (l >> 6) & 7u, lz = l >> 9, x = x0 + lx, y = y0 + ly, z = z0 + lz;
                    if (x >= nx || y >= ny || z >= nz) continue;
                    const uint32_t c = ((lz + 1u) * kWsHaloY + ly + 1u) * kWsHaloX + lx + 1u, i = (z * ny + y) * nx + x;
                    if (pass == 1) { P[i] = s_h[c] > 0 ? ws_follow(s_q, l) : kWsOutside; continue; }
                    if (s_h[c] <= 0) continue;
                    const int k = ws_ascent_step(conn, s_h[c], i, sy, sz, [&](int n) { return s_h[(int) c + ws_dx(n) + ws_dy(n) * (int) kWsHaloX + ws_dz(n) * (int) (kWsHaloX * kWsHaloY)]; });
                    s_q[l] = ws_tile_word(k, lx, ly, lz, i, sy, sz);
                }
        }
    }
    std::vector<uint32_t> walk(voxels);
    for (uint32_t i = 0; i < voxels; ++i) walk[i] = i;
    std::shuffle(walk.begin(), walk.end(), rng);
    for (const uint32_t i : walk)
        if (P[i] != kWsOutside) { const uint32_t r = ws_root(P.data(), i); if (r != i) P[i] = r; }
    std::vector<uint32_t> index, rank(voxels, 0u);
    std::vector<int32_t> height;
    for (uint32_t i = 0; i < voxels; ++i)
        if (P[i] == i) rank[i] = (uint32_t) index.size(), index.push_back(i), height.push_back(H[i]);
    const uint32_t n = (uint32_t) index.size();
    std::vector<int32_t> lab(n);
    for (uint32_t r = 0; r < n; ++r) lab[r] = (int32_t) r + 1;
    uint64_t seen = 0, distinct = 0, growths = 0, bytes = 0, survivors = n;
    if (min_depth > 0u && n >= 2u) {
        std::vector<unsigned long long> keys, list_k;
        std::vector<uint32_t> vals, list_v;
        uint32_t log2 = table_log2;
        if (!log2) for (log2 = kPtMinLog2; (1ull << log2) < 16ull * n; ++log2) {}
        for (;; ++log2, ++growths) {
            keys.assign(1ull << log2, kPtEmpty), vals.assign(1ull << log2, 0u);
            bool overflow = false;
            seen = distinct = 0;
            for (const uint32_t i : walk) {
                if (P[i] == kWsOutside) continue;
                const uint32_t x = i %% nx, y = i / nx %% ny, z = i / sz;
                for (int k = 0; k < 13; ++k) {
                    if (!ws_offset_on(conn, k)) continue;
                    const uint32_t X = x + (uint32_t) ws_dx(k), Y = y + (uint32_t) ws_dy(k), Z = z + (uint32_t) ws_dz(k);
                    if (X >= nx || Y >= ny || Z >= nz) continue;
                    const uint32_t j = ws_neighbour(i, k, sy, sz);
                    if (P[j] == kWsOutside || P[j] == P[i]) continue;
                    const int got = ws_table_insert(keys.data(), vals.data(), log2, pt_key(P[i], P[j]), (uint32_t) std::min(H[i], H[j]), cas64);
                    ++seen, distinct += got > 0, overflow |= got < 0;
                }
            }
            if (!overflow) break;
        }
        bytes = 12ull << log2;
        for (uint64_t s = 0; s < keys.size(); ++s)
            if (keys[s] != kPtEmpty) list_k.push_back(keys[s]), list_v.push_back(vals[s]);
        if (list_k.size() != distinct) return 1;
        survivors = ws_merge(n, index.data(), height.data(), distinct, list_k.data(), list_v.data(), min_depth, lab.data());
    }
    for (uint32_t i = 0; i < voxels; ++i) labels[i] = P[i] == kWsOutside ? 0 : lab[rank[P[i]]];
    out6[0] = n, out6[1] = seen, out6[2] = distinct, out6[3] = growths, out6[4] = bytes, out6[5] = survivors;
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_ws(tmp_path_factory):
    """build(defines) -> a library with the part of o2v_dev_k23_watershed.hpp between its constants and "kernels", compiled for the
    host behind the plain parts of o2v_dev_bits.hpp and o2v_dev_pair_table.hpp."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    text = open(K23).read()
    consts = text[text.index("constexpr uint32_t kWsOutside"):text.index("#ifndef O2V_WS_HOST")]
    part = text[text.index("// ---- the key, the offsets"):text.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_ws")
    built = {}

    def build(defines=()):
        if defines not in built:
            name = "ws_%d" % len(built)
            (tmp / (name + ".cpp")).write_text(HOST_WS % (bits_host.plain_part() + pair_table_host.plain_part() + consts + part))
            subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                           [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
            L = hip.C.CDLL(str(tmp / (name + ".so")))
            L.ws_host_key.restype = hip.C.c_uint64
            L.ws_host_key.argtypes = [hip.C.c_int32, hip.C.c_uint32]
            L.ws_host_merge.restype = hip.C.c_uint32
            built[defines] = L
        return built[defines]
    return build


def host_run(L, H, connectivity, min_depth, no_tiles=False, shuffle=1, table_log2=0):
    """(labels, the six counters) of the host build."""
    C = hip.C
    H = np.ascontiguousarray(H, np.int32)
    nz, ny, nx = H.shape
    labels, out6 = np.full(H.shape, -7, np.int32), np.zeros(6, np.uint64)
    rc = L.ws_host(C.c_void_p(H.ctypes.data), nx, ny, nz, connectivity, C.c_uint32(min_depth), int(no_tiles), shuffle, table_log2, C.c_void_p(labels.ctypes.data),
                   C.c_void_p(out6.ctypes.data))
    assert rc == 0
    return labels, tuple(int(v) for v in out6)


def test_the_key_and_the_offset_sets(host_ws):
    L = host_ws()
    for h, i in ((1, 0), (5, 77), (2 ** 31 - 1, 2 ** 31 - 2)):
        assert L.ws_host_key(h, i) == (h << 31 | i)
    assert L.ws_host_key(3, 5) > L.ws_host_key(2, 2 ** 31 - 2) and L.ws_host_key(3, 6) > L.ws_host_key(3, 5)
    for connectivity in CONNECTIVITIES:
        out = np.zeros((27, 4), np.int32)
        L.ws_host_offsets(connectivity, hip.C.c_void_p(out.ctypes.data))
        on = [(int(dz), int(dy), int(dx)) for o, dx, dy, dz in out if o]
        assert on == WR.offsets(connectivity) and len(on) == connectivity
        assert [tuple(r[1:]) for r in out.tolist()] == [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        assert sum(1 for k in range(13) if out[k, 0]) == {6: 3, 18: 9, 26: 13}[connectivity]          # the earlier neighbours


def test_the_table_keeps_the_distinct_keys_and_their_maxima(host_ws):
    L, C = host_ws(), hip.C
    rng = np.random.default_rng(23)
    distinct = (rng.integers(0, 2 ** 31, 300, dtype=np.uint64) << np.uint64(32)) | rng.integers(0, 2 ** 31, 300, dtype=np.uint64)
    k = np.ascontiguousarray(distinct[rng.integers(0, 300, 5000)])
    v = rng.integers(1, 2 ** 31, 5000).astype(np.uint32)
    want = {}
    for key, val in zip(k.tolist(), v.tolist()):
        want[key] = max(want.get(key, 0), val)
    for log2 in (9, 10, 14):
        out, keys, vals = np.zeros(5000, np.int32), np.zeros(1 << log2, np.uint64), np.zeros(1 << log2, np.uint32)
        L.ws_host_table(log2, C.c_void_p(k.ctypes.data), C.c_void_p(v.ctypes.data), 5000, *[C.c_void_p(a.ctypes.data) for a in (out, keys, vals)])
        taken = keys != np.uint64(2 ** 64 - 1)
        assert (out >= 0).all() and int((out == 1).sum()) == len(want) == int(taken.sum())
        assert dict(zip(keys[taken].tolist(), vals[taken].tolist())) == want
    # a table too small reports overflow (-1) and never writes outside its slots
    for log2 in (3, 7):
        out, keys, vals = np.zeros(5000, np.int32), np.zeros((1 << log2) + 1, np.uint64), np.zeros((1 << log2) + 1, np.uint32)
        keys[-1], vals[-1] = 99, 98
        L.ws_host_table(log2, C.c_void_p(k.ctypes.data), C.c_void_p(v.ctypes.data), 5000, *[C.c_void_p(a.ctypes.data) for a in (out, keys, vals)])
        assert (out == -1).any() and (keys[-1], vals[-1]) == (99, 98) and int((out == 1).sum()) <= 1 << log2


def test_the_merge_equals_the_reference(host_ws):
    L, C = host_ws(), hip.C
    for connectivity in CONNECTIVITIES:
        w = WR.Watershed(np.random.default_rng(5).integers(0, 7, (9, 10, 30)).astype(np.int32), connectivity)
        order = np.random.default_rng(6).permutation(len(w.a))
        keys = np.ascontiguousarray(((w.a.astype(np.uint64) << np.uint64(32)) | w.b.astype(np.uint64))[order])
        vals = np.ascontiguousarray(w.saddle[order].astype(np.uint32))
        index, heights = np.ascontiguousarray(w.peaks.astype(np.uint32)), np.ascontiguousarray(w.heights.astype(np.int32))
        for h in (1, 2, 3, 6, 2 ** 31 - 1, 2 ** 32 - 1):
            lab = np.zeros(len(index), np.int32)
            n = L.ws_host_merge(len(index), C.c_void_p(index.ctypes.data), C.c_void_p(heights.ctypes.data), len(keys), C.c_void_p(keys.ctypes.data),
                                C.c_void_p(vals.ctypes.data), C.c_uint32(h), C.c_void_p(lab.ctypes.data))
            want, count = w.labels(h)
            assert n == count and np.array_equal(lab, want.ravel()[w.peaks])


def tile_reliefs():
    rng = np.random.default_rng(26)
    yield "random 0..5", rng.integers(0, 6, (17, 19, 130)).astype(np.int32)
    yield "random int32", rng.integers(-2 ** 31, 2 ** 31, (9, 17, 70)).astype(np.int32)
    x = np.arange(140)
    for name, h in (("staircase up", x + 1), ("staircase down", 140 - x)):
        H = np.zeros((21, 21, 140), np.int32)
        H[np.minimum(x // 7, 19), np.minimum(x // 7, 19), x] = h
        yield name, H
    yield "dumbbell", WR.squared_edt(WR.dumbbell())
    yield "flat", np.full((9, 9, 65), 3, np.int32)


@pytest.mark.parametrize("no_tiles", [False, True])
def test_the_kernels_stages_on_the_host_equal_the_reference(host_ws, no_tiles):
    L = host_ws()
    for name, H in tile_reliefs():
        for connectivity in CONNECTIVITIES:
            w = WR.Watershed(H, connectivity)
            for h in (0, 1, 3, 2 ** 31 - 1):
                want, n = w.labels(h)
                for shuffle in (1, 2):
                    got, counters = host_run(L, H, connectivity, h, no_tiles, shuffle)
                    assert np.array_equal(got, want) and counters[0] == len(w.peaks) and counters[5] == n, (name, connectivity, h)
                    if h and len(w.peaks) >= 2:
                        assert counters[1:3] == (w.seen, len(w.a)), (name, connectivity)
    # a staircase is one part whose peak is its high end
    H = dict(tile_reliefs())["staircase up"]
    got, counters = host_run(L, H, 26, 0, no_tiles)
    assert counters[0] == 1 and WR.part_peaks(got, H, 1)[0].tolist() == [[139, 19, 19]]


def test_the_table_may_start_small(host_ws):
    L = host_ws()
    R = WR.random_relief()
    want, n = WR.Watershed(R, 6).labels(2)
    free, c0 = host_run(L, R, 6, 2)
    small, c1 = host_run(L, R, 6, 2, table_log2=4)
    assert np.array_equal(free, want) and np.array_equal(small, want) and n == 852
    assert c0[2] == c1[2] == 13042 and c0[3] == 0 and c1[3] >= 2 and c1[:3] == c0[:3]


def test_the_dropped_offset_is_caught(host_ws):
    """-DO2V_WS_MUTATE_DROP_DIAGONAL leaves the offset (+1, +1, -1) out of the ascent and of the pairs: other basins at 26
    neighbours, where it is the only way up for some voxels; 6 and 18 neighbours never had it."""
    L = host_ws(("O2V_WS_MUTATE_DROP_DIAGONAL",))
    R = WR.random_relief()
    differs = {c: not np.array_equal(host_run(L, R, c, 0)[0], WR.watershed(R, 0, c)[0]) for c in CONNECTIVITIES}
    assert differs == {6: False, 18: False, 26: True}
    assert np.array_equal(host_run(host_ws(), R, 26, 0)[0], WR.watershed(R, 0, 26)[0])


# ---- the torch layer against a stand-in ------------------------------------------------------------------------------------------------

class WsStub(StubVoxelizer):
    """Computes with the reference, on the tensors' own memory (CPU)."""

    def watershed_dense(self, relief_ptr, strides, dims, connectivity, min_depth, flags, labels_ptr, labels_strides):
        self.calls.append(("watershed", relief_ptr, tuple(strides), tuple(dims), connectivity, min_depth, flags, labels_ptr, tuple(labels_strides)))
        C = hip.C
        nx, ny, nz = dims

        def view(ptr, st):
            span = sum((d - 1) * s for d, s in zip(dims, st)) + 1
            raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), (span,))
            return np.lib.stride_tricks.as_strided(raw, (nz, ny, nx), (4 * st[2], 4 * st[1], 4 * st[0]))
        L, n = WR.watershed(view(relief_ptr, strides), min_depth, connectivity)
        view(labels_ptr, labels_strides)[...] = L
        return n

    def thickness_dense(self, grid_ptr, fmt, strides, dims, level, flags, cap, dst_ptr, dst_strides, depth2_ptr, depth2_strides):
        self.calls.append(("thickness", grid_ptr, flags))
        C = hip.C
        nx, ny, nz = dims

        def view(ptr, st, ctype, size):
            span = sum((d - 1) * s for d, s in zip(dims, st)) + 1
            raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (span,))
            return np.lib.stride_tricks.as_strided(raw, (nz, ny, nx), (size * st[2], size * st[1], size * st[0]))
        assert fmt == hip.GRID_U8 and flags & hip.THICK_BORDER and not flags & hip.THICK_BACKGROUND
        view(depth2_ptr, depth2_strides, C.c_int32, 4)[...] = WR.squared_edt(view(grid_ptr, strides, C.c_uint8, 1) != 0)


def test_watershed_arguments(on_cpu):  # noqa: F811
    dv = WsStub()
    R = WR.random_relief(3, (5, 6, 20))
    relief = torch.from_numpy(R)
    L, n = dense.watershed(dv, relief)
    assert dv.calls[-1][2:7] == ((1, 20, 120), (20, 6, 5), 26, 0, 0) and dv.calls[-1][8] == (1, 20, 120)
    want = WR.watershed(R, 0, 26)
    assert L.dtype == torch.int32 and L.is_contiguous() and np.array_equal(L.numpy(), want[0]) and n == want[1]
    L, n = dense.watershed(dv, relief, min_depth=2, connectivity=6)
    want = WR.watershed(R, 2, 6)
    assert dv.calls[-1][4:6] == (6, 2) and np.array_equal(L.numpy(), want[0]) and n == want[1]
    # views of relief and out=: written as they are
    wide = torch.zeros((5, 6, 40), dtype=torch.int32)
    wide[:, :, ::2] = relief
    out = torch.full((3, 5, 6, 20), 9, dtype=torch.int32)
    got, n2 = dense.watershed(dv, wide[:, :, ::2], min_depth=2, connectivity=6, out=out[1])
    assert dv.calls[-1][2] == (2, 40, 240) and got.data_ptr() == out[1].data_ptr() and n2 == n and np.array_equal(out[1].numpy(), want[0])
    assert bool((out[0] == 9).all()) and bool((out[2] == 9).all())
    swapped = torch.full((6, 5, 20), 9, dtype=torch.int32).permute(1, 0, 2)
    dense.watershed(dv, relief, min_depth=2, connectivity=6, out=swapped)
    assert dv.calls[-1][8] == (1, 100, 20) and np.array_equal(swapped.numpy(), want[0])
    dense.watershed(dv, relief, min_depth=2 ** 32 - 1)
    assert dv.calls[-1][5] == 2 ** 32 - 1
    # watershed_peaks: per label the voxel of greatest key
    xyz, heights = dense.watershed_peaks(torch.from_numpy(want[0]), relief, n)
    ref = WR.part_peaks(want[0], R, n)
    assert xyz.dtype == heights.dtype == torch.int32 and np.array_equal(xyz.numpy(), ref[0]) and np.array_equal(heights.numpy(), ref[1])
    empty = dense.watershed_peaks(torch.zeros((2, 2, 2), dtype=torch.int32), torch.zeros((2, 2, 2), dtype=torch.int32), 0)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)
    for text in ("section 26", "greatest key", "not by slope", "plateau"):
        assert text in " ".join(dense.watershed.__doc__.split())


I32 = torch.ones((4, 4, 4), dtype=torch.int32)


@pytest.mark.parametrize("kw, exc", [
    (dict(relief=torch.zeros((4, 4, 4))), TypeError), (dict(relief=torch.zeros((4, 4, 4), dtype=torch.uint8)), TypeError),
    (dict(relief=np.zeros((4, 4, 4), np.int32)), ValueError), (dict(relief=torch.zeros((4, 4), dtype=torch.int32)), ValueError),
    (dict(relief=torch.zeros((4, 0, 4), dtype=torch.int32)), ValueError), (dict(relief=torch.zeros((4, 4, 4), dtype=torch.int32, device="meta")), ValueError),
    (dict(relief=torch.zeros((1, 1, 1), dtype=torch.int32).expand(1, 1, 65537)), ValueError),
    (dict(relief=torch.zeros((1, 1, 1), dtype=torch.int32).expand(2048, 1024, 1024)), ValueError),
    (dict(min_depth=-1), ValueError), (dict(min_depth=1.0), ValueError), (dict(min_depth=True), ValueError), (dict(min_depth=2 ** 32), ValueError),
    (dict(connectivity=8), ValueError), (dict(connectivity=True), ValueError), (dict(connectivity="26"), ValueError),
    (dict(out=torch.zeros((4, 4, 4))), TypeError), (dict(out=torch.zeros((4, 4, 5), dtype=torch.int32)), ValueError),
    (dict(out=torch.zeros((4, 4, 4), dtype=torch.int32, device="meta")), ValueError), (dict(out=I32), ValueError), (dict(out=I32.transpose(0, 2)), ValueError),
])
def test_watershed_rejects(on_cpu, kw, exc):  # noqa: F811
    dv = WsStub()
    args = dict(relief=I32)
    args.update(kw)
    with pytest.raises(exc):
        dense.watershed(dv, args.pop("relief"), **args)
    assert not dv.calls


@pytest.mark.parametrize("kw", [dict(min_depth=-0.5), dict(min_depth="1"), dict(min_depth=float("inf")), dict(min_depth=float("nan")), dict(min_depth=True),
                                dict(scale=0), dict(scale=2.0), dict(scale=2 ** 15 + 1), dict(connectivity=7), dict(min_depth=2.0 ** 20, scale=2 ** 15)])
def test_split_parts_rejects(on_cpu, kw):  # noqa: F811
    dv = WsStub()
    with pytest.raises(ValueError):
        dense.split_parts(dv, torch.ones((4, 4, 4), dtype=torch.uint8), **kw)
    assert not dv.calls
    for args, exc in (((torch.zeros((2, 2, 2)), I32[:2, :2, :2], 1), ValueError), ((I32, I32[:2], 1), ValueError), ((I32, I32, -1), ValueError)):
        with pytest.raises(exc):
            dense.watershed_peaks(*args)


def test_split_parts(on_cpu):  # noqa: F811
    dv = WsStub()
    S = WR.dumbbell()
    D = WR.squared_edt(S)
    for min_depth, scale, parts in ((1.0, 4, 2), (3.25, 4, 1), (0, 1, None)):
        L, n = dense.split_parts(dv, torch.from_numpy(S), min_depth=min_depth, scale=scale)
        relief = np.array([math.isqrt(int(v) * scale * scale) for v in D.ravel()], np.int32).reshape(D.shape)
        steps = int(np.ceil(min_depth * scale))
        want = WR.watershed(relief, steps, 26)
        assert [c[0] for c in dv.calls[-2:]] == ["thickness", "watershed"] and dv.calls[-1][4:6] == (26, steps)
        assert np.array_equal(L.numpy(), want[0]) and n == want[1] and (parts is None or n == parts)
    for text in ("section 26", "not a connected component", "not smoothed"):
        assert text in " ".join(dense.split_parts.__doc__.split())


def test_the_scaled_root_is_exact():
    roots = np.array([0, 1, 2, 3, 255, 256, 1000, 46340], np.int64)
    values = np.unique(np.clip(np.concatenate([roots ** 2 - 1, roots ** 2, roots ** 2 + 1, [0x7FFFFFFF, 0x7FFFFFFE]]), 0, 0x7FFFFFFF))
    d = torch.from_numpy(values.astype(np.int32))
    for scale in (1, 3, 4, 1000, 2 ** 15):
        got = WS.scaled_root(d, scale)
        assert got.dtype == torch.int32 and got.tolist() == [math.isqrt(int(v) * scale * scale) for v in values]
    assert WS.scaled_root(torch.tensor([0x7FFFFFFF], dtype=torch.int32), 2 ** 15).item() == math.isqrt(0x7FFFFFFF << 30) < 2 ** 31


def test_refused_when_the_library_came_first(monkeypatch):
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: False)
    with pytest.raises(RuntimeError, match="before torch"):
        dense.watershed(WsStub(), I32)


def test_a_wait_comes_before_the_library(monkeypatch):
    dv = WsStub()
    own = torch.device("cpu")
    monkeypatch.setattr(dense, "_device", lambda v: own)
    monkeypatch.setattr(dense, "_sync", lambda device: dv.calls.append(("sync", device)))
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: True)
    dense.watershed(dv, I32.clone())
    names = [c[0] for c in dv.calls]
    assert "watershed" in names and "sync" in names[:names.index("watershed")] and all(c[1] is own for c in dv.calls if c[0] == "sync")
    del dv.calls[:]
    dense.split_parts(dv, torch.ones((4, 4, 4), dtype=torch.uint8))
    names = [c[0] for c in dv.calls]
    assert names.index("sync") < names.index("thickness") < names.index("watershed") and "sync" in names[names.index("thickness"):names.index("watershed")]


# ---- the scratch formula and the code object -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(1, 1, 1), (64, 8, 8), (65, 9, 9), (1024, 1024, 1024), (65536, 1, 7), (1000, 999, 17)])
def test_scratch_bytes_formula(dims):
    words = -(-dims[0] // 64) * dims[1] * dims[2]
    want = 4 * dims[0] * dims[1] * dims[2] + 12 * words + 8 * (-(-words // 256) + 1) + 64
    assert hip.watershed_scratch_bytes(dims) == want == hip.DeviceVoxelizer.watershed_scratch_bytes(None, dims)
    assert hip.watershed_scratch_bytes((4, 0, 4)) == 0


K23_KERNELS = ["k_ws_ascent_tilesE", "k_ws_ascentE", "k_ws_flattenE", "k_ws_peaksE", "k_ws_pairsILb0EE", "k_ws_pairsILb1EE", "k_pt_listIjLj1EE", "k_ws_labelsE"]
ASCENT_LDS = 66 * 10 * 10 * 4 + 4096 * 4   # the relief with its halo and a word per voxel of the tile: the kernel's comment, DESIGN.md section 26


@pytest.mark.parametrize("kernel", K23_KERNELS)
def test_k23_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    """From the code object's metadata only: no scratch, and the LDS bytes the ascent kernel's comment states."""
    meta = device_asm[device_asm.index("amdhsa.kernels:"):]
    entry = [e for e in meta.split("\n  - ") if re.search(r"\.name: +_ZN\S*" + kernel + r"\S*\n", e)]
    assert len(entry) == 1, kernel + " is not in the gfx950 code object"
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
    assert int(re.search(r"\.wavefront_size: +(\d+)", entry[0]).group(1)) == 64 and int(re.search(r"\.max_flat_workgroup_size: +(\d+)", entry[0]).group(1)) == 256
    lds = int(re.search(r"\.group_segment_fixed_size: +(\d+)", entry[0]).group(1))
    assert lds == (ASCENT_LDS if "tiles" in kernel else 0)
    text = open(K23).read()
    assert "26 400 bytes" in text and "16 384 bytes" in text and ASCENT_LDS == 26400 + 16384


def test_the_new_source_has_no_waiting_loop():
    """No kernel of K23 waits for another workgroup, lane or flag: nothing in the kernels polls or sleeps.  (The loops of ws_root,
    ws_follow and ws_table_insert end on their own: a key rises, a probe run is bounded.)"""
    text = open(K23).read()
    kernels = text[text.index("// ---- kernels"):]
    assert "s_sleep" not in kernels and "while (" not in kernels and "for (;;)" not in kernels
