"""The bit grid that K12, K13, K14, K16 and K20 share, without a GPU: the plain C++ part of
o2v_dev_bits.hpp compiled for the host - word <-> coordinates, membership, the faces of the box, tiles and their row words -
against plain div / mod on small grids whose rows end inside, at and just behind a word, and the arithmetic alone at the last
word and tile of the largest grids that the two host limits admit (index_limits: 2^31 - 1 voxels; ga_grid: 2^31 - 1 words; no
axis above 65 536)."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import bits_host

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

HOST_BITS = r"""
#include <cstdint>
%s
static BitGrid grid(uint32_t nx, uint32_t ny, uint32_t nz)
{
    BitGrid g;
    g.nx = nx, g.ny = ny, g.nz = nz, g.W = (nx + 63u) / 64u, g.words = (uint64_t) g.W * ny * nz;
    return g;
}
// every word, voxel (padding included) and tile of a small grid
extern "C" void bits_all(const unsigned long long *bits, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t *word_at, uint64_t *index_back, uint8_t *has,
                         uint8_t *face, uint32_t *tile_at, uint64_t *tile_words)
{
    const BitGrid g = grid(nx, ny, nz);
    for (uint64_t wi = 0; wi < g.words; ++wi) {
        const BitWord at = bits_word_at(g, wi);
        word_at[3u * wi] = at.wx, word_at[3u * wi + 1u] = at.y, word_at[3u * wi + 2u] = at.z;
        index_back[wi] = bits_word_index(g, at.wx, at.y, at.z);
    }
    for (uint32_t z = 0; z < nz; ++z)
        for (uint32_t y = 0; y < ny; ++y)
            for (uint32_t x = 0; x < g.W * 64u; ++x) {
                const uint64_t i = ((uint64_t) z * ny + y) * g.W * 64u + x;
                has[i] = x < nx && bits_has(g, bits, x, y, z);
                face[i] = bits_on_face(g, x, y, z);
            }
    const uint32_t tiles_y = (ny + 7u) / 8u, tiles_z = (nz + 7u) / 8u;
    for (uint32_t tile = 0; tile < g.W * tiles_y * tiles_z; ++tile) {
        uint32_t *const o = tile_at + 3u * tile;
        bits_tile_at(g, tiles_y, tile, o[0], o[1], o[2]);
        for (uint32_t row = 0; row < 64u; ++row) tile_words[64u * tile + row] = bits_tile_word(g, bits, o[0], o[1], o[2], row);
    }
}
// one word and one tile of a grid of any size: arithmetic only
extern "C" uint64_t bits_one(uint32_t nx, uint32_t ny, uint32_t nz, uint64_t wi, uint32_t tile, uint32_t *word_at, uint32_t *tile_at)
{
    const BitGrid g = grid(nx, ny, nz);
    const BitWord at = bits_word_at(g, wi);
    word_at[0] = at.wx, word_at[1] = at.y, word_at[2] = at.z;
    bits_tile_at(g, (ny + 7u) / 8u, tile, tile_at[0], tile_at[1], tile_at[2]);
    return bits_word_index(g, word_at[0], word_at[1], word_at[2]);
}
"""


@pytest.fixture(scope="module")
def host_bits(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    tmp = tmp_path_factory.mktemp("host_bits")
    (tmp / "bits.cpp").write_text(HOST_BITS % bits_host.plain_part())
    subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC", str(tmp / "bits.cpp"), "-o", str(tmp / "bits.so")], check=True,
                   capture_output=True)
    L = C.CDLL(str(tmp / "bits.so"))
    L.bits_all.argtypes = [C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p] * 6
    L.bits_all.restype = None
    L.bits_one.argtypes = [C.c_uint32] * 3 + [C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    L.bits_one.restype = C.c_uint64
    return L


def test_words_membership_faces_and_tiles_equal_plain_div_mod(host_bits):
    rng = np.random.default_rng(15)
    for nx, ny, nz in itertools.product((1, 63, 64, 65, 129), (1, 2, 9), (1, 2, 9)):
        W, ty, tz = -(-nx // 64), -(-ny // 8), -(-nz // 8)
        words, tiles = W * ny * nz, W * ty * tz
        S = rng.random((nz, ny, nx)) < 0.5
        pad = np.zeros((nz, ny, W * 64), bool)
        pad[:, :, :nx] = S
        bits = np.ascontiguousarray((pad.reshape(-1, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64))
        word_at, back = np.zeros((words, 3), np.uint32), np.zeros(words, np.uint64)
        has, face = np.zeros(pad.shape, np.uint8), np.zeros(pad.shape, np.uint8)
        tile_at, tile_words = np.zeros((tiles, 3), np.uint32), np.zeros((tiles, 64), np.uint64)
        host_bits.bits_all(bits.ctypes.data, nx, ny, nz, word_at.ctypes.data, back.ctypes.data, has.ctypes.data, face.ctypes.data, tile_at.ctypes.data,
                           tile_words.ctypes.data)
        dims = (nx, ny, nz)
        wi = np.arange(words)
        assert np.array_equal(word_at, np.stack([wi % W, wi // W % ny, wi // W // ny], axis=1)), dims
        assert np.array_equal(back, wi), dims                         # the inverse
        assert np.array_equal(has.astype(bool), pad), dims
        z, y, x = np.indices(pad.shape)
        assert np.array_equal(face.astype(bool), (x == 0) | (x == nx - 1) | (y == 0) | (y == ny - 1) | (z == 0) | (z == nz - 1)), dims
        t = np.arange(tiles)
        assert np.array_equal(tile_at, np.stack([t % W, t // W % ty, t // W // ty], axis=1)), dims
        # a tile's 64 row words: row = (y % 8) + 8 (z % 8), 0 outside the box
        want = np.zeros((tz * 8, ty * 8, W), np.uint64)
        want[:nz, :ny] = bits.reshape(nz, ny, W)
        want = want.reshape(tz, 8, ty, 8, W).transpose(0, 2, 4, 1, 3).reshape(tiles, 64)
        assert np.array_equal(tile_words, want), dims


def largest_grids():
    """(dims, which limit admits them): no axis above 65 536; 2^31 - 1 voxels (K12, K20) or 2^31 - 1 words (K13, K14, K16)."""
    limit = 2 ** 31 - 1
    for dims in ((65536, 32767, 1), (1, 65536, 32767), (65536, 1, 32767), (46340, 46340, 1), (1, 46340, 46340), (64, 65536, 511), (65, 65536, 504),
                 (1290, 1290, 1290)):
        assert max(dims) <= 65536 and dims[0] * dims[1] * dims[2] <= limit
        yield dims, "voxels"
    for dims in ((65536, 65536, 31), (65536, 31, 65536), (1, 65536, 32767), (65472, 65535, 32), (65473, 65536, 31), (64, 65536, 32767), (65, 32768, 32767),
                 (4096, 65536, 511)):
        assert max(dims) <= 65536 and -(-dims[0] // 64) * dims[1] * dims[2] <= limit
        yield dims, "words"


def test_the_last_word_and_tile_of_the_largest_grids_the_host_admits(host_bits):
    n = 0
    for (nx, ny, nz), _ in largest_grids():
        W, ty, tz = -(-nx // 64), -(-ny // 8), -(-nz // 8)
        words, tiles = W * ny * nz, W * ty * tz
        assert tiles <= words < 2 ** 31
        for wi, tile in ((words - 1, tiles - 1), (words - W, tiles - W), (words // 2, tiles // 2), (0, 0)):
            word_at, tile_at = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
            back = host_bits.bits_one(nx, ny, nz, wi, tile, word_at.ctypes.data, tile_at.ctypes.data)
            assert tuple(int(v) for v in word_at) == (wi % W, wi // W % ny, wi // W // ny), ((nx, ny, nz), wi)
            assert back == wi, ((nx, ny, nz), wi)
            assert tuple(int(v) for v in tile_at) == (tile % W, tile // W % ty, tile // W // ty), ((nx, ny, nz), tile)
            n += 1
    assert n == 64
