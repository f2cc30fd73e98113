"""The table of id pairs that K23 and K24 fill in global memory, without a GPU: the plain C++ part of
o2v_dev_pair_table.hpp compiled for the host alone - the key and the hash against values pinned from the two copies this header
replaced (K23's ws_pair_key / ws_hash, K24's adj_key / adj_hash, which agreed), the probe run at table sizes below, at and above
its limit of 128 slots with keys chosen to meet in one slot, the table's content whatever the order of insertion, and the first
size against values pinned from K23's and K24's former sizing rules."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import pair_table_host

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
EMPTY = NO_PLACE = 2 ** 64 - 1
LIMIT = 128

HOST_PT = r"""
#include <cstdint>
%s
static uint64_t cas64(unsigned long long *p, uint64_t expected, uint64_t desired)
{
    const uint64_t was = *p;
    if (was == expected) *p = desired;
    return was;
}
extern "C" uint64_t pt_host_key(uint32_t a, uint32_t b) { return pt_key(a, b); }
extern "C" uint64_t pt_host_hash(uint64_t key, uint32_t log2) { return pt_hash(key, log2); }
extern "C" uint32_t pt_host_max_axes(uint32_t conn) { return pt_max_axes(conn); }
extern "C" uint32_t pt_host_first_log2(uint64_t ids, int forced, uint32_t first_max_log2, uint32_t max_log2) { return pt_first_log2(ids, forced, first_max_log2, max_log2); }
extern "C" void pt_host_consts(uint64_t *out) { out[0] = kPtEmpty, out[1] = kPtNoPlace, out[2] = kPtProbeLimit, out[3] = kPtMinLog2; }
// n keys into the table as it stands, in the given order: per key pt_slot's result and its `fresh`
extern "C" void pt_host_insert(unsigned long long *keys, uint32_t log2, const unsigned long long *k, uint64_t n, uint64_t *slot, uint8_t *fresh)
{
    for (uint64_t e = 0; e < n; ++e) {
        bool f = true;
        slot[e] = pt_slot(keys, log2, k[e], cas64, f);
        fresh[e] = f;
    }
}
"""


@pytest.fixture(scope="module")
def host_pt(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    tmp = tmp_path_factory.mktemp("host_pt")
    (tmp / "pt.cpp").write_text(HOST_PT % pair_table_host.plain_part())
    subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC", str(tmp / "pt.cpp"), "-o", str(tmp / "pt.so")], check=True, capture_output=True)
    L = C.CDLL(str(tmp / "pt.so"))
    L.pt_host_key.restype = L.pt_host_hash.restype = C.c_uint64
    L.pt_host_key.argtypes = [C.c_uint32, C.c_uint32]
    L.pt_host_hash.argtypes = [C.c_uint64, C.c_uint32]
    L.pt_host_max_axes.restype = L.pt_host_first_log2.restype = C.c_uint32
    L.pt_host_first_log2.argtypes = [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32]
    L.pt_host_insert.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    return L


class Table:
    """A table of 2^log2 free slots with a guard word behind it; insert(keys) -> (slots, fresh) in the given order."""

    def __init__(self, L, log2):
        self.L, self.log2 = L, log2
        self.words = np.full((1 << log2) + 1, EMPTY, np.uint64)
        self.words[-1] = 99

    def insert(self, keys):
        k = np.ascontiguousarray(keys, np.uint64)
        slot, fresh = np.zeros(len(k), np.uint64), np.full(len(k), 7, np.uint8)
        self.L.pt_host_insert(self.words.ctypes.data, self.log2, k.ctypes.data, len(k), slot.ctypes.data, fresh.ctypes.data)
        assert self.words[-1] == 99, "a store behind the table"
        assert set(fresh.tolist()) <= {0, 1}
        return slot.tolist(), fresh.astype(bool).tolist()

    def occupied(self):
        keys = self.words[:-1]
        return sorted(keys[keys != np.uint64(EMPTY)].tolist())


def py_hash(key, log2):
    return ((key * 0x9e3779b97f4a7c15) & (2 ** 64 - 1)) >> (64 - log2) if log2 else 0


# ((a, b), the key, the hash at log2 = 1, 10, 24, 36, 40): what ws_pair_key / ws_hash and adj_key / adj_hash gave
LOG2S = (1, 10, 24, 36, 40)
PAIRS = [
    ((0, 1), 0x0000000000000001, (0x1, 0x278, 0x9e3779, 0x9e3779b97, 0x9e3779b97f)),
    ((1, 0), 0x0000000000000001, (0x1, 0x278, 0x9e3779, 0x9e3779b97, 0x9e3779b97f)),
    ((2147483647, 2147483646), 0x7ffffffe7fffffff, (0x1, 0x28b, 0xa2d8cc, 0xa2d8cc270, 0xa2d8cc2700)),
    ((65535, 65536), 0x0000ffff00010000, (0x0, 0x1da, 0x768403, 0x768403357, 0x768403357c)),
    ((65536, 65535), 0x0000ffff00010000, (0x0, 0x1da, 0x768403, 0x768403357, 0x768403357c)),
    ((1, 2), 0x0000000100000002, (0x1, 0x2ee, 0xbbb96f, 0xbbb96f87f, 0xbbb96f87fe)),
    ((2, 3), 0x0000000200000003, (0x1, 0x364, 0xd93b65, 0xd93b65567, 0xd93b65567d)),
    ((5, 5), 0x0000000500000005, (0x1, 0x24e, 0x9389cd, 0x9389cd087, 0x9389cd087c)),
    ((123456, 654321), 0x0001e2400009fbf1, (0x1, 0x2b9, 0xae5680, 0xae56804d3, 0xae56804d39)),
    ((2147483646, 0), 0x000000007ffffffe, (0x1, 0x20c, 0x83364a, 0x83364a978, 0x83364a9781)),
    ((1000000007, 998244353), 0x3b8000013b9aca07, (0x0, 0x1d1, 0x7447eb, 0x7447ebffb, 0x7447ebffbc)),
    ((77, 1073741824), 0x0000004d40000000, (0x1, 0x2a4, 0xa939f1, 0xa939f1564, 0xa939f15640)),
]


def test_the_key_and_the_hash_are_the_pinned_ones(host_pt):
    assert len(PAIRS) == 12
    for (a, b), key, hashes in PAIRS:
        assert host_pt.pt_host_key(a, b) == key == (min(a, b) << 32 | max(a, b)) == host_pt.pt_host_key(b, a)
        assert tuple(host_pt.pt_host_hash(key, log2) for log2 in LOG2S) == hashes == tuple(py_hash(key, log2) for log2 in LOG2S)
    out = np.zeros(4, np.uint64)
    host_pt.pt_host_consts(C.c_void_p(out.ctypes.data))
    assert out.tolist() == [EMPTY, NO_PLACE, LIMIT, 10]
    assert [host_pt.pt_host_max_axes(c) for c in (6, 18, 26)] == [1, 2, 3]


def keys_of_slot(slot, log2, n, first=1):
    """The first n keys from `first` on whose probe run starts at `slot` in a table of 2^log2 slots."""
    found, key = [], first
    while len(found) < n:
        if py_hash(key, log2) == slot:
            found.append(key)
        key += 1
    return found


@pytest.mark.parametrize("log2", [0, 1, 3, 7])
def test_a_probe_run_over_the_whole_table(host_pt, log2):
    """Up to 2^7 slots a probe run is the whole table: any 2^log2 distinct keys fill it, whatever their hashes, and the next finds
    no place."""
    slots = 1 << log2
    keys = (np.random.default_rng(28 + log2).permutation(5000)[:slots + 1] + 1).astype(np.uint64)
    t = Table(host_pt, log2)
    got, fresh = t.insert(keys[:slots])
    assert sorted(got) == list(range(slots)) and all(fresh) and t.occupied() == sorted(keys[:slots].tolist())
    assert got[0] == py_hash(int(keys[0]), log2)
    again, fresh = t.insert(keys[:slots][::-1])
    assert again == got[::-1] and not any(fresh)
    assert t.insert(keys[slots:]) == ([NO_PLACE], [False]) and t.occupied() == sorted(keys[:slots].tolist())
    assert t.insert(keys[:1]) == (got[:1], [False])


@pytest.mark.parametrize("start", [17, 2 ** 8 - 3])
def test_a_probe_run_shorter_than_the_table(host_pt, start):
    """At 2^8 slots the run is 128 slots: 128 keys that meet in one slot take it and the 127 behind it, around the table's end, and
    the 129th finds no place in a table that is half empty."""
    keys = keys_of_slot(start, 8, LIMIT + 1)
    assert len(set(keys)) == LIMIT + 1 and all(host_pt.pt_host_hash(k, 8) == start for k in keys)
    t = Table(host_pt, 8)
    want = [(start + i) % 256 for i in range(LIMIT)]
    assert t.insert(keys[:LIMIT]) == (want, [True] * LIMIT)
    assert (start == 17 or want[:4] == [253, 254, 255, 0]) and t.words[want].tolist() == keys[:LIMIT]
    assert t.insert(keys[:LIMIT][::-1]) == (want[::-1], [False] * LIMIT)
    assert t.insert(keys[LIMIT:]) == ([NO_PLACE], [False]) and len(t.occupied()) == LIMIT == 256 // 2
    # a key whose run starts in the last slot that was taken still has 127 free slots before it
    (late,) = keys_of_slot(want[-1], 8, 1)
    assert t.insert([late]) == ([(want[-1] + 1) % 256], [True])


def test_the_order_of_insertion_does_not_show(host_pt):
    rng = np.random.default_rng(2811)
    distinct = (rng.integers(0, 2 ** 31, 400, dtype=np.uint64) << np.uint64(32)) | rng.integers(0, 2 ** 31, 400, dtype=np.uint64)
    keys = distinct[rng.integers(0, 400, 1000)]
    want = sorted(set(keys.tolist()))
    assert 300 < len(want) < 1000
    for shuffle in range(5):
        t = Table(host_pt, 11)
        slot, fresh = t.insert(rng.permutation(keys))
        assert NO_PLACE not in slot and t.occupied() == want and sum(fresh) == len(want)


# pt_first_log2(ids, forced, first_max_log2, max_log2): [ids][forced], what K23's ws_table_log2 (40, 40) and K24's adj_table_log2
# (24, 36) gave
IDS = (0, 1, 64, 65, 2 ** 20, 2 ** 20 + 1, 2 ** 31)
FORCED = (0, 3, 12, 50)
SIZES = {
    (40, 40): [[10, 3, 12, 40], [10, 3, 12, 40], [10, 3, 12, 40], [11, 3, 12, 40], [24, 3, 12, 40], [25, 3, 12, 40], [35, 3, 12, 40]],
    (24, 36): [[10, 3, 12, 36], [10, 3, 12, 36], [10, 3, 12, 36], [11, 3, 12, 36], [24, 3, 12, 36], [24, 3, 12, 36], [24, 3, 12, 36]],
}


@pytest.mark.parametrize("caps", sorted(SIZES))
def test_the_first_size_is_the_pinned_one(host_pt, caps):
    got = [[host_pt.pt_host_first_log2(ids, forced, *caps) for forced in FORCED] for ids in IDS]
    assert got == SIZES[caps]
