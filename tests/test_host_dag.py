"""Sparse voxel DAGs without a GPU: the numpy reference (tests/dag_ref.py) against the closed forms of the
definition and against a second construction, a scalar walk with a dictionary; its descent against the tree's
(tests/octree_ref.py) and to_dense(dag) == g; the plain C++ of o2v_dev_k30_dag.hpp compiled for the host behind K26's - the
descent, the keys (hash, equality) driving a scalar copy of the kernels' table, the child-range check, corrupt arrays, one
mutation seen to fail; obj2voxel_amd.dense's octree_dag, dag_lookup and dag_to_dense against a stand-in for the device calls that
computes with the reference; the K30 kernels' metadata in the gfx950 code object."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import bits_host
from tests import dag_ref as G
from tests import octree_ref as R

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip, octree  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, device_asm, on_cpu  # noqa: E402,F401
from tests.test_host_label_stats import _strided  # noqa: E402
from tests.test_host_octree import OctStub, _array, box_points  # noqa: E402

K26 = os.path.join(SRC, "o2v_dev_k26_octree.hpp")
K30 = os.path.join(SRC, "o2v_dev_k30_dag.hpp")
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def row(g, origin=(0, 0, 0), collapse=True):
    """(tree nodes, DAG level counts, pointers) of the grid"""
    d = G.build(R.build(g, origin, None, collapse))
    return d["tree_nodes"], d["level_counts"], len(d["child"])


# ---- the reference ----------------------------------------------------------------------------------------------------------------

def test_closed_forms_of_the_definition():
    one = np.zeros((8, 8, 8), bool)
    one[3, 5, 6] = True
    for collapse in (True, False):
        assert row(R.checkerboard(16), collapse=collapse) == (585, [1, 1, 1, 1], 24)
        assert row(one, collapse=collapse) == (3, [1, 1, 1], 2)
        assert row(np.zeros((4, 4, 4), bool), collapse=collapse) == (1, [1, 0], 0)
    assert row(R.box((16, 16, 16)), collapse=False) == (585, [1, 1, 1, 1], 24)
    assert row(R.box((16, 16, 16)), collapse=True) == (1, [1, 0, 0, 0], 0)
    assert row(R.box((7, 5, 3)), (1, 3, 5), True) == (23, [1, 4, 7], 22)
    assert row(R.box((7, 5, 3)), (1, 3, 5), False) == (29, [1, 4, 8], 28)
    assert row(R.ball(), collapse=True) == (1417, [1, 8, 32, 104, 304, 94], 1384) and sum([1, 8, 32, 104, 304, 94]) == 543
    assert row(R.ball(), collapse=False) == (5553, [1, 8, 32, 105, 305, 95], 2288) and sum([1, 8, 32, 105, 305, 95]) == 546
    two = G.two_balls()
    assert two.shape == (64, 64, 128)
    assert row(two, collapse=True) == (2835, [1, 1, 8, 32, 104, 304, 94], 1386)
    assert row(two, collapse=False) == (11107, [1, 1, 8, 32, 105, 305, 95], 2290)
    # the arrays of the smallest cases, entry by entry
    d = G.build(R.build(one))
    assert d["valid"].tolist() == [0x08, 0x20, 0x40] and d["first_child"].tolist() == [0, 1, -1] and d["child"].tolist() == [1, 2] and d["skip"].tolist() == [0, 0]
    d = G.build(R.build(R.checkerboard(16)))
    assert d["valid"].tolist() == [255, 255, 255, 0x69] and d["first_child"].tolist() == [0, 8, 16, -1]
    assert d["child"].tolist() == [1] * 8 + [2] * 8 + [3] * 8 and d["skip"].tolist() == [256 * r for r in range(8)] + [32 * r for r in range(8)] + [4 * r for r in range(8)]
    d = G.build(R.build(np.ones((1, 1, 1), bool)))   # depth 1: the root is the last level
    assert (d["level_counts"], d["valid"].tolist(), d["first_child"].tolist(), len(d["child"])) == ([1], [1], [-1], 0)


def test_the_two_constructions_agree_on_random_grids():
    rng = np.random.default_rng(340)
    n = 0
    for dims, origin in (((5, 6, 7), (1, 3, 5)), ((9, 3, 4), (0, 0, 0)), ((13, 9, 10), (7, 7, 8)), ((1, 1, 1), (0, 0, 0)), ((17, 2, 3), (63, 0, 1)),
                         ((16, 16, 16), (0, 0, 0)), ((32, 32, 32), (0, 0, 0))):
        for collapse in (True, False):
            for extra in (0, 2):
                for p in (0.02, 0.6, 0.98):
                    t = R.build(R.blobs(rng, dims, p), origin, R.depth_of(origin, dims) + extra, collapse)
                    d = G.build(t)
                    G.same(G.build_scalar(t), d, (dims, origin, collapse, extra, p))
                    M, P = len(d["valid"]), len(d["child"])
                    assert sum(d["level_counts"]) == M <= len(t["valid"]) and P < max(2, len(t["valid"])) and d["tree_nodes"] == len(t["valid"])
                    # first_child is the exclusive scan of the stored children; the root is node 0; a class's first member rises with its number
                    stored = np.where(np.arange(M) < M - d["level_counts"][-1], d["valid"] & ~d["full"] if collapse else d["valid"], 0)
                    pc = R.popcount8(stored)
                    assert np.array_equal(d["first_child"], np.where(pc > 0, np.cumsum(pc) - pc, -1)) and d["classes"][0] == 0
                    first = np.unique(d["classes"], return_index=True)[1]
                    assert np.array_equal(np.sort(d["classes"]), np.sort(d["classes"][first][np.searchsorted(d["classes"][first], d["classes"])]))
                    assert (np.diff(first) > 0).all()
                    n += 1
    assert n == 84
    # 128^3 takes seconds
    g = rng.random((128, 128, 128)) < 0.5
    d = G.build(R.build(g, collapse=False))
    assert d["level_counts"][:6] == [1, 8, 64, 512, 4096, 32768] and d["level_counts"][6] <= 255


def small_grids():
    rng = np.random.default_rng(341)
    for dims in ((3, 2, 2), (5, 4, 3)):
        for ox in (0, 1, 63):
            origin = (ox, 1, 0)
            for extra in (0, 2):
                for collapse in (True, False):
                    yield R.blobs(rng, dims, 0.7, noise=0.1), origin, R.depth_of(origin, dims) + extra, collapse


def cube_points(depth, step=1):
    """every point of the root cube and two voxels around it (a lattice of `step` where the cube is large, with the edges)"""
    side = 2 ** depth
    axis = np.unique(np.concatenate([np.arange(-2, side + 2, step), [side - 1, side, side + 1]]))
    z, y, x = np.meshgrid(axis, axis, axis, indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3)


def test_the_descent_of_the_reference_against_the_tree():
    n = 0
    for g, origin, depth, collapse in small_grids():
        t = R.build(g, origin, depth, collapse)
        d = G.build(t)
        pts = cube_points(depth, 1 if depth <= 4 else 2 ** (depth - 4) - 1)
        pts = np.concatenate([pts, np.argwhere(g)[:, ::-1] + np.array(origin)])
        got, want = G.lookup(d, pts), R.lookup(t, pts)
        assert np.array_equal(got[:, [0, 1, 3]], want[:, [0, 1, 3]]), (origin, depth, collapse)
        ok = want[:, 2] >= 0
        assert np.array_equal(got[ok, 2], d["classes"][want[ok, 2]]) and (got[~ok, 2] == -1).all()
        assert (G.lookup(d, pts, skips=False)[:, 3] == -1).all()
        nz, ny, nx = g.shape
        assert np.array_equal(G.to_dense(d, g.shape, origin), g)
        want = np.zeros((nz + 3, ny + 2, nx + 1), bool)
        want[2:2 + nz, 1:1 + ny, 1:1 + nx] = g
        if min(origin) >= 1 and origin[2] >= 2:
            assert np.array_equal(G.to_dense(d, want.shape, (origin[0] - 1, origin[1] - 1, origin[2] - 2)), want)
        n += 1
    assert n == 24
    for g in (R.ball(16, 7.5, 30), R.checkerboard(8), R.box((8, 8, 8))):
        for collapse in (True, False):
            assert np.array_equal(G.to_dense(G.build(R.build(g, collapse=collapse)), g.shape), g)


# ---- the kernels' plain C++ on the host ---------------------------------------------------------------------------------------------

HOST_DAG = r"""
#include <cstdint>
#include <stddef.h>
%s
#define O2V_OCT_HOST
#define O2V_OCT_FN static inline
#define O2V_OCT_HD static inline
static inline uint32_t oct_popc(uint32_t v) { return (uint32_t) __builtin_popcount(v); }
%s
%s
extern "C" void dag_host_lookup(const uint8_t *valid, const uint8_t *full, const int32_t *first_child, const int32_t *child, const int32_t *skip, uint32_t n_nodes,
                                uint32_t n_pointers, uint32_t depth, uint32_t collapsed, const int32_t *points, uint64_t n, int32_t *out)
{
    const OctDag d{valid, full, first_child, child, skip, n_nodes, n_pointers, depth, collapsed, dag_skips(skip, n_pointers)};
    for (uint64_t p = 0; p < n; ++p) dag_descend(d, points[3u * p], points[3u * p + 1u], points[3u * p + 2u], out + 4u * p);
}
extern "C" void dag_host_blocks(const uint8_t *valid, const uint8_t *full, const int32_t *first_child, const int32_t *child, const int32_t *skip, uint32_t n_nodes,
                                uint32_t n_pointers, uint32_t depth, uint32_t collapsed, const uint32_t *blocks, uint64_t n, uint32_t *out)
{
    const OctDag d{valid, full, first_child, child, skip, n_nodes, n_pointers, depth, collapsed, dag_skips(skip, n_pointers)};
    for (uint64_t p = 0; p < n; ++p) out[p] = dag_block(d, blocks[3u * p], blocks[3u * p + 1u], blocks[3u * p + 2u]);
}
extern "C" int dag_host_range_ok(int32_t first_child, uint32_t n_stored, uint64_t lo, uint64_t hi) { return dag_child_range_ok(first_child, n_stored, lo, hi) ? 1 : 0; }
static DagLevel level_of(const uint8_t *valid, const uint8_t *full, const int32_t *first_child, const uint32_t *cls, const uint64_t *range, uint32_t collapsed)
{
    return DagLevel{valid, full, first_child, cls, range[0], range[1], range[2], collapsed};
}
extern "C" int dag_host_equal(const uint8_t *valid, const uint8_t *full, const int32_t *first_child, const uint32_t *cls, const uint64_t *range, uint32_t collapsed,
                              uint32_t i, uint32_t j)
{
    const DagLevel L = level_of(valid, full, first_child, cls, range, collapsed);
    return (dag_key_equal(L, i, j) ? 1 : 0) | (dag_key_hash(L, i) == dag_key_hash(L, j) ? 2 : 0);
}
// k_dag_insert and k_dag_find lane by lane, the nodes of the level (range: its first node, the next level's, the one after) taken in
// `order`: cls[first + i] = the smallest index of i's class.  -1: a stored child outside the next level, met before it was used.
extern "C" int dag_host_merge(const uint8_t *valid, const uint8_t *full, const int32_t *first_child, uint32_t *cls, const uint64_t *range, uint32_t collapsed,
                              const uint32_t *order, uint32_t n, uint32_t *tab, uint32_t mask)
{
    const DagLevel L = level_of(valid, full, first_child, cls, range, collapsed);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t i = order[k], v = valid[L.first + i], f = full[L.first + i];
        if (!dag_child_range_ok(first_child[L.first + i], oct_popc(oct_stored(v, f, collapsed)), L.lo, L.hi)) return -1;
    }
    for (uint32_t s = 0; s <= mask; ++s) tab[s] = kDagEmpty;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t i = order[k];
        for (uint32_t h = dag_key_hash(L, i) & mask;; h = (h + 1u) & mask) {
            if (tab[h] == kDagEmpty) tab[h] = i;
            if (tab[h] == i || dag_key_equal(L, i, tab[h])) {
                if (i < tab[h]) tab[h] = i;
                break;
            }
        }
    }
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t h = dag_key_hash(L, i) & mask;; h = (h + 1u) & mask)
            if (tab[h] == i || dag_key_equal(L, i, tab[h])) {
                cls[L.first + i] = tab[h];
                break;
            }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_dag(tmp_path_factory):
    """build(defines) -> the library of the plain C++ part of o2v_dev_k30_dag.hpp, compiled for the host behind K26's and the bit grid's."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    k = open(K26).read()
    k26 = k[k.index("constexpr uint32_t kOctMaxDepth"):k.index("#ifndef O2V_OCT_HOST")] + k[k.index("// ---- cells, bit pairs"):k.index("// ---- kernels")]
    k = open(K30).read()
    k30 = k[k.index("constexpr uint32_t kDagEmpty"):k.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_dag")

    def build(defines=()):
        name = "dag_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_DAG % (bits_host.plain_part(), k26, k30))
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = C.CDLL(str(tmp / (name + ".so")))
        dag = [C.c_void_p] * 5 + [C.c_uint32] * 4
        L.dag_host_lookup.argtypes = L.dag_host_blocks.argtypes = dag + [C.c_void_p, C.c_uint64, C.c_void_p]
        L.dag_host_lookup.restype = L.dag_host_blocks.restype = None
        L.dag_host_range_ok.argtypes = [C.c_int32, C.c_uint32, C.c_uint64, C.c_uint64]
        L.dag_host_equal.argtypes = [C.c_void_p] * 5 + [C.c_uint32] * 3
        L.dag_host_merge.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        return L
    return build


def dag_ptrs(d, skips=True):
    d["_keep"] = [np.ascontiguousarray(d[k]) for k in ("valid", "full", "first_child", "child", "skip")]
    p = [a.ctypes.data if len(a) else None for a in d["_keep"]]
    return p[:4] + [p[4] if skips else None] + [len(d["valid"]), len(d["child"]), d["depth"], int(d["collapsed"])]


def run_lookup(L, d, points, skips=True):
    points = np.ascontiguousarray(points, np.int32).reshape(-1, 3)
    out = np.full((len(points), 4), -9, np.int32)
    L.dag_host_lookup(*dag_ptrs(d, skips), points.ctypes.data, len(points), out.ctypes.data)
    return out


def test_the_descent_on_the_host(host_dag):
    L = host_dag()
    n = 0
    for g, origin, depth, collapse in small_grids():
        t = R.build(g, origin, depth, collapse)
        d = G.build(t)
        pts = cube_points(depth, 1 if depth <= 4 else 2 ** (depth - 4) - 1)
        got = run_lookup(L, d, pts)
        assert np.array_equal(got, G.lookup(d, pts)), (origin, depth, collapse)
        assert np.array_equal(got[:, [0, 1, 3]], R.lookup(t, pts)[:, [0, 1, 3]])
        assert np.array_equal(run_lookup(L, d, pts, skips=False), G.lookup(d, pts, skips=False))
        n += 1
    assert n == 24
    # a voxel's slot and a block at a time, on a grid with full cells
    g = R.blobs(np.random.default_rng(342), (16, 16, 16), 0.6)
    for collapse in (True, False):
        t = R.build(g, collapse=collapse)
        d = G.build(t)
        pts = box_points(-2, 18)
        got = run_lookup(L, d, pts)
        assert np.array_equal(got[:, [0, 1, 3]], R.lookup(t, pts)[:, [0, 1, 3]]) and got[:, 0].sum() == g.sum()
        assert np.array_equal(np.sort(got[got[:, 3] >= 0, 3]), np.arange(t["voxels_listed"]))
        b = np.ascontiguousarray(box_points(0, 8) * 2, np.uint32)
        masks = np.zeros(len(b), np.uint32)
        L.dag_host_blocks(*dag_ptrs(d), b.ctypes.data, len(b), masks.ctypes.data)
        for o in range(8):
            assert np.array_equal((masks >> o) & 1, R.lookup(t, b.astype(np.int64) + np.array([o & 1, (o >> 1) & 1, o >> 2]))[:, 0]), (collapse, o)
    assert run_lookup(L, d, [[INT32_MIN, 0, 0], [0, INT32_MAX, 0]]).tolist() == [[0, -1, -1, -1]] * 2


def test_corrupt_arrays_end_the_descent_on_the_host(host_dag):
    """first_child and child values of -2, INT32_MIN, M, P and INT32_MAX, and a child in the wrong level: (0, -2, -1, -1), or an
    answer of the arrays as they are, and nothing is read outside them (the arrays end where their allocation ends)."""
    L = host_dag()
    g = R.blobs(np.random.default_rng(343), (16, 16, 16), 0.5, noise=0.1)
    pts = box_points(0, 16)
    for collapse in (True, False):
        d = G.build(R.build(g, collapse=collapse))
        M, P = len(d["valid"]), len(d["child"])
        top = d["level_counts"][0] + d["level_counts"][1]
        for bad in (-2, INT32_MIN, M, P, INT32_MAX):
            for field, n in (("first_child", top), ("child", int(d["first_child"][top]))):
                broken = dict(d)
                broken[field] = np.where(np.arange(len(d[field])) < n, bad, d[field]).astype(np.int32)
                got = run_lookup(L, broken, pts)
                assert np.array_equal(got, G.lookup(broken, pts)), (collapse, bad, field)
                rows = got[:, 1] == -2
                assert (got[rows] == (0, -2, -1, -1)).all() and (rows.any() or (field == "first_child" and 0 <= bad < P) or (field == "child" and 0 <= bad < M))
        # a child in the wrong level: the descent follows it (the arrays hold it) and ends within D steps, as the reference's does
        broken = dict(d, child=np.where(np.arange(P) < 8, 0, d["child"]).astype(np.int32))   # the root's children: the root again
        assert np.array_equal(run_lookup(L, broken, pts), G.lookup(broken, pts))
    # ... and the merge refuses a tree with one: the child-range check
    assert [L.dag_host_range_ok(fc, n, 10, 20) for fc, n in ((10, 8), (12, 8), (13, 8), (9, 1), (20, 1), (19, 1), (-1, 1), (-1, 0), (INT32_MIN, 1), (INT32_MAX, 8), (-2, 8))] == \
        [1, 1, 0, 0, 0, 1, 0, 1, 0, 0, 0]
    assert L.dag_host_range_ok(INT32_MAX - 1, 8, 0, 2 ** 32) == 1 and L.dag_host_range_ok(INT32_MAX, 8, 0, INT32_MAX) == 0


def host_merge(L, t, rng=None):
    """The classes of every tree node by the kernels' table on the host, level by level: (per level the class counts, the classes
    as DAG nodes), or None where the child-range check refuses the tree.  Level D - 1 (keyed by `valid` alone) by numpy."""
    D, N = t["depth"], len(t["valid"])
    off = [int(v) for v in np.concatenate([[0], np.cumsum(t["level_counts"])])] + [N]
    cls = np.zeros(max(N, 1), np.uint32)
    valid, full, first = (np.ascontiguousarray(t[k]) for k in ("valid", "full", "first_child"))
    counts = [0] * D
    for l in range(D - 1, -1, -1):   # noqa: E741
        a, n = off[l], off[l + 1] - off[l]
        if not n:
            continue
        if l == D - 1:
            _, idx, inv = np.unique(valid[a:a + n], return_index=True, return_inverse=True)
            rep = idx[inv.reshape(-1)]
        else:
            slots = 256
            while slots < 2 * n:
                slots *= 2
            tab = np.zeros(slots, np.uint32)
            order = np.arange(n, dtype=np.uint32) if rng is None else rng.permutation(n).astype(np.uint32)
            rng_ = np.array([off[l], off[l + 1], off[l + 2]], np.uint64)
            if L.dag_host_merge(valid.ctypes.data, full.ctypes.data, first.ctypes.data, cls.ctypes.data, rng_.ctypes.data, int(t["collapsed"]), order.ctypes.data, n,
                                tab.ctypes.data, slots - 1):
                return None
            rep = cls[a:a + n].astype(np.int64)
        is_rep = rep == np.arange(n)
        rank = np.cumsum(is_rep) - is_rep
        cls[a:a + n] = rank[rep].astype(np.uint32) | (is_rep.astype(np.uint32) << 31)
        counts[l] = int(is_rep.sum())
    doff = np.concatenate([[0], np.cumsum(counts)])
    return counts, np.concatenate([doff[l] + (cls[off[l]:off[l + 1]] & 0x7fffffff).astype(np.int64) for l in range(D)])


def test_the_keys_and_the_table_on_the_host(host_dag):
    """The kernels' hash and equality drive a scalar copy of their table: the classes are the reference's whatever order the nodes
    come in."""
    L = host_dag()
    rng = np.random.default_rng(344)
    n = 0
    for g, origin in ((R.ball(), (0, 0, 0)), (G.two_balls(), (0, 0, 0)), (R.checkerboard(16), (0, 0, 0)), (R.box((16, 16, 16)), (0, 0, 0)), (R.box((7, 5, 3)), (1, 3, 5)),
                      (R.blobs(rng, (32, 32, 32), 0.5), (0, 0, 0)), (R.blobs(rng, (13, 9, 10), 0.6), (7, 7, 8)), (np.zeros((4, 4, 4), bool), (0, 0, 0)),
                      (np.tile(rng.random((8, 8, 8)) < 0.5, (4, 4, 4)), (0, 0, 0))):
        for collapse in (True, False):
            t = R.build(g, origin, None, collapse)
            d = G.build(t)
            for order in (None, rng):
                counts, classes = host_merge(L, t, order)
                assert counts == d["level_counts"] and np.array_equal(classes, d["classes"]), (g.shape, collapse)
                n += 1
    assert n == 36
    # equality, pair by pair, on one level of the ball: equal keys have equal hashes, and equal is what the reference calls one class
    t = R.build(R.ball(), collapse=True)
    d = G.build(t)
    _, classes = host_merge(L, t)
    off = np.concatenate([[0], np.cumsum(t["level_counts"])]).astype(np.uint64)
    cls = classes.astype(np.uint32)   # (the low bits are compared; the offsets of the levels cancel within one level)
    valid, full, first = (np.ascontiguousarray(t[k]) for k in ("valid", "full", "first_child"))
    level = 3
    rng_ = off[level:level + 3].copy()
    for i in range(t["level_counts"][level]):
        for j in range(0, t["level_counts"][level], 3):
            r = L.dag_host_equal(valid.ctypes.data, full.ctypes.data, first.ctypes.data, cls.ctypes.data, rng_.ctypes.data, 1, i, j)
            same = d["classes"][int(off[level]) + i] == d["classes"][int(off[level]) + j]
            assert bool(r & 1) == same and (not same or r & 2), (i, j, r)


def test_a_tree_that_is_not_one_is_refused_on_the_host(host_dag):
    L = host_dag()
    t = R.build(R.ball(), collapse=False)
    off = np.concatenate([[0], np.cumsum(t["level_counts"])])
    assert host_merge(L, t) is not None
    for level, value in ((1, int(off[3])), (2, int(off[2])), (0, -1), (3, int(off[5]) - 1), (1, INT32_MAX), (4, INT32_MIN), (2, len(t["valid"]))):
        broken = dict(t, first_child=t["first_child"].copy())
        broken["first_child"][off[level]] = value   # the first node of the level: all of them have stored children
        assert host_merge(L, broken) is None, (level, value)
        with pytest.raises(ValueError, match="not a tree of these level counts"):
            G.build(broken)
    # the last child of the last node of a level may end exactly where the next level ends
    assert int(t["first_child"][off[2] - 1]) + bin(int(t["valid"][off[2] - 1])).count("1") == off[3]


def test_equality_that_ignores_full_is_caught_on_the_host(host_dag):
    """With O2V_DAG_MUTATE_IGNORE_FULL two nodes whose `full` masks differ merge where their valid masks and their stored children
    agree.  A collapsed grid tells it: of the eight cells of side 4 of an 8^3 grid, seven are full but for one voxel - the same
    voxel - and one is full; per parent another octant holds the full one.  A tree that is not collapsed does not notice: there
    `full` follows from the children."""
    L, M = host_dag(), host_dag(("O2V_DAG_MUTATE_IGNORE_FULL",))
    cell = np.ones((4, 4, 4), bool)
    cell[1, 2, 3] = False
    g = np.zeros((16, 16, 16), bool)
    for k, whole in enumerate((1, 2)):   # two cells of side 8: in the first octant 1 is full, in the second octant 2
        for o in range(8):
            z, y, x = 4 * (o >> 2), 4 * ((o >> 1) & 1), 8 * k + 4 * (o & 1)
            g[z:z + 4, y:y + 4, x:x + 4] = True if o == whole else cell
    t = R.build(g, collapse=True)
    d = G.build(t)
    assert t["level_counts"] == [1, 2, 14, 14] and d["level_counts"] == [1, 2, 1, 1]
    assert t["full"][1:3].tolist() == [2, 4] and t["valid"][1:3].tolist() == [255, 255]
    counts, classes = host_merge(L, t)
    assert counts == d["level_counts"] and np.array_equal(classes, d["classes"])
    counts, classes = host_merge(M, t)
    assert counts == [1, 1, 1, 1] and not np.array_equal(classes, d["classes"])   # the two cells of side 8 merged: one voxel's worth of `full` lost
    plain = R.build(g, collapse=False)
    assert host_merge(M, plain)[0] == G.build(plain)["level_counts"]
    for other in (R.ball(), R.checkerboard(16)):
        assert host_merge(M, R.build(other, collapse=False))[0] == G.build(R.build(other, collapse=False))["level_counts"]


# ---- dense.* against a stand-in ------------------------------------------------------------------------------------------------------

class DagStub(OctStub):
    """The octree calls of OctStub and the four DAG calls, computed with the reference on the host memory behind the pointers."""

    def octree_dag_build(self, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags, level_counts):
        self.calls.append(dict(call="dag_build", n_nodes=n_nodes, depth=depth, flags=flags, level_counts=list(level_counts)))
        t = self._tree(valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags)
        t.update(level_counts=list(level_counts), voxels_listed=0)
        self.dag = d = G.build(t)
        return tuple(d["level_counts"]), len(d["valid"]), len(d["child"])

    def octree_dag_write(self, valid_ptr, full_ptr, first_child_ptr, child_ptr, skip_ptr=None):
        self.calls.append(dict(call="dag_write", child=child_ptr, skip=skip_ptr))
        d, M, P = self.dag, len(self.dag["valid"]), len(self.dag["child"])
        _array(valid_ptr, C.c_uint8, M)[:] = d["valid"]
        _array(full_ptr, C.c_uint8, M)[:] = d["full"]
        _array(first_child_ptr, C.c_int32, M)[:] = d["first_child"]
        if P:
            _array(child_ptr, C.c_int32, P)[:] = d["child"]
        if P and skip_ptr is not None:
            _array(skip_ptr, C.c_int32, P)[:] = d["skip"]

    def _dag(self, valid_ptr, full_ptr, first_child_ptr, child_ptr, skip_ptr, n_nodes, n_pointers, depth, flags):
        none = np.zeros(0, np.int32)
        return dict(valid=_array(valid_ptr, C.c_uint8, n_nodes), full=_array(full_ptr, C.c_uint8, n_nodes), first_child=_array(first_child_ptr, C.c_int32, n_nodes),
                    child=_array(child_ptr, C.c_int32, n_pointers) if n_pointers else none,
                    skip=_array(skip_ptr, C.c_int32, n_pointers) if n_pointers and skip_ptr is not None else none, depth=depth, collapsed=bool(flags & hip.OCT_COLLAPSE))

    def octree_dag_lookup(self, valid_ptr, full_ptr, first_child_ptr, child_ptr, skip_ptr, n_nodes, n_pointers, depth, flags, points_ptr, n, out_ptr):
        self.calls.append(dict(call="dag_lookup", n_nodes=n_nodes, n_pointers=n_pointers, depth=depth, flags=flags, n=n, skip=skip_ptr))
        d = self._dag(valid_ptr, full_ptr, first_child_ptr, child_ptr, skip_ptr, n_nodes, n_pointers, depth, flags)
        skips = skip_ptr is not None or not n_pointers
        _array(out_ptr, C.c_int32, 4 * n)[:] = G.lookup(d, _array(points_ptr, C.c_int32, 3 * n).reshape(-1, 3), skips=skips).reshape(-1)

    def octree_dag_to_dense(self, valid_ptr, full_ptr, first_child_ptr, child_ptr, n_nodes, n_pointers, depth, flags, origin, dims, out_ptr, out_strides):
        self.calls.append(dict(call="dag_to_dense", origin=tuple(origin), dims=tuple(dims), strides=tuple(out_strides), flags=flags))
        d = self._dag(valid_ptr, full_ptr, first_child_ptr, child_ptr, None, n_nodes, n_pointers, depth, flags)
        _strided(out_ptr, C.c_uint8, tuple(dims), tuple(out_strides))[...] = G.to_dense(d, tuple(dims)[::-1], tuple(origin))


def as_ref(dag):
    """an OctreeDag as the reference's dict"""
    offs = dag.level_offsets
    return dict(valid=dag.valid.numpy(), full=dag.full.numpy(), first_child=dag.first_child.numpy(), child=dag.child.numpy(),
                skip=None if dag.skip is None else dag.skip.numpy(), level_counts=[b - a for a, b in zip(offs, offs[1:])], depth=dag.depth, collapsed=dag.collapsed)


def test_octree_dag_through_the_stand_in(on_cpu):  # noqa: F811
    dv = DagStub()
    g = R.blobs(np.random.default_rng(345), (11, 6, 5), 0.6)
    for collapse in (True, False):
        for skips in (True, False):
            tree = dense.build_octree(dv, torch.from_numpy(g), origin=(3, 1, 2), collapse=collapse)
            dag = dense.octree_dag(dv, tree, skips) if skips else dense.octree_dag(dv, tree, skips=False)
            want = G.build(R.build(g, (3, 1, 2), None, collapse))
            assert isinstance(dag, dense.OctreeDag) and dense.OctreeDag is octree.OctreeDag
            G.same(as_ref(dag), want, (collapse, skips))
            b, w = dv.calls[-2], dv.calls[-1]
            assert (b["call"], b["n_nodes"], b["depth"], b["flags"]) == ("dag_build", len(tree.valid), 4, hip.OCT_COLLAPSE * collapse)
            assert b["level_counts"] == [y - x for x, y in zip(tree.level_offsets, tree.level_offsets[1:])]
            assert w["call"] == "dag_write" and w["child"] == dag.child.data_ptr() and w["skip"] == (dag.skip.data_ptr() if skips else None)
            assert (dag.skip is None) == (not skips) and dag.collapsed is collapse and dag.depth == 4 and dag.voxels_listed == tree.voxels_listed
            assert dag.tree_nodes == len(tree.valid) and all(type(v) is int for v in dag.level_offsets) and len(dag.level_offsets) == 5
            assert dag.valid.dtype == dag.full.dtype == torch.uint8 and dag.first_child.dtype == dag.child.dtype == torch.int32
            assert dag.nbytes == 6 * len(dag.valid) + (8 if skips else 4) * len(dag.child) and (not skips or dag.nbytes == G.nbytes(want))
    with pytest.raises(dataclasses.FrozenInstanceError):
        dag.depth = 3
    # a DAG without pointers: null child and skip go to the library
    tree = dense.build_octree(dv, torch.ones((4, 4, 4), dtype=torch.bool))
    dag = dense.octree_dag(dv, tree)
    assert len(dag.child) == 0 == len(dag.skip) and dv.calls[-1]["child"] is None and dv.calls[-1]["skip"] is None and dag.level_offsets == (0, 1, 1)
    assert dense.dag_lookup(dv, dag, torch.tensor([[1, 2, 3], [4, 0, 0]], dtype=torch.int32)).tolist() == [[1, 0, 0, -1], [0, -1, -1, -1]]
    assert bool(dense.dag_to_dense(dv, dag, (4, 4, 4)).all())


def test_lookup_and_to_dense_through_the_stand_in(on_cpu):  # noqa: F811
    dv = DagStub()
    g = R.blobs(np.random.default_rng(346), (11, 6, 5), 0.6)
    for collapse in (True, False):
        tree = dense.build_octree(dv, torch.from_numpy(g), origin=(3, 1, 2), collapse=collapse)
        dag = dense.octree_dag(dv, tree)
        pts = torch.from_numpy(box_points(-1, 17).astype(np.int32))
        got, of_tree = dense.dag_lookup(dv, dag, pts), dense.octree_lookup(dv, tree, pts)
        assert got.dtype == torch.int32 and tuple(got.shape) == (len(pts), 4) and torch.equal(got[:, [0, 1, 3]], of_tree[:, [0, 1, 3]])
        assert dv.calls[-2]["flags"] == hip.OCT_COLLAPSE * collapse and dv.calls[-2]["n_nodes"] == len(dag.valid) and dv.calls[-2]["n_pointers"] == len(dag.child)
        cube = pts.reshape(18, 18, 18, 3)[1:17:2, :, 3:]
        assert torch.equal(dense.dag_lookup(dv, dag, cube), got.reshape(18, 18, 18, 4)[1:17:2, :, 3:])
        n_calls = len(dv.calls)
        assert tuple(dense.dag_lookup(dv, dag, pts[:0]).shape) == (0, 4) and len(dv.calls) == n_calls   # nothing to look up: no call
        bare = dense.dag_lookup(dv, dataclasses.replace(dag, skip=None), pts)
        assert dv.calls[-1]["skip"] is None and torch.equal(bare[:, :3], got[:, :3]) and bool((bare[:, 3] == -1).all())
        back = dense.dag_to_dense(dv, dag, g.shape, origin=(3, 1, 2))
        assert back.dtype == torch.bool and np.array_equal(back.numpy(), g)
        wide = torch.zeros((12, 13, 40), dtype=torch.uint8)
        out = dense.dag_to_dense(dv, dag, (12, 13, 20), origin=(1, 0, 0), out=wide[:, :, ::2])
        assert out.data_ptr() == wide.data_ptr() and dv.calls[-1]["strides"] == (2, 40, 520) and dv.calls[-1]["dims"] == (20, 13, 12)
        assert torch.equal(out != 0, dense.octree_to_dense(dv, tree, (12, 13, 20), origin=(1, 0, 0))) and not wide[:, :, 1::2].any()


def test_the_wait_comes_before_every_library_call(monkeypatch):
    dv = DagStub()
    order = []
    monkeypatch.setattr(dense, "_device", lambda dv: torch.device("cpu"))
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: True)
    monkeypatch.setattr(dense, "_sync", lambda device: order.append("sync"))
    tree = dense.build_octree(dv, torch.ones((4, 4, 4), dtype=torch.bool), collapse=False)
    for name in ("octree_dag_build", "octree_dag_write", "octree_dag_lookup", "octree_dag_to_dense"):
        monkeypatch.setattr(dv, name, (lambda real, name: lambda *a, **kw: order.append(name) or real(*a, **kw))(getattr(dv, name), name))
    del order[:]
    dag = dense.octree_dag(dv, tree)
    assert order == ["sync", "octree_dag_build", "octree_dag_write"]
    del order[:]
    dense.dag_lookup(dv, dag, torch.zeros((5, 3), dtype=torch.int32))
    dense.dag_to_dense(dv, dag, (4, 4, 4))
    assert order == ["sync", "octree_dag_lookup", "sync", "octree_dag_to_dense"]


def test_every_refusal_comes_before_any_device_call(on_cpu):  # noqa: F811
    dv = DagStub()
    tree = dense.build_octree(dv, torch.ones((4, 4, 4), dtype=torch.bool), collapse=False)
    dag = dense.octree_dag(dv, tree)
    del dv.calls[:]
    r = dataclasses.replace
    # octree_dag: what the octree queries refuse of a tree, and its own arguments
    for bad_tree, exc in ((dag, TypeError), (None, TypeError), (r(tree, valid=tree.valid[:-1]), ValueError), (r(tree, valid=tree.valid.to(torch.int32)), TypeError),
                          (r(tree, first_child=tree.first_child.to(torch.int64)), TypeError), (r(tree, full=tree.full.numpy()), TypeError),
                          (r(tree, valid=tree.valid.repeat_interleave(2)[::2]), TypeError), (r(tree, depth=0), ValueError), (r(tree, depth=17), ValueError),
                          (r(tree, depth=True), ValueError), (r(tree, collapsed=0), ValueError), (r(tree, valid=tree.valid.to("meta")), ValueError),
                          (r(tree, valid=tree.valid[:0], full=tree.full[:0], first_child=tree.first_child[:0]), ValueError),
                          (r(tree, level_offsets=(0, 1)), ValueError), (r(tree, level_offsets=[0, 1, 9]), ValueError), (r(tree, level_offsets=(0, 1, 8)), ValueError),
                          (r(tree, level_offsets=(0, 2, 9)), ValueError), (r(tree, level_offsets=(1, 2, 9)), ValueError), (r(tree, level_offsets=(0, 1.0, 9)), ValueError),
                          (r(tree, level_offsets=(0, 1, True)), ValueError), (r(tree, depth=3), ValueError)):
        with pytest.raises(exc):
            dense.octree_dag(dv, bad_tree)
    for skips in (1, None, "yes"):
        with pytest.raises(ValueError):
            dense.octree_dag(dv, tree, skips)
    # the queries: the DAG, then their own arguments
    pts = torch.zeros((5, 3), dtype=torch.int32)
    for bad_dag, exc in ((tree, TypeError), (as_ref(dag), TypeError), (r(dag, valid=dag.valid[:-1]), ValueError), (r(dag, child=dag.child.to(torch.int64)), TypeError),
                         (r(dag, skip=dag.skip[:-1]), ValueError), (r(dag, skip=dag.skip.numpy()), TypeError), (r(dag, full=dag.full.to(torch.int8)), TypeError),
                         (r(dag, child=dag.child.repeat_interleave(2)[::2]), TypeError), (r(dag, depth=0), ValueError), (r(dag, depth=17), ValueError),
                         (r(dag, depth=True), ValueError), (r(dag, collapsed=None), ValueError), (r(dag, child=dag.child.to("meta")), ValueError),
                         (r(dag, valid=dag.valid[:0], full=dag.full[:0], first_child=dag.first_child[:0]), ValueError)):
        with pytest.raises(exc):
            dense.dag_lookup(dv, bad_dag, pts)
        with pytest.raises(exc):
            dense.dag_to_dense(dv, bad_dag, (4, 4, 4))
    for bad, exc in ((pts.to(torch.int64), TypeError), (pts.float(), TypeError), (pts.numpy(), ValueError), (torch.zeros((5, 4), dtype=torch.int32), ValueError),
                     (torch.zeros((), dtype=torch.int32), ValueError), (pts.to("meta"), ValueError)):
        with pytest.raises(exc):
            dense.dag_lookup(dv, dag, bad)
    for args, kw, exc in ((((4, 4),), {}, ValueError), (((4, 0, 4),), {}, ValueError), (((4, 4, 4),), dict(origin=(0, -1, 0)), ValueError),
                          (((1, 1, 65537),), {}, ValueError), (((2048, 1024, 1024),), {}, ValueError), (((4, 4, 4),), dict(origin=(2 ** 32 - 3, 0, 0)), ValueError),
                          (((4, 4, 4),), dict(out=torch.zeros((4, 4, 5), dtype=torch.bool)), ValueError), (((4, 4, 4),), dict(out=torch.zeros((4, 4, 4))), TypeError),
                          (((4, 4, 4),), dict(out=np.zeros((4, 4, 4), bool)), ValueError), (((4, 4, 4),), dict(out=torch.zeros((4, 4, 4), dtype=torch.bool, device="meta")), ValueError)):
        with pytest.raises(exc):
            dense.dag_to_dense(dv, dag, *args, **kw)
    assert not dv.calls


def test_the_docstrings_and_constants():
    assert "section 34" in dense.__doc__ and "o2v_hip_octree_dag_build" in dense.__doc__ and "section 34" in dense.octree_dag.__doc__
    header = open(os.path.join(os.path.dirname(SRC), "..", "include", "o2v_hip.h")).read()
    for name in ("build", "write", "lookup", "to_dense", "times", "scratch_bytes"):
        assert "o2v_hip_octree_dag_%s(" % name in header, name
    for name in ("octree_dag_build", "octree_dag_write", "octree_dag_lookup", "octree_dag_to_dense", "octree_dag_times"):
        assert callable(getattr(hip.DeviceVoxelizer, name))
    for name in ("OctreeDag", "octree_dag", "dag_lookup", "dag_to_dense"):
        assert getattr(dense, name) is getattr(octree, name)
    # the scratch question needs no device: 8 bytes per node, the table and the scans of the widest levels, a DAG that merges nothing
    counts = [1, 8, 64, 512]
    want = 8 * 585 + 4 * 512 + 8 * (512 // 256 + 2) + 4 * 256 + 8 * 56 + 6 * 585 + 8 * 584
    assert hip.octree_dag_scratch_bytes(counts, 4) == want
    assert hip.octree_dag_scratch_bytes([1, 8, 64, 300, 512], 5) == want + 22 * 300 + 4 * (1024 - 256)
    assert hip.octree_dag_scratch_bytes(counts, 5) == want + 4 * (1024 - 256)   # (an empty last level: 512 nodes are now keyed through the table)
    for bad, depth in ((counts, 3), (counts, 0), (counts, 17), ([2, 8], 2), ([1, 2 ** 31], 2), ([0], 1)):
        assert hip.octree_dag_scratch_bytes(bad, depth) == 0, (bad, depth)


# ---- the code object ---------------------------------------------------------------------------------------------------------------

K30_KERNELS = ["k_dag_leaf_minE", "k_dag_leaf_repE", "k_dag_insertE", "k_dag_findE", "k_dag_flagsE", "k_dag_idsE", "k_dag_ptr_countE", "k_dag_emitE", "k_dag_lookupE",
               "k_dag_denseE"]
SCAN_LDS = 4 * 8   # fill_block_exscan64's word per wavefront: the only LDS of K30


@pytest.mark.parametrize("kernel", K30_KERNELS)
def test_k30_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    """From the code object's metadata only: wave64, at most 256 threads, no private segment, no LDS but the block scan's."""
    meta = device_asm[device_asm.index("amdhsa.kernels:"):]
    entry = [e for e in meta.split("\n  - ") if re.search(r"\.name: +_ZN\S*" + kernel + r"\S*\n", e)]
    assert len(entry) == 1, kernel + " is not in the gfx950 code object"
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
    assert int(re.search(r"\.wavefront_size: +(\d+)", entry[0]).group(1)) == 64
    assert int(re.search(r"\.max_flat_workgroup_size: +(\d+)", entry[0]).group(1)) == 256
    lds = int(re.search(r"\.group_segment_fixed_size: +(\d+)", entry[0]).group(1))
    assert lds == (SCAN_LDS if "flags" in kernel or "ptr_count" in kernel else 0)
