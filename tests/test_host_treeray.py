"""Rays through sparse voxel octrees and DAGs without a GPU: the walk of o2v_dev_k31_treeray.hpp compiled for
the host behind K11's walk part and the plain parts of K26 and K30, against the reference (tests/treeray_ref.py: to_dense of the
arrays, then the fine walk of tests/raycast_ref.py, then the lookup's slot) - tree and DAG, collapsed and not, with the stack and
without, on the grids of the device test; one mutation seen to fail; arrays that are no tree, through the same walk and, as a
stand-alone program with the arrays in exactly sized heap blocks, under the address and undefined-behaviour sanitizers;
obj2voxel_amd.dense's octree_raycast and dag_raycast against a stand-in for the device calls; the K31 kernels' metadata in the
gfx950 code object."""
import ctypes as C
import dataclasses
import functools
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import bits_host
from tests import octree_ref as R
from tests import raycast_ref as RC
from tests import treeray_ref as TR

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip, octree  # noqa: E402
from tests.test_host_dag import DagStub  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, device_asm, on_cpu  # noqa: E402,F401
from tests.test_host_octree import _array  # noqa: E402

F = np.float32
INF = float("inf")

HOST_TREERAY = r"""
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stddef.h>
#define __device__
#define __forceinline__ inline
using std::max;
using std::min;
%(bits)s
#define O2V_OCT_HOST
#define O2V_OCT_FN static inline
#define O2V_OCT_HD static inline
static inline uint32_t oct_popc(uint32_t v) { return (uint32_t) __builtin_popcount(v); }
%(k11)s
%(k26)s
%(k30)s
%(k31)s
// k_tree_cast ray by ray: its prologue and epilogue around tree_walk; the stack is a heap block of exactly depth - 1 entries
template <class Src, bool Stack>
static void cast_rays(const Src &src, const float *origins, const float *directions, uint64_t n, float t_max, int32_t *hit, float *t_out, int32_t *slot_out)
{
    TreeRayEntry *const entries = Stack ? new TreeRayEntry[src.depth() - 1u] : nullptr;
    for (uint64_t i = 0; i < n; ++i) {
        Ray r;
        bool valid = true;
        for (int b = 0; b < 3; ++b) {
            const float of = origins[i * 3 + b], df = directions[i * 3 + b];
            valid = valid && std::isfinite(of) && std::isfinite(df) && std::fabs(of) <= 4194304.f;
            r.o[b] = (double) of;
            r.d[b] = (double) df;
        }
        int32_t out[4] = {-1, -1, -1, -2}, slot = -1;
        float t = __builtin_nanf("");
        if (valid) {
            for (int b = 0; b < 3; ++b) {
                r.s[b] = r.d[b] > 0.0 ? 1 : r.d[b] < 0.0 ? -1 : 0;
                r.inv[b] = r.s[b] != 0 ? 1.0 / r.d[b] : 0.0;
                r.c[b] = (int32_t) floor(r.o[b]);
                r.nxt[b] = r.c[b] + (r.s[b] > 0 ? 1 : 0);
            }
            r.T = 0.0;
            r.face = -1;
            const TreeRayStack st{entries, 1u};
            if (tree_walk<Src, Stack>(r, (double) t_max, src, st, slot)) {
                out[0] = r.c[0], out[1] = r.c[1], out[2] = r.c[2], out[3] = r.face;
                t = (float) r.T;
            } else {
                out[3] = -1, slot = -1;
                t = __builtin_inff();
            }
        }
        for (int b = 0; b < 4; ++b) hit[i * 4 + b] = out[b];
        t_out[i] = t;
        slot_out[i] = slot;
    }
    delete[] entries;
}
extern "C" void treeray_host(const uint8_t *valid, const uint8_t *full, const int32_t *first_child, const int32_t *child, const int32_t *skip, uint32_t n_nodes,
                             uint32_t n_pointers, uint32_t depth, uint32_t collapsed, int dag, int stack, const float *origins, const float *directions, uint64_t n,
                             float t_max, int32_t *hit, float *t_out, int32_t *slot_out)
{
    const bool st = stack && depth > 1u;   // (as the launch decides)
    if (dag) {
        const TreeRayDag src{OctDag{valid, full, first_child, child, skip, n_nodes, n_pointers, depth, collapsed, dag_skips(skip, n_pointers)}};
        st ? cast_rays<TreeRayDag, true>(src, origins, directions, n, t_max, hit, t_out, slot_out)
           : cast_rays<TreeRayDag, false>(src, origins, directions, n, t_max, hit, t_out, slot_out);
    } else {
        const TreeRayOct src{OctTree{valid, full, first_child, n_nodes, depth, collapsed}};
        st ? cast_rays<TreeRayOct, true>(src, origins, directions, n, t_max, hit, t_out, slot_out)
           : cast_rays<TreeRayOct, false>(src, origins, directions, n, t_max, hit, t_out, slot_out);
    }
}
#ifdef TREERAY_MAIN
// The stand-alone program: argv[1] holds cases - nine words (dag, stack, depth, collapsed, n_nodes, n_pointers, has_skip, n_rays, the
// bits of t_max), then valid, full, first_child, child, skip, origins, directions -, argv[2] takes hit, t and slot of each.  Every
// array is read into a heap block of exactly its size, so a read outside one is the sanitizer's to report.
template <class T>
static T *block(FILE *f, size_t n)
{
    T *p = (T *) malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, f) != n) exit(3);
    return p;
}
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t h[9];
    int cases = 0;
    while (fread(h, 4, 9, in) == 9) {
        uint8_t *valid = block<uint8_t>(in, h[4]), *full = block<uint8_t>(in, h[4]);
        int32_t *first_child = block<int32_t>(in, h[4]), *child = block<int32_t>(in, h[5]), *skip = block<int32_t>(in, h[6] ? h[5] : 0);
        float *origins = block<float>(in, 3 * (size_t) h[7]), *directions = block<float>(in, 3 * (size_t) h[7]), t_max;
        __builtin_memcpy(&t_max, &h[8], 4);
        int32_t *hit = (int32_t *) malloc(16 * (size_t) h[7] + 1), *slot = (int32_t *) malloc(4 * (size_t) h[7] + 1);
        float *t = (float *) malloc(4 * (size_t) h[7] + 1);
        treeray_host(valid, full, first_child, h[5] ? child : nullptr, h[6] && h[5] ? skip : nullptr, h[4], h[5], h[2], h[3], (int) h[0], (int) h[1], origins,
                     directions, h[7], t_max, hit, t, slot);
        fwrite(hit, 16, h[7], out), fwrite(t, 4, h[7], out), fwrite(slot, 4, h[7], out);
        free(valid), free(full), free(first_child), free(child), free(skip), free(origins), free(directions), free(hit), free(slot), free(t);
        ++cases;
    }
    fclose(in);
    if (fclose(out)) return 4;
    printf("%%d cases\n", cases);
    return 0;
}
#endif
"""


def _between(path, start, end):
    text = open(path).read()
    return text[text.index(start):text.index(end)]


def host_source():
    """the translation unit: the bit grid's plain part, K11's declarations and walk, K26's and K30's plain parts, K31's walk"""
    k11 = os.path.join(SRC, "o2v_dev_k11_raycast.hpp")
    k26 = os.path.join(SRC, "o2v_dev_k26_octree.hpp")
    k30 = os.path.join(SRC, "o2v_dev_k30_dag.hpp")
    k31 = os.path.join(SRC, "o2v_dev_k31_treeray.hpp")
    return HOST_TREERAY % dict(
        bits=bits_host.plain_part(),
        k11=_between(k11, "constexpr uint32_t kRayU8", "// ---- build") + _between(k11, "// ---- the walk", "// ---- the cast kernel"),
        k26=_between(k26, "constexpr uint32_t kOctMaxDepth", "#ifndef O2V_OCT_HOST") + _between(k26, "// ---- cells, bit pairs", "// ---- kernels"),
        k30=_between(k30, "constexpr uint32_t kDagEmpty", "// ---- kernels"),
        k31=_between(k31, "// ---- the walk", "// ---- the cast kernel"))


def _compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    return cxx


def array_args(a):
    """(keep-alive list, the nine leading arguments of treeray_host) of a tree's or a DAG's dict"""
    dag = TR.is_dag(a)
    names = ("valid", "full", "first_child") + (("child", "skip") if dag else ())
    keep = [np.ascontiguousarray(a[k]) for k in names if a.get(k) is not None]
    p = [k.ctypes.data if len(k) else None for k in keep] + [None] * (5 - len(keep))
    return keep, p + [len(a["valid"]), len(a["child"]) if dag else 0, a["depth"], int(a["collapsed"]), int(dag)]


@pytest.fixture(scope="module")
def host_treeray(tmp_path_factory):
    """build(defines) -> cast(arrays, o, d, t_max, stack): (hit, t, slot) by the kernels' walk on the host"""
    cxx = _compiler()
    tmp = tmp_path_factory.mktemp("host_treeray")

    @functools.lru_cache(None)
    def build(defines=()):
        name = "treeray_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(host_source())
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = C.CDLL(str(tmp / (name + ".so")))
        L.treeray_host.argtypes = [C.c_void_p] * 5 + [C.c_uint32] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_float] + [C.c_void_p] * 3
        L.treeray_host.restype = None

        def cast(a, o, d, t_max=INF, stack=True):
            keep, args = array_args(a)
            o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
            n = len(o)
            hit, t, slot = np.full((n, 4), -9, np.int32), np.full(n, -9, F), np.full(n, -9, np.int32)
            L.treeray_host(*args, int(stack), o.ctypes.data, d.ctypes.data, n, t_max, hit.ctypes.data, t.ctypes.data, slot.ctypes.data)
            return hit, t, slot
        return cast
    return build


scene = TR.scene   # (grid k with its rays and the reference's casts, made once: the numpy walk is slow)


@pytest.mark.parametrize("k", range(len(TR.grids())))
def test_the_walk_on_the_host_equals_the_reference(host_treeray, k):
    cast = host_treeray()
    name, g, origin, depth, o, d, want, short = scene(k)
    n = 0
    for what, a in TR.sources(g, origin, depth):
        # the solid set of the arrays is the grid (tests/test_host_octree.py, test_host_dag.py): the reference's walk is made once
        want_slot = TR.slots(a, want[0])
        for stack in (True, False):
            got = cast(a, o, d, INF, stack)
            assert TR.same(got, want + (want_slot,)), (name, what, stack, TR.first_difference(got, want + (want_slot,), o, d))
            for t_max, w in short.items():
                got = cast(a, o[:TR.N_SHORT], d[:TR.N_SHORT], t_max, stack)
                assert TR.same(got, w + (TR.slots(a, w[0]),)), (name, what, stack, t_max)
            n += 1
        if TR.is_dag(a) and len(a["child"]):   # (a DAG of a root alone has nothing to skip)
            bare = cast(dict(a, skip=None), o, d, INF, True)
            assert RC.same(bare[:2], want) and (bare[2] == -1).all()
    assert n == 8
    # a collapsed tree has no slot inside a full cell; the plain one has a slot for every hit
    plain = TR.slots(TR.sources(g, origin, depth)[2][1], want[0])
    assert ((plain >= 0) == (want[0][:, 0] >= 0)).all()


def test_the_reference_over_the_root_cube_and_over_the_box_agree(host_treeray):
    """The reference's own two routes - to_dense over the root cube and over the grid's box - give one result, and the host walk
    gives it too, the slot included (the other tests take the walk over the box)."""
    cast = host_treeray()
    name, g, origin, depth, o, d, want, _ = scene(3)   # the 7 x 5 x 3 box at (1, 3, 5)
    for what, a in TR.sources(g, origin, depth):
        assert np.array_equal(TR.solid_set(a, (g.shape, origin))[0], g)
        cube = TR.solid_set(a)
        assert cube[0].sum() == g.sum() and cube[0].shape == (8, 8, 8)
        over_cube = TR.cast(a, o[:500], d[:500], solid=cube)
        assert TR.same(over_cube, (want[0][:500], want[1][:500]))
        assert TR.same(cast(a, o[:500], d[:500]), over_cube), what


def test_a_block_one_level_too_large_is_caught(host_treeray):
    """With O2V_TREERAY_MUTATE_BLOCK_SHIFT the empty octant's block is taken twice as wide: rays jump over solid voxels."""
    cast = host_treeray(("O2V_TREERAY_MUTATE_BLOCK_SHIFT",))
    for k in (0, 4):
        name, g, origin, depth, o, d, want, _ = scene(k)
        for what, a in TR.sources(g, origin, depth):
            for stack in (True, False):
                assert not RC.same(cast(a, o, d, INF, stack)[:2], want), (name, what, stack)


@functools.lru_cache(None)
def broken_scenes():
    """[(name, arrays, their solid set, o, d, the reference's (hit, t, slot))] of treeray_ref.not_a_tree()"""
    out = []
    for k, (name, a) in enumerate(TR.not_a_tree()):
        solid = TR.solid_set(a)
        o, d = TR.broken_rays(k, solid)
        out.append((name, a, solid[0], o, d, TR.cast(a, o, d, solid=solid)))
    return out


def test_arrays_that_are_no_tree_on_the_host(host_treeray):
    """Whatever the arrays hold, the walk gives what RayCaster's reference gives on to_dense of the same arrays."""
    cast = host_treeray()
    scenes = broken_scenes()
    assert len(scenes) == 2 * (8 + 2 + 8 + 4)
    changed = 0
    for name, a, solid, o, d, want in scenes:
        for stack in (True, False):
            got = cast(a, o, d, INF, stack)
            assert TR.same(got, want), (name, stack, TR.first_difference(got, want, o, d))
        changed += not np.array_equal(solid, TR.broken_grid())
    assert changed >= len(scenes) // 2, changed   # (the cases are not vacuous: most of them change the solid set)


def test_the_walk_under_the_sanitizers(tmp_path):
    """The stand-alone program - its own main, the walk, the arrays of treeray_ref.not_a_tree() in exactly sized heap blocks - built
    with -fsanitize=address,undefined and run as a process of its own: no report, and the reference's results."""
    cxx = _compiler()
    src, exe = tmp_path / "treeray_main.cpp", tmp_path / "treeray_main"
    src.write_text(host_source())
    cmd = [cxx, "-x", "c++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DTREERAY_MAIN", str(src),
           "-o", str(exe)]
    # the runtimes linked into the program where the compiler has them as archives: the program then starts whatever else a process loads first
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"asan|ubsan|sanitizer|-fsanitize", r.stderr, re.I):
        pytest.skip("the compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    scenes = broken_scenes()
    with open(tmp_path / "in.bin", "wb") as f:
        for name, a, _, o, d, want in scenes:
            for stack in (1, 0):
                dag = TR.is_dag(a)
                P = len(a["child"]) if dag else 0
                f.write(struct.pack("<8If", int(dag), stack, a["depth"], int(a["collapsed"]), len(a["valid"]), P, int(dag), len(o), INF))
                for key, dtype in (("valid", np.uint8), ("full", np.uint8), ("first_child", np.int32)) + ((("child", np.int32), ("skip", np.int32)) if dag else ()):
                    f.write(np.ascontiguousarray(a[key], dtype).tobytes())
                f.write(np.ascontiguousarray(o, F).tobytes() + np.ascontiguousarray(d, F).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env, timeout=300)
    if r.returncode != 0 and "runtime does not come first" in r.stderr:
        pytest.fail("the sanitized program did not start: its sanitizer runtime is a shared one (the compiler has no archive to link into the program) and "
                    "another library is loaded before it, so the walk over the arrays that are no tree was NOT checked under the sanitizers here")
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip() == "%d cases" % (2 * len(scenes))
    raw = open(tmp_path / "out.bin", "rb").read()
    at = 0
    for name, a, _, o, d, want in scenes:
        for stack in (1, 0):
            n = len(o)
            hit = np.frombuffer(raw, np.int32, 4 * n, at).reshape(n, 4)
            t = np.frombuffer(raw, F, n, at + 16 * n)
            slot = np.frombuffer(raw, np.int32, n, at + 20 * n)
            at += 24 * n
            assert TR.same((hit, t, slot), want), (name, stack)
    assert at == len(raw)


# ---- dense.* against a stand-in -------------------------------------------------------------------------------------------------------

class TreeRayStub(DagStub):
    """DagStub and the two casts, computed with the reference on the host memory behind the pointers."""

    def _cast(self, a, origins_ptr, directions_ptr, n, t_max, hit_ptr, t_ptr, voxel_index_ptr, skips=True):
        o, d = (_array(p, C.c_float, 3 * n).reshape(-1, 3) for p in (origins_ptr, directions_ptr))
        hit, t, slot = TR.cast(a, o, d, t_max, skips=skips)
        _array(hit_ptr, C.c_int32, 4 * n)[:] = hit.reshape(-1)
        _array(t_ptr, C.c_float, n)[:] = t
        if voxel_index_ptr is not None:
            _array(voxel_index_ptr, C.c_int32, n)[:] = slot

    def octree_raycast(self, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags, origins_ptr, directions_ptr, n, t_max, hit_ptr, t_ptr, voxel_index_ptr=None):
        self.calls.append(dict(call="raycast", n_nodes=n_nodes, depth=depth, flags=flags, n=n, t_max=t_max, origins=origins_ptr, voxel_index=voxel_index_ptr))
        self._cast(self._tree(valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags), origins_ptr, directions_ptr, n, t_max, hit_ptr, t_ptr, voxel_index_ptr)

    def octree_dag_raycast(self, valid_ptr, full_ptr, first_child_ptr, child_ptr, skip_ptr, n_nodes, n_pointers, depth, flags, origins_ptr, directions_ptr, n, t_max,
                           hit_ptr, t_ptr, voxel_index_ptr=None):
        self.calls.append(dict(call="dag_raycast", n_nodes=n_nodes, n_pointers=n_pointers, depth=depth, flags=flags, n=n, t_max=t_max, skip=skip_ptr,
                               voxel_index=voxel_index_ptr))
        a = self._dag(valid_ptr, full_ptr, first_child_ptr, child_ptr, skip_ptr, n_nodes, n_pointers, depth, flags)
        self._cast(a, origins_ptr, directions_ptr, n, t_max, hit_ptr, t_ptr, voxel_index_ptr, skips=skip_ptr is not None or not n_pointers)


def small_scene(dv, collapse):
    g = R.blobs(np.random.default_rng(352), (7, 6, 5), 0.6)
    tree = dense.build_octree(dv, torch.from_numpy(g), origin=(1, 0, 2), collapse=collapse)
    dag = dense.octree_dag(dv, tree)
    o, d = RC.ray_set(np.random.default_rng(353), g, (1, 0, 2), n=300, far=0, limit=0)
    return g, tree, dag, torch.from_numpy(o), torch.from_numpy(d)


def test_casts_through_the_stand_in(on_cpu):  # noqa: F811
    dv = TreeRayStub()
    for collapse in (True, False):
        g, tree, dag, o, d = small_scene(dv, collapse)
        want = RC.cast(g, (1, 0, 2), o.numpy(), d.numpy())[:2]
        out = dense.octree_raycast(dv, tree, o, d)
        assert len(out) == 2 and out[0].dtype == torch.int32 and out[1].dtype == torch.float32 and RC.same((out[0].numpy(), out[1].numpy()), want)
        c = dv.calls[-1]
        assert (c["call"], c["n_nodes"], c["depth"], c["flags"], c["n"], c["t_max"], c["voxel_index"]) == ("raycast", len(tree.valid), 3, hip.OCT_COLLAPSE * collapse,
                                                                                                            len(o), INF, None)
        hit, t, slot = dense.octree_raycast(dv, tree, o, d, voxel_index=True)
        assert dv.calls[-1]["voxel_index"] == slot.data_ptr() and slot.dtype == torch.int32 and tuple(slot.shape) == (len(o),)
        looked = dense.octree_lookup(dv, tree, hit[:, :3].contiguous())[:, 3]
        assert torch.equal(slot, torch.where(hit[:, 0] >= 0, looked, torch.full_like(looked, -1)))
        hit2, t2, slot2 = dense.dag_raycast(dv, dag, o, d, voxel_index=True)
        assert torch.equal(hit2, hit) and torch.equal(slot2, slot) and RC.same((hit2.numpy(), t2.numpy()), want)
        c = dv.calls[-1]
        assert (c["call"], c["n_nodes"], c["n_pointers"], c["skip"]) == ("dag_raycast", len(dag.valid), len(dag.child), dag.skip.data_ptr())
        bare = dense.dag_raycast(dv, dataclasses.replace(dag, skip=None), o, d, voxel_index=True)
        assert dv.calls[-1]["skip"] is None and torch.equal(bare[0], hit) and bool((bare[2] == -1).all())
        assert len(dense.dag_raycast(dv, dag, o, d, t_max=2.5)) == 2 and dv.calls[-1]["t_max"] == 2.5 and dv.calls[-1]["voxel_index"] is None
        # shapes [..., 3], rays that are not contiguous, no rays: no call
        for shape in ((5, 3), (2, 3, 3), (3,), (4, 1, 2, 3)):
            oo, dd = o[:int(np.prod(shape[:-1]))].reshape(shape), d[:int(np.prod(shape[:-1]))].reshape(shape)
            h, tt, s = dense.octree_raycast(dv, tree, oo, dd, voxel_index=True)
            assert tuple(h.shape) == shape[:-1] + (4,) and tuple(tt.shape) == shape[:-1] == tuple(s.shape)
            assert torch.equal(h.reshape(-1, 4), hit[:h.numel() // 4]) and torch.equal(s.reshape(-1), slot[:s.numel()])
        wide = torch.zeros((len(o), 6))
        wide[:, ::2] = o
        h, _ = dense.octree_raycast(dv, tree, wide[:, ::2], d)
        assert dv.calls[-1]["origins"] != wide.data_ptr() and torch.equal(h, hit)
        before = len(dv.calls)
        h, tt, s = dense.dag_raycast(dv, dag, o[:0], d[:0], voxel_index=True)
        assert tuple(h.shape) == (0, 4) and tuple(tt.shape) == (0,) == tuple(s.shape) and len(dv.calls) == before
    # camera_rays feeds the call
    co, cd = dense.camera_rays(9, 7, (20.0, -15.0, 12.0), (4.0, 3.0, 4.0), (0, 0, 1), 40.0, torch.device("cpu"))
    h, tt = dense.dag_raycast(dv, dag, co, cd)
    assert tuple(h.shape) == (7, 9, 4) and tuple(tt.shape) == (7, 9) and bool((h[..., 0] >= 0).any())


def test_the_wait_comes_before_the_library_call(monkeypatch):
    dv = TreeRayStub()
    order = []
    monkeypatch.setattr(dense, "_device", lambda dv: torch.device("cpu"))
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: True)
    monkeypatch.setattr(dense, "_sync", lambda device: order.append("sync"))
    g, tree, dag, o, d = small_scene(dv, False)
    for name in ("octree_raycast", "octree_dag_raycast"):
        monkeypatch.setattr(dv, name, (lambda real, name: lambda *a, **kw: order.append(name) or real(*a, **kw))(getattr(dv, name), name))
    del order[:]
    dense.octree_raycast(dv, tree, o, d)
    dense.dag_raycast(dv, dag, o, d, voxel_index=True)
    assert order == ["sync", "octree_raycast", "sync", "octree_dag_raycast"]


def test_every_refusal_comes_before_any_device_call(on_cpu):  # noqa: F811
    dv = TreeRayStub()
    g, tree, dag, o, d = small_scene(dv, False)
    del dv.calls[:]
    r = dataclasses.replace
    for bad_tree, exc in ((dag, TypeError), (None, TypeError), (r(tree, valid=tree.valid[:-1]), ValueError), (r(tree, first_child=tree.first_child.to(torch.int64)), TypeError),
                          (r(tree, depth=0), ValueError), (r(tree, depth=17), ValueError), (r(tree, collapsed=0), ValueError), (r(tree, valid=tree.valid.to("meta")), ValueError),
                          (r(tree, valid=tree.valid[:0], full=tree.full[:0], first_child=tree.first_child[:0]), ValueError)):
        with pytest.raises(exc):
            dense.octree_raycast(dv, bad_tree, o, d)
    for bad_dag, exc in ((tree, TypeError), (r(dag, child=dag.child.to(torch.int64)), TypeError), (r(dag, skip=dag.skip[:-1]), ValueError), (r(dag, depth=True), ValueError),
                         (r(dag, collapsed=None), ValueError), (r(dag, child=dag.child.to("meta")), ValueError)):
        with pytest.raises(exc):
            dense.dag_raycast(dv, bad_dag, o, d)
    for kw, exc in ((dict(origins=o.double()), TypeError), (dict(directions=d.to(torch.int32)), TypeError), (dict(origins=o.numpy()), TypeError),
                    (dict(origins=torch.zeros((len(o), 4)), directions=torch.zeros((len(o), 4))), ValueError), (dict(origins=torch.zeros(())), ValueError),
                    (dict(origins=o[:-1]), ValueError), (dict(directions=d.to("meta")), ValueError), (dict(t_max=-1.0), ValueError), (dict(t_max=float("nan")), ValueError),
                    (dict(t_max="1"), ValueError), (dict(t_max=True), ValueError), (dict(voxel_index=1), ValueError), (dict(voxel_index=None), ValueError)):
        args = dict(origins=o, directions=d)
        args.update(kw)
        with pytest.raises(exc):
            dense.octree_raycast(dv, tree, args.pop("origins"), args.pop("directions"), **args)
        args = dict(origins=o, directions=d)
        args.update(kw)
        with pytest.raises(exc):
            dense.dag_raycast(dv, dag, args.pop("origins"), args.pop("directions"), **args)
    assert not dv.calls


def test_refused_when_the_library_came_first(monkeypatch):
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: False)
    with pytest.raises(RuntimeError, match="before torch"):
        dense.octree_raycast(TreeRayStub(), None, torch.zeros((1, 3)), torch.ones((1, 3)))


def test_the_docstrings_and_constants():
    assert "section 35" in dense.__doc__ and "o2v_hip_octree_raycast" in dense.__doc__ and "section 35" in dense.octree_raycast.__doc__
    header = open(os.path.join(os.path.dirname(SRC), "..", "include", "o2v_hip.h")).read()
    for name in ("o2v_hip_octree_raycast(", "o2v_hip_octree_dag_raycast(", "o2v_hip_octree_raycast_times(", "O2V_TREERAY_NO_STACK"):
        assert name in header, name
    for name in ("octree_raycast", "octree_dag_raycast", "octree_raycast_times"):
        assert callable(getattr(hip.DeviceVoxelizer, name))
    for name in ("octree_raycast", "dag_raycast"):
        assert getattr(dense, name) is getattr(octree, name)
    device = open(os.path.join(SRC, "o2v_device.hip")).read()
    assert 'env_on("O2V_TREERAY_NO_STACK")' in device and '#include "o2v_dev_host_k31_treeray.hpp"' in device
    # K11's header is used as it is: the walk of K31 names its ray, its step and its advance and defines none of them
    walk = _between(os.path.join(SRC, "o2v_dev_k31_treeray.hpp"), "// ---- the walk", "// ---- the cast kernel")
    assert "ray_advance(r, TE, aE, xE, lim)" in walk and "ray_step(r, tmax)" in walk and "struct Ray " not in walk and "__global__" not in walk


# ---- the code object ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["k_tree_castINS_10TreeRayOctELb1E", "k_tree_castINS_10TreeRayOctELb0E", "k_tree_castINS_10TreeRayDagELb1E",
                                    "k_tree_castINS_10TreeRayDagELb0E"])
def test_k31_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    """From the code object's metadata: wave64, 256 threads, no private segment, no vector register spilled, no LDS but the
    dynamic stack (which the launch sizes)."""
    meta = device_asm[device_asm.index("amdhsa.kernels:"):]
    entry = [e for e in meta.split("\n  - ") if re.search(r"\.name: +_ZN\S*" + kernel + r"\S*\n", e)]
    assert len(entry) == 1, kernel + " is not in the gfx950 code object"
    assert re.search(r"\.private_segment_fixed_size: +0\n", entry[0])
    assert int(re.search(r"\.vgpr_spill_count: +(\d+)", entry[0]).group(1)) == 0
    assert int(re.search(r"\.wavefront_size: +(\d+)", entry[0]).group(1)) == 64
    assert int(re.search(r"\.max_flat_workgroup_size: +(\d+)", entry[0]).group(1)) == 256
    assert int(re.search(r"\.group_segment_fixed_size: +(\d+)", entry[0]).group(1)) == 0
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m and "scratch_" not in m.group(2)
    assert re.findall(r"; ScratchSize: (\d+)", device_asm[m.end():m.end() + 4000])[:1] == ["0"]
    if "Lb1E" in kernel:
        assert re.search(r"ds_(read|write|load|store)_b64", m.group(2)), "the stack's entries move as one 8-byte LDS access"
