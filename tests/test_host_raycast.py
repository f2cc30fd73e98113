"""Ray casting without a GPU: the numpy reference (tests/raycast_ref.py) against a scalar pure-Python restatement of the
header's walk; an independent Python implementation that skips empty blocks and enters the box from outside, equal to the
reference on every ray (the exactness claim of include/o2v_hip.h); dense.RayCaster / raycast / camera_rays with the device
calls stubbed; the K11 kernels in the gfx950 code object; the scratch formula."""
import math
import os
import re

import numpy as np
import pytest

from tests import raycast_ref as R

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_dense import StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401

F = np.float32
INF = float("inf")


# ---- the header's walk, ray by ray, in Python floats (doubles; CPython does not fuse) ------------------------------------------

def scalar_cast(solid, origin, o32, d32, t_max=INF):
    nz, ny, nx = solid.shape
    lo, hi = list(origin), [origin[0] + nx, origin[1] + ny, origin[2] + nz]
    tmax = float(F(t_max))
    hits, ts = [], []
    for of, df in zip(np.asarray(o32, F).reshape(-1, 3), np.asarray(d32, F).reshape(-1, 3)):
        o, d = [float(v) for v in of], [float(v) for v in df]
        if not all(math.isfinite(v) for v in o + d) or any(abs(v) > 2.0 ** 22 for v in o):
            hits.append([-1, -1, -1, -2])
            ts.append(F(np.nan))
            continue
        s = [1 if v > 0 else (-1 if v < 0 else 0) for v in d]
        inv = [1.0 / v if v != 0 else 0.0 for v in d]
        c = [math.floor(v) for v in o]
        n = [c[a] + 1 if d[a] > 0 else c[a] for a in range(3)]

        def solid_at(c):
            return all(lo[a] <= c[a] < hi[a] for a in range(3)) and bool(solid[c[2] - lo[2], c[1] - lo[1], c[0] - lo[0]])
        if solid_at(c):
            hits.append(c + [-1])
            ts.append(F(0))
            continue
        while True:
            best, a = None, None
            for b in range(3):
                if s[b] != 0:
                    T = (float(n[b]) - o[b]) * inv[b]
                    if best is None or T < best:
                        best, a = T, b
            if a is None or best > tmax:
                hits.append([-1, -1, -1, -1])
                ts.append(F(np.inf))
                break
            c[a] += s[a]
            n[a] += s[a]
            if solid_at(c):
                hits.append(c + [2 * a + (0 if s[a] > 0 else 1)])
                with np.errstate(over="ignore"):
                    ts.append(F(best))
                break
            if any((s[b] > 0 and c[b] >= hi[b]) or (s[b] < 0 and c[b] < lo[b]) or (s[b] == 0 and not lo[b] <= c[b] < hi[b]) for b in range(3)):
                hits.append([-1, -1, -1, -1])
                ts.append(F(np.inf))
                break
    return np.array(hits, np.int32).reshape(-1, 4), np.array(ts, F)


def test_numpy_double_ops_are_not_fused():
    rng = np.random.default_rng(1)
    i = rng.integers(-2 ** 22, 2 ** 22, 64)
    o = (rng.normal(size=64) * 10.0 ** rng.uniform(-3, 6, 64)).astype(F).astype(np.float64)
    d = (rng.normal(size=64) * 10.0 ** rng.uniform(-40, 38, 64)).astype(F).astype(np.float64)
    d[d == 0] = 1.0
    inv = 1.0 / d
    got = R.plane_T(i, o, inv)
    for k in range(64):
        assert float(inv[k]) == 1.0 / float(d[k])
        assert float(got[k]) == (float(int(i[k])) - float(o[k])) * float(inv[k])


def family_rays(rng, solid, origin, m):
    """The families the issue names, on a small grid: lattice, axis-parallel, d = 0, rays from outside that miss, graze a face
    of the box, or enter it through an edge or a corner."""
    nz, ny, nx = solid.shape
    dims = np.array([nx, ny, nz], float)
    lo = np.asarray(origin, float)
    hi = lo + dims
    O, Dd = [], []
    # lattice
    O.append(lo + rng.integers(-3, int(dims.max()) + 3, (m, 3)) + rng.integers(0, 2, (m, 3)) * 0.5)
    Dd.append(rng.integers(-3, 4, (m, 3)).astype(float))
    # axis-parallel, on and off the planes
    o = lo + (rng.random((m, 3)) * 1.4 - 0.2) * dims
    o = np.where(rng.random((m, 3)) < 0.4, np.floor(o), o)
    d = np.zeros((m, 3))
    d[np.arange(m), rng.integers(0, 3, m)] = rng.choice([1.0, -1.0, 0.3, -7.0], m)
    O.append(o)
    Dd.append(d)
    # d = 0
    O.append(lo + (rng.random((m // 4, 3)) * 1.4 - 0.2) * dims)
    Dd.append(np.zeros((m // 4, 3)) * rng.choice([1.0, -1.0], (m // 4, 3)))
    # from outside: through a point of a face, an edge or a corner of the box (and past it: a graze or a miss)
    k = rng.integers(0, 4, m)                       # how many coordinates lie on the box's planes
    p = lo + rng.random((m, 3)) * dims
    on = np.argsort(rng.random((m, 3)), axis=1) < k[:, None]
    p = np.where(on, np.where(rng.random((m, 3)) < 0.5, lo, hi), p)
    d = rng.integers(-2, 3, (m, 3)).astype(float) + rng.choice([0.0, 0.0, 0.25], (m, 3))
    O.append(p - d * rng.integers(1, 6, (m, 1)))
    Dd.append(d)
    # along a face of the box, inside and outside of it
    o = lo + rng.random((m // 2, 3)) * dims
    d = rng.normal(size=(m // 2, 3))
    a = rng.integers(0, 3, m // 2)
    ar = np.arange(m // 2)
    o[ar, a] = np.where(rng.random(m // 2) < 0.5, lo[a], hi[a])
    d[ar, a] = rng.choice([0.0, -0.0, 1e-42, -1e-42], m // 2)
    O.append(o - d * 3)
    Dd.append(d)
    return np.concatenate(O).astype(F), np.concatenate(Dd).astype(F)


@pytest.mark.parametrize("dims, origin, seed", [((5, 6, 7), (0, 0, 0), 0), ((9, 1, 4), (3, 2, 1), 1), ((1, 1, 1), (7, 7, 7), 2),
                                                ((17, 5, 3), (0, 65000, 2), 3), ((4, 4, 4), (1, 0, 0), 4)])
def test_reference_equals_the_scalar_restatement(dims, origin, seed):
    rng = np.random.default_rng(seed)
    for density in (0.0, 0.03, 0.3, 1.0):
        solid = rng.random(dims[::-1]) < density
        o, d = family_rays(rng, solid, origin, 160)
        o2, d2 = R.ray_set(rng, solid, origin, 300, far=0, limit=0)
        o3, d3 = R.extreme_rays(rng, solid, origin, 100)
        o, d = np.concatenate([o, o2, o3]), np.concatenate([d, d2, d3])
        for t_max in (INF, 0.0, 2.5, 1e-3):
            got = R.cast_lockstep(solid, origin, o, d, t_max)
            want = scalar_cast(solid, origin, o, d, t_max)
            assert R.same(got, want), (density, t_max, np.nonzero((got[0] != want[0]).any(axis=1))[0][:5])


def test_t_max_equal_to_a_plane_still_crosses_it():
    solid = np.zeros((1, 1, 8), bool)
    solid[0, 0, 5] = True
    o, d = np.array([[0.5, 0.5, 0.5]], F), np.array([[0.3, 0, 0]], F)
    hit, t, _ = R.cast_lockstep(solid, (0, 0, 0), o, d)
    assert hit.tolist() == [[5, 0, 0, 0]]
    T = (5.0 - 0.5) * (1.0 / float(F(0.3)))
    assert float(t[0]) == float(F(T))
    # the smallest float32 t_max whose double is >= T hits; the one below it misses
    up = F(T) if float(F(T)) >= T else np.nextafter(F(T), F(np.inf))
    assert R.cast_lockstep(solid, (0, 0, 0), o, d, up)[0][0, 3] == 0
    assert R.cast_lockstep(solid, (0, 0, 0), o, d, np.nextafter(up, F(0)))[0][0, 3] == -1
    # d = 1: T is the integer 4.5 + ... exactly representable: t_max == T is a hit, since the test is T > t_max
    d1 = np.array([[1, 0, 0]], F)
    assert R.cast_lockstep(solid, (0, 0, 0), o, d1, 4.5)[0].tolist() == [[5, 0, 0, 0]]
    assert R.cast_lockstep(solid, (0, 0, 0), o, d1, np.nextafter(F(4.5), F(0)))[0].tolist() == [[-1, -1, -1, -1]]
    assert R.same(R.cast_lockstep(solid, (0, 0, 0), o, d1, 4.5)[:2], scalar_cast(solid, (0, 0, 0), o, d1, 4.5))


def test_a_ray_on_a_face_pointing_down_visits_floor_o_first():
    solid = np.zeros((1, 1, 6), bool)
    solid[0, 0, 3] = True
    o, d = np.array([[3.0, 0.5, 0.5], [4.0, 0.5, 0.5]], F), np.array([[-1, 0, 0], [-1, 0, 0]], F)
    hit, t, _ = R.cast_lockstep(solid, (0, 0, 0), o, d)
    assert hit.tolist() == [[3, 0, 0, -1], [3, 0, 0, 1]] and t.tolist() == [0.0, 0.0]


def test_the_event_walk_equals_the_lockstep_walk():
    rng = np.random.default_rng(5)
    solid = R.random_solid(rng, (40, 9, 21), 0.004)
    origin = (3, 4, 5)
    o, d = R.ray_set(rng, solid, origin, 1500, far=30, limit=0)
    o2, d2 = R.extreme_rays(rng, solid, origin, 300)
    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    near = R.distance_to_box(solid, origin, o) < 3000          # (the lockstep loop runs as long as its longest ray)
    o, d = o[near], d[near]
    for t_max in (INF, 30.0):
        hit, t, steps = R.cast_lockstep(solid, origin, o, d, t_max)
        total = 0
        for i in range(len(o)):
            h, tt, k = R.walk_events(solid, origin, o[i:i + 1], d[i:i + 1], t_max, first_chunk=8, max_chunk=64)
            assert np.array_equal(h, hit[i]) and F(tt).view(np.uint32) == t[i].view(np.uint32), (i, o[i], d[i], h, hit[i])
            total += k
        assert total == steps


# ---- skipping is exact: an independent implementation with blocks of 4 and 16 and entry from outside -----------------------------

def skip_cast(solid, origin, o32, d32, t_max=INF, blocks=(16, 4)):
    """Advance to event E, then put every other axis at its first plane behind E: include/o2v_hip.h, "why empty space can be
    skipped exactly".  Events are compared as tuples (T, axis).  Returns (hit, t, iterations)."""
    nz, ny, nx = solid.shape
    dims = [nx, ny, nz]
    lo, hi = list(origin), [origin[a] + dims[a] for a in range(3)]
    empty = {}
    for B in blocks:
        pad = np.zeros([-(-n // B) * B for n in (nz, ny, nx)], bool)
        pad[:nz, :ny, :nx] = solid
        empty[B] = ~pad.reshape(pad.shape[0] // B, B, pad.shape[1] // B, B, pad.shape[2] // B, B).any(axis=(1, 3, 5))
    tmax = float(F(t_max))
    hits, ts, iterations = [], [], 0
    for of, df in zip(np.asarray(o32, F).reshape(-1, 3), np.asarray(d32, F).reshape(-1, 3)):
        o, d = [float(v) for v in of], [float(v) for v in df]
        if not all(math.isfinite(v) for v in o + d) or any(abs(v) > 2.0 ** 22 for v in o):
            hits.append([-1, -1, -1, -2])
            ts.append(F(np.nan))
            continue
        s = [1 if v > 0 else (-1 if v < 0 else 0) for v in d]
        inv = [1.0 / v if v != 0 else 0.0 for v in d]
        c = [math.floor(v) for v in o]
        n = [c[a] + 1 if d[a] > 0 else c[a] for a in range(3)]
        T_of = lambda a, j: ((float(j) - o[a]) * inv[a], a)   # noqa: E731  (the event of plane j of axis a)
        T_now, face = 0.0, -1
        while True:
            iterations += 1
            inside = all(lo[a] <= c[a] < hi[a] for a in range(3))
            steppers = [a for a in range(3) if s[a] != 0]
            if inside:
                l = [c[a] - lo[a] for a in range(3)]
                if solid[l[2], l[1], l[0]]:
                    hits.append(c + [face])
                    with np.errstate(over="ignore"):
                        ts.append(F(T_now))
                    break
                size = next((B for B in blocks if empty[B][l[2] // B, l[1] // B, l[0] // B]), 1)
                # the planes through which the ray leaves the empty block (a single cell if size is 1)
                leave = {a: lo[a] + (l[a] // size + (1 if s[a] > 0 else 0)) * size for a in steppers}
                if not steppers:
                    E = None
                else:
                    E = min(T_of(a, leave[a]) for a in steppers)
                    limit = leave
            else:
                if any((s[a] > 0 and c[a] >= hi[a]) or (s[a] < 0 and c[a] < lo[a]) or (s[a] == 0 and not lo[a] <= c[a] < hi[a]) for a in range(3)):
                    E = None
                else:
                    still_out = [a for a in steppers if not lo[a] <= c[a] < hi[a]]
                    enter = {a: (lo[a] if s[a] > 0 else hi[a]) for a in still_out}
                    E = max(T_of(a, enter[a]) for a in still_out)
                    limit = {a: (hi[a] if s[a] > 0 else lo[a]) for a in steppers}
                    # an axis that leaves the box before E has left it for good
                    if any(T_of(a, limit[a]) < E for a in steppers if a != E[1]):
                        E = None
                    leave = enter
            if E is None or E[0] > tmax:
                hits.append([-1, -1, -1, -1])
                ts.append(F(np.inf))
                break
            aE = E[1]
            for b in steppers:
                if b == aE:
                    continue
                # the first plane j of b, from n[b] on and not past limit[b], with T_of(b, j) > E
                guess = math.floor(min(max(o[b] + E[0] * d[b], -2.0 ** 40), 2.0 ** 40)) + (1 if s[b] > 0 else 0)
                j = min(max(guess, n[b]), limit[b]) if s[b] > 0 else max(min(guess, n[b]), limit[b])
                while j != limit[b] and T_of(b, j) < E:
                    j += s[b]
                while j != n[b] and not T_of(b, j - s[b]) < E:
                    j -= s[b]
                n[b] = j
                c[b] = j - 1 if s[b] > 0 else j
            x = leave[aE]
            n[aE] = x + s[aE]
            c[aE] = x if s[aE] > 0 else x - 1
            T_now, face = E[0], 2 * aE + (0 if s[aE] > 0 else 1)
    return np.array(hits, np.int32).reshape(-1, 4), np.array(ts, F), iterations


@pytest.mark.parametrize("dims, origin, density, seed", [((70, 45, 37), (5, 0, 9), 0.003, 0), ((33, 64, 18), (0, 100, 0), 0.02, 1)])
def test_skipping_equals_the_fine_walk(dims, origin, density, seed):
    rng = np.random.default_rng(seed)
    solid = R.random_solid(rng, dims, density)
    o, d = R.ray_set(rng, solid, origin, 10000, far=24, limit=1)
    o2, d2 = R.extreme_rays(rng, solid, origin, 600)
    o3, d3 = family_rays(rng, solid, origin, 200)
    o, d = np.concatenate([o, o2, o3]), np.concatenate([d, d2, d3])
    assert len(o) >= 10000                       # (two grids: 20 000 rays and more)
    want = R.cast(solid, origin, o, d)
    got = skip_cast(solid, origin, o, d)
    bad = np.nonzero((got[0] != want[0]).any(axis=1) | (got[1].view(np.uint32) != want[1].view(np.uint32)))[0]
    assert len(bad) == 0, (len(bad), o[bad[:3]], d[bad[:3]], got[0][bad[:3]], want[0][bad[:3]])
    hits, misses = R.shares(want[0])
    print("rays", len(o), "hit", hits, "miss", misses, "fine steps", want[2], "skip iterations", got[2])
    assert hits >= 0.2 and misses >= 0.2 and got[2] * 20 < want[2]
    sub = rng.choice(len(o), 1500, replace=False)
    for t_max in (0.0, 3.0, 40.0):
        assert R.same(skip_cast(solid, origin, o[sub], d[sub], t_max)[:2], R.cast(solid, origin, o[sub], d[sub], t_max)[:2]), t_max


def test_formats_give_one_solid_set():
    rng = np.random.default_rng(3)
    solid = rng.random((5, 6, 70)) < 0.3
    assert np.array_equal(R.solid_bits(R.pack_bits(solid), 70), solid)
    assert R.pack_bits(solid).shape == (5, 6, 3) and R.pack_bits(solid).dtype == np.int32
    field = np.where(solid, F(-1), F(1))
    field[~solid & (rng.random(solid.shape) < 0.2)] = np.nan
    assert np.array_equal(R.solid_f32(field, 0.0), solid) and np.array_equal(R.solid_u8(solid.astype(np.uint8) * 2), solid)


# ---- the kernel's own walk, compiled for the host ---------------------------------------------------------------------------------

HOST_WALK = r"""
#include <algorithm>
#include <cmath>
#include <cstdint>
#define __device__
#define __forceinline__ inline
using std::max;
using std::min;
%s
extern "C" void cast_host(const float *origins, const float *directions, uint64_t n, float t_max, const RayGrid *g, int skip, int32_t *hit,
                          float *t_out)
{
    for (uint64_t i = 0; i < n; ++i) {
        Ray r;
        for (int b = 0; b < 3; ++b) {
            r.o[b] = (double) origins[i * 3 + b];
            r.d[b] = (double) directions[i * 3 + b];
            r.s[b] = r.d[b] > 0.0 ? 1 : r.d[b] < 0.0 ? -1 : 0;
            r.inv[b] = r.s[b] != 0 ? 1.0 / r.d[b] : 0.0;
            r.c[b] = (int32_t) floor(r.o[b]);
            r.nxt[b] = r.c[b] + (r.s[b] > 0 ? 1 : 0);
        }
        r.T = 0.0;
        r.face = -1;
        const bool found = skip ? ray_walk<true>(r, (double) t_max, *g) : ray_walk<false>(r, (double) t_max, *g);
        for (int b = 0; b < 3; ++b) hit[i * 4 + b] = found ? r.c[b] : -1;
        hit[i * 4 + 3] = found ? r.face : -1;
        t_out[i] = found ? (float) r.T : __builtin_inff();
    }
}
"""


class _RayGrid(hip.C.Structure):
    _fields_ = [("org", hip.C.c_int32 * 3), ("dim", hip.C.c_int32 * 3), ("b0", hip.C.c_uint32 * 3), ("b1", hip.C.c_uint32 * 3),
                ("b2", hip.C.c_uint32 * 3), ("m0", hip.C.c_void_p), ("m1", hip.C.c_void_p), ("m2", hip.C.c_void_p)]


def snapshot_words(solid):
    """The three levels of words of include/o2v_hip.h, [z][y][x] each, by numpy."""
    levels, cur = [], solid
    for _ in range(3):
        pz, py, px = [-(-n // 4) * 4 for n in cur.shape]
        pad = np.zeros((pz, py, px), bool)
        pad[:cur.shape[0], :cur.shape[1], :cur.shape[2]] = cur
        bits = pad.reshape(pz // 4, 4, py // 4, 4, px // 4, 4).transpose(0, 2, 4, 1, 3, 5).reshape(pz // 4, py // 4, px // 4, 64)
        levels.append(np.ascontiguousarray((bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=3, dtype=np.uint64)))
        cur = levels[-1] != 0
    return levels


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    """build(changes) -> cast(solid, origin, o, d, t_max, skip): the walk of o2v_dev_k11_raycast.hpp (its declarations and the
    part from "the walk" to "the cast kernel") compiled for the host, with `changes` (text, replacement) applied first."""
    import shutil
    import subprocess
    from tests.test_host_dense import HIPCC, SRC
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    text = open(os.path.join(SRC, "o2v_dev_k11_raycast.hpp")).read()
    parts = text[text.index("constexpr uint32_t kRayU8"):text.index("// ---- build")] + text[text.index("// ---- the walk"):text.index("// ---- the cast kernel")]
    tmp = tmp_path_factory.mktemp("host_walk")

    def build(changes=()):
        src = parts
        for old, new in changes:
            assert src.count(old) == 1, old
            src = src.replace(old, new)
        name = "walk_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_WALK % src)
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(tmp / (name + ".cpp")), "-o",
                        str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = hip.C.CDLL(str(tmp / (name + ".so")))

        def cast(solid, origin, o, d, t_max=INF, skip=True):
            C = hip.C
            words = snapshot_words(solid)
            g = _RayGrid()
            for a in range(3):
                g.org[a], g.dim[a] = origin[a], solid.shape[2 - a]
                g.b0[a], g.b1[a], g.b2[a] = (w.shape[2 - a] for w in words)
            g.m0, g.m1, g.m2 = (w.ctypes.data for w in words)
            valid = R.setup(o, d)[0]                   # (invalid rays never reach the walk)
            o, d = np.ascontiguousarray(o[valid], F), np.ascontiguousarray(d[valid], F)
            hit, t = np.full((len(valid), 4), -1, np.int32), np.full(len(valid), np.nan, F)
            hit[~valid, 3] = -2
            h, tt = np.empty((len(o), 4), np.int32), np.empty(len(o), F)
            L.cast_host(C.c_void_p(o.ctypes.data), C.c_void_p(d.ctypes.data), C.c_uint64(len(o)), C.c_float(t_max), C.byref(g), int(skip),
                        C.c_void_p(h.ctypes.data), C.c_void_p(tt.ctypes.data))
            hit[valid], t[valid] = h, tt
            return hit, t
        return cast
    return build


WALK_GRIDS = [((70, 45, 37), (5, 0, 9), 0.003), ((130, 70, 67), (65536 - 130, 0, 65536 - 67), 0.0015), ((5, 22, 45), (0, 3, 0), 0.03),
              ((1, 1, 1), (3, 3, 3), 1.0), ((200, 150, 90), (17, 0, 40), 0.0004), ((40, 40, 40), (0, 0, 0), 0.5)]


def walk_rays(seed, dims, origin, density):
    rng = np.random.default_rng(seed)
    solid = R.random_solid(rng, dims, density)
    o, d = R.ray_set(rng, solid, origin, 8000, far=16, limit=0)
    o2, d2 = R.extreme_rays(rng, solid, origin, 2000)
    return solid, np.concatenate([o, o2]), np.concatenate([d, d2])


@pytest.mark.parametrize("dims, origin, density", WALK_GRIDS)
def test_the_kernels_walk_on_the_host_equals_the_reference(host_walk, dims, origin, density):
    cast = host_walk()
    solid, o, d = walk_rays(21, dims, origin, density)
    for t_max in (INF, 0.0, 7.5):
        want = R.cast(solid, origin, o, d, t_max)[:2]
        for skip in (True, False):
            got = cast(solid, origin, o, d, t_max, skip)
            bad = np.nonzero((got[0] != want[0]).any(axis=1) | (got[1].view(np.uint32) != want[1].view(np.uint32)))[0]
            assert len(bad) == 0, (t_max, skip, len(bad), o[bad[:3]], d[bad[:3]], got[0][bad[:3]], want[0][bad[:3]])


@pytest.mark.parametrize("rule", ["kRayTieLowestAxis", "kRayFixUp"])
def test_a_changed_rule_is_caught(host_walk, rule):
    """DESIGN.md section 14, mutations: the tie rule turned to the highest axis; the correction after a skip left out."""
    cast = host_walk([(f"constexpr bool {rule} = true", f"constexpr bool {rule} = false")])
    dims, origin, density = WALK_GRIDS[0]
    solid, o, d = walk_rays(21, dims, origin, density)
    want = R.cast(solid, origin, o, d)[:2]
    assert not R.same(cast(solid, origin, o, d, INF, True), want)
    if rule == "kRayFixUp":      # (the fine walk never uses the estimate)
        assert R.same(cast(solid, origin, o, d, INF, False), want)


# ---- dense.RayCaster, cast and raycast against a stub ----------------------------------------------------------------------------

class RayStub(StubVoxelizer):
    """raycast_build counts generations as the context does; raycast fills the two arrays (the stub's "device" is the host)."""

    def __init__(self):
        super().__init__()
        self.generation = 0

    def raycast_build(self, grid_ptr, fmt, strides, dims, level=0.0, origin=(0, 0, 0)):
        self.generation += 1
        self.calls.append(("build", grid_ptr, fmt, tuple(strides), tuple(dims), level, tuple(origin)))
        return self.generation

    def raycast_generation(self):
        return self.generation

    def raycast(self, origins_ptr, directions_ptr, n, t_max, hit_ptr, t_ptr):
        self.calls.append(("cast", origins_ptr, directions_ptr, n, t_max))
        C = hip.C
        np.ctypeslib.as_array(C.cast(hit_ptr, C.POINTER(C.c_int32)), (n * 4,))[:] = np.arange(n * 4)
        np.ctypeslib.as_array(C.cast(t_ptr, C.POINTER(C.c_float)), (n,))[:] = np.arange(n) * 0.5


@pytest.mark.parametrize("dtype, fmt, level", [(torch.bool, hip.RAY_GRID_U8, None), (torch.uint8, hip.RAY_GRID_U8, None),
                                               (torch.int32, hip.RAY_GRID_BITS, None), (torch.float32, hip.RAY_GRID_F32_BELOW, 0.1)])
def test_raycaster_formats_and_strides(dtype, fmt, level):
    dv = RayStub()
    grid = torch.zeros((6, 7, 8), dtype=dtype)
    dense.RayCaster(dv, grid, level=level, origin=(1, 2, 3))
    nx = 8 * 32 if fmt == hip.RAY_GRID_BITS else 8
    assert dv.calls == [("build", grid.data_ptr(), fmt, (1, 8, 56), (nx, 7, 6), 0.0 if level is None else float(F(level)), (1, 2, 3))]
    # a slice of a batch seen with other axes: the strides go through as they are
    if fmt != hip.RAY_GRID_BITS:
        batch = torch.zeros((2, 6, 7, 5), dtype=dtype)
        view = batch[1].permute(1, 0, 2)[:, ::2]      # [z = 7, y = 3, x = 5]
        dense.RayCaster(dv, view, level=level)
        assert dv.calls[-1][1:5] == (batch[1].data_ptr(), fmt, (1, 70, 5), (5, 3, 7)) and dv.calls[-1][6] == (0, 0, 0)
        flat = torch.zeros((1, 7, 5), dtype=dtype).expand(9, -1, -1)
        dense.RayCaster(dv, flat, level=level)
        assert dv.calls[-1][3] == (1, 5, 0)


def test_cast_shapes_and_outputs():
    dv = RayStub()
    caster = dense.RayCaster(dv, torch.zeros((4, 4, 4), dtype=torch.bool))
    for shape in ((5, 3), (2, 3, 3), (3,), (0, 3), (4, 1, 2, 3)):
        o, d = torch.zeros(shape), torch.ones(shape)
        before = len(dv.calls)
        hit, t = caster.cast(o, d, 2.5)
        assert hit.dtype == torch.int32 and tuple(hit.shape) == shape[:-1] + (4,) and t.dtype == torch.float32 and tuple(t.shape) == shape[:-1]
        n = int(np.prod(shape[:-1]))
        if n:
            assert dv.calls[-1][0] == "cast" and dv.calls[-1][3:] == (n, 2.5)
            assert hit.reshape(-1).tolist() == list(range(4 * n)) and t.reshape(-1).tolist() == [0.5 * i for i in range(n)]
        else:
            assert len(dv.calls) == before         # (nothing is launched for no rays)
    # rays that are not contiguous are cast from a contiguous copy; t_max defaults to inf
    o = torch.zeros((3, 6))[:, ::2]
    caster.cast(o, torch.ones((3, 3)))
    assert dv.calls[-1][1] != o.data_ptr() and dv.calls[-1][4] == INF
    hit, t = dense.raycast(dv, torch.zeros((4, 4, 4)), torch.zeros((2, 3)), torch.ones((2, 3)), level=0.5, t_max=7.0, origin=(1, 1, 1))
    assert dv.calls[-2][0] == "build" and dv.calls[-2][5:] == (0.5, (1, 1, 1)) and dv.calls[-1][3:] == (2, 7.0) and tuple(hit.shape) == (2, 4)


def test_a_replaced_raycaster_raises():
    dv = RayStub()
    first = dense.RayCaster(dv, torch.zeros((4, 4, 4), dtype=torch.uint8))
    first.cast(torch.zeros((1, 3)), torch.ones((1, 3)))
    second = dense.RayCaster(dv, torch.ones((4, 4, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="replaced"):
        first.cast(torch.zeros((1, 3)), torch.ones((1, 3)))
    second.cast(torch.zeros((1, 3)), torch.ones((1, 3)))
    # a build that failed replaces the snapshot too
    dv.generation += 1
    with pytest.raises(RuntimeError, match="replaced"):
        second.cast(torch.zeros((1, 3)), torch.ones((1, 3)))


@pytest.mark.parametrize("kw, exc", [
    (dict(grid=torch.zeros((4, 4, 4), dtype=torch.float64)), TypeError), (dict(grid=torch.zeros((4, 4, 4), dtype=torch.int64)), TypeError),
    (dict(grid=torch.zeros((4, 4))), ValueError), (dict(grid=np.zeros((4, 4, 4), np.uint8)), ValueError),
    (dict(grid=torch.zeros((4, 4, 4))), ValueError),                                  # float32 without a level
    (dict(grid=torch.zeros((4, 4, 4)), level=float("nan")), ValueError), (dict(grid=torch.zeros((4, 4, 4)), level=float("inf")), ValueError),
    (dict(grid=torch.zeros((4, 4, 4)), level=1e39), ValueError), (dict(grid=torch.zeros((4, 4, 4)), level="0"), ValueError),
    (dict(grid=torch.zeros((4, 4, 4)), level=True), ValueError),
    (dict(grid=torch.zeros((4, 4, 4), dtype=torch.bool), level=0.0), ValueError),     # a level with another dtype
    (dict(grid=torch.zeros((4, 4, 4), dtype=torch.int32), level=0.0), ValueError),
    (dict(grid=torch.zeros((4, 4, 8), dtype=torch.int32)[:, :, ::2]), ValueError),    # bits need unit stride along x
    (dict(grid=torch.zeros((4, 0, 4), dtype=torch.uint8)), ValueError),
    (dict(grid=torch.zeros((4, 4, 4), dtype=torch.uint8, device="meta")), ValueError),
    (dict(origin=(0, 0)), ValueError), (dict(origin=(0, -1, 0)), ValueError), (dict(origin=(65533, 0, 0)), ValueError),
    (dict(grid=torch.zeros((1, 1, 4), dtype=torch.int32), origin=(65536 - 127, 0, 0)), ValueError),
])
def test_raycaster_rejects(kw, exc):
    dv = RayStub()
    args = dict(grid=torch.zeros((4, 4, 4), dtype=torch.uint8))
    args.update(kw)
    with pytest.raises(exc):
        dense.RayCaster(dv, args.pop("grid"), **args)
    assert not dv.calls


def test_raycaster_accepts_the_last_origin():
    dv = RayStub()
    dense.RayCaster(dv, torch.zeros((4, 4, 4), dtype=torch.uint8), origin=(65532, 0, 65532))
    dense.RayCaster(dv, torch.zeros((1, 1, 4), dtype=torch.int32), origin=(65536 - 128, 0, 0))
    assert dv.calls[0][6] == (65532, 0, 65532) and dv.calls[1][4] == (128, 1, 1)


@pytest.mark.parametrize("kw, exc", [
    (dict(origins=torch.zeros((2, 3), dtype=torch.float64)), TypeError), (dict(directions=torch.zeros((2, 3), dtype=torch.int32)), TypeError),
    (dict(origins=np.zeros((2, 3), F)), TypeError), (dict(origins=torch.zeros((2, 4)), directions=torch.zeros((2, 4))), ValueError),
    (dict(origins=torch.zeros(())), ValueError), (dict(origins=torch.zeros((3, 3))), ValueError),
    (dict(directions=torch.zeros((2, 3), device="meta")), ValueError),
    (dict(t_max=-1.0), ValueError), (dict(t_max=float("nan")), ValueError), (dict(t_max="1"), ValueError), (dict(t_max=True), ValueError),
])
def test_cast_rejects(kw, exc):
    dv = RayStub()
    caster = dense.RayCaster(dv, torch.zeros((4, 4, 4), dtype=torch.uint8))
    args = dict(origins=torch.zeros((2, 3)), directions=torch.ones((2, 3)), t_max=INF)
    args.update(kw)
    with pytest.raises(exc):
        caster.cast(args["origins"], args["directions"], args["t_max"])
    assert [c[0] for c in dv.calls] == ["build"]


def test_refused_when_the_library_came_first(monkeypatch):
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: False)
    with pytest.raises(RuntimeError, match="before torch"):
        dense.RayCaster(RayStub(), torch.zeros((4, 4, 4), dtype=torch.uint8))


# ---- camera_rays -----------------------------------------------------------------------------------------------------------------

def test_camera_rays():
    eye, target = (10.0, -20.0, 30.0), (40.0, 50.0, 60.0)
    o, d = dense.camera_rays(7, 5, eye, target, (0, 0, 1), 40.0, torch.device("cpu"))
    assert o.dtype == torch.float32 and d.dtype == torch.float32 and tuple(o.shape) == (5, 7, 3) and tuple(d.shape) == (5, 7, 3)
    assert o.is_contiguous() and d.is_contiguous() and bool((o == torch.tensor(eye)).all())
    forward = np.array(target) - np.array(eye)
    forward /= np.linalg.norm(forward)
    dn = d.numpy().astype(np.float64)
    assert np.allclose(np.linalg.norm(dn, axis=2), 1.0, atol=1e-6)
    assert np.allclose(dn[2, 3], forward, atol=1e-6)            # an odd image: the centre pixel's ray points at the target
    # the corner rays are symmetric about the axis: equal angles to it, and their sum points along it
    corners = dn[[0, 0, 4, 4], [0, 6, 0, 6]]
    assert np.allclose(corners @ forward, (corners @ forward)[0], atol=1e-6)
    total = corners.sum(axis=0)
    assert np.allclose(total / np.linalg.norm(total), forward, atol=1e-6)
    # the vertical field of view: the top and bottom edges of the image are fov / 2 from the axis
    o2, d2 = dense.camera_rays(1, 1000, eye, target, (0, 0, 1), 40.0, torch.device("cpu"))
    top = math.degrees(math.acos(float(d2[0, 0].numpy().astype(np.float64) @ forward)))
    assert abs(top - 20.0) < 0.05 and d2[0, 0, 2] > d2[-1, 0, 2]                     # row 0 is the top
    for bad in (dict(width=0), dict(fov_y_degrees=180.0), dict(target=eye), dict(up=tuple(forward))):
        kw = dict(width=4, height=4, eye=eye, target=target, up=(0, 0, 1), fov_y_degrees=40.0, device=torch.device("cpu"))
        kw.update(bad)
        with pytest.raises(ValueError):
            dense.camera_rays(**kw)


# ---- the code object and the scratch formula -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["k_ray_buildILj0ELb0E", "k_ray_buildILj0ELb1E", "k_ray_buildILj1ELb0E", "k_ray_buildILj2ELb0E",
                                    "k_ray_buildILj2ELb1E", "k_ray_build_topE", "k_ray_castILb0E", "k_ray_castILb1E"])
def test_k11_kernels_in_the_code_object_without_scratch(device_asm, kernel):  # noqa: F811
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    body = m.group(2)
    scratch = re.findall(r"; ScratchSize: (\d+)", device_asm[m.end():m.end() + 4000])
    assert scratch and scratch[0] == "0", scratch[:1]
    assert "scratch_" not in body and "buffer_store_dword v" not in body.replace("buffer_store_dwordx", "")
    assert re.search(r"^\s*\.set " + re.escape(m.group(1)) + r"\.private_seg_size, 0$", device_asm, re.M)
    spills = re.search(r"^\s*\.set " + re.escape(m.group(1)) + r"\.num_vgpr, (\d+)$", device_asm, re.M)
    assert spills and int(spills.group(1)) <= 128 and "v_accvgpr_write" not in body      # (no spill, to memory or to AGPRs)
    atomics = re.findall(r"^\s*(\S*atomic\S*)", body, re.M)
    if "k_ray_buildI" in kernel:
        assert atomics and set(atomics) == {"global_atomic_or_x2"}, atomics           # the vector atomicOr into the 16^3 words only
    else:
        assert not atomics, atomics
    if kernel in ("k_ray_buildILj0ELb1E", "k_ray_buildILj2ELb1E"):
        assert "global_load_dwordx4" in body                                          # 16-byte loads where the x stride is 1


@pytest.mark.parametrize("dims", [(1, 1, 1), (4, 4, 4), (5, 4, 4), (64, 64, 64), (65, 3, 130), (1024, 1024, 1024), (65536, 1, 7), (1000, 999, 17)])
def test_scratch_bytes_formula(dims):
    def blocks(k):
        return math.prod(-(-n // k) for n in dims)
    assert hip.raycast_scratch_bytes(dims) == 8 * (blocks(4) + blocks(16) + blocks(64))
    assert hip.DeviceVoxelizer.raycast_scratch_bytes(None, dims) == hip.raycast_scratch_bytes(dims)


def test_scratch_bytes_of_zero_dims():
    assert hip.raycast_scratch_bytes((4, 0, 4)) == 0
    # about 1/8 byte per voxel and 2 % more
    assert hip.raycast_scratch_bytes((1024, 1024, 1024)) == 2 ** 27 + 2 ** 21 + 2 ** 15
