"""The definition of o2v_hip_octree_raycast / o2v_hip_octree_dag_raycast (include/o2v_hip.h), restated with
what the other references already define and nothing else:

  the solid set   octree_ref.to_dense / dag_ref.to_dense of the arrays - the descent, voxel by voxel - over the root cube
                  [0, 2^D)^3 or, for a tree of a grid, over the grid's box (the tree is empty outside it);
  the walk        raycast_ref.cast on that dense set: the fine walk of o2v_hip_raycast, cell by cell, nothing skipped;
  the slot        column 3 of octree_ref.lookup / dag_ref.lookup at the hit cell, -1 where nothing is hit.

So cast(arrays) is, by construction, RayCaster(to_dense(arrays)).cast, whatever the arrays hold.  Comparison is raycast_ref.same
(hit as int32, t as float32 bits) plus integer equality of the slot.  The grids and the arrays that are no tree, which
tests/test_host_treeray.py and tests/treeray_cases.py share, are at the end.

Arrays are the dicts of tests/octree_ref.py (a tree) and tests/dag_ref.py (a DAG: it has "child"); grids are [z, y, x]."""
import functools
import os

import numpy as np

from tests import dag_ref as G
from tests import octree_ref as R
from tests import raycast_ref as C

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def is_dag(arrays):
    return "child" in arrays


def solid_set(arrays, box=None):
    """(solid bool [nz, ny, nx], origin (x, y, z)): the descent's `solid` over box = (shape, origin), by default the root cube"""
    shape, origin = ((2 ** arrays["depth"],) * 3, (0, 0, 0)) if box is None else box
    return (G if is_dag(arrays) else R).to_dense(arrays, tuple(shape), tuple(origin)), tuple(origin)


def slots(arrays, hit, skips=True):
    """int32 [n]: column 3 of the lookup at the hit cells, -1 where hit holds none"""
    hit = np.asarray(hit, np.int32).reshape(-1, 4)
    out = np.full(len(hit), -1, np.int64)
    rows = hit[:, 0] >= 0
    if rows.any():
        cells = hit[rows, :3].astype(np.int64)
        found = G.lookup(arrays, cells, skips=skips) if is_dag(arrays) else np.array([R.lookup_one(arrays, *(int(v) for v in c)) for c in cells], np.int64).reshape(-1, 4)
        assert (found[:, 0] == 1).all(), "a hit cell is not solid by the descent"
        out[rows] = found[:, 3]
    return (out & 0xffffffff).astype(np.uint32).view(np.int32)


def cast(arrays, origins, directions, t_max=np.inf, solid=None, skips=True):
    """(hit int32 [n, 4], t float32 [n], slot int32 [n]); solid: what solid_set returned (it is the slow part: make it once)"""
    grid, origin = solid_set(arrays) if solid is None else solid
    hit, t, _ = C.cast(grid, origin, origins, directions, t_max)
    return hit, t, slots(arrays, hit, skips)


def same(got, want):
    """hit, t and - where both have one - the slot, bit for bit"""
    return C.same(got[:2], want[:2]) and (len(got) < 3 or len(want) < 3 or np.array_equal(np.asarray(got[2], np.int32), np.asarray(want[2], np.int32)))


def first_difference(got, want, origins, directions):
    """what a failing comparison prints: the number of rays that differ and the first three of them"""
    bad = (np.asarray(got[0]) != np.asarray(want[0])).any(axis=1) | (np.asarray(got[1], C.F).view(np.uint32) != np.asarray(want[1], C.F).view(np.uint32))
    if len(got) > 2 and len(want) > 2:
        bad |= np.asarray(got[2]) != np.asarray(want[2])
    rows = np.nonzero(bad)[0][:3]
    return int(bad.sum()), [(origins[i].tolist(), directions[i].tolist(), [np.asarray(g)[i].tolist() for g in got], [np.asarray(w)[i].tolist() for w in want]) for i in rows]


# ---- the grids and the arrays of the tests ------------------------------------------------------------------------------------------

def ball(n, r):
    z, y, x = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    c = (n - 1) / 2
    return (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2 <= r * r


def grids():
    """[(name, grid [z, y, x], origin, depth or None, exempt)]: the grids of the case `shapes`.  exempt: the share of hits or of
    misses is 0 by construction."""
    rng = np.random.default_rng(350)
    one = np.zeros((64, 64, 64), bool)
    one[37, 10, 21] = True
    return [
        ("ball 13.3 in 32^3", ball(32, 13.3), (1, 3, 5), None, False),
        ("one voxel in 64^3", one, (0, 0, 0), None, False),
        ("checkerboard 16", R.checkerboard(16), (16, 0, 32), None, False),
        ("box 7x5x3", R.box((7, 5, 3)), (1, 3, 5), None, False),
        ("random 0.03", C.random_solid(rng, (40, 33, 21), 0.03), (3, 0, 9), None, False),
        ("random 0.3", C.random_solid(rng, (40, 33, 21), 0.3), (3, 0, 9), None, False),
        ("shell 18 - 15 in 40^3", ball(40, 18) & ~ball(40, 15), (0, 0, 0), None, False),
        ("empty 4^3", np.zeros((4, 4, 4), bool), (0, 0, 0), None, True),
        ("solid 16^3", np.ones((16, 16, 16), bool), (0, 0, 0), None, True),
        ("depth 1", np.array([[[1, 0], [0, 1]], [[0, 0], [1, 0]]], bool), (0, 0, 0), 1, False),
        ("depth 2", rng.random((4, 4, 4)) < 0.3, (0, 0, 0), 2, False),
        ("8^3 at 65528, depth 16", rng.random((8, 8, 8)) < 0.3, (65528, 65528, 65528), 16, False),
        ("two levels deeper", R.blobs(rng, (12, 9, 10), 0.5, noise=0.1), (2, 1, 0), 6, False),
    ]


def rays_of(rng, grid, origin, n=4000):
    """the ray set of a grid: raycast_ref.ray_set with 16 far rays and two from 2^22"""
    return C.ray_set(rng, grid, origin, n=n, far=16, limit=2)


SCENES_ENV = "O2V_TREERAY_SCENES"   # a directory: scene(k) keeps its result there, so that a child process need not walk again
T_MAX = (0.0, 3.5)                  # ... and a third: the t of one of the scene's own hits
N_SHORT = 1000                      # the rays cast with a finite t_max


def _scene_path(k):
    return os.path.join(os.environ[SCENES_ENV], "scene_%d.npz" % k) if os.environ.get(SCENES_ENV) else None


@functools.lru_cache(None)
def _scene(k):
    name, g, origin, depth, exempt = grids()[k]
    rng = np.random.default_rng(3500 + k)
    o, d = rays_of(rng, g, origin)
    extra = C.extreme_rays(rng, g, origin, 500)
    o, d = np.concatenate([o, extra[0]]), np.concatenate([d, extra[1]])
    path = _scene_path(k)
    if path and os.path.exists(path):
        z = np.load(path)
        hit, t, t_maxs, short_hit, short_t = (z[key] for key in ("hit", "t", "t_maxs", "short_hit", "short_t"))
        assert len(hit) == len(o)
    else:
        hit, t, _ = C.cast(g, origin, o, d)
        own = t[np.isfinite(t) & (t > 0)]
        t_maxs = np.array(T_MAX + ((float(own[0]),) if len(own) else (1.0,)), np.float64)
        short = [C.cast(g, origin, o[:N_SHORT], d[:N_SHORT], float(t_max))[:2] for t_max in t_maxs]
        short_hit, short_t = np.stack([s[0] for s in short]), np.stack([s[1] for s in short])
    share = C.shares(hit)
    assert exempt or min(share) >= 0.25, (name, share)
    return name, g, origin, depth, o, d, (hit, t), t_maxs, short_hit, short_t


def scene(k):
    """(name, grid, origin, depth, origins, directions, (hit, t), {t_max: (hit, t) of the first N_SHORT rays}) of grid k of grids():
    its 4 000 rays and 500 extreme ones, and the reference's walk over the grid's box - the slow part, made once per process and,
    where SCENES_ENV names a directory, once for all processes.  At least a quarter of the rays hit and a quarter miss, which is
    asserted here, before anything looks at a device (but where one of the shares is 0 by construction)."""
    name, g, origin, depth, o, d, want, t_maxs, short_hit, short_t = _scene(k)
    path = _scene_path(k)
    if path and not os.path.exists(path):
        tmp = path + ".%d.tmp.npz" % os.getpid()
        np.savez(tmp, hit=want[0], t=want[1], t_maxs=t_maxs, short_hit=short_hit, short_t=short_t)
        os.replace(tmp, path)
    return name, g, origin, depth, o, d, want, {float(t_max): (short_hit[i], short_t[i]) for i, t_max in enumerate(t_maxs)}


def sources(grid, origin, depth):
    """[(name, arrays)]: the grid as tree and DAG, collapsed and not"""
    out = []
    for collapse in (True, False):
        t = R.build(grid, origin, depth, collapse)
        out += [("tree" + ", collapsed" * collapse, t), ("DAG" + ", collapsed" * collapse, G.build(t))]
    return out


def broken_grid():
    """the 16^3 grid whose tree and DAG not_a_tree() breaks"""
    return R.blobs(np.random.default_rng(351), (16, 16, 16), 0.5, noise=0.1)


def broken_rays(k, solid):
    """the rays of case k of not_a_tree(), solid = solid_set(arrays): 1 500 and four far ones"""
    return C.ray_set(np.random.default_rng(3600 + k), solid[0], solid[1], n=1500, far=4, limit=0)


def not_a_tree():
    """[(name, arrays)]: arrays that are no tree - first_child of -2, INT32_MIN, n_nodes and INT32_MAX, child of -1, M and 0 (a cycle
    through the root), a child in the wrong level - made of the tree and the DAG of one 16^3 grid, collapsed and not.  The values
    sit in the two top levels, so that whole cells of side 8 and 4 turn empty, or turn into something else."""
    g = broken_grid()
    out = []
    for collapse in (True, False):
        tag = ", collapsed" * collapse
        t = R.build(g, (0, 0, 0), None, collapse)
        N = len(t["valid"])
        top = t["level_counts"][0] + t["level_counts"][1]
        leaves = N - t["level_counts"][-1]   # the first node of level D - 1
        for bad in (-2, INT32_MIN, N, INT32_MAX):
            for rows in (slice(0, 1), slice(1, top, 2)):   # the root; every other node of level 1
                fc = t["first_child"].copy()
                fc[rows] = bad
                out.append(("tree%s, first_child[%s:%s:%s] = %d" % (tag, rows.start, rows.stop, rows.step, bad), dict(t, first_child=fc)))
        fc = t["first_child"].copy()
        fc[1:top:2] = leaves          # level 1 -> level D - 1: a child in the wrong level
        out.append(("tree%s, children two levels down" % tag, dict(t, first_child=fc)))
        fc = t["first_child"].copy()
        fc[1:top] = 0                 # level 1 -> the root and what follows it: a cycle
        out.append(("tree%s, children are the root" % tag, dict(t, first_child=fc)))
        d = G.build(t)
        M, P = len(d["valid"]), len(d["child"])
        first = int(d["first_child"][d["level_counts"][0] + d["level_counts"][1]])   # the pointers of levels 0 and 1
        for bad in (-1, M, 0, M - 1):   # -1, past the end, the root (a cycle), a node of level D - 1 (the wrong level)
            for rows in (slice(0, first, 3), slice(0, 8)):
                ch = d["child"].copy()
                ch[rows] = bad
                out.append(("DAG%s, child[%s:%s:%s] = %d" % (tag, rows.start, rows.stop, rows.step, bad), dict(d, child=ch)))
        for bad in (-2, INT32_MIN, P, INT32_MAX):
            fc = d["first_child"].copy()
            fc[1:1 + d["level_counts"][1]:2] = bad
            out.append(("DAG%s, first_child of level 1 = %d" % (tag, bad), dict(d, first_child=fc)))
    return out
