"""The GPU cases of tests/test_gpu_dag.py, each run in a child process of its own: `python -m tests.dag_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison is bit for bit - valid, full,
first_child, child, skip and the level counts - against the numpy reference of tests/dag_ref.py on the tree of tests/octree_ref.py,
or against closed forms, never against the code under test, and there is no tolerance anywhere.  The output arrays are filled with
a guard value before every call at the C level.  A case prints what it covered and "ok" last when everything held."""
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import dag_ref as G
from tests import octree_ref as R
from tests.octree_cases import box_points, dev, indexed, tree_of

DEV = torch.device("cuda", 0)
COLLAPSE = hip.OCT_COLLAPSE
GUARD = 0x5a


def build(dv, t):
    """o2v_hip_octree_dag_build + _write at the C level on the tree t (the reference's dict, uploaded) into guarded arrays; the DAG
    as the reference's dict."""
    tv, tf, tfc = dev(t["valid"]), dev(t["full"]), dev(t["first_child"])
    torch.cuda.synchronize()
    counts, M, P = dv.octree_dag_build(tv.data_ptr(), tf.data_ptr(), tfc.data_ptr(), len(t["valid"]), t["depth"], COLLAPSE * t["collapsed"], t["level_counts"])
    assert sum(counts) == M and len(counts) == t["depth"]
    valid, full = (torch.full((M + 3,), GUARD, dtype=torch.uint8, device=DEV) for _ in range(2))
    first = torch.full((M + 3,), -77, dtype=torch.int32, device=DEV)
    child, skip = (torch.full((P + 3,), -77, dtype=torch.int32, device=DEV) for _ in range(2))
    torch.cuda.synchronize()
    dv.octree_dag_write(valid.data_ptr(), full.data_ptr(), first.data_ptr(), child.data_ptr(), skip.data_ptr())
    valid, full, first, child, skip = (a.cpu().numpy() for a in (valid, full, first, child, skip))
    assert (valid[M:] == GUARD).all() and (full[M:] == GUARD).all() and (first[M:] == -77).all() and (child[P:] == -77).all() and (skip[P:] == -77).all()
    return dict(valid=valid[:M], full=full[:M], first_child=first[:M], child=child[:P], skip=skip[:P], level_counts=list(counts), depth=t["depth"],
                collapsed=t["collapsed"])


def as_ref(dag):
    offs = dag.level_offsets
    return dict(valid=dag.valid.cpu().numpy(), full=dag.full.cpu().numpy(), first_child=dag.first_child.cpu().numpy(), child=dag.child.cpu().numpy(),
                skip=None if dag.skip is None else dag.skip.cpu().numpy(), level_counts=[b - a for a, b in zip(offs, offs[1:])], depth=dag.depth,
                collapsed=dag.collapsed)


# ---- shapes and layouts -----------------------------------------------------------------------------------------------------------

def case_shapes_and_layouts():
    """The grid family of tests/octree_cases.py's case of this name; each grid goes through build_octree and then octree_dag."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(300)
    calls = grids = merged = 0
    for dims in ((1, 1, 1), (2, 2, 2), (5, 6, 7), (63, 2, 3), (64, 3, 2), (65, 5, 4), (129, 9, 10)):
        nx, ny, nz = dims
        contents = [("empty", np.zeros((nz, ny, nx), bool)), ("full", np.ones((nz, ny, nx), bool))]
        for p in (0.02, 0.5, 0.98):
            contents.append(("density %.2f" % p, R.blobs(rng, dims, p, noise=0.1) if p == 0.5 else rng.random((nz, ny, nx)) < p))
        for c in range(8):
            one = np.zeros((nz, ny, nx), bool)
            one[(nz - 1) * (c >> 2), (ny - 1) * ((c >> 1) & 1), (nx - 1) * (c & 1)] = True
            contents.append(("corner %d" % c, one))
        for origin in ((0, 0, 0), (1, 3, 5), (63, 7, 8)):
            D0 = R.depth_of(origin, dims)
            for name, g in contents:
                t = dev(g)
                combos = [(D0 + 2 * (grids & 1), bool(grids >> 1 & 1))] if name.startswith("corner") else [(D0, False), (D0, True), (D0 + 2, False), (D0 + 2, True)]
                for depth, collapse in combos:
                    ref_tree = R.build(g, origin, depth, collapse)
                    want = G.build(ref_tree)
                    tree = dense.build_octree(dv, t, origin=origin, depth=depth, collapse=collapse)
                    assert np.array_equal(tree.first_child.cpu().numpy(), ref_tree["first_child"])
                    dag = dense.octree_dag(dv, tree, skips=bool(calls % 3))
                    G.same(as_ref(dag), want, (dims, origin, name, depth, collapse))
                    assert (dag.tree_nodes, dag.voxels_listed, dag.skip is None) == (len(ref_tree["valid"]), ref_tree["voxels_listed"], not calls % 3)
                    if calls % 5 == 0:   # ... and at the C level, into guarded arrays
                        G.same(build(dv, ref_tree), want, (dims, origin, name, depth, collapse, "guarded"))
                    merged += len(ref_tree["valid"]) - len(want["valid"])
                    calls += 1
                grids += 1
    assert len(dv.octree_dag_times()) == 4 and all(v >= 0 for v in dv.octree_dag_times())
    print("shapes_and_layouts: compared", calls, "DAGs of", grids, "grids;", merged, "nodes merged away")


# ---- the table --------------------------------------------------------------------------------------------------------------------

def case_table():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(301)
    # random 128^3, not collapsed: 262 144 nodes at level 6 for the table of 256, 32 768 nearly distinct keys at level 5
    g = rng.random((128, 128, 128)) < 0.5
    k, j, i = np.meshgrid(*(np.arange(64),) * 3, indexing="ij")
    o = rng.integers(0, 8, (64, 64, 64))
    g[2 * k + (o >> 2), 2 * j + ((o >> 1) & 1), 2 * i + (o & 1)] = True   # (a voxel of every 2^3 block, in any octant: none is empty)
    t = R.build(g, collapse=False)
    want = G.build(t)
    assert t["level_counts"][-2:] == [32768, 262144] and want["level_counts"][:6] == [1, 8, 64, 512, 4096, 32768] and 250 <= want["level_counts"][6] <= 255
    assert len(np.unique(t["valid"][-262144:])) == want["level_counts"][6]
    G.same(build(dv, t), want, "random 128^3")
    print("table: random 128^3:", len(t["valid"]), "tree nodes, DAG level counts", want["level_counts"], "pointers", len(want["child"]))
    # all solid, not collapsed: every key of a level is equal - the contended path
    t = R.build(R.box((128, 128, 128)), collapse=False)
    got = build(dv, t)
    assert len(t["valid"]) == 299593 and got["level_counts"] == [1] * 7 and len(got["child"]) == 48
    assert got["child"].tolist() == [1 + r // 8 for r in range(48)] and got["skip"][:8].tolist() == [262144 * r for r in range(8)]
    G.same(got, G.build(t), "box 128^3")
    ms = dv.octree_dag_times()
    print("table: box 128^3, not collapsed: 299593 tree nodes -> level counts", got["level_counts"], "; merge of level 6 %.3f, above %.3f, output %.3f ms" % ms[:3])
    for collapse in (True, False):
        t = R.build(R.checkerboard(64), collapse=collapse)
        got = build(dv, t)
        assert got["level_counts"] == [1] * 6 and got["valid"].tolist() == [255] * 5 + [0x69] and len(got["child"]) == 40
        G.same(got, G.build(t), ("checkerboard", collapse))
        # a random 8^3 block tiled to 128^3: compared against the reference, no closed form
        t = R.build(np.tile(rng.random((8, 8, 8)) < (0.5 if collapse else 0.9), (16, 16, 16)), collapse=collapse)
        got = build(dv, t)
        G.same(got, G.build(t), ("tiled", collapse))
        print("table: a random 8^3 block tiled to 128^3,", "collapsed:" if collapse else "plain:", len(t["valid"]), "tree nodes -> level counts", got["level_counts"])
    for g, collapse, nodes, counts, pointers in ((R.ball(), True, 1417, [1, 8, 32, 104, 304, 94], 1384), (R.ball(), False, 5553, [1, 8, 32, 105, 305, 95], 2288),
                                                 (G.two_balls(), True, 2835, [1, 1, 8, 32, 104, 304, 94], 1386),
                                                 (G.two_balls(), False, 11107, [1, 1, 8, 32, 105, 305, 95], 2290)):
        t = R.build(g, collapse=collapse)
        got = build(dv, t)
        assert (len(t["valid"]), got["level_counts"], len(got["child"])) == (nodes, counts, pointers), (len(t["valid"]), got["level_counts"], len(got["child"]))
        G.same(got, G.build(t), ("balls", g.shape, collapse))
    print("table: the ball and two balls side by side: level counts", counts, "pointers", pointers)


# ---- queries ----------------------------------------------------------------------------------------------------------------------

def case_queries():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(302)
    g = R.blobs(rng, (11, 6, 5), 0.6)
    origin = (3, 1, 2)
    far = np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1], [16, 0, 0], [0, 16, 0], [0, 0, 16], [-2 ** 31, 5, 5], [5, 2 ** 31 - 1, 5], [65536, 65536, 65536]], np.int32)
    n_points = n_boxes = 0
    for collapse in (True, False):
        tree = dense.build_octree(dv, dev(g), origin=origin, collapse=collapse)
        dag = dense.octree_dag(dv, tree)
        want = G.build(R.build(g, origin, None, collapse))
        G.same(as_ref(dag), want, ("queries", collapse))
        pts = np.concatenate([box_points(-2, 18), far])
        got = dense.dag_lookup(dv, dag, dev(pts)).cpu().numpy()
        assert np.array_equal(got, G.lookup(want, pts)), collapse
        of_tree = dense.octree_lookup(dv, tree, dev(pts)).cpu().numpy()
        assert np.array_equal(got[:, [0, 1, 3]], of_tree[:, [0, 1, 3]]) and (got[-len(far):] == (0, -1, -1, -1)).all() and got[:, 0].sum() == g.sum()
        ok = of_tree[:, 2] >= 0
        assert np.array_equal(got[ok, 2], want["classes"][of_tree[ok, 2]])   # column 2: the class of the tree's node
        bare = dense.dag_lookup(dv, dense.octree_dag(dv, tree, skips=False), dev(pts)).cpu().numpy()
        assert np.array_equal(bare[:, :3], got[:, :3]) and (bare[:, 3] == -1).all()
        n_points += len(pts)
        # to_dense: the box itself; an odd origin and a box that sticks out of the cube, contiguous and strided
        assert np.array_equal(dense.dag_to_dense(dv, dag, g.shape, origin=origin).cpu().numpy(), g)
        shape = (12, 13, 21)
        of_tree = dense.octree_to_dense(dv, tree, shape, origin=(1, 0, 0))
        assert torch.equal(dense.dag_to_dense(dv, dag, shape, origin=(1, 0, 0)), of_tree) and int(of_tree.sum()) == g.sum()
        wide = torch.full((12, 26, 21 * 3 + 1), 9, dtype=torch.uint8, device=DEV)
        out = dense.dag_to_dense(dv, dag, shape, origin=(1, 0, 0), out=wide[:, ::2, 1::3])
        assert out.data_ptr() == wide[:, ::2, 1::3].data_ptr() and torch.equal(out != 0, of_tree)
        wide[:, ::2, 1::3] = 9
        assert bool((wide == 9).all())   # (nothing beside the voxels was written)
        swapped = torch.empty((21, 13, 12), dtype=torch.bool, device=DEV).permute(2, 1, 0)
        assert torch.equal(dense.dag_to_dense(dv, dag, shape, origin=(1, 0, 0), out=swapped), of_tree)
        assert not dense.dag_to_dense(dv, dag, (3, 4, 5), origin=(16, 0, 0)).any() and not dense.dag_to_dense(dv, dag, (2, 2, 2), origin=(2 ** 32 - 2, 7, 7)).any()
        n_boxes += 6
    # round trips: sizes that are no multiple of a block, odd origins, depths above the smallest
    for dims, o, extra in (((1, 1, 1), (0, 0, 0), 0), ((1, 1, 1), (1, 1, 1), 3), ((65, 5, 4), (63, 7, 8), 0), ((129, 9, 10), (1, 3, 5), 2), ((70, 50, 40), (0, 0, 0), 0)):
        for collapse in (True, False):
            g2 = R.blobs(rng, dims, 0.6, noise=0.05)
            tree = dense.build_octree(dv, dev(g2), origin=o, depth=R.depth_of(o, dims) + extra, collapse=collapse)
            dag = dense.octree_dag(dv, tree)
            assert np.array_equal(dense.dag_to_dense(dv, dag, g2.shape, origin=o).cpu().numpy(), g2), (dims, o, collapse)
            solid = dev(np.argwhere(g2)[:, ::-1].astype(np.int32) + np.array(o, np.int32))
            assert torch.equal(dense.dag_lookup(dv, dag, solid)[:, [0, 1, 3]], dense.octree_lookup(dv, tree, solid)[:, [0, 1, 3]])
            n_boxes += 1
    # a DAG from the reference's arrays, as one loaded from disk, and arrays that point outside themselves: the reference's rows, no fault
    g3 = R.blobs(rng, (32, 32, 32), 0.5, noise=0.1)
    pts = box_points(0, 32)
    ref = G.build(R.build(g3))
    offs = tuple(int(v) for v in np.concatenate([[0], np.cumsum(ref["level_counts"])]))
    loaded = dense.OctreeDag(valid=dev(ref["valid"]), full=dev(ref["full"]), first_child=dev(ref["first_child"]), child=dev(ref["child"]), skip=dev(ref["skip"]),
                             level_offsets=offs, depth=5, collapsed=True, voxels_listed=0, tree_nodes=0)
    assert np.array_equal(dense.dag_lookup(dv, loaded, dev(pts)).cpu().numpy()[::7], G.lookup(ref, pts[::7]))
    # a tree whose first_child points into the wrong level, but inside the arrays: refused, the outputs untouched
    t = R.build(g3, collapse=False)
    off = np.concatenate([[0], np.cumsum(t["level_counts"])])
    n_refused = 0
    for level, value in ((1, int(off[3])), (2, int(off[2])), (2, int(off[4])), (0, 0)):   # a level too deep, the node's own level, two too deep, the root itself
        broken = dict(t, first_child=t["first_child"].copy())
        broken["first_child"][off[level]] = value
        tree = tree_of(broken)
        C = hip.C
        counts, M, P = (C.c_uint64 * 16)(*([99] * 16)), C.c_uint64(99), C.c_uint64(99)
        torch.cuda.synchronize()
        rc = hip._bind().o2v_hip_octree_dag_build(dv._ctx, tree.valid.data_ptr(), tree.full.data_ptr(), tree.first_child.data_ptr(), len(t["valid"]), t["depth"], 0,
                                                  hip._level_counts(t["level_counts"]), counts, C.byref(M), C.byref(P))
        err = hip._bind().o2v_hip_last_error(dv._ctx).decode()
        assert rc == 3 and "o2v_hip_octree_dag_build" in err and "not a tree of these level counts" in err, (rc, err)
        assert list(counts) == [99] * 16 and M.value == P.value == 99
        assert np.array_equal(tree.first_child.cpu().numpy(), broken["first_child"])
        try:
            dense.octree_dag(dv, tree)
        except hip.DeviceError as e:
            assert "not a tree" in str(e)
            n_refused += 1
    assert n_refused == 4
    G.same(build(dv, t), G.build(t), "after the refusals")
    print("queries:", n_points, "points looked up against the scalar descent and the tree's,", n_boxes, "boxes expanded,", n_refused, "trees that are none refused")


# ---- determinism --------------------------------------------------------------------------------------------------------------------

def case_determinism():
    rng = np.random.default_rng(303)
    g = R.blobs(rng, (100, 90, 80), 0.5, noise=0.05)
    dv, other = hip.DeviceVoxelizer(0), hip.DeviceVoxelizer(0)
    n = 0
    for collapse in (False, True):
        t = R.build(g, (5, 6, 7), None, collapse)
        a = build(dv, t)
        for d in (dv, other, dv):
            G.same(build(d, t), a, ("again", collapse))
            n += 1
        G.same(a, G.build(t), "the reference")
    print("determinism:", n, "builds on two contexts gave equal bytes")


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------

def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, *indexed(meshes.scan_like()))
    labels, origin = dense.voxelize_dense(dv, 128, fmt="labels", fill=True)
    solid = labels != 0
    palette = [0] + [0xff000000 | (i * 0x010307 & 0xffffff) for i in range(1, 256)]
    tree = dense.build_octree(dv, labels, origin=origin, collapse=False)
    dag = dense.octree_dag(dv, tree)
    G.same(as_ref(dag), G.build(R.build(solid.cpu().numpy(), origin, None, False)), "scan_like at 128")
    # colours scattered by the tree's voxel_index, as in the README ...
    rec = dense.to_voxels(dv, labels, origin=origin, palette=palette)
    points = rec[:, :3].contiguous()
    slots = dense.octree_lookup(dv, tree, points)[:, 3].long()
    argb = torch.zeros(tree.voxels_listed, dtype=torch.int32, device=DEV).scatter_(0, slots, rec[:, 3])
    # ... and read back through the DAG's voxel_index for every record
    hit = dense.dag_lookup(dv, dag, points)
    assert tree.voxels_listed == dag.voxels_listed == len(rec) == int(solid.sum()) and bool((hit[:, 0] == 1).all()) and bool((hit[:, 1] == dag.depth - 1).all())
    assert torch.equal(hit[:, 3].long(), slots) and torch.equal(argb[hit[:, 3].long()], rec[:, 3])
    assert torch.equal(torch.sort(hit[:, 3].long()).values, torch.arange(len(rec), device=DEV))
    assert torch.equal(dense.dag_to_dense(dv, dag, labels.shape, origin=origin), solid)
    tree_bytes = 6 * len(tree.valid)
    print("pipeline: scan_like at 128, filled:", len(rec), "voxels; tree", len(tree.valid), "nodes,", tree_bytes, "bytes; DAG", len(dag.valid), "nodes,", len(dag.child),
          "pointers,", dag.nbytes, "bytes (%.1f %%); colours read back through the DAG" % (100.0 * dag.nbytes / tree_bytes))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list but the failed scratch allocation.  This child runs with torch's caching allocator off:
    each tensor is an allocation of its own, so a short one is short."""
    dv = hip.DeviceVoxelizer(0)
    L = hip._bind()
    C = hip.C
    n = 24
    dims, s = (n, n, n), (1, n, n * n)
    g_np = R.blobs(np.random.default_rng(304), dims, 0.5, noise=0.05)
    t = R.build(g_np, (0, 0, 0), None, True)
    want = G.build(t)
    N, M, P, D = len(t["valid"]), len(want["valid"]), len(want["child"]), t["depth"]
    tv, tf, tfc = dev(t["valid"]), dev(t["full"]), dev(t["first_child"])
    host8, host32 = np.zeros(max(N, P), np.uint8), np.zeros(max(N, P), np.int32)
    short8, short32 = torch.zeros(M - 1, dtype=torch.uint8, device=DEV), torch.zeros(min(M, P) - 1, dtype=torch.int32, device=DEV)
    u3 = lambda a: None if a is None else (C.c_uint32 * 3)(*a)    # noqa: E731
    u64 = lambda a: None if a is None else (C.c_uint64 * 3)(*a)   # noqa: E731
    msgs = []

    def note(fn, what, ctx):
        if ctx:
            msgs.append(what + ": " + L.o2v_hip_last_error(ctx).decode())
            assert fn in msgs[-1], msgs[-1]
        else:
            msgs.append(what)

    # -- build
    def no_build(code, what, ctx=dv._ctx, v=tv.data_ptr(), f=tf.data_ptr(), fc=tfc.data_ptr(), nodes=N, depth=D, flags=COLLAPSE, lc=t["level_counts"], outs=(1, 1, 1)):
        counts, m, p = (C.c_uint64 * 16)(*([99] * 16)), C.c_uint64(99), C.c_uint64(99)
        rc = L.o2v_hip_octree_dag_build(ctx, v, f, fc, nodes, depth, flags, None if lc is None else hip._level_counts(lc), counts if outs[0] else None,
                                        C.byref(m) if outs[1] else None, C.byref(p) if outs[2] else None)
        assert rc == code and m.value == p.value == 99 and list(counts) == [99] * 16, (what, rc)
        note("o2v_hip_octree_dag_build", what, ctx)

    lc = list(t["level_counts"])
    for what, kw in [
        ("null context", dict(ctx=None)), ("null valid", dict(v=None)), ("null full", dict(f=None)), ("null first_child", dict(fc=None)), ("null level_counts", dict(lc=None)),
        ("null out_level_counts", dict(outs=(0, 1, 1))), ("null out_nodes", dict(outs=(1, 0, 1))), ("null out_pointers", dict(outs=(1, 1, 0))),
        ("unknown flag bits", dict(flags=COLLAPSE | 2)), ("depth 0", dict(depth=0)), ("depth 17", dict(depth=17)),
        ("level counts that do not add up", dict(lc=lc[:-1] + [lc[-1] + 1])), ("level counts past the depth", dict(depth=D - 1)), ("two roots", dict(lc=[2] + lc[1:], nodes=N + 1)),
        ("first_child not 4-byte aligned", dict(fc=tfc.data_ptr() + 2)), ("n_nodes past the arrays", dict(nodes=N + 1, lc=lc[:-1] + [lc[-1] + 1])),
        ("host valid", dict(v=host8.ctypes.data)), ("host first_child", dict(fc=host32.ctypes.data)),
    ]:
        no_build(3, what, **kw)
    no_build(5, "n_nodes 2^31", nodes=2 ** 31, lc=[1, 2 ** 31 - 1])
    # -- write: before any build, then with arrays that are short, on the host, misaligned or overlapping
    valid, full = (torch.full((M,), GUARD, dtype=torch.uint8, device=DEV) for _ in range(2))
    first = torch.full((M,), -77, dtype=torch.int32, device=DEV)
    child, skip = (torch.full((P,), -77, dtype=torch.int32, device=DEV) for _ in range(2))
    both8, both32 = torch.full((2 * M,), GUARD, dtype=torch.uint8, device=DEV), torch.full((2 * P,), -77, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def no_write(what, ctx=dv._ctx, v=valid.data_ptr(), f=full.data_ptr(), fc=first.data_ptr(), ch=child.data_ptr(), sk=skip.data_ptr()):
        assert L.o2v_hip_octree_dag_write(ctx, v, f, fc, ch, sk) == 3, what
        note("o2v_hip_octree_dag_write", what, ctx)
        assert bool((valid == GUARD).all()) and bool((full == GUARD).all()) and bool((first == -77).all()) and bool((child == -77).all()) and bool((skip == -77).all())
        assert bool((both8 == GUARD).all()) and bool((both32 == -77).all())

    no_write("write without a build")
    assert "no o2v_hip_octree_dag_build" in msgs[-1]
    G.same(build(dv, t), want, "a correct build")
    no_build(3, "a refused build leaves no DAG", depth=17)
    no_write("write after a refused build")
    assert "no o2v_hip_octree_dag_build" in msgs[-1]
    G.same(build(dv, t), want, "after the refusals")
    for what, kw in [
        ("null context", dict(ctx=None)), ("null valid", dict(v=None)), ("null full", dict(f=None)), ("null first_child", dict(fc=None)), ("null child", dict(ch=None)),
        ("first_child not 4-byte aligned", dict(fc=first.data_ptr() + 2)), ("child not 4-byte aligned", dict(ch=child.data_ptr() + 1)),
        ("skip not 4-byte aligned", dict(sk=skip.data_ptr() + 3)), ("short valid", dict(v=short8.data_ptr())), ("short first_child", dict(fc=short32.data_ptr())),
        ("short skip", dict(sk=short32.data_ptr())), ("host full", dict(f=host8.ctypes.data)), ("host child", dict(ch=host32.ctypes.data)),
        ("valid and full overlap", dict(v=both8.data_ptr(), f=both8.data_ptr() + M - 1)), ("child and skip overlap", dict(ch=both32.data_ptr(), sk=both32.data_ptr() + 4 * (P - 1))),
    ]:
        no_write(what, **kw)
    dv.octree_dag_write(valid.data_ptr(), full.data_ptr(), first.data_ptr(), child.data_ptr(), None)   # skip may be null
    assert np.array_equal(child.cpu().numpy(), want["child"]) and bool((skip == -77).all())
    valid.fill_(GUARD), full.fill_(GUARD), first.fill_(-77), child.fill_(-77)
    # -- lookup and to_dense: the DAG arguments, then their own
    dvv, df, dfc, dch, dsk = dev(want["valid"]), dev(want["full"]), dev(want["first_child"]), dev(want["child"]), dev(want["skip"])
    pts = dev(box_points(0, 4))
    Q = len(pts)
    res = torch.full((Q, 4), -77, dtype=torch.int32, device=DEV)
    out = torch.full((n, n, n), 9, dtype=torch.uint8, device=DEV)
    host_pts, host_grid = np.zeros((Q, 3), np.int32), np.zeros((n, n, n), np.uint8)
    torch.cuda.synchronize()

    def no_query(code, what, which, ctx=dv._ctx, v=dvv.data_ptr(), f=df.data_ptr(), fc=dfc.data_ptr(), ch=dch.data_ptr(), sk=dsk.data_ptr(), nodes=M, ptrs=P, depth=D,
                 flags=COLLAPSE, p=pts.data_ptr(), np_=Q, r=res.data_ptr(), origin=(0, 0, 0), dm=dims, o=out.data_ptr(), strides=s):
        if which == "lookup":
            rc = L.o2v_hip_octree_dag_lookup(ctx, v, f, fc, ch, sk, nodes, ptrs, depth, flags, p, np_, r)
        else:
            rc = L.o2v_hip_octree_dag_to_dense(ctx, v, f, fc, ch, nodes, ptrs, depth, flags, u3(origin), u3(dm), o, u64(strides))
        assert rc == code, (what, which, rc)
        note("o2v_hip_octree_dag_" + which, which + ": " + what, ctx)
        assert bool((res == -77).all()) and bool((out == 9).all())

    for which in ("lookup", "to_dense"):
        for what, kw in [
            ("null context", dict(ctx=None)), ("null valid", dict(v=None)), ("null first_child", dict(fc=None)), ("null child", dict(ch=None)), ("unknown flag bits", dict(flags=2)),
            ("depth 0", dict(depth=0)), ("depth 17", dict(depth=17)), ("n_nodes 0", dict(nodes=0)), ("first_child not 4-byte aligned", dict(fc=dfc.data_ptr() + 1)),
            ("child not 4-byte aligned", dict(ch=dch.data_ptr() + 2)), ("n_nodes past the arrays", dict(nodes=M + 1)), ("n_pointers past the arrays", dict(ptrs=P + 1)),
            ("host valid", dict(v=host8.ctypes.data)), ("host child", dict(ch=host32.ctypes.data)),
        ]:
            no_query(3, what, which, **kw)
        no_query(5, "n_nodes 2^31", which, nodes=2 ** 31)
        no_query(5, "n_pointers 2^31", which, ptrs=2 ** 31)
    for what, kw in [
        ("null points", dict(p=None)), ("null out", dict(r=None)), ("short points", dict(np_=Q + 1)), ("host points", dict(p=host_pts.ctypes.data)),
        ("out not 4-byte aligned", dict(r=res.data_ptr() + 2)), ("skip not 4-byte aligned", dict(sk=dsk.data_ptr() + 2)), ("host skip", dict(sk=host32.ctypes.data)),
        ("out overlaps points", dict(r=pts.data_ptr(), np_=2)), ("out overlaps the DAG", dict(r=dch.data_ptr(), np_=1)), ("out overlaps skip", dict(r=dsk.data_ptr(), np_=1)),
    ]:
        no_query(3, what, "lookup", **kw)
    no_query(5, "2^31 points", "lookup", np_=2 ** 31)
    assert L.o2v_hip_octree_dag_lookup(dv._ctx, dvv.data_ptr(), df.data_ptr(), dfc.data_ptr(), dch.data_ptr(), dsk.data_ptr(), M, P, D, COLLAPSE, None, 0, None) == 0   # no points
    for what, kw in [
        ("null origin", dict(origin=None)), ("null dims", dict(dm=None)), ("null out", dict(o=None)), ("null strides", dict(strides=None)), ("zero dims", dict(dm=(n, n, 0))),
        ("strides that map two voxels to one element", dict(strides=(1, n, 0))), ("short out", dict(dm=(n, n, n + 1))), ("host out", dict(o=host_grid.ctypes.data)),
        ("out overlaps the DAG", dict(o=dvv.data_ptr(), dm=(4, 1, 1))),
    ]:
        no_query(3, what, "to_dense", **kw)
    for what, kw in [("65 537 voxels along y", dict(dm=(1, 65537, 1))), ("2^31 voxels", dict(dm=(1024, 1024, 2048))), ("origin + dims above 2^32", dict(origin=(0, 2 ** 32 - n + 1, 0)))]:
        no_query(5, what, "to_dense", **kw)
    for m in msgs:
        what, _, err = m.partition(": o2v_hip")
        assert "overlap" not in what or "overlap" in err, m
    assert L.o2v_hip_octree_dag_times(None, None) == 3
    # then correct calls: the context still works
    G.same(build(dv, t), want, "at the end")
    dv.octree_dag_lookup(dvv.data_ptr(), df.data_ptr(), dfc.data_ptr(), dch.data_ptr(), dsk.data_ptr(), M, P, D, COLLAPSE, pts.data_ptr(), Q, res.data_ptr())
    assert np.array_equal(res.cpu().numpy(), G.lookup(want, pts.cpu().numpy()))
    dv.octree_dag_to_dense(dvv.data_ptr(), df.data_ptr(), dfc.data_ptr(), dch.data_ptr(), M, P, D, COLLAPSE, (0, 0, 0), dims, out.data_ptr(), s)
    assert np.array_equal(out.cpu().numpy() != 0, g_np)
    print("\n".join(msgs))
    print("refused", len(msgs), "calls")


# ---- one call per case and its wall time ------------------------------------------------------------------------------------------

CASES = {"shapes_and_layouts": case_shapes_and_layouts, "table": case_table, "queries": case_queries, "determinism": case_determinism, "pipeline": case_pipeline,
         "refusals": case_refusals}

if __name__ == "__main__":
    t0 = time.time()
    CASES[sys.argv[1]]()
    print("case", sys.argv[1], "took %.1f s" % (time.time() - t0))
    print("ok")
