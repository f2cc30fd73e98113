"""The GPU cases of tests/test_gpu_treeray.py, each run in a child process of its own: `python -m tests.treeray_cases <case>`, the
cases of one grid as `<case>:<k>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison is bit for bit - hit as int32, t as
float32 bits, the slot as int32 - against the numpy reference of tests/treeray_ref.py (to_dense of the arrays, the fine walk of
tests/raycast_ref.py, the lookup's slot), or against RayCaster on the device where the case says so; there is no tolerance
anywhere.  The outputs are filled with a guard value before every call at the C level and hold three entries more than the call
may write.  A case prints what it covered and "ok" last when everything held."""
import os
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import dag_ref as G
from tests import octree_ref as R
from tests import raycast_ref as RC
from tests import treeray_ref as TR
from tests.octree_cases import dev, indexed, tree_of

DEV = torch.device("cuda", 0)
COLLAPSE = hip.OCT_COLLAPSE
INF = float("inf")
GUARD = -77
NO_STACK = "O2V_TREERAY_NO_STACK"


def upload(a):
    """the arrays of a tree's or a DAG's dict on the device"""
    return dict(a, dev={k: dev(a[k]) for k in ("valid", "full", "first_child", "child", "skip") if a.get(k) is not None})


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def cast(dv, a, o, d, t_max=INF, voxel_index=True, skips=True):
    """o2v_hip_octree_raycast / o2v_hip_octree_dag_raycast at the C level on the uploaded arrays a and the device rays o, d, into
    guarded outputs: (hit, t, slot) as numpy, slot None without voxel_index."""
    n = len(o)
    hit = torch.full((n + 3, 4), GUARD, dtype=torch.int32, device=DEV)
    t = torch.full((n + 3,), float(GUARD), dtype=torch.float32, device=DEV)
    slot = torch.full((n + 3,), GUARD, dtype=torch.int32, device=DEV)
    u = a["dev"]
    torch.cuda.synchronize()
    rays = (o.data_ptr(), d.data_ptr(), n, t_max, hit.data_ptr(), t.data_ptr(), slot.data_ptr() if voxel_index else None)
    if TR.is_dag(a):
        dv.octree_dag_raycast(ptr(u["valid"]), ptr(u["full"]), ptr(u["first_child"]), ptr(u["child"]), ptr(u.get("skip")) if skips else None, len(a["valid"]),
                              len(a["child"]), a["depth"], COLLAPSE * a["collapsed"], *rays)
    else:
        dv.octree_raycast(ptr(u["valid"]), ptr(u["full"]), ptr(u["first_child"]), len(a["valid"]), a["depth"], COLLAPSE * a["collapsed"], *rays)
    hit, t, slot = hit.cpu().numpy(), t.cpu().numpy(), slot.cpu().numpy()
    assert (hit[n:] == GUARD).all() and (t[n:] == GUARD).all() and (slot[n:] == GUARD).all(), "a guard was written"
    assert voxel_index or (slot == GUARD).all()
    return hit[:n], t[:n], slot[:n] if voxel_index else None


def check(got, want, what, o, d):
    assert TR.same(tuple(g for g in got if g is not None), want), (what, TR.first_difference(tuple(g for g in got if g is not None), want, o, d))


# ---- shapes, extremes, the stack A/B ----------------------------------------------------------------------------------------------

def case_shapes(k):
    """Grid k as tree and DAG, collapsed and not: its ray set with t_max inf, and 1 000 of the rays with t_max 0, 3.5 and one ray's own t."""
    name, g, origin, depth, o, d, want, short = TR.scene(k)
    dv = hip.DeviceVoxelizer(0)
    od, dd = dev(o), dev(d)
    os_, ds_ = dev(o[:TR.N_SHORT]), dev(d[:TR.N_SHORT])
    casts = 0
    for what, a in TR.sources(g, origin, depth):
        u = upload(a)
        want_slot = TR.slots(a, want[0])
        check(cast(dv, u, od, dd), want + (want_slot,), (name, what), o, d)
        check(cast(dv, u, od, dd, voxel_index=False), want, (name, what, "no voxel_index"), o, d)
        for t_max, w in short.items():
            check(cast(dv, u, os_, ds_, t_max), w + (TR.slots(a, w[0]),), (name, what, t_max), o, d)
        casts += 2 + len(short)
        if TR.is_dag(a) and len(a["child"]):
            bare = cast(dv, u, od, dd, skips=False)
            assert RC.same(bare[:2], want) and (bare[2] == -1).all(), (name, what, "without skip")
            casts += 1
    assert dv.octree_raycast_times()[0] > 0.0
    share = RC.shares(want[0])
    print("shapes[%d]: %s, depth %d: %d casts of %d rays as tree and DAG, collapsed and not; %.0f %% hit, %.0f %% miss" %
          (k, name, TR.sources(g, origin, depth)[0][1]["depth"], casts, len(o), 100 * share[0], 100 * share[1]))


def case_stack_ab(k):
    """Grid k with and without O2V_TREERAY_NO_STACK=1 (read at the entry of every call): both equal the reference and each other."""
    name, g, origin, depth, o, d, want, _ = TR.scene(k)
    dv = hip.DeviceVoxelizer(0)
    od, dd = dev(o), dev(d)
    n = 0
    for what, a in TR.sources(g, origin, depth):
        u = upload(a)
        ref = want + (TR.slots(a, want[0]),)
        got = {}
        for no_stack in ("1", None, "1", None):
            os.environ.pop(NO_STACK, None)
            if no_stack:
                os.environ[NO_STACK] = no_stack
            got[no_stack] = cast(dv, u, od, dd)
            check(got[no_stack], ref, (name, what, no_stack), o, d)
            n += 1
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(got["1"], got[None]))
    os.environ.pop(NO_STACK, None)
    print("stack_ab[%d]: %s: %d casts with and without %s=1 gave the reference's bits" % (k, name, n, NO_STACK))


EXTREME_GRIDS = (0, 2, 1)   # the ball, the checkerboard, the one voxel


def case_extremes():
    dv = hip.DeviceVoxelizer(0)
    n = 0
    for k in EXTREME_GRIDS:
        name, g, origin, depth, _ = TR.grids()[k]
        o, d = RC.extreme_rays(np.random.default_rng(3700 + k), g, origin)
        want = RC.cast(g, origin, o, d)[:2]
        od, dd = dev(o), dev(d)
        for what, a in TR.sources(g, origin, depth):
            check(cast(dv, upload(a), od, dd), want + (TR.slots(a, want[0]),), (name, what), o, d)
            n += 1
    print("extremes:", n, "casts of 4000 rays with denormal, 3e38 and -0.0 components from planes, edges and corners")


# ---- against RayCaster on the device --------------------------------------------------------------------------------------------------

RAYCASTER_GRIDS = (0, 1, 2, 4, 5, 6)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def case_against_raycaster():
    dv = hip.DeviceVoxelizer(0)
    n = 0
    for k in RAYCASTER_GRIDS:
        name, g, origin, depth, _ = TR.grids()[k]
        o, d = RC.ray_set(np.random.default_rng(3800 + k), g, origin)
        od, dd, grid = dev(o), dev(d), dev(g)
        want = dense.RayCaster(dv, grid, origin=origin).cast(od, dd)
        assert int((want[0][:, 0] >= 0).sum()) > len(o) // 4
        for collapse in (True, False):
            tree = dense.build_octree(dv, grid, origin=origin, depth=depth, collapse=collapse)
            dag = dense.octree_dag(dv, tree)
            for got in (dense.octree_raycast(dv, tree, od, dd), dense.dag_raycast(dv, dag, od, dd)):
                assert torch.equal(got[0], want[0]) and torch.equal(bits(got[1]), bits(want[1])), (name, collapse)
                n += 1
    print("against_raycaster:", n, "casts of", len(o), "rays through trees and DAGs gave RayCaster's bits on", len(RAYCASTER_GRIDS), "grids")


# ---- arrays that are no tree ---------------------------------------------------------------------------------------------------------

def case_not_a_tree():
    """The arrays of tests/test_host_treeray.py, on which the walk has run on the host under the sanitizers: the device gives the
    reference's bits on to_dense of the same arrays, and to_dense on the device is that set."""
    dv = hip.DeviceVoxelizer(0)
    n = 0
    for k, (name, a) in enumerate(TR.not_a_tree()):
        solid = TR.solid_set(a)
        o, d = TR.broken_rays(k, solid)
        want = TR.cast(a, o, d, solid=solid)
        u = upload(a)
        od, dd = dev(o), dev(d)
        for no_stack in (None, "1"):
            os.environ.pop(NO_STACK, None)
            if no_stack:
                os.environ[NO_STACK] = no_stack
            check(cast(dv, u, od, dd), want, (name, no_stack), o, d)
            n += 1
        os.environ.pop(NO_STACK, None)
        out = torch.full((16, 16, 16), 9, dtype=torch.uint8, device=DEV)
        v = u["dev"]
        torch.cuda.synchronize()
        if TR.is_dag(a):
            dv.octree_dag_to_dense(ptr(v["valid"]), ptr(v["full"]), ptr(v["first_child"]), ptr(v["child"]), len(a["valid"]), len(a["child"]), a["depth"],
                                   COLLAPSE * a["collapsed"], (0, 0, 0), (16, 16, 16), out.data_ptr(), (1, 16, 256))
        else:
            dv.octree_to_dense(ptr(v["valid"]), ptr(v["full"]), ptr(v["first_child"]), len(a["valid"]), a["depth"], COLLAPSE * a["collapsed"], (0, 0, 0), (16, 16, 16),
                               out.data_ptr(), (1, 16, 256))
        assert np.array_equal(out.cpu().numpy() != 0, solid[0]), name
    print("not_a_tree:", n, "casts through", k + 1, "sets of arrays that are no tree gave the reference's bits on to_dense of the same arrays")


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------

def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, *indexed(meshes.scan_like()))
    labels, origin = dense.voxelize_dense(dv, 128, fmt="labels", fill=True)
    palette = [0] + [0xff000000 | (i * 0x010307 & 0xffffff) for i in range(1, 256)]
    tree = dense.build_octree(dv, labels, origin=origin, collapse=False)
    dag = dense.octree_dag(dv, tree)
    # colours scattered by the tree's voxel_index, as in the README, and the same colours as a grid
    rec = dense.to_voxels(dv, labels, origin=origin, palette=palette)
    slots = dense.octree_lookup(dv, tree, rec[:, :3].contiguous())[:, 3].long()
    argb = torch.zeros(tree.voxels_listed, dtype=torch.int32, device=DEV).scatter_(0, slots, rec[:, 3])
    colours = torch.zeros(labels.shape, dtype=torch.int32, device=DEV)
    at = rec[:, :3].long() - torch.tensor(origin, device=DEV)
    colours[at[:, 2], at[:, 1], at[:, 0]] = rec[:, 3]
    nz, ny, nx = labels.shape
    centre = (origin[0] + nx / 2, origin[1] + ny / 2, origin[2] + nz / 2)
    eye = (centre[0] + 1.6 * nx, centre[1] - 1.3 * ny, centre[2] + 0.9 * nz)
    o, d = dense.camera_rays(128, 128, eye, centre, (0, 0, 1), 40.0, DEV)
    want = dense.RayCaster(dv, labels, origin=origin).cast(o, d)
    hits = want[0][..., 0] >= 0
    assert 128 * 128 // 10 < int(hits.sum()) < 128 * 128
    for name, got in (("tree", dense.octree_raycast(dv, tree, o, d, voxel_index=True)), ("DAG", dense.dag_raycast(dv, dag, o, d, voxel_index=True))):
        hit, t, slot = got
        assert torch.equal(hit, want[0]) and torch.equal(bits(t), bits(want[1])), name
        assert tuple(slot.shape) == (128, 128) and torch.equal(slot >= 0, hits), name
        cell = hit[hits][:, :3].long() - torch.tensor(origin, device=DEV)
        assert torch.equal(argb[slot[hits].long()], colours[cell[:, 2], cell[:, 1], cell[:, 0]]), name
        image = argb[slot.clamp(min=0).long()].where(slot >= 0, torch.zeros((), dtype=torch.int32, device=DEV))
        assert tuple(image.shape) == (128, 128) and bool((image[hits] != 0).all()) and bool((image[~hits] == 0).all())
    print("pipeline: scan_like at 128, filled: a 128 x 128 image,", int(hits.sum()), "pixels hit; tree", 6 * len(tree.valid), "bytes, DAG", dag.nbytes,
          "bytes, grid", labels.numel(), "bytes; every pixel's colour through the slot")


# ---- determinism --------------------------------------------------------------------------------------------------------------------

def case_determinism():
    rng = np.random.default_rng(3900)
    g = R.blobs(rng, (100, 90, 80), 0.5, noise=0.05)
    o, d = RC.ray_set(rng, g, (5, 6, 7))
    od, dd = dev(o), dev(d)
    dv, other = hip.DeviceVoxelizer(0), hip.DeviceVoxelizer(0)
    t = R.build(g, (5, 6, 7), None, True)
    n = 0
    for a in (t, G.build(t)):
        u = upload(a)
        first = cast(dv, u, od, dd)
        assert int((first[0][:, 0] >= 0).sum()) > len(o) // 4
        for c in (other, dv, other):
            again = cast(c, u, od, dd)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
            n += 1
    print("determinism:", n, "casts on two contexts gave equal bytes")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list, the outputs untouched, a correct cast behind each.  This child runs with torch's caching
    allocator off: each tensor is an allocation of its own, so a short one is short."""
    dv = hip.DeviceVoxelizer(0)
    L, C = hip._bind(), hip.C
    g = R.blobs(np.random.default_rng(3950), (24, 24, 24), 0.5, noise=0.05)
    t = R.build(g, (0, 0, 0), None, True)
    dag = G.build(t)
    N, M, P, D = len(t["valid"]), len(dag["valid"]), len(dag["child"]), t["depth"]
    o, d = RC.ray_set(np.random.default_rng(3951), g, (0, 0, 0), n=500, far=0, limit=0)
    Q = len(o)
    want = RC.cast(g, (0, 0, 0), o, d)[:2]
    want = {"tree": want + (TR.slots(t, want[0]),), "dag": want + (TR.slots(dag, want[0]),)}
    ut, ud = upload(t), upload(dag)
    od, dd = dev(o), dev(d)
    hit = torch.full((Q, 4), GUARD, dtype=torch.int32, device=DEV)
    tt = torch.full((Q,), float(GUARD), dtype=torch.float32, device=DEV)
    slot = torch.full((Q,), GUARD, dtype=torch.int32, device=DEV)
    both = torch.full((8 * Q,), GUARD, dtype=torch.int32, device=DEV)
    short = torch.full((Q - 1,), GUARD, dtype=torch.int32, device=DEV)
    short_rays = torch.zeros((Q - 1, 3), dtype=torch.float32, device=DEV)
    host8, host32, hostf = np.zeros(max(N, 16 * Q), np.uint8), np.zeros(max(N, P, 4 * Q), np.int32), np.zeros((Q, 3), np.float32)
    torch.cuda.synchronize()
    msgs = []

    def untouched():
        return bool((hit == GUARD).all()) and bool((tt == GUARD).all()) and bool((slot == GUARD).all()) and bool((both == GUARD).all()) and bool((short == GUARD).all())

    def refused(code, which, what, ctx=dv._ctx, v=None, f=None, fc=None, ch=None, sk=None, nodes=None, ptrs=P, depth=D, flags=COLLAPSE, o_=od.data_ptr(),
                d_=dd.data_ptr(), n=Q, t_max=INF, h=hit.data_ptr(), t_=tt.data_ptr(), s=slot.data_ptr(), **own):
        u = (ut if which == "tree" else ud)["dev"]
        a = dict(v=u["valid"].data_ptr(), f=u["full"].data_ptr(), fc=u["first_child"].data_ptr(), ch=u["child"].data_ptr() if which == "dag" else None,
                 sk=u["skip"].data_ptr() if which == "dag" else None, nodes=N if which == "tree" else M)
        a.update({k: val for k, val in dict(v=v, f=f, fc=fc, ch=ch, sk=sk, nodes=nodes).items() if val is not None})
        a.update({k: None for k in own.get("null", ())})
        if which == "tree":
            rc = L.o2v_hip_octree_raycast(ctx, a["v"], a["f"], a["fc"], a["nodes"], depth, flags, o_, d_, n, t_max, h, t_, s)
        else:
            rc = L.o2v_hip_octree_dag_raycast(ctx, a["v"], a["f"], a["fc"], a["ch"], a["sk"], a["nodes"], ptrs, depth, flags, o_, d_, n, t_max, h, t_, s)
        assert rc == code, (which, what, rc, L.o2v_hip_last_error(dv._ctx).decode())
        assert untouched(), (which, what)
        if ctx:
            msgs.append("%s: %s: %s" % (which, what, L.o2v_hip_last_error(ctx).decode()))
            assert ("o2v_hip_octree_raycast" if which == "tree" else "o2v_hip_octree_dag_raycast") in msgs[-1], msgs[-1]
        else:
            msgs.append("%s: %s" % (which, what))
        # a correct cast behind it: the context still works
        check(cast(dv, ut if which == "tree" else ud, od, dd), want[which], (which, "after", what), o, d)

    for which in ("tree", "dag"):
        u = (ut if which == "tree" else ud)["dev"]
        fcp = u["first_child"].data_ptr()
        for what, kw in [
            ("null context", dict(ctx=None)), ("null valid", dict(null=("v",))), ("null full", dict(null=("f",))), ("null first_child", dict(null=("fc",))),
            ("null origins", dict(o_=None)), ("null directions", dict(d_=None)), ("null hit", dict(h=None)), ("null t", dict(t_=None)),
            ("unknown flag bits", dict(flags=COLLAPSE | 2)), ("the stage-times flag", dict(flags=COLLAPSE | hip.FLAG_STAGE_TIMES)), ("depth 0", dict(depth=0)),
            ("depth 17", dict(depth=17)), ("n_nodes 0", dict(nodes=0, null=())), ("t_max NaN", dict(t_max=float("nan"))), ("t_max negative", dict(t_max=-1.0)),
            ("first_child not 4-byte aligned", dict(fc=fcp + 2)), ("origins not 4-byte aligned", dict(o_=od.data_ptr() + 2, n=Q - 1)),
            ("directions not 4-byte aligned", dict(d_=dd.data_ptr() + 1, n=Q - 1)), ("hit not 4-byte aligned", dict(h=both.data_ptr() + 2)),
            ("t not 4-byte aligned", dict(t_=both.data_ptr() + 1)), ("voxel_index not 4-byte aligned", dict(s=both.data_ptr() + 3)),
            ("hit and t overlap", dict(h=both.data_ptr(), t_=both.data_ptr() + 16 * Q - 4)), ("hit and voxel_index overlap", dict(h=both.data_ptr() + 4 * Q - 4, s=both.data_ptr())),
            ("t and voxel_index overlap", dict(t_=both.data_ptr(), s=both.data_ptr() + 4 * Q - 4)), ("hit overlaps origins", dict(h=od.data_ptr(), n=Q // 2)),
            ("t overlaps directions", dict(t_=dd.data_ptr())), ("voxel_index overlaps first_child", dict(s=fcp, n=1)), ("hit overlaps valid", dict(h=u["valid"].data_ptr(), n=1)),
            ("host valid", dict(v=host8.ctypes.data)), ("host first_child", dict(fc=host32.ctypes.data)), ("host origins", dict(o_=hostf.ctypes.data)),
            ("host hit", dict(h=host8.ctypes.data)), ("host voxel_index", dict(s=host32.ctypes.data)), ("n_nodes past the arrays", dict(nodes=(N if which == "tree" else M) + 1)),
            ("short origins", dict(o_=short_rays.data_ptr())), ("short directions", dict(d_=short_rays.data_ptr())), ("short hit", dict(h=short.data_ptr())),
            ("short t", dict(t_=short.data_ptr())), ("short voxel_index", dict(s=short.data_ptr())),
        ]:
            refused(3, which, what, **kw)
        refused(5, which, "n_nodes 2^31", nodes=2 ** 31)
        refused(5, which, "2^31 rays", n=2 ** 31)
    chp, skp = ud["dev"]["child"].data_ptr(), ud["dev"]["skip"].data_ptr()
    for what, kw in [
        ("null child", dict(null=("ch",))), ("child not 4-byte aligned", dict(ch=chp + 2)), ("skip not 4-byte aligned", dict(sk=skp + 1)), ("host child", dict(ch=host32.ctypes.data)),
        ("host skip", dict(sk=host32.ctypes.data)), ("n_pointers past the arrays", dict(ptrs=P + 1)), ("hit overlaps child", dict(h=chp, n=1)),
        ("voxel_index overlaps skip", dict(s=skp, n=1)),
    ]:
        refused(3, "dag", what, **kw)
    refused(5, "dag", "n_pointers 2^31", ptrs=2 ** 31)
    for m in msgs:
        what, _, err = m.partition(": o2v_hip")
        assert "overlap" not in what or "overlap" in err, m
    # no rays: success, nothing written, null pointers allowed; voxel_index and skip may be null
    v = ut["dev"]
    assert L.o2v_hip_octree_raycast(dv._ctx, v["valid"].data_ptr(), v["full"].data_ptr(), v["first_child"].data_ptr(), N, D, COLLAPSE, None, None, 0, INF, None, None, None) == 0
    v = ud["dev"]
    assert L.o2v_hip_octree_dag_raycast(dv._ctx, v["valid"].data_ptr(), v["full"].data_ptr(), v["first_child"].data_ptr(), chp, skp, M, P, D, COLLAPSE, od.data_ptr(),
                                        dd.data_ptr(), 0, INF, hit.data_ptr(), tt.data_ptr(), slot.data_ptr()) == 0
    assert untouched() and L.o2v_hip_octree_raycast_times(None, None) == 3
    check(cast(dv, ud, od, dd, voxel_index=False), want["dag"][:2], "no voxel_index", o, d)
    bare = cast(dv, ud, od, dd, skips=False)
    assert RC.same(bare[:2], want["dag"][:2]) and (bare[2] == -1).all()
    print("\n".join(msgs))
    print("refused", len(msgs), "calls, a correct cast behind each")


# ---- one call per case and its wall time ------------------------------------------------------------------------------------------

CASES = {"shapes": case_shapes, "stack_ab": case_stack_ab, "extremes": case_extremes, "against_raycaster": case_against_raycaster, "not_a_tree": case_not_a_tree,
         "pipeline": case_pipeline, "determinism": case_determinism, "refusals": case_refusals}

if __name__ == "__main__":
    t0 = time.time()
    case, _, k = sys.argv[1].partition(":")
    CASES[case](*([int(k)] if k else []))
    print("case", sys.argv[1], "took %.1f s" % (time.time() - t0))
    print("ok")
