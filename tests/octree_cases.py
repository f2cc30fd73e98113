"""The GPU cases of tests/test_gpu_octree.py, each run in a child process of its own: `python -m tests.octree_cases <case>`.

torch is imported before the library is loaded (the grids are torch tensors; see tests/dense_cases.py).  Every comparison is bit for
bit - valid, full, first_child, coords, the level counts and voxels_listed - against the numpy reference of tests/octree_ref.py or
against closed forms in Python ints, never against the code under test, and there is no tolerance anywhere.  The output arrays are
filled with a guard value before every call.  A case prints what it covered and "ok" last when everything held."""
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import octree_ref as R

DEV = torch.device("cuda", 0)
U8, BITS, F32 = hip.GRID_U8, hip.GRID_BITS, hip.GRID_F32_BELOW
COLLAPSE = hip.OCT_COLLAPSE
GUARD = 0x5a


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def st(t):
    """(x, y, z) element strides of a tensor [z, y, x]."""
    return t.stride(2), t.stride(1), t.stride(0)


def build(dv, t, fmt, dims, origin, depth, flags, level=0.0):
    """o2v_hip_octree_build + _write at the C level on the tensor view t [z, y, x] into guarded arrays; the tree as the reference's dict."""
    torch.cuda.synchronize()
    d, counts, nodes, listed = dv.octree_build(t.data_ptr(), fmt, st(t), dims, level, origin, depth, flags)
    assert sum(counts) == nodes and len(counts) == d
    valid, full = (torch.full((nodes + 3,), GUARD, dtype=torch.uint8, device=DEV) for _ in range(2))
    first, coords = torch.full((nodes + 3,), -77, dtype=torch.int32, device=DEV), torch.full((nodes + 3, 3), -77, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    dv.octree_write(valid.data_ptr(), full.data_ptr(), first.data_ptr(), coords.data_ptr())
    valid, full, first, coords = (a.cpu().numpy() for a in (valid, full, first, coords))
    assert (valid[nodes:] == GUARD).all() and (full[nodes:] == GUARD).all() and (first[nodes:] == -77).all() and (coords[nodes:] == -77).all()
    return dict(valid=valid[:nodes], full=full[:nodes], first_child=first[:nodes], coords=coords[:nodes], level_counts=list(counts), voxels_listed=listed,
                depth=d, collapsed=bool(flags & COLLAPSE))


def as_ref(tree):
    offs = tree.level_offsets
    return dict(valid=tree.valid.cpu().numpy(), full=tree.full.cpu().numpy(), first_child=tree.first_child.cpu().numpy(),
                coords=None if tree.coords is None else tree.coords.cpu().numpy(), level_counts=[b - a for a, b in zip(offs, offs[1:])],
                voxels_listed=tree.voxels_listed, depth=tree.depth, collapsed=tree.collapsed)


def tree_of(ref):
    """the reference's dict as an Octree on the device"""
    offs = tuple(int(v) for v in np.concatenate([[0], np.cumsum(ref["level_counts"])]))
    return dense.Octree(valid=dev(ref["valid"]), full=dev(ref["full"]), first_child=dev(ref["first_child"]), coords=None, level_offsets=offs, depth=ref["depth"],
                        collapsed=ref["collapsed"], voxels_listed=ref["voxels_listed"])


# ---- shapes and layouts -----------------------------------------------------------------------------------------------------------

def layouts(g):
    """(name, format, tensor view, level) of the grid g [z, y, x] (bool) in every format and layout of the case."""
    nz, ny, nx = g.shape
    t = dev(g)
    out = [("bool, contiguous", U8, t, 0.0)]
    flat = torch.zeros(g.size + 40, dtype=torch.uint8, device=DEV)
    flat[1:1 + g.size] = t.reshape(-1)
    out.append(("uint8, one element into an allocation", U8, flat[1:1 + g.size].view(g.shape), 0.0))     # (rows not aligned for 16-byte loads)
    aligned = torch.zeros((nz, ny, -(-nx // 16) * 16), dtype=torch.uint8, device=DEV)
    aligned[:, :, :nx] = t * 3
    out.append(("uint8, rows of 16 bytes", U8, aligned[:, :, :nx], 0.0))                                  # (every row 16-byte aligned)
    wide = torch.zeros((nz, ny, 2 * nx), dtype=torch.uint8, device=DEV)
    wide[:, :, ::2] = t
    out.append(("uint8, x stride 2", U8, wide[:, :, ::2], 0.0))
    out.append(("bool, x and z swapped", U8, t.permute(2, 1, 0).contiguous().permute(2, 1, 0), 0.0))
    if g.all() or not g.any():
        out.append(("uint8, stride 0", U8, torch.full((1, 1, 1), int(g.flat[0]), dtype=torch.uint8, device=DEV).expand(nz, ny, nx), 0.0))
    f = dev(np.where(g, 0.25, 0.75).astype(np.float32))
    out.append(("float32 below 0.5, contiguous", F32, f, 0.5))
    wide_f = torch.ones((nz, 2 * ny, nx + 1), dtype=torch.float32, device=DEV)
    wide_f[:, ::2, 1:] = f
    out.append(("float32 below 0.5, sliced", F32, wide_f[:, ::2, 1:], 0.5))
    W = -(-nx // 32)
    padded = np.zeros((nz, ny, W * 32), np.uint8)
    padded[:, :, :nx] = g
    words = dev(np.packbits(padded, axis=-1, bitorder="little").view("<i4"))
    out.append(("bits, contiguous", BITS, words, 0.0))
    tall = torch.zeros((nz, 2 * ny, W), dtype=torch.int32, device=DEV)
    tall[:, 1::2] = words
    out.append(("bits, y stride 2", BITS, tall[:, 1::2], 0.0))
    return out


def case_shapes_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(300)
    calls = grids = 0
    used = set()
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
                views = layouts(g)
                combos = [(D0 + 2 * (grids & 1), COLLAPSE * (grids >> 1 & 1))] if name.startswith("corner") else [(D0, 0), (D0, COLLAPSE), (D0 + 2, 0), (D0 + 2, COLLAPSE)]
                for depth, flags in combos:
                    want = R.build(g, origin, depth, bool(flags))
                    # the smallest depth is also what depth 0 asks for
                    for k in range(2):
                        what, fmt, t, level = views[5 if k and len(views) == 10 else (calls + k * 5) % len(views)]   # (a uniform grid: also as one expanded byte)
                        got = build(dv, t, fmt, dims, origin, 0 if depth == D0 and k else depth, flags, level)
                        R.same(got, want, (dims, origin, name, depth, flags, what))
                        used.add(what)
                        calls += 1
                grids += 1
    assert len(used) == 10, sorted(used)
    assert len(dv.octree_times()) == 4 and all(v >= 0 for v in dv.octree_times())
    print("shapes_and_layouts: compared", calls, "builds of", grids, "grids in", len(used), "formats and layouts")


# ---- block edges ------------------------------------------------------------------------------------------------------------------

def case_block_edges():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(301)
    g = rng.random((128, 128, 128)) < 0.5
    g[::2, ::2, ::2], g[1::2, 1::2, 1::2] = True, False   # (no 2^3 block empty, none full: every one is a node of level 6, collapsed or not)
    t = dev(g)
    for flags in (0, COLLAPSE):
        want = R.build(g, (0, 0, 0), None, bool(flags))
        assert want["level_counts"][-1] == 262144 and want["level_counts"][-2] == 32768
        R.same(build(dv, t, U8, (128, 128, 128), (0, 0, 0), 0, flags), want, ("random 128^3", flags))
    print("block_edges: random 128^3: 262144 nodes at level 6, first_child to", int(want["first_child"][-1]), "across 1024 blocks of 256")
    g = R.checkerboard(64)
    for flags in (0, COLLAPSE):
        got = build(dv, dev(g), U8, (64, 64, 64), (0, 0, 0), 0, flags)
        R.same(got, R.build(g, (0, 0, 0), None, bool(flags)), ("checkerboard", flags))
        assert got["level_counts"] == [8 ** l for l in range(6)] and set(got["valid"][-8 ** 5:].tolist()) == {0x69} and got["voxels_listed"] == 64 ** 3 // 2
    g = R.ball()
    for flags, table in ((COLLAPSE, [1, 8, 32, 104, 336, 936]), (0, [1, 8, 32, 136, 696, 4680])):
        got = build(dv, dev(g), U8, (64, 64, 64), (0, 0, 0), 0, flags)
        assert got["level_counts"] == table, got["level_counts"]
        R.same(got, R.build(g, (0, 0, 0), None, bool(flags)), ("ball", flags))
    print("block_edges: the checkerboard at 64^3 and the ball: level counts", table)


# ---- queries ----------------------------------------------------------------------------------------------------------------------

def box_points(lo, hi):
    z, y, x = np.meshgrid(*(np.arange(lo, hi),) * 3, indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.int32)


def case_queries():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(302)
    g = R.blobs(rng, (11, 6, 5), 0.6)
    origin = (3, 1, 2)
    far = np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1], [16, 0, 0], [0, 16, 0], [0, 0, 16], [-2 ** 31, 5, 5], [5, 2 ** 31 - 1, 5], [65536, 65536, 65536]], np.int32)
    n_points = 0
    for collapse in (True, False):
        tree = dense.build_octree(dv, dev(g), origin=origin, collapse=collapse, coords=True)
        ref = R.build(g, origin, None, collapse)
        R.same(as_ref(tree), ref, ("queries", collapse))
        pts = np.concatenate([box_points(-2, 18), far])
        got = dense.octree_lookup(dv, tree, dev(pts)).cpu().numpy()
        assert np.array_equal(got, R.lookup(ref, pts)), collapse
        assert (got[-len(far):] == (0, -1, -1, -1)).all() and got[:, 0].sum() == g.sum()
        n_points += len(pts)
        # the tree from the reference's arrays, as one loaded from disk: the same answers
        assert np.array_equal(dense.octree_lookup(dv, tree_of(ref), dev(pts)).cpu().numpy(), got)
        # to_dense: the box itself; an odd origin and a box that sticks out of the cube, contiguous and strided
        assert np.array_equal(dense.octree_to_dense(dv, tree, g.shape, origin=origin).cpu().numpy(), g)
        want = np.zeros((12, 13, 21), bool)
        want[2:7, 1:7, 2:13] = g
        assert np.array_equal(dense.octree_to_dense(dv, tree, want.shape, origin=(1, 0, 0)).cpu().numpy(), want)
        wide = torch.full((12, 26, 21 * 3 + 1), 9, dtype=torch.uint8, device=DEV)
        out = dense.octree_to_dense(dv, tree, want.shape, origin=(1, 0, 0), out=wide[:, ::2, 1::3])
        assert out.data_ptr() == wide[:, ::2, 1::3].data_ptr() and np.array_equal(out.cpu().numpy(), want.astype(np.uint8))
        wide[:, ::2, 1::3] = 9
        assert bool((wide == 9).all())   # (nothing beside the voxels was written)
        swapped = torch.empty((21, 13, 12), dtype=torch.bool, device=DEV).permute(2, 1, 0)
        assert np.array_equal(dense.octree_to_dense(dv, tree, want.shape, origin=(1, 0, 0), out=swapped).cpu().numpy(), want)
        assert not dense.octree_to_dense(dv, tree, (3, 4, 5), origin=(16, 0, 0)).any() and not dense.octree_to_dense(dv, tree, (2, 2, 2), origin=(2 ** 32 - 2, 7, 7)).any()
    # to_dense(build(g)) == g: sizes that are no multiple of a block, odd origins, depths above the smallest
    n_round = 0
    for dims, o, extra in (((1, 1, 1), (0, 0, 0), 0), ((1, 1, 1), (1, 1, 1), 3), ((65, 5, 4), (63, 7, 8), 0), ((129, 9, 10), (1, 3, 5), 2), ((70, 50, 40), (0, 0, 0), 0)):
        for collapse in (True, False):
            for p in (0.1, 0.6, 1.0):
                g2 = R.blobs(rng, dims, p, noise=0.0 if p == 1.0 else 0.05)
                tree = dense.build_octree(dv, dev(g2), origin=o, depth=R.depth_of(o, dims) + extra, collapse=collapse)
                assert np.array_equal(dense.octree_to_dense(dv, tree, g2.shape, origin=o).cpu().numpy(), g2), (dims, o, collapse, p)
                solid = dense.octree_lookup(dv, tree, dev(np.argwhere(g2)[:, ::-1].astype(np.int32) + np.array(o, np.int32)))
                assert bool((solid[:, 0] == 1).all())
                n_round += 1
    # a tree whose first_child was overwritten: (0, -2, -1, -1) rows, the reference's, and no fault
    g3 = R.blobs(rng, (32, 32, 32), 0.5, noise=0.1)
    pts = box_points(0, 32)
    n_bad = 0
    for collapse in (True, False):
        ref = R.build(g3, (0, 0, 0), None, collapse)
        top = ref["level_counts"][0] + ref["level_counts"][1] + ref["level_counts"][2]
        for bad in (len(ref["valid"]), 2 ** 31 - 1, -1, -2 ** 31, 2 ** 30):
            broken = dict(ref, first_child=np.where(np.arange(len(ref["valid"])) < top, bad, ref["first_child"]).astype(np.int32))
            got = dense.octree_lookup(dv, tree_of(broken), dev(pts)).cpu().numpy()
            rows = got[:, 1] == -2
            assert rows.any() and (got[rows] == (0, -2, -1, -1)).all() and np.array_equal(got[::37], R.lookup(broken, pts[::37])), (collapse, bad)
            assert not dense.octree_to_dense(dv, tree_of(broken), g3.shape)[torch.from_numpy(rows.reshape(g3.shape)).to(DEV)].any()
            n_bad += int(rows.sum())
    print("queries:", n_points, "points looked up against the scalar descent,", n_round, "round trips,", n_bad, "rows (0, -2, -1, -1) of corrupt trees")


# ---- determinism --------------------------------------------------------------------------------------------------------------------

def case_determinism():
    rng = np.random.default_rng(303)
    g = dev(R.blobs(rng, (100, 90, 80), 0.5, noise=0.05))
    dv, other = hip.DeviceVoxelizer(0), hip.DeviceVoxelizer(0)
    n = 0
    for flags in (0, COLLAPSE):
        a = build(dv, g, U8, (100, 90, 80), (5, 6, 7), 0, flags)
        for d in (dv, other, dv):
            R.same(build(d, g, U8, (100, 90, 80), (5, 6, 7), 0, flags), a, ("again", flags))
            n += 1
    R.same(a, R.build(g.cpu().numpy(), (5, 6, 7), None, True), "the reference")
    print("determinism:", n, "builds on two contexts gave equal bytes")


# ---- magnitudes -------------------------------------------------------------------------------------------------------------------

def case_magnitudes():
    """One byte of 1 expanded with stride 0 to (2048, 1024, 1023) [x, y, z]: 2 146 435 072 voxels, every read a cache hit."""
    dv = hip.DeviceVoxelizer(0)
    dims = (2048, 1024, 1023)
    one = torch.ones((1, 1, 1), dtype=torch.uint8, device=DEV).expand(dims[2], dims[1], dims[0])
    want_counts, want_listed = R.solid_box_counts((0, 0, 0), dims, None, True)
    assert len(want_counts) == 11 and want_counts[:2] == [1, 2] and want_counts[10] == 1024 * 512 and want_listed == 4 * 1024 * 512
    t0 = time.time()
    tree = dense.build_octree(dv, one, coords=True)
    took = time.time() - t0
    got = [b - a for a, b in zip(tree.level_offsets, tree.level_offsets[1:])]
    assert tree.depth == 11 and got == want_counts and tree.voxels_listed == want_listed, (got, want_counts, tree.voxels_listed, want_listed)
    # the last level: the cells of the layer z = 1022, every one the lower half of a block; their voxel indices rise by 4
    valid, full, first, coords = (a.cpu().numpy() for a in dense.octree_level(tree, 10))
    assert (valid == 0x0f).all() and (full == 0x0f).all() and (coords[:, 2] == 1022).all() and np.array_equal(first, 4 * np.arange(len(first), dtype=np.int64))
    pts = dev(np.array([[0, 0, 0], [2047, 1023, 1022], [2047, 1023, 1023], [0, 1024, 0], [2046, 1022, 1021]], np.int32))
    hit = dense.octree_lookup(dv, tree, pts).cpu().numpy()
    assert hit[:, 0].tolist() == [1, 1, 0, 0, 1] and hit[0].tolist() == [1, 1, 1, -1] and hit[1, 1] == 10 and hit[1, 3] == want_listed - 1 and hit[4, 3] == -1
    ms = dv.octree_times()
    print("magnitudes: 2 146 435 072 voxels,", sum(got), "nodes,", want_listed, "voxels listed; classify %.1f, pyramid %.1f, order %.1f, write %.1f ms; %.2f s" % (ms + (took,)))


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------

def indexed(verts):
    positions, faces = np.unique(np.asarray(verts, np.float32).reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    return dev(positions.view(np.float32)), dev(faces.reshape(-1, 3).astype(np.int32))


def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, *indexed(meshes.scan_like()))
    labels, origin = dense.voxelize_dense(dv, 128, fmt="labels", fill=True)
    solid = labels != 0
    palette = [0] + [0xff000000 | (i * 0x010307 & 0xffffff) for i in range(1, 256)]
    for collapse in (True, False):
        tree = dense.build_octree(dv, labels, origin=origin, collapse=collapse, coords=True)
        R.same(as_ref(tree), R.build(solid.cpu().numpy(), origin, None, collapse), ("scan_like at 128", collapse))
        assert torch.equal(dense.octree_to_dense(dv, tree, labels.shape, origin=origin), solid)
    # (collapse=False) colours attached through to_voxels + octree_lookup: every solid voxel has a slot, each slot once
    rec = dense.to_voxels(dv, labels, origin=origin, palette=palette)
    hit = dense.octree_lookup(dv, tree, rec[:, :3].contiguous())
    assert tree.voxels_listed == len(rec) == int(solid.sum()) and bool((hit[:, 0] == 1).all()) and bool((hit[:, 1] == tree.depth - 1).all())
    slots = hit[:, 3].long()
    assert torch.equal(torch.sort(slots).values, torch.arange(len(rec), device=DEV))
    argb = torch.zeros(tree.voxels_listed, dtype=torch.int32, device=DEV).scatter_(0, slots, rec[:, 3])
    # ... read back node by node: the voxel at first_child + rank of octant o of a last-level node has its label's colour
    valid, _, first, coords = dense.octree_level(tree, tree.depth - 1)
    pal = torch.tensor(palette, dtype=torch.int64, device=DEV).to(torch.int32)
    o3 = torch.tensor(origin, device=DEV)
    checked = 0
    for o in range(8):
        has = (valid.int() >> o & 1) == 1
        rank = torch.zeros_like(first)
        for b in range(o):
            rank += valid.int() >> b & 1
        c = coords[has] + torch.tensor([o & 1, o >> 1 & 1, o >> 2], dtype=torch.int32, device=DEV) - o3
        assert torch.equal(argb[(first + rank)[has].long()], pal[labels[c[:, 2].long(), c[:, 1].long(), c[:, 0].long()].long()])
        checked += int(has.sum())
    assert checked == len(rec)
    # level D - 2 (cells of side 4) is the occupancy at 1 / 4: downsample's "any"
    coarse, corigin = dense.downsample(dv, labels, 4, origin=origin, reduce="any")
    cells = dense.octree_level(tree, tree.depth - 2)[3] // 4 - torch.tensor(corigin, dtype=torch.int32, device=DEV)
    occ = torch.zeros_like(coarse)
    occ[cells[:, 2].long(), cells[:, 1].long(), cells[:, 0].long()] = True
    assert torch.equal(occ, coarse) and len(cells) == int(coarse.sum())
    print("pipeline: scan_like at 128, filled:", len(rec), "voxels,", len(tree.valid), "nodes,", len(cells), "cells of side 4 = downsample(4, any); colours attached")


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
    want = R.build(g_np, (0, 0, 0), None, True)
    N = len(want["valid"])
    grid, short, byte = dev(g_np), dev(g_np[:n // 2]), torch.zeros((1, 1, 1), dtype=torch.uint8, device=DEV)
    f32 = dev(g_np.astype(np.float32))
    host_grid = g_np.copy()
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
    def no_build(code, what, ctx=dv._ctx, p=grid.data_ptr(), fmt=U8, strides=s, dm=dims, level=0.0, origin=(0, 0, 0), depth=0, flags=COLLAPSE, outs=(1, 1, 1, 1)):
        d, counts, nodes, listed = C.c_uint32(99), (C.c_uint64 * 16)(*([99] * 16)), C.c_uint64(99), C.c_uint64(99)
        rc = L.o2v_hip_octree_build(ctx, p, fmt, u64(strides), u3(dm), level, u3(origin), depth, flags, C.byref(d) if outs[0] else None,
                                    counts if outs[1] else None, C.byref(nodes) if outs[2] else None, C.byref(listed) if outs[3] else None)
        assert rc == code and d.value == nodes.value == listed.value == 99 and list(counts) == [99] * 16, (what, rc)
        note("o2v_hip_octree_build", what, ctx)

    for what, kw in [
        ("null context", dict(ctx=None)), ("null grid", dict(p=None)), ("null strides", dict(strides=None)), ("null dims", dict(dm=None)),
        ("zero dims", dict(dm=(n, 0, n))), ("unknown format", dict(fmt=3)), ("a BITS grid with x stride 2", dict(fmt=BITS, strides=(2, n, n * n))),
        ("a level that is not finite", dict(p=f32.data_ptr(), fmt=F32, level=float("nan"))), ("short grid", dict(p=short.data_ptr())),
        ("host grid", dict(p=host_grid.ctypes.data)), ("null origin", dict(origin=None)), ("depth 17", dict(depth=17)),
        ("origin + dims above 2^depth", dict(depth=4)), ("origin + dims above 2^depth with an origin", dict(origin=(9, 0, 0), depth=5)),
        ("unknown flag bits", dict(flags=COLLAPSE | 1)), ("null out_depth", dict(outs=(0, 1, 1, 1))), ("null level_counts", dict(outs=(1, 0, 1, 1))),
        ("null out_nodes", dict(outs=(1, 1, 0, 1))), ("null out_voxels_listed", dict(outs=(1, 1, 1, 0))),
    ]:
        no_build(3, what, **kw)
    for what, kw in [
        ("65 537 voxels along x", dict(p=byte.data_ptr(), dm=(65537, 1, 1), strides=(0, 0, 0))),
        ("2^31 voxels", dict(p=byte.data_ptr(), dm=(1024, 1024, 2048), strides=(0, 0, 0))),
        ("origin + dims above 65 536", dict(origin=(65536 - n + 1, 0, 0))), ("origin + dims above 65 536 with a depth", dict(origin=(0, 65530, 0), depth=16)),
    ]:
        no_build(5, what, **kw)
    # -- write: before any build, then with arrays that are short, on the host, misaligned or overlapping
    valid, full = (torch.full((N,), GUARD, dtype=torch.uint8, device=DEV) for _ in range(2))
    first, coords = torch.full((N,), -77, dtype=torch.int32, device=DEV), torch.full((N, 3), -77, dtype=torch.int32, device=DEV)
    both = torch.full((2 * N,), GUARD, dtype=torch.uint8, device=DEV)
    short8, short32 = torch.zeros(N - 1, dtype=torch.uint8, device=DEV), torch.zeros(N - 1, dtype=torch.int32, device=DEV)
    host8 = np.zeros(N, np.uint8)
    torch.cuda.synchronize()

    def no_write(what, ctx=dv._ctx, v=valid.data_ptr(), f=full.data_ptr(), fc=first.data_ptr(), co=coords.data_ptr()):
        assert L.o2v_hip_octree_write(ctx, v, f, fc, co) == 3, what
        note("o2v_hip_octree_write", what, ctx)
        assert bool((valid == GUARD).all()) and bool((full == GUARD).all()) and bool((first == -77).all()) and bool((coords == -77).all()) and bool((both == GUARD).all())

    no_write("write without a build")
    assert "no o2v_hip_octree_build" in msgs[-1]
    no_build(3, "a refused build leaves no tree", depth=17)
    no_write("write after a refused build")
    assert "no o2v_hip_octree_build" in msgs[-1]
    got = build(dv, grid, U8, dims, (0, 0, 0), 0, COLLAPSE)
    R.same(got, want, "after the refusals")
    for what, kw in [
        ("null context", dict(ctx=None)), ("null valid", dict(v=None)), ("null full", dict(f=None)), ("null first_child", dict(fc=None)),
        ("first_child not 4-byte aligned", dict(fc=first.data_ptr() + 2)), ("coords not 4-byte aligned", dict(co=coords.data_ptr() + 1)),
        ("short valid", dict(v=short8.data_ptr())), ("short first_child", dict(fc=short32.data_ptr())), ("short coords", dict(co=first.data_ptr())),
        ("host full", dict(f=host8.ctypes.data)), ("valid and full overlap", dict(v=both.data_ptr(), f=both.data_ptr() + N - 1)),
        ("first_child and coords overlap", dict(fc=coords.data_ptr() + 8 * N)),
    ]:
        no_write(what, **kw)
    # -- lookup and to_dense: the tree arguments, then their own
    tv, tf, tfc = dev(want["valid"]), dev(want["full"]), dev(want["first_child"])
    pts = dev(box_points(0, 4))
    P = len(pts)
    res = torch.full((P, 4), -77, dtype=torch.int32, device=DEV)
    out = torch.full((n, n, n), 9, dtype=torch.uint8, device=DEV)
    host_pts = np.zeros((P, 3), np.int32)
    torch.cuda.synchronize()

    def no_query(code, what, which, ctx=dv._ctx, v=tv.data_ptr(), f=tf.data_ptr(), fc=tfc.data_ptr(), nodes=N, depth=5, flags=COLLAPSE, p=pts.data_ptr(), np_=P,
                 r=res.data_ptr(), origin=(0, 0, 0), dm=dims, o=out.data_ptr(), strides=s):
        if which == "lookup":
            rc = L.o2v_hip_octree_lookup(ctx, v, f, fc, nodes, depth, flags, p, np_, r)
        else:
            rc = L.o2v_hip_octree_to_dense(ctx, v, f, fc, nodes, depth, flags, u3(origin), u3(dm), o, u64(strides))
        assert rc == code, (what, which, rc)
        note("o2v_hip_octree_" + which, which + ": " + what, ctx)
        assert bool((res == -77).all()) and bool((out == 9).all())

    for which in ("lookup", "to_dense"):
        for what, kw in [
            ("null context", dict(ctx=None)), ("null valid", dict(v=None)), ("null first_child", dict(fc=None)), ("depth 0", dict(depth=0)), ("depth 17", dict(depth=17)),
            ("unknown flag bits", dict(flags=2)), ("n_nodes 0", dict(nodes=0)), ("first_child not 4-byte aligned", dict(fc=tfc.data_ptr() + 1)),
            ("n_nodes past the arrays", dict(nodes=N + 1)), ("host valid", dict(v=host8.ctypes.data)),
        ]:
            no_query(3, what, which, **kw)
        no_query(5, "n_nodes 2^31", which, nodes=2 ** 31)
    for what, kw in [
        ("null points", dict(p=None)), ("null out", dict(r=None)), ("short points", dict(np_=P + 1)), ("host points", dict(p=host_pts.ctypes.data)),
        ("out not 4-byte aligned", dict(r=res.data_ptr() + 2)), ("out overlaps points", dict(r=pts.data_ptr(), np_=2)), ("out overlaps the tree", dict(r=tfc.data_ptr(), np_=1)),
    ]:
        no_query(3, what, "lookup", **kw)
    no_query(5, "2^31 points", "lookup", np_=2 ** 31)
    assert L.o2v_hip_octree_lookup(dv._ctx, tv.data_ptr(), tf.data_ptr(), tfc.data_ptr(), N, 5, COLLAPSE, None, 0, None) == 0   # no points: nothing to do
    for what, kw in [
        ("null origin", dict(origin=None)), ("null dims", dict(dm=None)), ("null out", dict(o=None)), ("null strides", dict(strides=None)), ("zero dims", dict(dm=(n, n, 0))),
        ("strides that map two voxels to one element", dict(strides=(1, n, 0))), ("short out", dict(dm=(n, n, n + 1))), ("host out", dict(o=host_grid.ctypes.data)),
        ("out overlaps the tree", dict(o=tv.data_ptr(), dm=(4, 1, 1))),
    ]:
        no_query(3, what, "to_dense", **kw)
    for what, kw in [("65 537 voxels along y", dict(dm=(1, 65537, 1))), ("2^31 voxels", dict(dm=(1024, 1024, 2048))), ("origin + dims above 2^32", dict(origin=(0, 2 ** 32 - n + 1, 0)))]:
        no_query(5, what, "to_dense", **kw)
    for t in msgs:
        what, _, err = t.partition(": o2v_hip")
        assert "overlap" not in what or "overlap" in err, t
    assert L.o2v_hip_octree_times(None, None) == 3
    # then correct calls: the context still works
    R.same(build(dv, grid, U8, dims, (0, 0, 0), 0, COLLAPSE), want, "at the end")
    dv.octree_lookup(tv.data_ptr(), tf.data_ptr(), tfc.data_ptr(), N, 5, COLLAPSE, pts.data_ptr(), P, res.data_ptr())
    assert np.array_equal(res.cpu().numpy(), R.lookup(want, pts.cpu().numpy()))
    dv.octree_to_dense(tv.data_ptr(), tf.data_ptr(), tfc.data_ptr(), N, 5, COLLAPSE, (0, 0, 0), dims, out.data_ptr(), s)
    assert np.array_equal(out.cpu().numpy() != 0, g_np)
    print("\n".join(msgs))
    assert len(msgs) == 80
    print("refused", len(msgs), "calls")


# ---- one call per case and its wall time ------------------------------------------------------------------------------------------

CASES = {"shapes_and_layouts": case_shapes_and_layouts, "block_edges": case_block_edges, "queries": case_queries, "determinism": case_determinism,
         "magnitudes": case_magnitudes, "pipeline": case_pipeline, "refusals": case_refusals}

if __name__ == "__main__":
    t0 = time.time()
    CASES[sys.argv[1]]()
    print("case", sys.argv[1], "took %.1f s" % (time.time() - t0))
    print("ok")
