"""The GPU cases of tests/test_gpu_labelmesh.py, each run in a child process of its own: `python -m tests.labelmesh_cases <case>`.

torch is imported before the library is loaded (the grids are torch tensors; see tests/dense_cases.py).  Every comparison with the
numpy reference of tests/labelmesh_ref.py is np.array_equal - on the bits of the float32 positions too - and there is no tolerance
anywhere.  The limits at 2^31 vertices or triangles cannot be reached by a grid that runs in seconds (2^31 active cells need as
many samples): they are checked by reading o2v_dev_host_k29_label_surface.hpp, where the counts are compared with kSurfMaxVertices
before anything is written.  A case prints what it covered and "ok" last when everything held."""
import os
import sys
import tempfile
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import labelmesh_ref as R

DEV = torch.device("cuda", 0)
I32, U8 = hip.LABELS_I32, hip.LABELS_U8
CLOSED = hip.LABEL_SURFACE_CLOSED
GUARD = -7
NAMES = ("positions", "faces", "pairs", "cells", "links")
MODE = "every row re-read through L2" if os.environ.get("O2V_LSF_NO_TILE") == "1" else "the tile in LDS"   # (k_lsf_classify / k_lsf_classify_tile)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def st(t):
    """(x, y, z) element strides of a tensor [z, y, x]."""
    return t.stride(2), t.stride(1), t.stride(0)


def fmt_of(t):
    return I32 if t.dtype == torch.int32 else U8


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(mesh, want, what):
    """A LabelMesh against the reference's (positions, faces, pairs, cells, links), bit for bit."""
    for name, w in zip(NAMES, want):
        got = getattr(mesh, name).cpu().numpy()
        assert got.dtype == w.dtype and got.shape == w.shape, (what, name, got.dtype, got.shape, w.dtype, w.shape)
        bad = np.argwhere(bits(got) != bits(w))
        assert not len(bad), (what, name, len(bad), "elements differ, the first at", bad[0].tolist(), got[tuple(bad[0])], w[tuple(bad[0])])


def layouts(g):
    """name -> tensor view on the device: the grid g [z, y, x] in every layout of the cases."""
    nz, ny, nx = g.shape
    t = dev(g)
    out = {"contiguous": t}
    wide = torch.zeros((nz, ny, 2 * nx), dtype=t.dtype, device=DEV)
    wide[:, :, ::2] = t
    out["x step 2"] = wide[:, :, ::2]
    out["x and z swapped"] = t.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    big = torch.full((nz + 2, ny + 3, nx + 5), 3, dtype=torch.uint8, device=DEV).to(t.dtype)   # (rows not aligned for 16-byte loads)
    big[1:1 + nz, 2:2 + ny, 3:3 + nx] = t
    out["a view inside a larger tensor"] = big[1:1 + nz, 2:2 + ny, 3:3 + nx]
    return out


def grid_of(rng, dims, kind):
    if kind == "int32":
        return R.random_labels(rng, dims, (0, 5, R.INT32_MAX, -3))
    if kind == "uint8":
        return R.random_labels(rng, dims, (0, 1, 200, 255), np.uint8)
    return R.random_labels(rng, dims, (0, 1)).astype(bool)


def raw(dv, t, closed, slack=0):
    """The C-level count and write on the view t into arrays with `slack` more rows, filled with a guard: (cells, links, faces,
    pairs) as numpy, the guard rows checked and cut off."""
    nz, ny, nx = t.shape
    args = (t.data_ptr(), fmt_of(t), st(t), (nx, ny, nz), CLOSED if closed else 0)
    torch.cuda.synchronize()
    V, Q = dv.label_surface_count(*args)
    arrays = [torch.full((n + slack, w), GUARD, dtype=torch.int32, device=DEV) for n, w in ((V, 3), (V, 6), (2 * Q, 3), (Q, 2))]
    torch.cuda.synchronize()
    dv.label_surface_write(*args, arrays[0].data_ptr(), arrays[1].data_ptr(), V + slack, arrays[2].data_ptr(), arrays[3].data_ptr(), Q + slack // 2)
    out = []
    for a, n in zip(arrays, (V, V, 2 * Q, Q)):
        a = a.cpu().numpy()
        assert (a[n:] == GUARD).all(), "written past the counted rows"
        out.append(a[:n])
    return out


# ---- shapes and layouts -----------------------------------------------------------------------------------------------------------

def case_shapes_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2911)
    yz = [(1, 1), (2, 3), (3, 5), (5, 2), (1, 3), (5, 1), (2, 2), (3, 3), (1, 5), (5, 5)]
    calls = grids = 0
    for n, nx in enumerate((1, 2, 3, 62, 63, 64, 65, 66, 127, 129)):
        for ny, nz in (yz[n], yz[(n + 3) % 10]):
            for kind in ("int32", "uint8", "bool"):
                g = grid_of(rng, (nx, ny, nz), kind)
                views = layouts(g)
                for closed in (True, False):
                    origin = (7, 0, 65535 - nz - closed) if closed else (0, 3, 1)
                    want = R.label_surfaces(g, origin, closed, iterations=2)
                    for name, t in views.items():
                        assert t.shape == g.shape and np.array_equal(t.cpu().numpy(), g), (nx, ny, nz, kind, name)
                        same(dense.label_surfaces(dv, t, origin=origin, closed=closed, iterations=2), want, ((nx, ny, nz), kind, name, closed))
                        calls += 1
                grids += 1
    # nothing active: empty tensors of the right shapes
    empty = dense.label_surfaces(dv, torch.full((3, 4, 5), 9, dtype=torch.int32, device=DEV), closed=False, iterations=3)
    assert [tuple(getattr(empty, n).shape) for n in NAMES] == [(0, 3), (0, 3), (0, 2), (0, 3), (0, 6)]
    assert len(dv.label_surface_times()) == 5 and all(v >= 0 for v in dv.label_surface_times())
    print("shapes_and_layouts: compared", calls, "calls on", grids, "grids in 4 layouts with", MODE)


# ---- block ends -------------------------------------------------------------------------------------------------------------------

def case_block_ends():
    dv = hip.DeviceVoxelizer(0)
    nx, ny, nz = 130, 9, 15
    z, y, x = np.indices((nz, ny, nx))
    grids = {"checkerboard of 2": ((x + y + z) % 2).astype(np.uint8), "checkerboard of 3": ((x + y + z) % 3).astype(np.int32)}
    for closed in (True, False):
        # voxels at the two ends of the first and the last word of every block of 256 words of the extended lattice
        E = int(closed)
        X, Y, Z = nx + 2 * E, ny + 2 * E, nz + 2 * E
        W = (X + 63) // 64
        items = W * Y * Z
        assert items > 256
        g = np.zeros((nz, ny, nx), np.int32)
        for item in sorted({0, items - 1} | {b + d for b in range(256, items, 256) for d in (-1, 0)}):
            w, row = item % W, item // W
            for xe in (64 * w, min(64 * w + 63, X - 1)):
                c = (xe - E, row % Y - E, row // Y - E)
                if 0 <= c[0] < nx and 0 <= c[1] < ny and 0 <= c[2] < nz:
                    g[c[2], c[1], c[0]] = 1 + item % 3
        assert g.any()
        grids[f"block ends, closed={closed}"] = g
    n = 0
    for name, g in grids.items():
        for closed in (True, False):
            want = R.net(g, closed)
            got = raw(dv, dev(g), closed, slack=4)
            for a, b, what in zip(got, want, ("cells", "links", "faces", "pairs")):
                assert a.shape == b.shape and np.array_equal(a, b), (name, closed, what)
            if "checkerboard" in name and not closed:
                assert len(got[0]) == (nx - 1) * (ny - 1) * (nz - 1), "every cell is active"
                assert len(got[3]) == (nx - 1) * (ny - 2) * (nz - 2) + (nx - 2) * (ny - 1) * (nz - 2) + (nx - 2) * (ny - 2) * (nz - 1), "every interior edge is a quad"
            same(dense.label_surfaces(dv, dev(g), closed=closed, iterations=3), R.label_surfaces(g, (0, 0, 0), closed, 3), (name, closed))
            n += 1
    print("block_ends: compared", n, "nets on 130 x 9 x 15 with", MODE)


# ---- against K10, K14 and K24 -----------------------------------------------------------------------------------------------------

def case_against_k10():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2913)
    n = 0
    for dims in ((70, 21, 13), (64, 2, 9), (129, 5, 3)):
        nx, ny, nz = dims
        z, y, x = np.indices((nz, ny, nx))
        for g in (rng.random((nz, ny, nx)) < 0.4, (x - nx / 2) ** 2 / 16 + (y - ny / 2) ** 2 + (z - nz / 2) ** 2 < 3):
            t = dev(g)
            mesh = dense.label_surfaces(dv, t, closed=False)
            field = torch.where(t, -1.0, 1.0).to(torch.float32)
            positions, faces = dense.extract_surface(dv, field, 0.0)
            assert mesh.positions.shape[0] == positions.shape[0] and torch.equal(mesh.faces, faces), dims
            assert mesh.faces.shape[0] > 0
            n += 1
    print("against_k10:", n, "bool grids, the faces and the vertex count of extract_surface")


def case_against_adjacency():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2914)
    n = 0
    for dims, k in (((37, 21, 13), 5), ((66, 7, 9), 40)):
        g = rng.integers(0, k + 1, dims[::-1]).astype(np.int32)
        t = dev(g)
        mesh = dense.label_surfaces(dv, t)
        adj = dense.label_adjacency(dv, t, k)
        want = {(int(b), int(a)): int(f) for (a, b), f in zip(adj.pairs.cpu().numpy(), adj.faces.cpu().numpy()) if f}
        got = {pr: c for pr, c in R.pair_counts(mesh.pairs.cpu().numpy()).items() if pr[1] != 0}
        assert got == want and len(got) > 5, dims
        assert R.pair_counts(mesh.pairs.cpu().numpy()) == R.face_contacts(g)
        n += 1
    for g in (rng.random((13, 21, 70)) < 0.4, np.ones((3, 4, 5), bool)):
        t = dev(g)
        mesh = dense.label_surfaces(dv, t)
        assert mesh.pairs.shape[0] == dense.count_faces(dv, t, merge="none") > 0
        n += 1
    print("against_adjacency:", n, "grids, the faces of label_adjacency and of count_faces")


# ---- invariants -------------------------------------------------------------------------------------------------------------------

def case_invariants():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2915)
    z, y, x = np.indices((20, 30, 40))
    blobs = np.zeros((20, 30, 40), np.int32)
    for label, (cx, cy, cz, r) in enumerate(((12, 12, 9, 9), (24, 14, 10, 8), (20, 22, 12, 7)), 1):
        blobs[((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 < r * r) & (blobs == 0)] = label
    n = 0
    for name, g in (("random", R.random_labels(rng, (23, 9, 11), (0, 1, 2, -4))), ("three balls that touch", blobs)):
        mesh = dense.label_surfaces(dv, dev(g), origin=(2, 0, 5))
        smooth = dense.relax_surface(dv, mesh, 6)
        for label in np.unique(g).tolist():
            p, f = dense.part_mesh(mesh, label)
            assert p.dtype == torch.float32 and f.dtype == torch.int32 and int(f.max()) == p.shape[0] - 1 and int(f.min()) == 0
            assert len(np.unique(f.cpu().numpy())) == p.shape[0], "an unused vertex"
            assert (R.edge_uses(f.cpu().numpy())[1] % 2 == 0).all(), (name, label)
            want_p, want_f = R.part_mesh(mesh.positions.cpu().numpy(), mesh.faces.cpu().numpy(), mesh.pairs.cpu().numpy(), label)
            assert np.array_equal(p.cpu().numpy(), want_p) and np.array_equal(f.cpu().numpy(), want_f), (name, label)
            if label:
                assert R.signed_volume(p.cpu().numpy(), f.cpu().numpy()) == float((g == label).sum()), (name, label)
                ps, fs = dense.part_mesh(smooth, label)
                assert torch.equal(fs, f) and 0 < R.signed_volume(ps.cpu().numpy(), fs.cpu().numpy()) < float((g == label).sum())
            n += 1
        assert np.array_equal(R.link_edges(mesh.links.cpu().numpy()), R.quad_edges(mesh.faces.cpu().numpy())), name
        p, f = dense.part_mesh(mesh, 77)
        assert p.shape == (0, 3) and f.shape == (0, 3)
    print("invariants:", n, "part meshes closed, their volumes the voxel counts")


# ---- relax ------------------------------------------------------------------------------------------------------------------------

def case_relax():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2916)
    z, y, x = np.indices((21, 26, 33))
    g = ((x - 16) ** 2 + (y - 13) ** 2 + (z - 10) ** 2 < 81).astype(np.int32)
    g[(g == 1) & (x > 18)] = 2
    g[rng.random(g.shape) < 0.02] = 3                       # and noise: single voxels collapse
    origin = (100, 0, 17)
    t = dev(g)
    mesh = dense.label_surfaces(dv, t, origin=origin)
    cells, links = mesh.cells.cpu().numpy(), mesh.links.cpu().numpy()
    centre = R.centres(cells, origin)
    n = 0
    for iterations in (1, 2, 7):
        for relaxation in (0.3, 0.5, 1.0):
            for reach in (0.5, 0.25):
                want = R.relax(cells, links, origin, iterations, relaxation, reach)
                again = dense.relax_surface(dv, mesh, iterations, relaxation=relaxation, reach=reach)
                inside = dense.label_surfaces(dv, t, origin=origin, iterations=iterations, relaxation=relaxation, reach=reach)
                got = again.positions.cpu().numpy()
                assert np.array_equal(bits(got), bits(want)), (iterations, relaxation, reach)
                assert torch.equal(again.positions, inside.positions) and torch.equal(again.faces, inside.faces) and again.links is mesh.links
                assert (np.abs(got - centre) <= np.float32(reach)).all()
                n += 1
    assert np.array_equal(bits(dense.relax_surface(dv, mesh, 0).positions.cpu().numpy()), bits(centre))
    # links from anywhere: below 0, -2, at and above the number of vertices - no link, never followed
    V = len(cells)
    wild = links.copy()
    pick = rng.random(wild.shape)
    wild[pick < 0.1] = -2
    wild[(pick >= 0.1) & (pick < 0.2)] = V
    wild[(pick >= 0.2) & (pick < 0.3)] = R.INT32_MAX
    wild[(pick >= 0.3) & (pick < 0.4)] = -2 ** 31
    wild[(pick >= 0.4) & (pick < 0.5)] = rng.integers(0, V, int(((pick >= 0.4) & (pick < 0.5)).sum()))   # and links across the net
    out = torch.full((V + 1, 3), float(GUARD), dtype=torch.float32, device=DEV)
    wl = dev(wild)
    torch.cuda.synchronize()
    for iterations in (1, 4):
        dv.label_surface_relax(mesh.cells.data_ptr(), wl.data_ptr(), V, origin, iterations, 0.5, 0.5, out.data_ptr())
        got = out.cpu().numpy()
        assert (got[V] == GUARD).all() and np.array_equal(bits(got[:V]), bits(R.relax(cells, wild, origin, iterations))), iterations
    print("relax: compared", n, "settings and 2 calls with links from anywhere on", V, "vertices")


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------

def indexed(verts):
    positions, faces = np.unique(np.asarray(verts, np.float32).reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    return dev(positions.view(np.float32)), dev(faces.reshape(-1, 3).astype(np.int32))


def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, *indexed(meshes.scan_like()))
    solid, origin = dense.voxelize_dense(dv, 64, fill=True)
    parts, n = dense.split_parts(dv, solid)
    assert n >= 2
    g = parts.cpu().numpy()
    blocky = dense.label_surfaces(dv, parts, origin=origin)
    same(blocky, R.label_surfaces(g, origin), "the parts of scan_like at 64")
    pairs, areas = dense.interface_areas(blocky)
    counts = R.pair_counts(blocky.pairs.cpu().numpy())
    assert pairs.dtype == torch.int32 and areas.dtype == torch.float64
    assert [tuple(p) for p in pairs.tolist()] == sorted(counts) and areas.tolist() == [float(counts[k]) for k in sorted(counts)]
    mesh = dense.label_surfaces(dv, parts, origin=origin, iterations=4)
    same(mesh, R.label_surfaces(g, origin, iterations=4), "the parts of scan_like at 64, 4 iterations")
    _, smooth_areas = dense.interface_areas(mesh)
    assert float(smooth_areas.sum()) < float(areas.sum())
    with tempfile.TemporaryDirectory() as tmp:
        for label in range(1, n + 1):
            p, f = dense.part_mesh(mesh, label)
            assert f.shape[0] > 0 and (R.edge_uses(f.cpu().numpy())[1] % 2 == 0).all(), label
            path = os.path.join(tmp, f"part{label}.ply")
            dense.save_mesh(path, p, f)
            assert os.path.getsize(path) > 12 * p.shape[0]
    # one part back into the voxelizer: its mesh lies in the voxel space of resolution 64
    label = int(np.bincount(g[g > 0]).argmax())
    p, f = dense.part_mesh(blocky, label)
    dense.set_mesh(dv, p, f)
    again, _ = dense.voxelize_dense(dv, 64, fill=True)      # (the part alone now fills the cube: more voxels than it had)
    assert int((again != 0).sum()) >= int((g == label).sum())
    print(f"pipeline: scan_like at 64: {n} parts, {mesh.positions.shape[0]} vertices, {mesh.pairs.shape[0]} quads, {len(counts)} interfaces; part {label} voxelized again")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list but the failed scratch allocation.  This child runs with torch's caching allocator off:
    each tensor is an allocation of its own, so a short one is short."""
    dv = hip.DeviceVoxelizer(0)
    L = hip._bind()
    C = hip.C
    n = 24
    dims, s = (n, n, n), (1, n, n * n)
    rng = np.random.default_rng(2918)
    g_np = R.random_labels(rng, dims, (0, 1, 2))
    want = R.net(g_np)
    V, Q = len(want[0]), len(want[3])
    lab, lab8 = dev(g_np), dev(g_np.astype(np.uint8))
    cells, links = torch.full((V, 3), GUARD, dtype=torch.int32, device=DEV), torch.full((V, 6), GUARD, dtype=torch.int32, device=DEV)
    faces, pairs = torch.full((2 * Q, 3), GUARD, dtype=torch.int32, device=DEV), torch.full((Q, 2), GUARD, dtype=torch.int32, device=DEV)
    pos = torch.full((V, 3), float(GUARD), dtype=torch.float32, device=DEV)
    short = torch.full((n // 2, n, n), 5, dtype=torch.int32, device=DEV)
    short_out = torch.full((V, 2), GUARD, dtype=torch.int32, device=DEV)
    shared = torch.full((n ** 3 + 6 * V + 8,), 5, dtype=torch.int32, device=DEV)   # the grid and an output in one allocation
    host_grid, host_out = g_np.copy(), np.zeros((V, 6), np.int32)
    torch.cuda.synchronize()
    G, S = lab.data_ptr(), shared.data_ptr()
    u3 = lambda a: None if a is None else (C.c_uint32 * 3)(*a)    # noqa: E731
    u64 = lambda a: None if a is None else (C.c_uint64 * 3)(*a)   # noqa: E731
    msgs = []

    def untouched():
        assert all(bool((a == GUARD).all()) for a in (cells, links, faces, pairs, pos, short_out)) and bool((shared == 5).all())
        assert np.array_equal(lab.cpu().numpy(), g_np)

    def note(what, fn, ctx=True):
        if ctx:
            msgs.append(what + ": " + L.o2v_hip_last_error(dv._ctx).decode())
            assert fn in msgs[-1], msgs[-1]
        untouched()

    def count(grid=G, fmt=I32, strides=s, dm=dims, flags=CLOSED, ctx=dv._ctx, out=(True, True)):
        v, q = C.c_uint64(99), C.c_uint64(99)
        rc = L.o2v_hip_label_surface_count(ctx, grid, fmt, u64(strides), u3(dm), flags, C.byref(v) if out[0] else None, C.byref(q) if out[1] else None)
        return rc, v.value, q.value

    def write(grid=G, fmt=I32, strides=s, dm=dims, flags=CLOSED, ctx=dv._ctx, c=cells.data_ptr(), l=links.data_ptr(), vcap=V, f=faces.data_ptr(),
              p=pairs.data_ptr(), qcap=Q):
        return L.o2v_hip_label_surface_write(ctx, grid, fmt, u64(strides), u3(dm), flags, c, l, vcap, f, p, qcap)

    def relax(c=cells.data_ptr(), l=links.data_ptr(), nv=V, origin=(0, 0, 0), it=2, relaxation=0.5, reach=0.5, p=pos.data_ptr(), ctx=dv._ctx):
        return L.o2v_hip_label_surface_relax(ctx, c, l, nv, u3(origin), it, relaxation, reach, p)

    # a write before any count
    assert write() == 3
    note("write before any count", "no matching o2v_hip_label_surface_count")
    for what, code, kw in [
        ("null context", 3, dict(ctx=None)), ("null grid", 3, dict(grid=None)), ("null strides", 3, dict(strides=None)), ("null dims", 3, dict(dm=None)),
        ("null out_vertices", 3, dict(out=(False, True))), ("null out_quads", 3, dict(out=(True, False))), ("zero dims", 3, dict(dm=(n, 0, n))),
        ("unknown format", 3, dict(fmt=2)), ("unknown flag bit", 3, dict(flags=2)), ("an int32 grid that is not 4-byte aligned", 3, dict(grid=G + 2)),
        ("short grid", 3, dict(grid=short.data_ptr())), ("host grid", 3, dict(grid=host_grid.ctypes.data)),
        ("65 535 samples along x, closed", 5, dict(dm=(65535, 1, 1), strides=(0, 0, 0))),
        ("65 537 samples along z, open", 5, dict(dm=(1, 1, 65537), strides=(0, 0, 0), flags=0)),
        ("the limit before the pointer", 5, dict(grid=host_grid.ctypes.data, dm=(1, 65535, 1), strides=(0, 0, 0))),
    ]:
        rc, v, q = count(**kw)
        assert rc == code and (v, q) == (99, 99), (what, rc, v, q)
        note(what, "o2v_hip_label_surface_count", kw.get("ctx", True))
        assert write() == 3, what                                                     # a refused count replaces the last one
        note(what + ", then write", "no matching o2v_hip_label_surface_count")
    assert count() == (0, V, Q)
    for what, kw in [
        ("null context", dict(ctx=None)), ("other flags than counted", dict(flags=0)), ("another format than counted", dict(grid=lab8.data_ptr(), fmt=U8)),
        ("other strides than counted", dict(strides=(1, n, 2 * n * n), dm=(n, n, n // 2))), ("vertex capacity below the count", dict(vcap=V - 1)),
        ("quad capacity below the count", dict(qcap=Q - 1)), ("null cells", dict(c=None)), ("null links", dict(l=None)), ("null faces", dict(f=None)),
        ("null pairs", dict(p=None)), ("links that are not 4-byte aligned", dict(l=links.data_ptr() + 2)),
        ("cells overlaps links", dict(c=links.data_ptr() + 12 * V)), ("pairs overlaps faces", dict(p=faces.data_ptr())),
        ("short links", dict(l=short_out.data_ptr())), ("host links", dict(l=host_out.ctypes.data)),
    ]:
        assert write(**kw) == 3, what
        note(what, "o2v_hip_label_surface_write", kw.get("ctx", True))
        assert "overlaps" not in what or "overlap" in msgs[-1].split(": ", 1)[1], msgs[-1]
    # the grid and an output in one allocation, overlapping in the last element of the grid
    shared[:n ** 3] = lab.reshape(-1)
    torch.cuda.synchronize()
    assert count(grid=S) == (0, V, Q)
    assert write(grid=S, l=S + 4 * n ** 3 - 4) == 3
    msgs.append("links overlap the grid's last element: " + L.o2v_hip_last_error(dv._ctx).decode())
    assert "overlap" in msgs[-1]
    assert bool((shared[n ** 3:] == 5).all())
    # ... and beside it: a correct call
    assert write(grid=S, l=S + 4 * n ** 3) == 0
    assert np.array_equal(shared[n ** 3:n ** 3 + 6 * V].cpu().numpy().reshape(V, 6), want[1]) and bool((shared[n ** 3 + 6 * V:] == 5).all())
    shared.fill_(5)
    for a, w in zip((cells, faces, pairs), (want[0], want[2], want[3])):
        assert np.array_equal(a.cpu().numpy(), w)
        a.fill_(GUARD)
    torch.cuda.synchronize()
    for what, code, kw in [
        ("null context", 3, dict(ctx=None)), ("null cells", 3, dict(c=None)), ("null links", 3, dict(l=None)), ("null positions", 3, dict(p=None)),
        ("null origin", 3, dict(origin=None)), ("relaxation 0", 3, dict(relaxation=0.0)), ("relaxation above 1", 3, dict(relaxation=1.5)),
        ("relaxation NaN", 3, dict(relaxation=float("nan"))), ("reach below 0", 3, dict(reach=-0.25)), ("reach above 0.5", 3, dict(reach=0.75)),
        ("reach NaN", 3, dict(reach=float("nan"))), ("positions that are not 4-byte aligned", 3, dict(p=pos.data_ptr() + 1)),
        ("positions overlap links", 3, dict(p=links.data_ptr())), ("short positions", 3, dict(p=short_out.data_ptr())),
        ("host positions", 3, dict(p=host_out.ctypes.data)), ("1025 iterations", 5, dict(it=1025)), ("2^31 vertices", 5, dict(nv=2 ** 31)),
        ("an origin above 65 536", 5, dict(origin=(0, 65537, 0))),
    ]:
        assert relax(**kw) == code, what
        note(what, "o2v_hip_label_surface_relax", kw.get("ctx", True))
        assert "overlap " not in what or "overlap" in msgs[-1].split(": ", 1)[1], msgs[-1]
    assert L.o2v_hip_label_surface_times(None, None) == 3
    # after all refusals the context still works
    same(dense.label_surfaces(dv, lab, iterations=2), R.label_surfaces(g_np, iterations=2), "after the refusals")
    print("\n".join(msgs))
    print("refused", len(msgs) + 3, "calls")   # (three with a null context leave no message)


# ---- one call per case and its wall time ------------------------------------------------------------------------------------------

CASES = {"shapes_and_layouts": case_shapes_and_layouts, "block_ends": case_block_ends, "against_k10": case_against_k10,
         "against_adjacency": case_against_adjacency, "invariants": case_invariants, "relax": case_relax, "pipeline": case_pipeline,
         "refusals": case_refusals}

if __name__ == "__main__":
    t0 = time.time()
    CASES[sys.argv[1]]()
    print("case", sys.argv[1], "took %.1f s" % (time.time() - t0))
    print("ok")
