"""The GPU cases of tests/test_gpu_rects.py, each run in a child process of its own: `python -m tests.rects_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison is np.array_equal on uint32 views of
positions, faces and colours against the numpy reference (tests/rects_ref.py) or a closed form, never against the code under
test.  A case prints what it compared and "ok" last when everything held."""
import os
import sys
import tempfile
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import components_ref as CR
from tests import faces_ref as FR
from tests import fill_ref
from tests import rects_ref as RR
from tests.faces_cases import mesh, same
from tests.gather_cases import FMT, grid_args
from tests.raycast_cases import dev, expect_code, formats, layouts

DEV = torch.device("cuda", 0)
F = np.float32


def blocky(dims, cell, values):
    """[z, y, x] of dims (nx, ny, nz): `values(shape)` drawn on a coarse grid of cells (cx, cy, cz) voxels large - flat walls
    that end off the word, block and row boundaries."""
    coarse = values(tuple(-(-n // c) for n, c in zip(dims[::-1], cell[::-1])))
    for axis, c in enumerate(cell[::-1]):
        coarse = np.repeat(coarse, c, axis=axis)
    return np.ascontiguousarray(coarse[:dims[2], :dims[1], :dims[0]])


def blocky_solid(rng, dims, density=0.6, cell=(5, 3, 2)):
    return blocky(dims, cell, lambda shape: rng.random(shape) < density)


def by_key(rows, dims):
    """Rectangles (x, y, z, d, length, height, argb) in the contract's order."""
    r = np.asarray(rows, np.int64).reshape(-1, 7)
    return r[np.argsort(((r[:, 2] * dims[1] + r[:, 1]) * 6 + r[:, 3]) * dims[0] + r[:, 0], kind="stable")]


def box_rects(a, b, c, argb=0xFFFFFFFF):
    """The six rectangles of the all-solid box of (a, b, c) voxels."""
    return by_key([(0, 0, 0, 0, b, c, argb), (a - 1, 0, 0, 1, b, c, argb), (0, 0, 0, 2, a, c, argb), (0, b - 1, 0, 3, a, c, argb),
                   (0, 0, 0, 4, a, b, argb), (0, 0, c - 1, 5, a, b, argb)], (a, b, c))


def closed_form(r, origin=(0, 0, 0)):
    return RR.geometry(r, origin) + (r[:, 6].astype(np.uint32),)


# ---- formats_and_layouts ---------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 37, 29), (63, 20, 18), (64, 17, 21), (65, 40, 40), (129, 9, 7), (40, 1, 30), (33, 29, 1), (200, 3, 5)]   # (nx, ny, nz)


def case_formats_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2029)
    palette = rng.integers(0, 2 ** 32, 256, dtype=np.uint64).astype(np.uint32)
    palette[2] = palette[1]                                      # labels 1 and 2 share a colour, label 255 does not
    n = stacked = 0
    assert -(-6 * 2 * 40 * 40 // 256) == 75                       # (65, 40, 40): 75 blocks of items
    for k, dims in enumerate(SHAPES):
        solid = blocky_solid(rng, dims, 0.6, ((5, 3, 2), (7, 2, 3), (1, 1, 1))[k % 3])   # (every third: no walls, voxel noise)
        for fmt, t, level in formats(solid, rng):
            a = t.cpu().numpy()
            S = FR.solid(a, FMT[fmt], level)
            nx = S.shape[2]                                       # (bits: 32 voxels per word)
            origin = ((0, 0, 0), (5, 7, 11), (65536 - nx, 0, 65000), (100, 65536 - dims[1], 3))[k % 4]   # (the last x, y reach 65 536)
            colors = blocky((nx,) + dims[1:], (9, 4, 3), lambda shape: rng.integers(-1, 2, shape)).astype(np.int32)   # three colours
            batch = torch.full((3,) + S.shape[:2] + (2 * S.shape[2],), -1, dtype=torch.int32, device=DEV)
            batch[1, :, :, ::2] = dev(colors)                     # every second element of a batch's second grid
            cview = batch[1, :, :, ::2]
            want = RR.quads(a, FMT[fmt], level, origin, argb=0x80FF4020)
            same(mesh(dense.voxel_faces(dv, t, level=level, origin=origin, merge="rects", argb=0x80FF4020)), want, (dims, fmt, "constant"))
            assert dense.count_faces(dv, t, level=level, merge="rects") == len(want[2])
            want_c = RR.quads(a, FMT[fmt], level, origin, colors=colors)
            same(mesh(dense.voxel_faces(dv, t, level=level, origin=origin, merge="rects", colors=cview)), want_c, (dims, fmt, "colour grid"))
            assert dense.count_faces(dv, t, level=level, merge="rects", colors=cview) == len(want_c[2])
            stacked += FR.count(a, FMT[fmt], level, FR.RUNS, colors=colors) - len(want_c[2])
            n += 4
            if FMT[fmt] == FR.U8:
                if fmt == "labels":                               # labels in cells, so that walls of one label exist
                    a = np.where(S, blocky(dims, (6, 5, 4), lambda shape: rng.choice(np.array([1, 2, 255], np.uint8), shape)), 0).astype(np.uint8)
                    t = dev(a)
                got = mesh(dense.voxel_faces(dv, t, origin=origin, merge="rects", palette=palette.tolist()))
                same(got, RR.quads(a, FR.U8, None, origin, palette=palette), (dims, fmt, "palette"))
                n += 1
            # the other modes after a rects call on the same context: what they were
            for merge, m in (("runs", FR.RUNS), ("none", FR.NONE)):
                same(mesh(dense.voxel_faces(dv, t, level=level, origin=origin, merge=merge, colors=cview)),
                     FR.quads(a, FMT[fmt], level, origin, m, colors=colors), (dims, fmt, merge, "after rects"))
                n += 1
            if dims in ((65, 40, 40), (129, 9, 7), (63, 20, 18)) and fmt != "labels":
                for layout, v in layouts(fmt, t):
                    same(mesh(dense.voxel_faces(dv, v, level=level, origin=origin, merge="rects", argb=0x80FF4020)), want, (dims, fmt, layout))
                    n += 1
        # a colour grid with a stride of 0: one colour per row
        row_colors = torch.arange(1, 1 + solid.shape[1], dtype=torch.int32, device=DEV)[None, :, None].expand(solid.shape)
        same(mesh(dense.voxel_faces(dv, dev(solid), merge="rects", colors=row_colors)), RR.quads(solid, FR.U8, colors=row_colors.cpu().numpy()),
             (dims, "expanded colours"))
        n += 1
    assert stacked > 1000                                         # (the grids do have walls)
    # empty and full grids
    for a, b, c in ((65, 40, 40), (1, 1, 1), (64, 3, 2), (1, 5, 1), (1, 1, 9)):
        shape = (c, b, a)
        p, f, q = dense.voxel_faces(dv, torch.zeros(shape, dtype=torch.uint8, device=DEV), merge="rects")
        assert (tuple(p.shape), tuple(f.shape), tuple(q.shape)) == ((0, 3), (0, 3), (0,))
        full = torch.ones(shape, dtype=torch.bool, device=DEV)
        assert dense.count_faces(dv, full, merge="rects") == 6
        same(mesh(dense.voxel_faces(dv, full, merge="rects", argb=7, origin=(1, 2, 3))), closed_form(box_rects(a, b, c, 7), (1, 2, 3)), ("full", shape))
        full_bits = torch.full((c, b, -(-a // 32)), -1, dtype=torch.int32, device=DEV)
        same(mesh(dense.voxel_faces(dv, full_bits, merge="rects")), RR.quads(full_bits.cpu().numpy(), FR.BITS), ("full bits", shape))
        n += 3
    print("compared", n, "calls,", stacked, "runs stacked with the colour grids; times", dv.faces_times())


# ---- boundaries ------------------------------------------------------------------------------------------------------------------------

def case_boundaries():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2030)

    def check(solid, what, colors=None, origin=(0, 0, 0)):
        kw = {} if colors is None else dict(colors=colors.astype(np.int32))
        got = mesh(dense.voxel_faces(dv, dev(solid), merge="rects", origin=origin, **({} if colors is None else dict(colors=dev(colors.astype(np.int32))))))
        same(got, RR.quads(solid, FR.U8, None, origin, **kw), what)
        return got

    # rows equal over two whole words that differ in the third
    S = np.ones((1, 2, 130), bool)
    S[0, 1, 129] = False
    assert len(check(S, "(130, 2, 1) less a voxel")[2]) == 10
    S = np.ones((2, 2, 192), bool)
    S[:, :, 129:] = False
    S[0, 1, 128] = S[1, 0, 128] = False
    check(S, "rows that differ at bit 0 of the third word")
    # the last row of a layer and the first of the next are no neighbours
    S = np.zeros((2, 3, 4), bool)
    S[0, 2, :] = S[1, 0, :] = True
    assert len(check(S, "two bars across y = ny - 1")[2]) == 12
    # a rectangle that begins at the last bit of item 255, its second run in the next block of items: W = 5 words a row, so
    # item 255 is word 0 of (row 8 = (y 2, z 2), direction +y) and the row behind it along z is row 11, items from 345
    nx, ny, nz = 320, 3, 4
    assert (8 * 6 + 3) * 5 == 255 and 8 == 2 * ny + 2 and (11 * 6 + 3) * 5 >= 256
    S = CR.random_grid(rng, (nx, ny, nz), 0.3)
    S[2:4, 2, :] = False
    S[2:4, 2, 63:65] = True
    d, lo, hi, _ = FR.quad_boxes(check(S, "a rectangle across a block of items")[0])
    assert ((d == 3) & (lo == (63, 3, 2)).all(axis=1) & (hi == (65, 3, 4)).all(axis=1)).sum() == 1
    # equal runs at z = 0 / z = 1 of the first and the last rows
    S = CR.random_grid(rng, (70, 4, 2), 0.5)
    S[1, 0], S[1, 3] = S[0, 0], S[0, 3]
    got = check(S, "equal runs in the first and last rows", origin=(65536 - 70, 65532, 65534))
    d, lo, hi, _ = FR.quad_boxes(got[0])
    assert ((d == 2) & (lo[:, 1] == 65532) & (hi[:, 2] - lo[:, 2] == 2)).sum() == (np.diff(np.concatenate([[0], S[0, 0].astype(np.int64)])) == 1).sum()
    assert ((d == 3) & (lo[:, 1] == 65536) & (hi[:, 2] - lo[:, 2] == 2)).sum() == (np.diff(np.concatenate([[0], S[0, 3].astype(np.int64)])) == 1).sum()
    # colours that make runs of equal start and different length, and of equal start and length and different colour
    S = np.ones((2, 4, 100), bool)
    Cv = np.zeros(S.shape, np.int64)
    Cv[:, 0, 40:], Cv[:, 1, 50:] = 1, 1                            # y 0: [0, 40) [40, 100); y 1: [0, 50) [50, 100)
    Cv[:, 2, 50:], Cv[:, 3, 50:] = 2, 3                            # y 2: colours 0, 2; y 3: colours 0, 3, the same cut as y 1
    got = check(S, "equal starts, other lengths and other colours", Cv)
    d, lo, hi, _ = FR.quad_boxes(got[0])
    top = (d == 5)
    assert sorted(zip(lo[top, 0].tolist(), lo[top, 1].tolist(), hi[top, 0].tolist(), hi[top, 1].tolist())) == \
        [(0, 0, 40, 1), (0, 1, 50, 4), (40, 0, 100, 1), (50, 1, 100, 2), (50, 2, 100, 3), (50, 3, 100, 4)]
    print("compared 6 boundary grids; times", dv.faces_times())


# ---- long_rects ------------------------------------------------------------------------------------------------------------------------

def case_long_rects():
    dv = hip.DeviceVoxelizer(0)
    n = 0
    for a, b, c in ((65536, 2, 2), (2, 65536, 2), (2, 2, 65536), (4096, 4096, 1)):
        full = torch.ones((c, b, a), dtype=torch.bool, device=DEV)
        t0 = time.time()
        assert dense.count_faces(dv, full, merge="rects") == 6
        got = mesh(dense.voxel_faces(dv, full, merge="rects", argb=0xFF010203))
        print((a, b, c), "all solid:", len(got[2]), "quads in %.2f s" % (time.time() - t0), "times", dv.faces_times())
        same(got, closed_form(box_rects(a, b, c, 0xFF010203)), ((a, b, c), "all solid"))
        n += 1
    # the plate less voxel (h, h): the rows below it one rectangle, its own row two, the rows above it one; a face each way inside
    N, h = 4096, 2048
    plate = torch.ones((1, N, N), dtype=torch.bool, device=DEV)
    plate[0, h, h] = False
    torch.cuda.synchronize()
    W = 0xFFFFFFFF
    rows = []
    for d, z in ((4, 0), (5, 0)):
        rows += [(0, 0, z, d, N, h, W), (0, h, z, d, h, 1, W), (h + 1, h, z, d, N - h - 1, 1, W), (0, h + 1, z, d, N, N - h - 1, W)]
    rows += [(0, 0, 0, 2, N, 1, W), (0, N - 1, 0, 3, N, 1, W), (h, h - 1, 0, 3, 1, 1, W), (h, h + 1, 0, 2, 1, 1, W)]
    rows += [(0, 0, 0, 0, N, 1, W), (N - 1, 0, 0, 1, N, 1, W), (h - 1, h, 0, 1, 1, 1, W), (h + 1, h, 0, 0, 1, 1, W)]
    t0 = time.time()
    got = mesh(dense.voxel_faces(dv, plate, merge="rects"))
    print("the plate less a voxel:", len(got[2]), "quads in %.2f s" % (time.time() - t0), "times", dv.faces_times())
    assert len(rows) == 16
    same(got, closed_form(by_key(rows, (N, N, 1))), "the plate less a voxel")
    # the all-solid plate with colours that change at x = 64 and x = 4 096 (past its last voxel), and at 64 and 1 000: a
    # rectangle per colour on the four faces the cuts cross, one on each of the other two
    plate = torch.ones((1, N, N), dtype=torch.bool, device=DEV)
    for cuts in ((64, 4096), (64, 1000)):
        x = np.arange(N)
        line = ((x >= cuts[0]).astype(np.int32) + (x >= cuts[1])).astype(np.int32)
        colors = dev(line)[None, None, :].expand(1, N, N)         # (strides of 0 along y and z)
        edges = [0] + [v for v in cuts if v < N] + [N]
        rows = [(0, 0, 0, 0, N, 1, int(line[0])), (N - 1, 0, 0, 1, N, 1, int(line[-1]))]
        for lo, hi in zip(edges[:-1], edges[1:]):
            rows += [(lo, 0, 0, 2, hi - lo, 1, int(line[lo])), (lo, N - 1, 0, 3, hi - lo, 1, int(line[lo])),
                     (lo, 0, 0, 4, hi - lo, N, int(line[lo])), (lo, 0, 0, 5, hi - lo, N, int(line[lo]))]
        t0 = time.time()
        got = mesh(dense.voxel_faces(dv, plate, merge="rects", colors=colors))
        print("the plate with colours cut at", cuts, ":", len(got[2]), "quads in %.2f s" % (time.time() - t0), "times", dv.faces_times())
        assert len(rows) == 4 * (len(edges) - 1) + 2
        same(got, closed_form(by_key(rows, (N, N, 1))), ("the plate with colours", cuts))
    print("compared", n + 3, "meshes")


# ---- snapshot --------------------------------------------------------------------------------------------------------------------------

def case_snapshot():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(4)
    shape = (40, 40, 130)
    labels = np.where(blocky_solid(rng, (130, 40, 40), 0.5, (11, 4, 3)), rng.integers(1, 256, shape), 0).astype(np.uint8)
    colors = blocky((130, 40, 40), (17, 6, 5), lambda s: rng.integers(0, 3, s)).astype(np.int32)
    t, c = dev(labels), dev(colors)
    want = RR.quads(labels, FR.U8, origin=(9, 8, 7), colors=colors)
    Q, guard = len(want[2]), 4096
    assert Q < FR.count(labels, FR.U8, merge=FR.RUNS, colors=colors) - 1000     # (runs do stack here)
    args = grid_args(t, FR.U8) + (hip.FACES_MERGE_RECTS, hip.GATHER_COLOR_GRID, 0, c.data_ptr(), (1, 130, 130 * 40), None)
    assert dv.faces_count(*args) == Q
    t.copy_(dev(rng.integers(0, 256, shape).astype(np.uint8)))                 # noise over the grid ...
    noise = rng.integers(100, 200, shape).astype(np.int32)
    c.copy_(dev(noise))                                                         # ... and over the colours
    torch.cuda.synchronize()
    pos = torch.full((12 * Q + 2 * guard,), 7.5, dtype=torch.float32, device=DEV)
    fac = torch.full((6 * Q + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    col = torch.full((Q + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    dv.faces_write(*args, (9, 8, 7), pos[guard:].data_ptr(), fac[guard:].data_ptr(), col[guard:].data_ptr(), Q)
    p, f, q = pos.cpu().numpy(), fac.cpu().numpy(), col.cpu().numpy()
    assert np.array_equal(p[guard:-guard].reshape(-1, 3).view(np.uint32), want[0].view(np.uint32)), "coordinates changed with the grid"
    assert np.array_equal(f[guard:-guard].reshape(-1, 3), want[1])
    for a, fill in ((p, F(7.5)), (f, 0x5A5A5A5A), (q, 0x5A5A5A5A)):
        assert (a[:guard] == fill).all() and (a[-guard:] == fill).all(), "a guard band was written"
    # the colours are read at the time of the write, at the first voxel of the rectangle's first run
    d, lo, _, _ = FR.quad_boxes(want[0])
    lo = lo - (9, 8, 7)
    lo[np.arange(Q), d >> 1] -= d & 1
    assert np.array_equal(q[guard:-guard], noise[lo[:, 2], lo[:, 1], lo[:, 0]])
    # faces and colours may be left out
    pos.fill_(7.5)
    torch.cuda.synchronize()
    dv.faces_write(*args, (9, 8, 7), pos[guard:].data_ptr(), None, None, Q)
    assert np.array_equal(pos.cpu().numpy()[guard:-guard].reshape(-1, 3).view(np.uint32), want[0].view(np.uint32))
    print("compared", Q, "quads, guard bands of", guard, "elements around three arrays")


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------

def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    res = 40
    c = meshes.unit_cube().reshape(-1, 9)
    dense.set_mesh(dv, dev(np.concatenate([c * 16 + 4.03, c * 16 + 10.07]).astype(F)))
    surface, origin = dense.voxelize_dense(dv, res, fmt="labels")
    solid = dense.solidify(dv, surface)
    s = solid.cpu().numpy()
    palette = [0] * 256
    palette[1], palette[2] = 0xFFFFFFFF, 0xFF00FF00
    p, f, q = dense.voxel_faces(dv, solid, origin=origin, merge="rects", palette=palette)
    want = RR.quads(s, FR.U8, origin=origin, palette=palette)
    same(mesh((p, f, q)), want, "solidify, surface / fill palette")
    n_runs = FR.count(s, FR.U8, merge=FR.RUNS, palette=palette)
    assert dense.count_faces(dv, solid, merge="rects", palette=palette) == len(want[2]) < n_runs // 4
    # the mesh back into the context: where its signed distance is negative is the parity set of the emitted triangles
    dense.set_mesh(dv, p, f)
    bounds = np.array([0, 0, 0, res, res, res], F)
    again, _ = dense.mesh_distance(dv, res, band=3.0, signed=True, bounds=bounds)
    dv.voxelize(res, read=False, bounds=bounds)
    xf = dv.transform()
    keys = fill_ref.parity_keys(fill_ref.sample_vertices(want[0][want[1]].reshape(-1, 9), xf), res, 1)
    z, y, x = np.nonzero(np.signbit(again.cpu().numpy()))
    assert np.array_equal(np.sort((x.astype(np.int64) * res + y) * res + z), keys)
    identity = bool(np.array_equal(xf, np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F)))
    if identity:   # voxel space is sample space bit for bit: the set is the solid set itself
        z, y, x = np.nonzero(s)
        assert np.array_equal(np.sort(((x + origin[0]).astype(np.int64) * res + y + origin[1]) * res + z + origin[2]), keys)
    print("pipeline: two cubes at 40:", n_runs, "runs,", len(want[2]), "rectangles,", len(keys), "voxels inside, identity transform", identity)
    # a coloured sphere, filled: the colours of the argb grid on the rectangles
    verts = meshes.uv_sphere(16)
    T = len(verts)
    types = np.full(T, hip.TRI_UNTEXTURED, np.uint32)
    dense.set_mesh(dv, dev(verts), types=dev(types.view(np.int32)), colors=dev(meshes.triangle_colors(T)))
    occupancy, origin = dense.voxelize_dense(dv, 96, fill=True, fill_argb=0xFF102030)
    argb, _ = dense.voxelize_dense(dv, 96, fmt="argb", fill=True, fill_argb=0xFF102030)
    model = dense.voxel_faces(dv, occupancy, origin=origin, merge="rects", colors=argb)
    want = RR.quads(occupancy.cpu().numpy(), FR.U8, origin=origin, colors=argb.cpu().numpy())
    same(mesh(model), want, "voxel_faces(occupancy, colors=argb)")
    assert len(np.unique(want[2])) > 100
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "sphere.obj")
        dense.save_mesh(path, *model[:2], argb=model[2])
        back, mat, _ = hip.load_mesh_file(path)
        assert len(back) == 2 * len(want[2]) and os.path.exists(os.path.join(tmp, "sphere.mtl"))
        kd = np.unique(np.round(mat["colors"] * 255).astype(np.int64), axis=0)
        rgb = np.unique(np.stack([want[2] >> 16 & 255, want[2] >> 8 & 255, want[2] & 255], axis=1).astype(np.int64), axis=0)
        assert np.array_equal(kd, rgb)
    print("sphere at 96:", len(want[2]), "rectangles,", len(back), "triangles through the OBJ reader")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """What MERGE_RECTS adds to the refusals of tests/faces_cases.py, made before any launch; the context stays usable.  (This
    child runs with torch's caching allocator off: each tensor is an allocation of its own, so a short one is short.)"""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(6)
    N = 48
    solid = blocky_solid(rng, (N, N, N), 0.4, (5, 4, 3))
    grid = dev(solid.astype(np.uint8))
    want = RR.quads(solid, FR.U8, argb=5)
    want_runs = FR.quads(solid, FR.U8, argb=5)
    Q, Qr = len(want[2]), len(want_runs[2])
    assert Q < Qr
    pos = torch.full((4 * Qr, 3), 7.0, dtype=torch.float32, device=DEV)
    fac = torch.full((2 * Qr, 3), 7, dtype=torch.int32, device=DEV)
    col = torch.full((Qr,), 7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st, dims = (1, N, N * N), (N, N, N)
    C, RECTS, RUNS, NONE = hip.GATHER_COLOR_CONSTANT, hip.FACES_MERGE_RECTS, hip.FACES_MERGE_RUNS, hip.FACES_MERGE_NONE
    bad, limit = hip.ERR_BAD_ARGUMENT, hip.ERR_LIMIT

    def count(merge=RECTS, ptr=grid.data_ptr(), strides=st, d=dims):
        return lambda: dv.faces_count(ptr, hip.GRID_U8, strides, d, 0.0, merge, C, 5, None, None, None)

    def write(merge=RECTS, ptr=grid.data_ptr(), strides=st, d=dims, cap=Qr, origin=(0, 0, 0), pp=pos.data_ptr()):
        return lambda: dv.faces_write(ptr, hip.GRID_U8, strides, d, 0.0, merge, C, 5, None, None, None, origin, pp, fac.data_ptr(), col.data_ptr(), cap)

    def untouched():
        torch.cuda.synchronize()
        return bool((pos == 7).all()) and bool((fac == 7).all()) and bool((col == 7).all())

    def correct(merge, mesh_want):
        n = count(merge)()
        assert n == len(mesh_want[2])
        write(merge, cap=n)()
        same((pos.cpu().numpy()[:4 * n], fac.cpu().numpy()[:2 * n], col.cpu().numpy().view(np.uint32)[:n]), mesh_want, ("a correct call, merge", merge))
        pos.fill_(7.0), fac.fill_(7), col.fill_(7)

    msgs = []
    for merge in (2, 4, 7):
        for what, make in (("count", count), ("write", write)):
            msgs.append(expect_code(bad, make(merge=merge), "%s: merge %d" % (what, merge)))
            assert "unknown merge %d" % merge in msgs[-1], msgs[-1]
        assert untouched()
        correct(RECTS, want)
    # a rects write after a runs count, and the reverse
    assert count(RUNS)() == Qr
    msgs.append(expect_code(bad, write(RECTS), "a rects write after a runs count"))
    assert "no matching o2v_hip_faces_count" in msgs[-1] and untouched()
    correct(RECTS, want)
    assert count(RECTS)() == Q
    for merge in (RUNS, NONE):
        msgs.append(expect_code(bad, write(merge), "a write with merge %d after a rects count" % merge))
        assert "no matching o2v_hip_faces_count" in msgs[-1] and untouched()
    correct(RUNS, want_runs)
    # a capacity below Q; an origin past the float32 box; positions off their alignment
    assert count(RECTS)() == Q
    msgs.append(expect_code(bad, write(cap=Q - 1), "a capacity below the count"))
    assert "quad_capacity %d is below the counted %d quads" % (Q - 1, Q) in msgs[-1]
    msgs.append(expect_code(limit, write(origin=(0, 65536 - N + 1, 0)), "origin + dims above 65 536"))
    msgs.append(expect_code(bad, write(pp=pos.data_ptr() + 4), "positions off a 16-byte boundary"))
    assert untouched()
    write(cap=Q)()                                                # (the count is still the one to match)
    same((pos.cpu().numpy()[:4 * Q], fac.cpu().numpy()[:2 * Q], col.cpu().numpy().view(np.uint32)[:Q]), want, "after the refusals")
    pos.fill_(7.0), fac.fill_(7), col.fill_(7)
    # 4 Q above 2^31 - 1: a checkerboard, where no two runs are equal, as a view whose voxel (x, y, z) is element x + y + z
    nx, ny, nz = 1024, 512, 512
    line = (torch.arange(nx + ny + nz, device=DEV) % 2).to(torch.uint8)
    big = 6 * (nx * ny * nz // 2)
    assert big == 805306368 and 4 * big > 2 ** 31 - 1
    t0 = time.time()
    assert count(ptr=line.data_ptr(), strides=(1, 1, 1), d=(nx, ny, nz))() == big
    print("count", big, "merge rects in %.2f s" % (time.time() - t0), "stage times", dv.faces_times())
    msgs.append(expect_code(limit, write(ptr=line.data_ptr(), strides=(1, 1, 1), d=(nx, ny, nz), cap=2 ** 40), "a write of 805 M quads"))
    assert "805306368 quads" in msgs[-1] and untouched()
    correct(RECTS, want)
    print("ok refusals:", len(msgs), "refused; last:", msgs[-1])


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]]()
    print("ok")
