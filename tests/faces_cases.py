"""The GPU cases of tests/test_gpu_faces.py, each run in a child process of its own: `python -m tests.faces_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison is np.array_equal on uint32 views of
positions, faces and colours against the numpy reference (tests/faces_ref.py) or a closed form, never against the code under
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
from tests import gather_ref as GR
from tests.gather_cases import FMT, grid_args
from tests.raycast_cases import dev, expect_code, formats, layouts

DEV = torch.device("cuda", 0)
F = np.float32
MERGES = (("none", FR.NONE), ("runs", FR.RUNS))


def mesh(result):
    """The three device tensors of voxel_faces as numpy arrays (positions float32, faces int32, argb uint32)."""
    p, f, c = result
    assert p.dtype == torch.float32 and f.dtype == torch.int32 and c.dtype == torch.int32
    assert p.is_contiguous() and f.is_contiguous() and c.is_contiguous()
    assert tuple(p.shape) == (4 * len(c), 3) and tuple(f.shape) == (2 * len(c), 3)
    return p.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy().view(np.uint32)


def same(got, want, what):
    for name, g, w in zip(("positions", "faces", "colours"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(g), -1).any(axis=1))[0]
        assert len(bad) == 0, (what, name, len(bad), "of", len(w), "rows differ, first", bad[:3], g[bad[:3]], w[bad[:3]])


# ---- formats_and_layouts ---------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 37, 29), (63, 20, 18), (64, 17, 21), (65, 40, 40), (129, 9, 7), (40, 1, 30), (33, 29, 1), (200, 3, 5)]   # (nx, ny, nz)


def case_formats_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2027)
    palette = rng.integers(0, 2 ** 32, 256, dtype=np.uint64).astype(np.uint32)
    palette[2] = palette[1]                                      # labels 1 and 2 share a colour, label 255 does not
    n = 0
    for k, dims in enumerate(SHAPES):
        solid = CR.random_grid(rng, dims, 0.6)
        for fmt, t, level in formats(solid, rng):
            a = t.cpu().numpy()
            S = FR.solid(a, FMT[fmt], level)
            nx = S.shape[2]                                       # (bits: 32 voxels per word)
            origin = ((0, 0, 0), (5, 7, 11), (65536 - nx, 0, 65000), (100, 65536 - dims[1], 3))[k % 4]   # (the last x, y reach 65 536)
            colors = rng.integers(-1, 2, S.shape, dtype=np.int64).astype(np.int32)   # three colours: runs and cuts
            batch = torch.full((3,) + S.shape[:2] + (2 * S.shape[2],), -1, dtype=torch.int32, device=DEV)
            batch[1, :, :, ::2] = dev(colors)                     # every second element of a batch's second grid
            for merge, m in MERGES:
                want = FR.quads(a, FMT[fmt], level, origin, m, argb=0x80FF4020)
                same(mesh(dense.voxel_faces(dv, t, level=level, origin=origin, merge=merge, argb=0x80FF4020)), want, (dims, fmt, merge, "constant"))
                assert dense.count_faces(dv, t, level=level, merge=merge) == len(want[2])
                got = mesh(dense.voxel_faces(dv, t, level=level, origin=origin, merge=merge, colors=batch[1, :, :, ::2]))
                same(got, FR.quads(a, FMT[fmt], level, origin, m, colors=colors), (dims, fmt, merge, "colour grid"))
                assert dense.count_faces(dv, t, level=level, merge=merge, colors=batch[1, :, :, ::2]) == len(got[2])
                n += 4
                if FMT[fmt] == FR.U8:
                    got = mesh(dense.voxel_faces(dv, t, origin=origin, merge=merge, palette=palette.tolist()))
                    same(got, FR.quads(a, FR.U8, None, origin, m, palette=palette), (dims, fmt, merge, "palette"))
                    n += 1
                if dims in ((65, 40, 40), (129, 9, 7), (63, 20, 18)):
                    for layout, v in layouts(fmt, t):
                        same(mesh(dense.voxel_faces(dv, v, level=level, origin=origin, merge=merge, argb=0x80FF4020)), want, (dims, fmt, merge, layout))
                        n += 1
        # a colour grid with a stride of 0: one colour per row
        row_colors = torch.arange(1, 1 + solid.shape[1], dtype=torch.int32, device=DEV)[None, :, None].expand(solid.shape)
        same(mesh(dense.voxel_faces(dv, dev(solid), colors=row_colors)), FR.quads(solid, FR.U8, colors=row_colors.cpu().numpy()), (dims, "expanded colours"))
        n += 1
    # voxels that share elements: a layer expanded along z, a plane expanded along x
    layer = CR.random_grid(rng, (50, 40, 1), 0.55)
    for name, S, t in (("expanded z", np.broadcast_to(layer, (30, 40, 50)), dev(layer).expand(30, -1, -1)),
                       ("expanded x", np.broadcast_to(layer[0][:, :1], (30, 40, 50)), dev(layer[0][:, :1].copy()).unsqueeze(0).expand(30, -1, 50))):
        assert 0 in t.stride()
        same(mesh(dense.voxel_faces(dv, t, origin=(1, 2, 3))), FR.quads(S, FR.U8, origin=(1, 2, 3)), name)
        f32 = torch.where(t, -1.0, 1.0)
        same(mesh(dense.voxel_faces(dv, f32, level=0.0, merge="none")), FR.quads(S, FR.U8, merge=FR.NONE), name + " f32")
        n += 2
    # empty and full grids
    for a, b, c in ((65, 40, 40), (1, 1, 1), (64, 3, 2)):
        shape = (c, b, a)
        p, f, q = dense.voxel_faces(dv, torch.zeros(shape, dtype=torch.uint8, device=DEV))
        assert (tuple(p.shape), tuple(f.shape), tuple(q.shape)) == ((0, 3), (0, 3), (0,)) and dense.count_faces(dv, torch.zeros(shape, device=DEV), level=0.0) == 0
        full = torch.ones(shape, dtype=torch.bool, device=DEV)
        assert dense.count_faces(dv, full) == 2 * (a * b + b * c + c * a) and dense.count_faces(dv, full, merge="runs") == 2 * b + 4 * c
        same(mesh(dense.voxel_faces(dv, full, argb=7)), FR.quads(np.ones(shape, bool), FR.U8, argb=7), ("full", shape))
        full_bits = torch.full((c, b, -(-a // 32)), -1, dtype=torch.int32, device=DEV)
        same(mesh(dense.voxel_faces(dv, full_bits)), FR.quads(full_bits.cpu().numpy(), FR.BITS), ("full bits", shape))
        n += 3
    print("compared", n, "calls; times", dv.faces_times())


# ---- long_runs -------------------------------------------------------------------------------------------------------------------------

def case_long_runs():
    dv = hip.DeviceVoxelizer(0)
    n = 0
    for shape, q_runs, cuts in (((2, 2, 65536), 12, (64, 4096)), ((2, 65536, 2), 131080, (256, 4096))):
        full = torch.ones(shape, dtype=torch.bool, device=DEV)
        host = np.ones(shape, bool)
        t0 = time.time()
        assert dense.count_faces(dv, full, merge="runs") == q_runs
        got = mesh(dense.voxel_faces(dv, full))
        print(shape, "runs", len(got[2]), "in %.2f s" % (time.time() - t0), "times", dv.faces_times())
        same(got, FR.quads(host, FR.U8), (shape, "one colour"))
        d, lo, hi, _ = FR.quad_boxes(got[0])
        along = 0 if shape[2] > shape[1] else 1
        assert ((hi - lo)[:, along] == 65536).sum() == (8 if along == 0 else 4)      # uncut: across 1 024 words / 65 536 rows
        # colours that change at a word boundary and far from one / at a block boundary of rows and far from one
        pos = np.arange(65536)
        stripe = ((pos >= cuts[0]).astype(np.int32) + (pos >= cuts[1])).reshape((1, 1, -1) if along == 0 else (1, -1, 1))
        colors = np.broadcast_to(stripe, shape).astype(np.int32)
        want = FR.quads(host, FR.U8, colors=colors)
        same(mesh(dense.voxel_faces(dv, full, colors=dev(colors))), want, (shape, "three colours"))
        assert len(want[2]) == q_runs + 2 * (8 if along == 0 else 4)
        same(mesh(dense.voxel_faces(dv, full, merge="none", colors=dev(colors))), FR.quads(host, FR.U8, merge=FR.NONE, colors=colors), (shape, "none"))
        n += 3
    # a run from the last bit of a block of 256 items to the first bit of the next: W = 5 words a row, so item 255 is word 0
    # and item 256 word 1 of (row 8, direction +y)
    nx, ny, nz = 320, 3, 4
    assert ((8 * 6 + 3) * 5, (8 * 6 + 3) * 5 + 1) == (255, 256) and 8 == 2 * ny + 2
    solid = CR.random_grid(np.random.default_rng(5), (nx, ny, nz), 0.3)
    solid[2, 2, :] = False
    solid[2, 2, 63:65] = True
    got = mesh(dense.voxel_faces(dv, dev(solid)))
    same(got, FR.quads(solid, FR.U8), "a run across a block of items")
    d, lo, hi, _ = FR.quad_boxes(got[0])
    assert ((d == 3) & (lo == (63, 3, 2)).all(axis=1) & (hi == (65, 3, 3)).all(axis=1)).sum() == 1
    print("compared", n + 1, "meshes")


# ---- snapshot --------------------------------------------------------------------------------------------------------------------------

def case_snapshot():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(3)
    shape = (40, 40, 130)
    labels = np.where(CR.random_grid(rng, (130, 40, 40), 0.5), rng.integers(1, 256, shape), 0).astype(np.uint8)
    colors = rng.integers(0, 3, shape).astype(np.int32)
    t, c = dev(labels), dev(colors)
    want = FR.quads(labels, FR.U8, origin=(9, 8, 7), colors=colors)
    Q, guard = len(want[2]), 4096
    args = grid_args(t, FR.U8) + (hip.FACES_MERGE_RUNS, hip.GATHER_COLOR_GRID, 0, c.data_ptr(), (1, 130, 130 * 40), None)
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
    # the colours are read at the time of the write, at the run's first voxel
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


# ---- count_above_2_32 ------------------------------------------------------------------------------------------------------------------

def case_count_above_2_32():
    dv = hip.DeviceVoxelizer(0)
    nx, ny, nz = 2048, 1024, 1024
    line = (torch.arange(nx + ny + nz, device=DEV) % 2).to(torch.uint8)        # voxel (x, y, z) is element x + y + z: a checkerboard
    want = 6 * (nx * ny * nz // 2)
    assert want > 2 ** 32 and want == 6442450944
    scratch = dv.faces_scratch_bytes((nx, ny, nz))
    t0 = time.time()
    got = dense.count_faces(dv, torch.as_strided(line, (nz, ny, nx), (1, 1, 1)), merge="none")
    print("count", got, "merge none in %.2f s" % (time.time() - t0), "stage times", dv.faces_times(), "scratch", scratch)
    assert got == want, (got, want)
    args = (line.data_ptr(), hip.GRID_U8, (1, 1, 1), (nx, ny, nz), 0.0, hip.FACES_MERGE_RUNS, hip.GATHER_COLOR_CONSTANT, 0xFFFFFFFF, None, None, None)
    t0 = time.time()
    got = dv.faces_count(*args)
    print("count", got, "merge runs in %.2f s" % (time.time() - t0), "stage times", dv.faces_times())
    assert got == want, (got, want)
    out = torch.full((64,), 7, dtype=torch.int32, device=DEV)
    msg = expect_code(hip.ERR_LIMIT, lambda: dv.faces_write(*args, (0, 0, 0), out.data_ptr(), None, None, 2 ** 40), "a write of 6 G quads")
    assert "6442450944 quads" in msg and bool((out == 7).all()), msg
    # the context stays usable
    small = np.ones((2, 3, 5), bool)
    same(mesh(dense.voxel_faces(dv, dev(small))), FR.quads(small, FR.U8), "after the refusal")
    print("refused:", msg)


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------

def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    res = 40
    c = meshes.unit_cube().reshape(-1, 9)
    dense.set_mesh(dv, dev(np.concatenate([c * 16 + 4.03, c * 16 + 10.07]).astype(F)))
    surface, origin = dense.voxelize_dense(dv, res, fmt="labels")
    solid = dense.solidify(dv, surface)
    s = solid.cpu().numpy()
    area = dense.count_faces(dv, solid, merge="none")
    assert area == FR.count(s, FR.U8, merge=FR.NONE) == len(FR.unit_faces(s != 0, np.zeros(s.shape, np.uint32)))
    palette = [0] * 256
    palette[1], palette[2] = 0xFFFFFFFF, 0xFF00FF00
    p, f, q = dense.voxel_faces(dv, solid, origin=origin, palette=palette)
    want = FR.quads(s, FR.U8, origin=origin, palette=palette)
    same(mesh((p, f, q)), want, "solidify, surface / fill palette")
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
    print("pipeline: surface area", area, "faces,", len(want[2]), "runs,", len(keys), "voxels inside, identity transform", identity)
    # a coloured sphere, filled: the colours of the argb grid on the quads
    verts = meshes.uv_sphere(16)
    T = len(verts)
    types = np.full(T, hip.TRI_UNTEXTURED, np.uint32)
    dense.set_mesh(dv, dev(verts), types=dev(types.view(np.int32)), colors=dev(meshes.triangle_colors(T)))
    occupancy, origin = dense.voxelize_dense(dv, 96, fill=True, fill_argb=0xFF102030)
    argb, _ = dense.voxelize_dense(dv, 96, fmt="argb", fill=True, fill_argb=0xFF102030)
    model = dense.voxel_faces(dv, occupancy, origin=origin, colors=argb)
    want = FR.quads(occupancy.cpu().numpy(), FR.U8, origin=origin, colors=argb.cpu().numpy())
    same(mesh(model), want, "voxel_faces(occupancy, colors=argb)")
    assert len(np.unique(want[2])) > 100
    in_model_space = dense.voxel_faces(dv, occupancy, origin=origin, colors=argb, transform=dv.transform())[0].cpu().numpy()
    assert 0.9 < np.abs(in_model_space).max() < 1.1                              # (the unit sphere, a voxel of 1 / 48 more at most)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "sphere.obj")
        dense.save_mesh(path, *model[:2], argb=model[2])
        back, mat, _ = hip.load_mesh_file(path)
        assert len(back) == 2 * len(want[2]) and os.path.exists(os.path.join(tmp, "sphere.mtl"))
        kd = np.unique(np.round(mat["colors"] * 255).astype(np.int64), axis=0)
        rgb = np.unique(np.stack([want[2] >> 16 & 255, want[2] >> 8 & 255, want[2] & 255], axis=1).astype(np.int64), axis=0)
        assert np.array_equal(kd, rgb)
    print("sphere at 96:", len(want[2]), "quads,", len(back), "triangles through the OBJ reader")


# ---- interleaved -----------------------------------------------------------------------------------------------------------------------

def case_interleaved():
    """Calls of the faces and of the gather in turns on one context.  The two share the device copy of the palette and the host
    code of their counts, while each keeps the arrays of its own count: a _write must find its _count's bits and offsets, and its
    own palette, after the other feature has counted and written in between."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2028)
    shape = (2, 3, 130)                                            # two full words of 64 voxels and a tail of 2 per row
    A, B = (rng.integers(0, 4, shape).astype(np.uint8) for _ in range(2))
    PA, PB = (rng.integers(0, 2 ** 32, 256, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    assert not np.array_equal(A, B) and not np.array_equal(PA[:4], PB[:4])
    ta, tb = dev(A), dev(B)
    want_quads = FR.quads(A, FR.U8, merge=FR.RUNS, palette=PA)
    want_records = GR.records(B, GR.U8, palette=PB)
    Q, n = len(want_quads[2]), len(want_records)
    assert Q > 100 and n > 100
    faces_a = grid_args(ta, FR.U8) + (hip.FACES_MERGE_RUNS, hip.GATHER_COLOR_PALETTE, 0, None, None, PA.tolist())
    faces_b = grid_args(tb, FR.U8) + (hip.FACES_MERGE_RUNS, hip.GATHER_COLOR_PALETTE, 0, None, None, PB.tolist())
    gather_b = grid_args(tb, GR.U8)
    pos = torch.full((4 * Q, 3), 7.0, dtype=torch.float32, device=DEV)
    fac = torch.full((2 * Q, 3), 7, dtype=torch.int32, device=DEV)
    col = torch.full((Q,), 7, dtype=torch.int32, device=DEV)
    rec = torch.full((2, n, 4), 7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def write_b(k):
        dv.gather_write(*gather_b, (0, 0, 0), hip.GATHER_COLOR_PALETTE, 0, None, None, PB.tolist(), 0, n, rec[k].data_ptr())

    assert dv.faces_count(*faces_a) == Q                                                              # 1
    msg = expect_code(hip.ERR_BAD_ARGUMENT, lambda: dv.faces_write(*faces_b, (0, 0, 0), pos.data_ptr(), fac.data_ptr(), col.data_ptr(), Q),
                      "faces_write(B) after faces_count(A)")
    assert "no matching o2v_hip_faces_count" in msg
    torch.cuda.synchronize()
    assert bool((pos == 7).all()) and bool((fac == 7).all()) and bool((col == 7).all()), "the refused write wrote something"
    assert dv.gather_count(*gather_b) == n                                                            # 2
    write_b(0)                                                                                        # 3
    dv.faces_write(*faces_a, (0, 0, 0), pos.data_ptr(), fac.data_ptr(), col.data_ptr(), Q)            # 4
    write_b(1)                                                                                        # 5
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy().view(np.uint32), want_quads[0].view(np.uint32)), "positions of A"
    assert np.array_equal(fac.cpu().numpy(), want_quads[1]), "faces of A"
    assert np.array_equal(col.cpu().numpy().view(np.uint32), want_quads[2]), "colours of A: palette PA"
    for k in range(2):
        assert np.array_equal(rec[k].cpu().numpy().view(np.uint32), want_records), ("records of B: palette PB, write", k)
    print("interleaved:", Q, "quads of A and twice", n, "records of B compared; refused:", msg)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list, made before any launch; the context stays usable.  (This child runs with torch's
    caching allocator off: each tensor is an allocation of its own, so a short one is short.)"""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(1)
    N = 96                                     # a U8 grid of 0.9 MB; its short twin is half of it
    solid = CR.random_grid(rng, (N, N, N), 0.25)
    grid = dev(solid.astype(np.uint8))
    want = FR.quads(solid, FR.U8, argb=5)
    Q = len(want[2])                           # ~ 0.5 M quads: 24 MB of positions
    half = torch.zeros((N // 2, N, N), dtype=torch.uint8, device=DEV)
    field = torch.ones((N, N, N), dtype=torch.float32, device=DEV)
    words = torch.zeros((N, N, N // 32), dtype=torch.int32, device=DEV)
    colors = torch.zeros((N, N, N), dtype=torch.int32, device=DEV)
    pos = torch.full((4 * Q, 3), 7.0, dtype=torch.float32, device=DEV)
    fac = torch.full((2 * Q, 3), 7, dtype=torch.int32, device=DEV)
    col = torch.full((Q,), 7, dtype=torch.int32, device=DEV)
    short = torch.full((Q // 4,), 7, dtype=torch.int32, device=DEV)     # a quarter of the smallest output
    host, host_out = np.zeros((N, N, N), np.uint8), np.zeros((4 * Q, 3), F)
    torch.cuda.synchronize()
    st, dims, pal = (1, N, N * N), (N, N, N), list(range(256))
    C, G, P = hip.GATHER_COLOR_CONSTANT, hip.GATHER_COLOR_GRID, hip.GATHER_COLOR_PALETTE
    RUNS, NONE = hip.FACES_MERGE_RUNS, hip.FACES_MERGE_NONE

    def count(ptr=grid.data_ptr(), fmt=hip.GRID_U8, strides=st, d=dims, level=0.0, merge=RUNS, mode=C, argb=5, cp=None, cs=None, palette=None):
        return lambda: dv.faces_count(ptr, fmt, strides, d, level, merge, mode, argb, cp, cs, palette)

    def write(ptr=grid.data_ptr(), fmt=hip.GRID_U8, strides=st, d=dims, level=0.0, merge=RUNS, mode=C, argb=5, cp=None, cs=None, palette=None,
              origin=(0, 0, 0), pp=pos.data_ptr(), fp=fac.data_ptr(), qp=col.data_ptr(), cap=Q):
        return lambda: dv.faces_write(ptr, fmt, strides, d, level, merge, mode, argb, cp, cs, palette, origin, pp, fp, qp, cap)
    bad, limit = hip.ERR_BAD_ARGUMENT, hip.ERR_LIMIT
    msgs = [expect_code(bad, write(), "a write without a count")]
    assert "no matching o2v_hip_faces_count" in msgs[0]
    assert count()() == Q
    for what, make in (("count", count), ("write", write)):
        msgs += [
            expect_code(bad, make(ptr=None), what + ": null grid"),
            expect_code(bad, make(d=(N, 0, N)), what + ": zero dims"),
            expect_code(bad, make(fmt=3), what + ": unknown format"),
            expect_code(bad, make(ptr=words.data_ptr(), fmt=hip.GRID_BITS, strides=(2, N // 32, N * N // 32)), what + ": BITS with an x stride of 2"),
            expect_code(bad, make(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("nan")), what + ": a NaN level"),
            expect_code(bad, make(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("inf")), what + ": an infinite level"),
            expect_code(bad, make(ptr=host.ctypes.data), what + ": a host grid"),
            expect_code(bad, make(ptr=half.data_ptr()), what + ": a short grid"),
            expect_code(bad, make(merge=2), what + ": unknown merge"),
            expect_code(bad, make(mode=3), what + ": unknown colour mode"),
            expect_code(bad, make(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, mode=P, palette=pal), what + ": a palette with a float grid"),
            expect_code(bad, make(mode=P), what + ": PALETTE without a palette"),
            expect_code(bad, make(mode=G), what + ": GRID without colours"),
            expect_code(bad, make(mode=G, cp=colors.data_ptr()), what + ": GRID without colour strides"),
            expect_code(bad, make(mode=G, cp=host.ctypes.data, cs=st), what + ": host colours"),
            expect_code(bad, make(mode=G, cp=half.data_ptr(), cs=st), what + ": short colours"),
            expect_code(limit, make(d=(65537, 1, 1), strides=(0, 0, 0)), what + ": a dim above 65 536"),
            expect_code(limit, make(d=(1, 65536, 32768), strides=(0, 0, 0)), what + ": 2^31 words"),
        ]
        assert "2147483648 words" in msgs[-1] and "unknown merge 2" in msgs[-10]
    # (the refused counts replaced the last one)
    assert "no matching" in expect_code(bad, write(), "a write after refused counts")
    assert count()() == Q
    msgs += [
        expect_code(limit, write(origin=(65536 - N + 1, 0, 0)), "origin + dims above 65 536"),
        expect_code(limit, write(origin=(0, 0, 2 ** 32 - 1)), "origin + dims above 2^32"),
        expect_code(bad, write(cap=Q - 1), "a capacity below the count"),
        expect_code(bad, write(pp=None), "null positions"),
        expect_code(bad, write(pp=host_out.ctypes.data), "host positions"),
        expect_code(bad, write(pp=short.data_ptr()), "short positions"),
        expect_code(bad, write(fp=short.data_ptr()), "short faces"),
        expect_code(bad, write(qp=short.data_ptr()), "short colours out"),
        expect_code(bad, write(pp=pos.data_ptr() + 4), "positions off a 16-byte boundary"),
        expect_code(bad, write(fp=fac.data_ptr() + 4), "faces off an 8-byte boundary"),
        expect_code(bad, write(fp=pos.data_ptr()), "faces in the positions"),
        expect_code(bad, write(qp=fac.data_ptr() + 1024), "colours in the faces"),
        expect_code(bad, write(qp=pos.data_ptr() + 1024, fp=None), "colours in the positions"),
    ]
    assert "overlap" in msgs[-1] and "overlap" in msgs[-2] and "overlap" in msgs[-3] and "65 536" in msgs[-13]
    # outputs inside the grid or the colours: a count over a grid large enough to hold them
    big = torch.zeros((48 * Q,), dtype=torch.uint8, device=DEV)
    cbig = torch.zeros((12 * Q,), dtype=torch.int32, device=DEV)
    assert 12 * Q > N ** 3 and count(mode=G, cp=cbig.data_ptr(), cs=(1, N, N * N))() == Q
    msgs += [expect_code(bad, write(mode=G, cp=cbig.data_ptr(), cs=(1, N, N * N), pp=cbig.data_ptr()), "positions in the colours")]
    assert "positions and colors overlap" in msgs[-1]
    big[0] = 1                                                                   # (one solid voxel: six quads)
    torch.cuda.synchronize()
    assert count(ptr=big.data_ptr(), strides=(1, N, N * N))() == 6
    msgs += [expect_code(bad, write(ptr=big.data_ptr(), strides=(1, N, N * N), pp=big.data_ptr() + 4096, cap=6), "positions in the grid")]
    assert "positions and grid overlap" in msgs[-1]
    # a write after a count with another merge mode, colour mode, colour, strides, dims or level
    assert count()() == Q
    for kw, what in ((dict(merge=NONE), "another merge"), (dict(mode=P, palette=pal), "another colour mode"), (dict(argb=6), "another colour"),
                     (dict(mode=G, cp=colors.data_ptr(), cs=st), "a colour grid"), (dict(strides=(1, N, N * N - 1)), "other strides"),
                     (dict(d=(N, N, N - 1)), "other dims")):
        assert "no matching" in expect_code(bad, write(**kw), what + " than counted"), what
        msgs.append(what)
    assert count(mode=P, palette=pal)() == Q
    assert "no matching" in expect_code(bad, write(mode=P, palette=pal[::-1]), "another palette than counted")
    assert count(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=2.0)() == 2 * N + 4 * N
    assert "no matching" in expect_code(bad, write(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=2.5), "another level than counted")
    torch.cuda.synchronize()
    assert bool((pos == 7).all()) and bool((fac == 7).all()) and bool((col == 7).all()) and bool((short == 7).all()), "a refused call wrote something"
    assert bool((cbig == 0).all()) and np.array_equal(grid.cpu().numpy(), solid.astype(np.uint8))
    # the context stays usable
    assert count()() == Q
    write()()
    same((pos.cpu().numpy(), fac.cpu().numpy(), col.cpu().numpy().view(np.uint32)), want, "after the refusals")
    print("ok refusals:", len(msgs), "refused; last:", msgs[-8])


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]]()
    print("ok")
