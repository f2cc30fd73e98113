"""The GPU cases of tests/test_gpu_gather.py, each run in a child process of its own: `python -m tests.gather_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison is np.array_equal on uint32 records
against the numpy reference (tests/gather_ref.py) or a closed form, never against the code under test.  A case prints what it
compared and "ok" last when everything held."""
import os
import sys
import tempfile
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import components_ref as CR
from tests import gather_ref as GR
from tests.raycast_cases import dev, expect_code, formats, layouts

DEV = torch.device("cuda", 0)
F = np.float32
FMT = {"bool": GR.U8, "labels": GR.U8, "bits": GR.BITS, "f32": GR.F32_BELOW}


def u32(t):
    """A device tensor of records as a uint32 numpy array [n, 4]."""
    assert t.dtype == torch.int32 and t.dim() == 2 and t.shape[1] == 4 and t.is_contiguous()
    return t.cpu().numpy().view(np.uint32)


def same(got, want, what):
    assert got.dtype == np.uint32 and want.dtype == np.uint32
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert np.array_equal(got, want), (what, len(bad), "of", len(want), "records differ, first", bad[:3], got[bad[:3]], want[bad[:3]])


def grid_args(t, fmt, level=None):
    """(ptr, format, strides, dims, level) of a tensor [z, y, x] for the hip-level calls."""
    nz, ny, nx = t.shape
    return t.data_ptr(), fmt, (t.stride(2), t.stride(1), t.stride(0)), (nx * 32 if fmt == GR.BITS else nx, ny, nz), 0.0 if level is None else level


# ---- formats_and_layouts ---------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 37, 29), (63, 20, 18), (64, 17, 21), (65, 40, 40), (129, 9, 7), (40, 1, 30), (33, 29, 1), (200, 3, 5)]   # (nx, ny, nz)


def case_formats_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2026)
    palette = rng.integers(0, 2 ** 32, 256, dtype=np.uint64).astype(np.uint32)
    n = 0
    for k, dims in enumerate(SHAPES):
        solid = CR.random_grid(rng, dims, 0.3)
        for fmt, t, level in formats(solid, rng):
            a = t.cpu().numpy()
            nx = GR.solid(a, FMT[fmt], level).shape[2]           # (bits: 32 voxels per word)
            origin = ((0, 0, 0), (5, 7, 11), (2 ** 32 - nx, 0, 65000), (100, 2 ** 31, 3))[k % 4]   # (the third: the last x is 2^32 - 1)
            want = GR.records(a, FMT[fmt], level, origin, 0x80FF4020)
            got = u32(dense.to_voxels(dv, t, level=level, origin=origin, argb=0x80FF4020))
            same(got, want, (dims, fmt, "constant"))
            assert dense.count_voxels(dv, t, level=level) == len(want)
            # a colour grid: a strided slice of a batch (every second element along x, the second of three grids)
            S = GR.solid(a, FMT[fmt], level)
            colors = rng.integers(-2 ** 31, 2 ** 31, S.shape, dtype=np.int64).astype(np.int32)
            batch = torch.full((3,) + S.shape[:2] + (2 * S.shape[2],), -1, dtype=torch.int32, device=DEV)
            batch[1, :, :, ::2] = dev(colors)
            got = u32(dense.to_voxels(dv, t, level=level, origin=origin, colors=batch[1, :, :, ::2]))
            same(got, GR.records(a, FMT[fmt], level, origin, colors=colors), (dims, fmt, "colour grid"))
            n += 3
            if FMT[fmt] == GR.U8:
                got = u32(dense.to_voxels(dv, t, origin=origin, palette=palette.tolist()))
                same(got, GR.records(a, GR.U8, None, origin, palette=palette), (dims, fmt, "palette"))
                n += 1
            if dims in ((65, 40, 40), (129, 9, 7), (63, 20, 18)):
                for layout, v in layouts(fmt, t):
                    same(u32(dense.to_voxels(dv, v, level=level, origin=origin, argb=0x80FF4020)), want, (dims, fmt, layout))
                    n += 1
        # a colour grid with a stride of 0: one colour per row
        row_colors = torch.arange(1, 1 + solid.shape[1], dtype=torch.int32, device=DEV)[None, :, None].expand(solid.shape)
        same(u32(dense.to_voxels(dv, dev(solid), colors=row_colors)), GR.records(solid, GR.U8, colors=row_colors.cpu().numpy()), (dims, "expanded colours"))
        n += 1
    # voxels that share elements: a layer expanded along z, a plane expanded along x
    layer = CR.random_grid(rng, (50, 40, 1), 0.45)
    for name, S, t in (("expanded z", np.broadcast_to(layer, (30, 40, 50)), dev(layer).expand(30, -1, -1)),
                       ("expanded x", np.broadcast_to(layer[0][:, :1], (30, 40, 50)), dev(layer[0][:, :1].copy()).unsqueeze(0).expand(30, -1, 50))):
        assert 0 in t.stride()
        same(u32(dense.to_voxels(dv, t, origin=(1, 2, 3))), GR.records(S, GR.U8, origin=(1, 2, 3)), name)
        f32 = torch.where(t, -1.0, 1.0)
        same(u32(dense.to_voxels(dv, f32, level=0.0)), GR.records(S, GR.U8), name + " f32")
        n += 2
    # empty and full grids
    for dims in ((65, 40, 40), (1, 1, 1), (64, 3, 2)):
        shape = dims[::-1]
        empty = dense.to_voxels(dv, torch.zeros(shape, dtype=torch.uint8, device=DEV))
        assert tuple(empty.shape) == (0, 4) and empty.dtype == torch.int32
        same(u32(dense.to_voxels(dv, torch.ones(shape, dtype=torch.bool, device=DEV), argb=7)), GR.records(np.ones(shape, bool), GR.U8, argb=7), ("full", dims))
        full_bits = torch.full((shape[0], shape[1], -(-shape[2] // 32)), -1, dtype=torch.int32, device=DEV)
        same(u32(dense.to_voxels(dv, full_bits)), GR.records(full_bits.cpu().numpy(), GR.BITS), ("full bits", dims))
        n += 3
    # the round trip
    g = dev(CR.random_grid(rng, (70, 50, 40), 0.2).astype(np.uint8) * 3)
    assert bool((dense.from_voxels(dense.to_voxels(dv, g), g.shape) == (g != 0)).all())
    print("compared", n, "calls; times", dv.gather_times())


# ---- ranges ----------------------------------------------------------------------------------------------------------------------------

def boundaries(S, rng):
    """Record numbers at which ranges begin and end: inside a word, on word boundaries, on block boundaries (256 words) and one
    either side of those, 0 and the count."""
    pop = np.array([bin(int(w)).count("1") for w in GR.words64(S)], np.int64)
    ends = np.cumsum(pop)
    total = int(ends[-1])
    words = np.unique(ends[rng.integers(0, len(ends), 40)])
    blocks = np.concatenate([[0], ends[255::256]])
    inside = rng.integers(0, total + 1, 40)
    cuts = np.unique(np.concatenate([[0, total], words, blocks, blocks - 1, blocks + 1, inside]))
    return [int(c) for c in cuts if 0 <= c <= total], [int(b) for b in blocks], total


def case_ranges():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(7)
    n_ranges = 0
    for name, dims, density in (("dense", (130, 40, 40), 0.3), ("with empty blocks", (70, 64, 40), 0.5), ("sparse", (200, 50, 30), 0.002)):
        solid = CR.random_grid(rng, dims, density)
        if name == "with empty blocks":
            solid[10:25] = False            # 15 layers of 64 rows of 2 words: 7.5 blocks without a record
            solid[30, 5:40] = False
        t = dev(solid.astype(np.uint8))
        want = GR.records(solid, GR.U8, origin=(3, 2, 1), argb=0x11223344)
        cuts, blocks, total = boundaries(solid, rng)
        assert total == len(want) and len(blocks) > 3
        args = grid_args(t, GR.U8)
        color = ((3, 2, 1), hip.GATHER_COLOR_CONSTANT, 0x11223344, None, None, None)
        assert dv.gather_count(*args) == total                       # one count
        whole = torch.full((total, 4), -1, dtype=torch.int32, device=DEV)
        dv.gather_write(*args, *color, 0, total, whole.data_ptr())
        same(u32(whole), want, (name, "one call"))
        parts = {}
        for lo, hi in reversed(list(zip(cuts[:-1], cuts[1:]))):      # descending order
            out = torch.full((hi - lo, 4), -1, dtype=torch.int32, device=DEV)
            dv.gather_write(*args, *color, lo, hi - lo, out.data_ptr())
            parts[lo] = u32(out)
            n_ranges += 1
        same(np.concatenate([parts[lo] for lo in cuts[:-1]]), want, (name, "the ranges in turn"))
        # n = 0 reads no pointer, at any first up to the count
        for first in (0, total // 2, total):
            dv.gather_write(*args, *color, first, 0, None)
        assert tuple(dense.to_voxels(dv, t, first=total).shape) == (0, 4)
        mid = cuts[len(cuts) // 2]
        same(u32(dense.to_voxels(dv, t, origin=(3, 2, 1), argb=0x11223344, first=mid, count=total - mid)), want[mid:], (name, "first / count"))
        # single records either side of every block boundary
        for b in blocks[1:-1]:
            for first in (b - 1, b):
                if not 0 <= first < total:
                    continue
                out = torch.full((1, 4), -1, dtype=torch.int32, device=DEV)
                dv.gather_write(*args, *color, first, 1, out.data_ptr())
                same(u32(out), want[first:first + 1], (name, "record", first))
                n_ranges += 1
        print(name, dims, total, "records,", len(cuts) - 1, "ranges,", len(blocks) - 1, "blocks")
    print("compared", n_ranges, "ranges")


# ---- snapshot --------------------------------------------------------------------------------------------------------------------------

def case_snapshot():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(3)
    labels = np.where(CR.random_grid(rng, (130, 40, 40), 0.3), rng.integers(1, 256, (40, 40, 130)), 0).astype(np.uint8)
    t = dev(labels)
    want = GR.records(labels, GR.U8, origin=(9, 8, 7), argb=0xAABBCCDD)
    n, guard = len(want), 4096
    args = grid_args(t, GR.U8)
    assert dv.gather_count(*args) == n
    t.copy_(dev(rng.integers(0, 256, labels.shape).astype(np.uint8)))          # noise over the grid
    torch.cuda.synchronize()
    buf = torch.full((n + 2 * guard, 4), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    dv.gather_write(*args, (9, 8, 7), hip.GATHER_COLOR_CONSTANT, 0xAABBCCDD, None, None, None, 0, n, buf[guard:].data_ptr())
    got = buf.cpu().numpy().view(np.uint32)
    same(got[guard:guard + n], want, "the records of the grid that was counted")
    assert (got[:guard] == 0x5A5A5A5A).all() and (got[guard + n:] == 0x5A5A5A5A).all(), "the guard band was written"
    palette = (np.arange(256, dtype=np.uint32) * 0x01010101) ^ 0xFF000000
    buf.fill_(0x5A5A5A5A)
    torch.cuda.synchronize()
    dv.gather_write(*args, (9, 8, 7), hip.GATHER_COLOR_PALETTE, 0, None, None, palette.tolist(), 0, n, buf[guard:].data_ptr())
    got = buf.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[guard:guard + n, :3], want[:, :3]), "coordinates changed with the grid"
    assert np.isin(got[guard:guard + n, 3], palette).all()
    assert (got[:guard] == 0x5A5A5A5A).all() and (got[guard + n:] == 0x5A5A5A5A).all(), "the guard band was written"
    # the bytes read at the time of the write are the noise's
    noise = t.cpu().numpy()
    x, y, z = (want[:, 0] - 9).astype(np.int64), (want[:, 1] - 8).astype(np.int64), (want[:, 2] - 7).astype(np.int64)
    assert np.array_equal(got[guard:guard + n, 3], palette[noise[z, y, x]])
    print("compared", n, "records twice, guard bands of", guard, "records")


# ---- above_2_32 ------------------------------------------------------------------------------------------------------------------------

def case_above_2_32():
    dv = hip.DeviceVoxelizer(0)
    nx, ny, nz = 2048, 2048, 1025
    row = torch.ones(nx, dtype=torch.uint8, device=DEV)
    t = row[None, None, :].expand(nz, ny, nx)
    assert t.stride() == (0, 0, 1)
    scratch = dv.gather_scratch_bytes((nx, ny, nz))
    assert 0.8e9 < scratch < 0.83e9, scratch
    t0 = time.time()
    total = dense.count_voxels(dv, t)
    print("count", total, "in %.2f s" % (time.time() - t0), "stage times", dv.gather_times(), "scratch", scratch)
    assert total > 2 ** 32, total
    assert total == 2 ** 32 + 2 ** 22 == 4299161600
    for first in (2 ** 32 - 500, total - 1000):
        got = u32(dense.to_voxels(dv, t, first=first, count=1000))
        same(got, GR.closed_form_expanded_row(np.arange(first, first + 1000, dtype=np.uint64), nx, ny), ("records from", first))
    print("compared 2000 records either side of 2^32 and at the end")


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------

def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    verts = meshes.uv_sphere(16)
    T = len(verts)
    types = np.full(T, hip.TRI_UNTEXTURED, np.uint32)
    dense.set_mesh(dv, dev(verts), types=dev(types.view(np.int32)), colors=dev(meshes.triangle_colors(T)))
    occupancy, origin = dense.voxelize_dense(dv, 96, fill=True, fill_argb=0xFF102030)
    argb, _ = dense.voxelize_dense(dv, 96, fmt="argb", fill=True, fill_argb=0xFF102030)
    vox = dv.read_voxels()
    want = vox[np.lexsort((vox[:, 0], vox[:, 1], vox[:, 2]))]
    assert origin == (0, 0, 0) and len(np.unique(want[:, 3])) > 100 and (want[:, 3] == 0xFF102030).sum() > 1000
    same(u32(dense.to_voxels(dv, occupancy, colors=argb)), want, "to_voxels(occupancy, colors=argb) against read_voxels")
    assert bool((dense.from_voxels(dense.to_voxels(dv, occupancy, colors=argb), occupancy.shape, fmt="argb") == argb).all())
    print("sphere at 96:", len(want), "records, argb included")
    # the README's two cubes: solidify keeps the overlap, and its labels leave as a surface and a fill colour
    c = meshes.unit_cube().reshape(-1, 9)
    dense.set_mesh(dv, dev(np.concatenate([c * 16 + 4.03, c * 16 + 10.07]).astype(F)))
    surface, origin = dense.voxelize_dense(dv, 40, fmt="labels")
    solid = dense.solidify(dv, surface)
    palette = [0] * 256
    palette[1], palette[2] = 0xFFFFFFFF, 0xFF00FF00
    rec = dense.to_voxels(dv, solid, palette=palette)
    got, s = u32(rec), solid.cpu().numpy()
    same(got, GR.records(s, GR.U8, palette=palette), "solidify, labels != 0")
    n_surface = int((s == 1).sum())
    assert int((got[:, 3] == 0xFF00FF00).sum()) == 33636 and len(got) == 33636 + n_surface == int((s != 0).sum())
    assert bool((dense.from_voxels(rec, solid.shape) == (solid != 0)).all())
    print("pipeline:", len(got), "records,", n_surface, "surface and 33636 enclosed")


# ---- files -----------------------------------------------------------------------------------------------------------------------------

def case_files():
    from tests.test_gpu_io import _parse_vox
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(5)
    shades = np.array([0xFFFF0000, 0xFF00FF00, 0xFF0000FF, 0xFF102030, 0xFFFFFFFF, 0xFF000000, 0xFF808080], np.uint32)
    with tempfile.TemporaryDirectory() as tmp:
        # (130 and not 128 along x: 128^3 is 2^21 voxels, exactly two batches; this makes three and crosses 2^20 records twice)
        for name, dims, density, origin in (("small", (37, 20, 11), 0.3, (1, 2, 3)), ("three batches", (130, 128, 128), 0.99, (0, 0, 0))):
            solid = CR.random_grid(rng, dims, density)
            colors = shades[rng.integers(0, len(shades), solid.shape)].view(np.int32)
            want = GR.records(solid, GR.U8, origin=origin, colors=colors)
            assert name == "small" or 2 * 2 ** 20 < len(want) < 3 * 2 ** 20
            t, c = dev(solid), dev(colors)
            res = max(o + d for o, d in zip(origin, dims))
            times = {}
            for ext in ("vl32", "xyzrgb", "ply", "qef", "vox"):
                path = os.path.join(tmp, name.replace(" ", "_") + "." + ext)
                t0 = time.time()
                assert dense.save_voxels(dv, t, path, origin=origin, colors=c) == len(want)
                times[ext] = round(time.time() - t0, 2)
                data = open(path, "rb").read()
                if ext == "vl32":
                    assert data == want.astype(">u4").tobytes(), "the VL32 bytes are the big-endian records in gather order"
                    got = GR.parse_vl32(data)
                elif ext == "ply":
                    got = GR.parse_ply(data)
                    same(got, want, (name, ext, "in order"))
                elif ext == "xyzrgb":
                    got = GR.parse_xyzrgb(data)
                    same(got, want, (name, ext, "in order"))
                elif ext == "qef":
                    size, got = GR.parse_qef(data)
                    assert size == [res] * 3
                else:
                    models, trans, pal = _parse_vox(data)
                    assert len(models) == 1 and models[0][0] == (res,) * 3
                    got = GR.vox_records(models, trans, pal)
                same(GR.as_set(got), GR.as_set(want), (name, ext))
            print(name, dims, len(want), "records; save times (s)", times)
        # fmt= names the type whatever the extension; a constant colour; an explicit resolution
        path = os.path.join(tmp, "named.bin")
        assert dense.save_voxels(dv, t, path, fmt="vl32", argb=0xFF336699, resolution=512) == len(want)
        same(GR.parse_vl32(open(path, "rb").read()), GR.records(solid, GR.U8, argb=0xFF336699), "fmt=vl32")
        # an empty grid is an empty list
        path = os.path.join(tmp, "empty.ply")
        assert dense.save_voxels(dv, torch.zeros((3, 4, 5), dtype=torch.bool, device=DEV), path) == 0
        assert len(GR.parse_ply(open(path, "rb").read())) == 0
        # failures carry the library's message and code 6
        small = dev(CR.random_grid(rng, (9, 8, 7), 0.5))
        msg = expect_code(hip.ERR_IO, lambda: dense.save_voxels(dv, small, os.path.join(tmp, "no_such_dir", "a.vl32")), "an unwritable path")
        assert "o2v_hip_gather_save" in msg and "cannot open" in msg and "no_such_dir" in msg, msg
        obj = os.path.join(tmp, "a.obj")
        msg = expect_code(hip.ERR_IO, lambda: dense.save_voxels(dv, small, obj), "an .obj path")
        assert "not an output format" in msg and not os.path.exists(obj), msg
        msg = expect_code(hip.ERR_IO, lambda: dense.save_voxels(dv, small, os.path.join(tmp, "b.vl32"), fmt="obj"), "fmt=obj")
        assert "not an output format" in msg and not os.path.exists(os.path.join(tmp, "b.vl32")), msg
        assert dense.save_voxels(dv, small, os.path.join(tmp, "after.vl32")) == int(small.sum())   # the context stays usable
    print("compared 5 formats twice")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list, made before any launch; the context stays usable.  (This child runs with torch's
    caching allocator off: each tensor is an allocation of its own, so a short one is short.)"""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(1)
    N = 160                                    # a U8 grid of 4 MB; its short twin is half of it
    solid = CR.random_grid(rng, (N, N, N), 0.25)
    grid = dev(solid.astype(np.uint8))
    want = GR.records(solid, GR.U8, argb=5)
    n = len(want)                              # ~ 1 M records: 16 MB
    half = torch.zeros((N // 2, N, N), dtype=torch.uint8, device=DEV)
    field = torch.ones((N, N, N), dtype=torch.float32, device=DEV)
    words = torch.zeros((N, N, N // 32), dtype=torch.int32, device=DEV)
    colors = torch.zeros((N, N, N), dtype=torch.int32, device=DEV)
    rec = torch.full((n, 4), 7, dtype=torch.int32, device=DEV)
    short = torch.full((n // 4, 4), 7, dtype=torch.int32, device=DEV)   # at most a quarter of the records, and megabytes below them
    host, host_rec = np.zeros((N, N, N), np.uint8), np.zeros((n, 4), np.int32)
    torch.cuda.synchronize()
    st, dims, pal = (1, N, N * N), (N, N, N), list(range(256))
    C, G, P = hip.GATHER_COLOR_CONSTANT, hip.GATHER_COLOR_GRID, hip.GATHER_COLOR_PALETTE
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "refused.vl32")

    def count(ptr=grid.data_ptr(), fmt=hip.GRID_U8, strides=st, d=dims, level=0.0):
        return lambda: dv.gather_count(ptr, fmt, strides, d, level)

    def write(ptr=grid.data_ptr(), fmt=hip.GRID_U8, strides=st, d=dims, level=0.0, origin=(0, 0, 0), mode=C, cp=None, cs=None, palette=None,
              first=0, m=n, rp=rec.data_ptr()):
        return lambda: dv.gather_write(ptr, fmt, strides, d, level, origin, mode, 5, cp, cs, palette, first, m, rp)

    def save(ptr=grid.data_ptr(), fmt=hip.GRID_U8, strides=st, d=dims, level=0.0, origin=(0, 0, 0), mode=C, cp=None, cs=None, palette=None,
             p=path, file_type=None, resolution=N):
        return lambda: dv.gather_save(ptr, fmt, strides, d, level, origin, mode, 5, cp, cs, palette, p, file_type, resolution)
    bad, limit = hip.ERR_BAD_ARGUMENT, 5
    msgs = [expect_code(bad, write(), "a write without a count")]
    assert "no matching o2v_hip_gather_count" in msgs[0]
    assert dv.gather_count(*grid_args(grid, GR.U8)) == n
    for what, make in (("count", count), ("write", write), ("save", save)):
        msgs += [
            expect_code(bad, make(ptr=None), what + ": null grid"),
            expect_code(bad, make(d=(N, 0, N)), what + ": zero dims"),
            expect_code(bad, make(fmt=3), what + ": unknown format"),
            expect_code(bad, make(ptr=words.data_ptr(), fmt=hip.GRID_BITS, strides=(2, N // 32, N * N // 32)), what + ": BITS with an x stride of 2"),
            expect_code(bad, make(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("nan")), what + ": a NaN level"),
            expect_code(bad, make(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("inf")), what + ": an infinite level"),
            expect_code(bad, make(ptr=host.ctypes.data), what + ": a host grid"),
            expect_code(bad, make(ptr=half.data_ptr()), what + ": a short grid"),
            expect_code(limit, make(d=(65537, 1, 1), strides=(0, 0, 0)), what + ": a dim above 65 536"),
            expect_code(limit, make(d=(1, 65536, 32768), strides=(0, 0, 0)), what + ": 2^31 words"),
        ]
        assert "2147483648 words" in msgs[-1]
    # (the refused counts replaced the last one)
    assert "no matching" in expect_code(bad, write(), "a write after refused counts")
    assert dv.gather_count(*grid_args(grid, GR.U8)) == n
    for what, make in (("write", write), ("save", save)):
        msgs += [
            expect_code(bad, make(mode=3), what + ": unknown colour mode"),
            expect_code(bad, make(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, mode=P, palette=pal), what + ": a palette with a float grid"),
            expect_code(bad, make(mode=P), what + ": PALETTE without a palette"),
            expect_code(bad, make(mode=G), what + ": GRID without colours"),
            expect_code(bad, make(mode=G, cp=colors.data_ptr()), what + ": GRID without colour strides"),
            expect_code(bad, make(mode=G, cp=host.ctypes.data, cs=st), what + ": host colours"),
            expect_code(bad, make(mode=G, cp=half.data_ptr(), cs=st), what + ": short colours"),
            expect_code(limit, make(origin=(2 ** 32 - N + 1, 0, 0)), what + ": origin + dims above 2^32"),
        ]
        if what == "save":
            assert dv.gather_count(*grid_args(grid, GR.U8)) == n     # (a save, refused or not, replaces the count)
    msgs += [
        expect_code(bad, write(first=1), "first + n above the count"),
        expect_code(bad, write(first=n + 1, m=0), "first above the count"),
        expect_code(bad, write(first=2 ** 64 - 1, m=2), "first + n wraps"),
        expect_code(bad, write(rp=None), "null records"),
        expect_code(bad, write(rp=host_rec.ctypes.data), "host records"),
        expect_code(bad, write(rp=short.data_ptr()), "short records"),
        expect_code(bad, write(rp=rec.data_ptr() + 4, m=n - 1), "records off a 16-byte boundary"),
        expect_code(bad, write(rp=grid.data_ptr(), m=1000), "records in the grid"),
        expect_code(bad, write(mode=G, cp=rec.data_ptr(), cs=(1, 0, 0), m=1000), "records in the colours"),
        expect_code(bad, write(strides=(1, N, N * N - 1)), "other strides than counted"),
        expect_code(bad, write(d=(N, N, N - 1)), "other dims than counted"),
        expect_code(bad, save(origin=(1, 0, 0)), "origin + dims above the resolution"),
        expect_code(bad, save(resolution=N - 1), "dims above the resolution"),
        expect_code(bad, save(p=None), "a null path"),
    ]
    assert "no matching" in msgs[-5] and "no matching" in msgs[-4]
    torch.cuda.synchronize()
    assert bool((rec == 7).all()) and bool((short == 7).all()) and not os.path.exists(path), "a refused call wrote something"
    assert np.array_equal(grid.cpu().numpy(), solid.astype(np.uint8))
    # a level that differs from the counted one: no match, F32 only matters here through the bits compared
    assert dv.gather_count(field.data_ptr(), hip.GRID_F32_BELOW, st, dims, 2.0) == N ** 3
    assert "no matching" in expect_code(bad, write(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=2.5, m=10), "another level than counted")
    # the context stays usable
    assert dv.gather_count(*grid_args(grid, GR.U8)) == n
    write()()
    same(u32(rec), want, "after the refusals")
    assert save()() == n and os.path.getsize(path) == 16 * n
    os.remove(path)
    os.rmdir(tmp)
    print("ok refusals:", len(msgs), "refused; last:", msgs[-3])


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]]()
    print("ok")
