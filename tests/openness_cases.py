"""The GPU cases of tests/test_gpu_openness.py, each run in a child process of its own: `python -m tests.openness_cases <case>`.

torch is imported before the library is loaded (the grids are torch tensors; see tests/dense_cases.py).  Every comparison is bit for
bit and covers every voxel of dst and mask - against the numpy reference of tests/openness_ref.py or against closed forms, never
against the code under test, and there is no tolerance anywhere.  The outputs are filled with a guard value before every call.  A
case prints what it covered and "ok" last when everything held."""
import os
import sys
import tempfile
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import openness_ref as R

DEV = torch.device("cuda", 0)
U8, BITS, F32 = hip.GRID_U8, hip.GRID_BITS, hip.GRID_F32_BELOW
MODES = {"surface": hip.OPEN_SURFACE, "solid": hip.OPEN_SOLID, "empty": hip.OPEN_EMPTY}
CUSTOM = [(127, 1, 0), (0, 0, -1), (3, -5, 7), (-2, -2, 1), (1, 126, -127)]
GUARD, MASK_GUARD = 0x5a, -0x5a5a5a5a5a5a5a5b


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def st(t):
    """(x, y, z) element strides of a tensor [z, y, x]."""
    return t.stride(2), t.stride(1), t.stride(0)


def directions_of(which):
    return CUSTOM if which == "custom" else [tuple(v) for v in R.direction_set(which).tolist()]


def call(dv, t, fmt, dims, level, dirs, mode, md2, mask, strided_out=False):
    """o2v_hip_openness at the C level on the tensor view t into guarded outputs: (count, mask or None, targets) as numpy arrays,
    after the guards around strided outputs are seen intact.  mode: a name or a numpy bool grid."""
    nx, ny, nz = dims
    tgrid = None if isinstance(mode, str) else dev(mode)
    if strided_out:
        wide, wide_m = torch.full((nz, ny, 2 * nx + 1), GUARD, dtype=torch.uint8, device=DEV), torch.full((nz, 2 * ny, nx), MASK_GUARD, dtype=torch.int64, device=DEV)
        dst, mk = wide[:, :, 1::2], wide_m[:, 1::2, :]
    else:
        dst, mk = torch.full((nz, ny, nx), GUARD, dtype=torch.uint8, device=DEV), torch.full((nz, ny, nx), MASK_GUARD, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    n = dv.openness(t.data_ptr(), fmt, st(t), dims, level, dirs, MODES[mode] if tgrid is None else hip.OPEN_GRID, None if tgrid is None else tgrid.data_ptr(),
                    None if tgrid is None else st(tgrid), md2, dst.data_ptr(), st(dst), mk.data_ptr() if mask else None, st(mk) if mask else None)
    if strided_out:
        assert bool((wide[:, :, ::2] == GUARD).all()) and bool((wide_m[:, ::2, :] == MASK_GUARD).all())
    if not mask:
        assert bool((mk == MASK_GUARD).all())
    return dst.cpu().numpy(), mk.cpu().numpy() if mask else None, n


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "count", int((got[0] != want[0]).sum()), np.argwhere(got[0] != want[0])[:4].tolist())
    assert (got[1] is None) == (want[1] is None) and (got[1] is None or np.array_equal(got[1], want[1])), (what, "mask")
    assert got[2] == int((want[0] != 255).sum()), (what, "targets", got[2])


# ---- shapes and formats -----------------------------------------------------------------------------------------------------------

def layouts(g):
    """(name, format, tensor view, level) of the grid g [z, y, x] (bool) in every format and layout of the case."""
    nz, ny, nx = g.shape
    t = dev(g)
    out = [("bool, contiguous", U8, t, 0.0)]
    flat = torch.zeros(g.size + 40, dtype=torch.uint8, device=DEV)
    flat[1:1 + g.size] = t.reshape(-1) * 5
    out.append(("uint8, one element into an allocation", U8, flat[1:1 + g.size].view(g.shape), 0.0))
    wide = torch.zeros((nz, ny, 2 * nx), dtype=torch.uint8, device=DEV)
    wide[:, :, ::2] = t
    out.append(("uint8, x stride 2", U8, wide[:, :, ::2], 0.0))
    out.append(("bool, x and z swapped", U8, t.permute(2, 1, 0).contiguous().permute(2, 1, 0), 0.0))
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


def case_shapes_and_formats():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(320)
    calls = 0
    used = {"layout": set(), "set": set(), "mode": set(), "cut": set()}
    sets, modes, cuts = (6, 26, 98, "custom"), ("surface", "solid", "empty", "grid"), (None, 1, 2.5, 16)
    for dims in ((1, 1, 1), (5, 6, 7), (17, 4, 3), (65, 9, 4), (70, 67, 66), (130, 20, 18)):
        nx, ny, nz = dims
        for density in (0.001, 0.05, 0.6):
            g = R.blobs(rng, dims, density)
            views = layouts(g)
            for k in range(8):
                # every layout once per grid; the set, the mode and the cut-off rotate against each other over the calls
                what, fmt, t, level = views[k]
                which, mode_name, cut = sets[calls % 4], modes[(calls // 4 + calls) % 4], cuts[(calls // 16 + calls // 4 + calls) % 4]
                mode = (rng.random(g.shape) < 0.3) if mode_name == "grid" else mode_name
                tg = R.targets(g, mode)
                dirs, md2 = directions_of(which), R.max_distance2(cut)
                rays = int(tg.sum()) * len(dirs) * {None: 10, 1: 1, 2.5: 3, 16: 10}[cut]
                if rays > 600000:
                    # (too many voxels for the reference to walk from: a sample of them, as a target grid)
                    mode, mode_name = tg & (rng.random(g.shape) < 600000.0 / rays), "grid"
                mask = len(dirs) <= 64 and calls % 3 != 2
                want = R.openness(g, dirs, mode, md2, mask=mask)
                same(call(dv, t, fmt, dims, level, dirs, mode, md2, mask, strided_out=calls % 2 == 1), want, (dims, density, what, which, mode_name, cut))
                for key, v in (("layout", what), ("set", which), ("mode", mode_name), ("cut", cut)):
                    used[key].add(v)
                calls += 1
    assert len(used["layout"]) == 8 and used["set"] == set(sets) and used["mode"] == set(modes) and used["cut"] == set(cuts), used
    # the torch layer on the device: bool, float32 with a level and the words of fmt="bits", out= as a view, a bool target tensor
    g = R.blobs(rng, (64, 9, 5), 0.05)
    t = dev(g)
    wide = torch.full((5, 9, 129), GUARD, dtype=torch.uint8, device=DEV)
    out = dense.openness(dv, t, directions=98, max_distance=2.5, out=wide[:, :, 1::2])
    assert out.data_ptr() == wide[:, :, 1::2].data_ptr() and np.array_equal(out.cpu().numpy(), R.openness(g, 98, "surface", 6)[0]) and bool((wide[:, :, ::2] == GUARD).all())
    words = dev(np.packbits(g, axis=-1, bitorder="little").view("<i4"))
    tg = rng.random(g.shape) < 0.5
    got = dense.openness(dv, words, directions=torch.tensor(CUSTOM), targets=dev(tg), mask=True)
    want = R.openness(g, CUSTOM, tg, 0, mask=True)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    f = dev(np.where(g, -1.0, 1.0).astype(np.float32))
    assert np.array_equal(dense.openness(dv, f, level=0.0, targets="empty", max_distance=16).cpu().numpy(), R.openness(g, 26, "empty", 256)[0])
    assert np.array_equal((dense.openness(dv, t, directions=[(1, 2, 3)]) == 0).cpu().numpy(), R.openness(g, [(1, 2, 3)])[0] == 0)
    assert len(dv.openness_times()) == 3 and all(v >= 0 for v in dv.openness_times())
    print("shapes_and_formats: compared", calls, "calls on 18 grids in", len(used["layout"]), "formats and layouts,", len(sets), "direction sets,", len(modes),
          "target modes and", len(cuts), "cut-offs, and 4 calls of the torch layer")


# ---- skip equals fine -------------------------------------------------------------------------------------------------------------

def case_skip_equals_fine():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(321)
    dims = (130, 70, 70)
    g = np.zeros((70, 70, 130), bool)
    for _ in range(7):
        g[int(rng.integers(0, 64)), int(rng.integers(0, 64)), int(rng.integers(0, 64))] = True   # (a handful, all in the first 64^3 block)
    g[69, 69, 129] = True
    pyr = R.pyramid(g)
    empty = {L: int((~pyr[L]).sum()) for L in (6, 4, 2)}
    assert empty[6] >= 4 and pyr[6].size == 3 * 2 * 2
    tg = rng.random(g.shape) < 0.003
    tg |= g
    n = 0
    for dirs, md2, mask in ((directions_of(98), 0, False), (directions_of("custom"), 0, True), (directions_of(26), 256, True), (directions_of(6), 6, True)):
        want = R.openness(g, dirs, tg, md2, mask=mask)
        got = {}
        for no_skip in ("0", "1"):
            os.environ["O2V_OPEN_NO_SKIP"] = no_skip   # (read at the entry of every call)
            got[no_skip] = call(dv, dev(g), U8, dims, 0.0, dirs, tg, md2, mask)
            same(got[no_skip], want, ("no_skip", no_skip, len(dirs), md2))
        assert got["0"][0].tobytes() == got["1"][0].tobytes() and (not mask or got["0"][1].tobytes() == got["1"][1].tobytes())
        n += 1
    os.environ.pop("O2V_OPEN_NO_SKIP")
    print("skip_equals_fine:", n, "calls with and without O2V_OPEN_NO_SKIP=1 gave equal bytes on 130x70x70 with", int(g.sum()), "voxels;", empty[6], "of", pyr[6].size,
          "64^3 blocks,", empty[4], "of", pyr[4].size, "16^3 blocks and", empty[2], "of", pyr[2].size, "4^3 blocks are empty")


# ---- closed forms -----------------------------------------------------------------------------------------------------------------

def counts_on_device(dv, g, n, mode="surface"):
    """int [z, y, x]: the open directions of set n (290: in two halves of 145, added), -1 where no target."""
    d = directions_of(n)
    total = None
    for part in ([d] if len(d) <= 254 else [d[:145], d[145:]]):
        got = dense.openness(dv, dev(g), directions=part, targets=mode).cpu().numpy()
        total = got.astype(np.int64) if total is None else total + got
        target = got != 255
    return np.where(target, total, -1)


def case_closed_forms():
    dv = hip.DeviceVoxelizer(0)
    box = R.box_in(12, 1, 11)
    for n, face, edge, corner in ((6, 1, 2, 3), (26, 9, 15, 19), (98, 25, 45, 61), (290, 65, 121, 169)):
        got = counts_on_device(dv, box, n)
        assert (got[10, 5, 5], got[10, 1, 5], got[10, 1, 1]) == (face, edge, corner), (n, got[10, 5, 5], got[10, 1, 5], got[10, 1, 1])
        assert np.array_equal(got, R.open_counts(box, n))
    hollow = R.box_in(12, 1, 11, hollow=True)
    inner = np.zeros_like(hollow)
    inner[2:10, 2:10, 2:10] = True
    for n in (26, 98):
        got = counts_on_device(dv, hollow, n, "empty")
        assert (got[inner] == 0).all() and (got[~inner & ~hollow] > 0).all() and (got[hollow] == -1).all()
    for depth, want in ((1, (9, 25, 65)), (2, (1, 1, 9)), (3, (1, 1, 1))):
        g, floor = R.shaft(depth)
        assert tuple(int(counts_on_device(dv, g, n, "empty")[floor[2], floor[1], floor[0]]) for n in (26, 98, 290)) == want, depth
    ball = R.ball()
    assert tuple(int(counts_on_device(dv, ball, n)[30, 16, 16]) for n in (26, 98, 290)) == (17, 57, 161)
    lone = np.zeros((5, 5, 5), bool)
    lone[2, 2, 2] = True
    for n in (6, 26, 98, 290):
        got = counts_on_device(dv, lone, n)
        assert got[2, 2, 2] == n and (got == -1).sum() == 124
    count, mask = dense.openness(dv, dev(lone), mask=True)
    assert int(mask[2, 2, 2]) == 2 ** 26 - 1 and int(mask.abs().sum()) == 2 ** 26 - 1
    print("closed_forms: the box's face, edge and corner (65, 121, 169 of 290), the hollow box, the shafts, the ball's top (17, 57, 161) and the lone voxel")


# ---- determinism ------------------------------------------------------------------------------------------------------------------

def case_determinism():
    rng = np.random.default_rng(322)
    dims = (100, 90, 80)
    g_np = R.blobs(rng, dims, 0.02)
    g = dev(g_np)
    dv, other = hip.DeviceVoxelizer(0), hip.DeviceVoxelizer(0)
    # a RayCaster built before: its hits and its generation are the same after the calls
    caster = dense.RayCaster(dv, g)
    generation = dv.raycast_generation()
    origins = dev(rng.random((4096, 3)).astype(np.float32) * np.array(dims, np.float32))
    directions = dev(rng.standard_normal((4096, 3)).astype(np.float32))
    hit0, t0 = caster.cast(origins, directions)
    dirs = directions_of(26)
    first = call(dv, g, U8, dims, 0.0, dirs, "surface", 0, True)
    n = 0
    for d in (dv, other, dv, other):
        again = call(d, g, U8, dims, 0.0, dirs, "surface", 0, True)
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes() and again[2] == first[2]
        n += 1
    # (a grid of another size in between: the scratch is regrown, the snapshot stays)
    small = R.blobs(rng, (200, 100, 90), 0.01)
    same(call(dv, dev(small), U8, (200, 100, 90), 0.0, directions_of(6), "surface", 0, True), R.openness(small, 6, "surface", 0, mask=True), "another size")
    same(first, R.openness(g_np, 26, "surface", 0, mask=True), "the reference")
    assert dv.raycast_generation() == generation
    hit1, t1 = caster.cast(origins, directions)
    assert torch.equal(hit0, hit1) and torch.equal(t0.view(torch.int32), t1.view(torch.int32)) and int((hit0[:, 3] >= 0).sum()) > 100
    print("determinism:", n, "repeated calls on two contexts gave equal bytes; the RayCaster built before casts the same", int((hit0[:, 3] >= 0).sum()),
          "hits, generation", generation)


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------

def indexed(verts):
    positions, faces = np.unique(np.asarray(verts, np.float32).reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    return dev(positions.view(np.float32)), dev(faces.reshape(-1, 3).astype(np.int32))


def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, *indexed(meshes.scan_like()))
    labels, origin = dense.voxelize_dense(dv, 128, fmt="labels", fill=True)
    solid = labels != 0
    count = dense.openness(dv, solid, directions=26, max_distance=16)
    want = R.openness(solid.cpu().numpy(), 26, "surface", 256)[0]
    assert np.array_equal(count.cpu().numpy(), want)
    surface = int((want != 255).sum())
    argb = torch.where(solid, torch.tensor(-0x3f7f40, dtype=torch.int32, device=DEV), torch.zeros((), dtype=torch.int32, device=DEV))   # 0xffc080c0
    shaded = dense.shade_colors(argb, count, 26)
    assert torch.equal(shaded.cpu(), dense.shade_colors(argb.cpu(), count.cpu(), 26)) and torch.equal(shaded[count == 255], argb[count == 255])
    darker = int(((shaded & 0xff) < (argb & 0xff)).sum())
    assert 0 < darker <= surface and bool((((shaded >> 24) & 0xff) == ((argb >> 24) & 0xff)).all())
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "shaded.vox")
        n = dense.save_voxels(dv, solid, path, origin=origin, colors=shaded)
        head, size = open(path, "rb").read(4), os.path.getsize(path)
    assert head == b"VOX " and size > 4 * n
    rec = dense.to_voxels(dv, solid, origin=origin, colors=shaded)
    assert n == len(rec) == int(solid.sum())
    grid_back = dense.from_voxels(rec, tuple(solid.shape), origin=origin, fmt="argb")
    assert torch.equal(grid_back != 0, solid) and torch.equal(grid_back[solid], shaded[solid])
    print("pipeline: scan_like at 128, filled:", int(solid.sum()), "voxels,", surface, "on the surface,", darker, "of them darkened;", n, "voxels saved as .vox (%d bytes) and gathered back with their colours" % size)


# ---- magnitudes -------------------------------------------------------------------------------------------------------------------

def case_magnitudes():
    """65 536 x 2 x 2: (2 K - 1) * m reaches its bound with m = 127, the cut-off's squares pass 2^32.  The rays along x are too
    long for the reference to walk: the closed form of openness_ref.open_along_x stands in for it there."""
    dv = hip.DeviceVoxelizer(0)
    dims = (65536, 2, 2)
    g = np.zeros((2, 2, 65536), bool)
    g[1, 1, 40000] = g[0, 0, 3] = True
    short = [(127, 1, 0), (-127, 0, 1), (-126, 1, 1), (0, 0, 1), (127, -1, -1), (5, 0, -1)]
    along = [(1, 0, 0), (-1, 0, 0), (127, 0, 0), (-127, 0, 0)]
    tg = np.zeros_like(g)
    for x in (0, 1, 2, 3, 4, 39999, 40001, 65535, 32768):
        tg[:, :, x] = True
    t = dev(g)
    n = 0
    t0 = time.time()
    for md2 in (0, 2 ** 32 - 1, 65535 ** 2, 39996 ** 2, 39995 ** 2):
        want = R.openness(g, short, tg, md2, mask=True)
        want_x = np.stack([R.open_along_x(g, tg, 1 if d[0] > 0 else -1, md2) for d in along], 1)
        for no_skip in ("0", "1"):
            os.environ["O2V_OPEN_NO_SKIP"] = no_skip
            same(call(dv, t, U8, dims, 0.0, short, tg, md2, True), want, (md2, no_skip))
            got = call(dv, t, U8, dims, 0.0, along, tg, md2, True)
            assert np.array_equal((got[1][tg][:, None] >> np.arange(4)) & 1, want_x) and (got[0][~tg] == 255).all() and not got[1][~tg].any(), (md2, no_skip)
            assert np.array_equal(got[0][tg], want_x.sum(1)) and got[2] == int(tg.sum())
            n += 2
    os.environ.pop("O2V_OPEN_NO_SKIP")
    print("magnitudes:", n, "calls at 65 536 x 2 x 2 with m = 127 and cut-offs up to 2^32 - 1, with and without the skip; %.2f s" % (time.time() - t0))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list but the failed scratch allocation.  This child runs with torch's caching allocator off:
    each tensor is an allocation of its own, so a short one is short."""
    dv = hip.DeviceVoxelizer(0)
    L = hip._bind()
    C = hip.C
    n = 24
    dims, s = (n, n, n), (1, n, n * n)
    g_np = R.blobs(np.random.default_rng(323), dims, 0.05)
    grid, short, byte = dev(g_np), dev(g_np[:n // 2]), torch.zeros((1, 1, 1), dtype=torch.uint8, device=DEV)
    f32 = dev(g_np.astype(np.float32))
    tgrid = dev(g_np)
    host_grid = g_np.copy()
    dst = torch.full((n, n, n), GUARD, dtype=torch.uint8, device=DEV)
    mask = torch.full((n, n, n), MASK_GUARD, dtype=torch.int64, device=DEV)
    short8, short64 = torch.zeros((n - 1, n, n), dtype=torch.uint8, device=DEV), torch.zeros((n - 1, n, n), dtype=torch.int64, device=DEV)
    both = torch.full((n ** 3 + 1,), MASK_GUARD, dtype=torch.int64, device=DEV)   # (a grid and a mask in one allocation)
    host8, host64 = np.zeros(n ** 3, np.uint8), np.zeros(n ** 3, np.int64)
    s8 = tuple(8 * v for v in s)
    u3 = lambda a: None if a is None else (C.c_uint32 * 3)(*a)    # noqa: E731
    u64 = lambda a: None if a is None else (C.c_uint64 * 3)(*a)   # noqa: E731
    d26 = directions_of(26)
    msgs = []
    torch.cuda.synchronize()

    def no(code, what, ctx=dv._ctx, p=grid.data_ptr(), fmt=U8, strides=s, dm=dims, level=0.0, dirs=d26, nd=None, mode=hip.OPEN_SURFACE, tp=None, ts=None, md2=0,
           flags=0, d=dst.data_ptr(), ds=s, m=None, ms=None, out=True):
        flat = None if dirs is None else (C.c_int32 * (3 * len(dirs)))(*[v for row in dirs for v in row])
        got = C.c_uint64(99)
        rc = L.o2v_hip_openness(ctx, p, fmt, u64(strides), u3(dm), level, flat, len(dirs) if nd is None else nd, mode, tp, u64(ts), md2, flags, d, u64(ds), m, u64(ms),
                                C.byref(got) if out else None)
        assert rc == code and got.value == 99, (what, rc)
        if ctx:
            msgs.append(what + ": " + L.o2v_hip_last_error(ctx).decode())
            assert "o2v_hip_openness" in msgs[-1], msgs[-1]
        else:
            msgs.append(what)
        assert bool((dst == GUARD).all()) and bool((mask == MASK_GUARD).all()) and bool((both == MASK_GUARD).all()), what

    with_mask = dict(m=mask.data_ptr(), ms=s)
    for what, kw in [
        ("null context", dict(ctx=None)), ("null grid", dict(p=None)), ("null strides", dict(strides=None)), ("null dims", dict(dm=None)),
        ("zero dims", dict(dm=(n, 0, n))), ("unknown format", dict(fmt=3)), ("a BITS grid with x stride 2", dict(fmt=BITS, strides=(2, n, n * n))),
        ("a level that is not finite", dict(p=f32.data_ptr(), fmt=F32, level=float("nan"))), ("short grid", dict(p=short.data_ptr())),
        ("host grid", dict(p=host_grid.ctypes.data)), ("null directions", dict(dirs=None, nd=26)), ("no directions", dict(nd=0)),
        ("a zero direction", dict(dirs=[(1, 0, 0), (0, 0, 0)])), ("a component of 128", dict(dirs=[(1, 0, 0), (0, 128, 1)])),
        ("a component of -128", dict(dirs=[(-128, 0, 0)])), ("a mask with 65 directions", dict(dirs=directions_of(98)[:65], **with_mask)),
        ("unknown target mode", dict(mode=4)), ("unknown flag bits", dict(flags=64)), ("null dst", dict(d=None)), ("null dst strides", dict(ds=None)),
        ("null mask strides", dict(m=mask.data_ptr())), ("null out_targets", dict(out=False)), ("mask not 8-byte aligned", dict(m=mask.data_ptr() + 4, ms=s)),
        ("target mode GRID without a grid", dict(mode=hip.OPEN_GRID, ts=s)), ("target mode GRID without strides", dict(mode=hip.OPEN_GRID, tp=tgrid.data_ptr())),
        ("short target grid", dict(mode=hip.OPEN_GRID, tp=short.data_ptr(), ts=s)), ("host target grid", dict(mode=hip.OPEN_GRID, tp=host_grid.ctypes.data, ts=s)),
        ("dst strides that map two voxels to one element", dict(ds=(1, n, 0))), ("mask strides that map two voxels to one element", dict(m=mask.data_ptr(), ms=(1, 0, n * n))),
        ("short dst", dict(d=short8.data_ptr())), ("short mask", dict(m=short64.data_ptr(), ms=s)), ("host dst", dict(d=host8.ctypes.data)),
        ("host mask", dict(m=host64.ctypes.data, ms=s)), ("dst overlaps the grid", dict(d=grid.data_ptr())),
        ("dst overlaps the target grid", dict(mode=hip.OPEN_GRID, tp=tgrid.data_ptr(), ts=s, d=tgrid.data_ptr())),
        ("dst overlaps mask", dict(d=mask.data_ptr(), ds=s8, **with_mask)), ("mask overlaps the grid", dict(p=both.data_ptr() + 16, m=both.data_ptr() + 8, ms=s)),
    ]:
        no(3, what, **kw)
    for what, kw in [
        ("255 directions", dict(dirs=[(1, 0, 0)] * 255)), ("65 537 voxels along x", dict(p=byte.data_ptr(), dm=(65537, 1, 1), strides=(0, 0, 0))),
        ("2^31 voxels", dict(p=byte.data_ptr(), dm=(1024, 1024, 2048), strides=(0, 0, 0))),
    ]:
        no(5, what, **kw)
    for t in msgs:
        what, _, err = t.partition(": o2v_hip")
        assert "overlap" not in what or "overlap" in err, t
    assert L.o2v_hip_openness_times(None, None) == 3 and hip.openness_scratch_bytes((0, 1, 1)) == 0
    # then a correct call: the context still works
    got = call(dv, grid, U8, dims, 0.0, d26, g_np, 6, True)
    same(got, R.openness(g_np, 26, g_np, 6, mask=True), "at the end")
    print("\n".join(msgs))
    assert len(msgs) == 40
    print("refused", len(msgs), "calls")


# ---- one call per case and its wall time ------------------------------------------------------------------------------------------

CASES = {"shapes_and_formats": case_shapes_and_formats, "skip_equals_fine": case_skip_equals_fine, "closed_forms": case_closed_forms, "determinism": case_determinism,
         "pipeline": case_pipeline, "magnitudes": case_magnitudes, "refusals": case_refusals}

if __name__ == "__main__":
    t0 = time.time()
    CASES[sys.argv[1]]()
    print("case", sys.argv[1], "took %.1f s" % (time.time() - t0))
    print("ok")
