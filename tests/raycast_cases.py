"""The GPU cases of tests/test_gpu_raycast.py, each run in a child process of its own: `python -m tests.raycast_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison with the reference
(tests/raycast_ref.py, the fine walk of include/o2v_hip.h) is bit for bit: hit as int32, t as the uint32 bits of its float32
(so +inf and NaN count).  A case prints what it covered and "ok" last when everything held."""
import os
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import fill_ref
from tests import raycast_ref as R
from tests.dense_cases import expect_code3

DEV = torch.device("cuda", 0)
F = np.float32
INF = float("inf")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)   # (a copy: views of broadcast arrays are not writable)


def cast(caster, o, d, t_max=INF):
    """The device's (hit, t) of float32 rays [n, 3] as numpy arrays."""
    hit, t = caster.cast(dev(o), dev(d), t_max)
    assert hit.dtype == torch.int32 and t.dtype == torch.float32 and hit.is_contiguous() and t.is_contiguous()
    return hit.cpu().numpy(), t.cpu().numpy()


def compare(got, want, what, o=None, d=None):
    bad = np.nonzero((got[0] != want[0]).any(axis=1) | (got[1].view(np.uint32) != want[1].view(np.uint32)))[0]
    detail = () if o is None or not len(bad) else (o[bad[:3]], d[bad[:3]])
    assert len(bad) == 0, (what, len(bad), "of", len(want[0]), bad[:5], got[0][bad[:3]], want[0][bad[:3]], got[1][bad[:3]], want[1][bad[:3]]) + detail


def no_skip(on):
    """O2V_RAY_NO_SKIP for the calls that follow (the library reads its switches at every call)."""
    if on:
        os.environ["O2V_RAY_NO_SKIP"] = "1"
    else:
        os.environ.pop("O2V_RAY_NO_SKIP", None)


# ---- the grids of formats_and_shapes and no_skip_ab: one solid set in three formats and several layouts ----------------------

GRIDS = [  # (nx, ny, nz), origin, density
    ((1, 37, 29), (5, 0, 9), 0.05), ((3, 40, 33), (0, 0, 0), 0.03), ((4, 31, 18), (7, 7, 7), 0.03), ((5, 22, 45), (0, 3, 0), 0.03),
    ((63, 20, 18), (1, 2, 3), 0.01), ((64, 17, 21), (0, 0, 0), 0.01), ((65, 19, 16), (100, 2000, 30000), 0.01),
    ((130, 70, 67), (65536 - 160, 0, 65536 - 67), 0.0015), ((40, 1, 30), (3, 9, 4), 0.04), ((33, 29, 1), (0, 0, 11), 0.04),
    ((200, 150, 90), (17, 0, 40), 0.0004),
]


def formats(solid, rng):
    """(name, tensor [z, y, x], level) in the three formats, plain contiguous tensors."""
    labels = np.where(solid, rng.choice(np.array([1, 2, 255], np.uint8), solid.shape), 0).astype(np.uint8)
    field = np.where(solid, -rng.random(solid.shape) - 0.01, rng.random(solid.shape) + 0.25).astype(F)
    field[~solid & (rng.random(solid.shape) < 0.1)] = np.nan
    field[~solid & (rng.random(solid.shape) < 0.05)] = 0.25       # (equal to the level: not below it)
    field[solid & (rng.random(solid.shape) < 0.1)] = -np.inf
    return [("bool", dev(solid), None), ("labels", dev(labels), None), ("bits", dev(R.pack_bits(solid)), None), ("f32", dev(field), 0.25)]


def layouts(name, t):
    """(layout, view) of a contiguous device tensor [z, y, x]: the same elements stored in other ways."""
    nz, ny, nx = t.shape
    out = []
    if name != "bits":
        out.append(("x and z swapped in memory", t.permute(2, 1, 0).contiguous().permute(2, 1, 0)))
        wide = torch.zeros((nz, ny, 2 * nx), dtype=t.dtype, device=DEV)
        wide[:, :, ::2] = t
        wide[:, :, 1::2] = 1                                       # (what lies between must not be read as a voxel)
        out.append(("every second element along x", wide[:, :, ::2]))
    out.append(("y and z swapped in memory", t.permute(1, 0, 2).contiguous().permute(1, 0, 2)))
    batch = torch.ones((3, nz, ny, nx), dtype=t.dtype, device=DEV)
    batch[1] = t
    out.append(("slice of a batch", batch[1]))
    big = torch.ones((nz + 3, ny + 5, nx + 7), dtype=t.dtype, device=DEV)
    big[2:2 + nz, 3:3 + ny, 5:5 + nx] = t
    out.append(("box inside a larger tensor", big[2:2 + nz, 3:3 + ny, 5:5 + nx]))
    rows = torch.ones((nz, ny, (nx + 31) // 16 * 16), dtype=t.dtype, device=DEV)   # rows padded to 16 elements: aligned rows with a tail
    rows[:, :, :nx] = t
    out.append(("padded rows", rows[:, :, :nx]))
    for _, v in out:
        assert tuple(v.shape) == tuple(t.shape) and bool((v == t).all() if t.dtype != torch.float32 else (v.view(torch.int32) == t.view(torch.int32)).all())
    return out


def ray_sets(seed):
    """(name, solid, origin, o, d, reference for t_max = inf) per grid, the expanded grids behind them."""
    rng = np.random.default_rng(seed)
    for dims, origin, density in GRIDS:
        yield str(dims), R.random_solid(rng, dims, density), origin, rng
    # voxels that share elements: a layer expanded along z, a plane expanded along x
    layer = R.random_solid(rng, (50, 40, 1), 0.02)
    yield "expanded z", np.broadcast_to(layer, (30, 40, 50)), (4, 5, 6), rng
    plane = R.random_solid(rng, (1, 40, 30), 0.02)
    yield "expanded x", np.broadcast_to(plane, (30, 40, 50)), (0, 0, 0), rng


def checked_set(name, solid, origin, rng, n=20000):
    o, d = R.ray_set(rng, solid, origin, n)
    assert len(o) >= n
    t0 = time.time()
    want = R.cast(solid, origin, o, d)
    hits, misses = R.shares(want[0])
    print(f"{name}: {len(o)} rays, hit {hits:.3f}, miss {misses:.3f}, {want[2]} fine steps, reference {time.time() - t0:.1f} s", flush=True)
    assert hits >= 0.2 and misses >= 0.2, (name, hits, misses)     # a condition on the inputs, by the reference alone
    return o, d, want


def finite_t_max(caster, solid, origin, o, d, rng, what):
    """A seeded part of the set again with finite t_max: 0, a few cells, and one ray's own T exactly."""
    near = np.nonzero(R.distance_to_box(solid, origin, o) < R.FAR)[0]
    sub = rng.choice(near, min(len(near), 2500), replace=False)
    own = R.cast_lockstep(solid, origin, o[sub], d[sub])[1]
    own = own[np.isfinite(own) & (own > 0)]
    for t_max in [0.0, 3.5, 60.0] + ([float(own[len(own) // 2])] if len(own) else []):
        compare(cast(caster, o[sub], d[sub], t_max), R.cast_lockstep(solid, origin, o[sub], d[sub], t_max)[:2], (what, "t_max", t_max))


def expanded_tensor(name, a):
    """The array [z, y, x], constant along z or x, as a device tensor that holds one layer / one plane of it (stride 0)."""
    t = dev(a[:1]).expand(a.shape[0], -1, -1) if name == "expanded z" else dev(a[:, :, :1]).expand(-1, -1, a.shape[2])
    assert 0 in t.stride() and tuple(t.shape) == a.shape
    return t


def case_formats_and_shapes():
    dv = hip.DeviceVoxelizer(0)
    n_casts = 0
    for name, solid, origin, rng in ray_sets(2024):
        o, d, want = checked_set(name, solid, origin, rng)
        if name.startswith("expanded"):
            views = [("bool", name, expanded_tensor(name, solid), None),
                     ("f32", name, expanded_tensor(name, np.where(solid, F(-1), F(1))), 0.0)]
        else:
            views = []
            for fmt, t, level in formats(solid, rng):
                views.append((fmt, "contiguous", t, level))
                if name in ("(65, 19, 16)", "(130, 70, 67)", "(3, 40, 33)"):
                    views += [(fmt, layout, v, level) for layout, v in layouts(fmt, t)]
        for fmt, layout, t, level in views:
            caster = dense.RayCaster(dv, t, level=level, origin=origin)
            compare(cast(caster, o, d), want[:2], (name, fmt, layout), o, d)
            n_casts += 1
            if layout == "contiguous":
                finite_t_max(caster, solid, origin, o, d, rng, (name, fmt))
    print("compared", n_casts, "casts; times", dv.raycast_times())


def case_no_skip_ab():
    dv = hip.DeviceVoxelizer(0)
    for name, solid, origin, rng in ray_sets(2024):
        o, d, want = checked_set(name, solid, origin, rng)
        t = expanded_tensor(name, solid) if name.startswith("expanded") else dev(solid)
        caster = dense.RayCaster(dv, t, origin=origin)
        skipping = cast(caster, o, d)
        ms_skip = dv.raycast_times()[1]
        no_skip(True)
        try:
            walking = cast(caster, o, d)
            ms_walk = dv.raycast_times()[1]
            finite_t_max(caster, solid, origin, o, d, rng, (name, "no skip"))
        finally:
            no_skip(False)
        compare(walking, want[:2], (name, "no skip against the reference"), o, d)
        compare(skipping, want[:2], (name, "skip against the reference"), o, d)
        compare(walking, skipping, (name, "no skip against skip"), o, d)
        print(f"{name}: cast {ms_skip:.3f} ms skipping, {ms_walk:.3f} ms walking every cell", flush=True)
    print("compared")


def case_extremes():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(77)
    z, y, x = np.meshgrid(np.arange(40), np.arange(37), np.arange(70), indexing="ij")
    grids = [("sparse", R.random_solid(rng, (70, 37, 40), 0.002), (9, 8, 7)), ("checkerboard", (x + y + z) % 2 == 1, (0, 0, 0)),
             ("empty", np.zeros((40, 37, 70), bool), (3, 3, 3)), ("full", np.ones((40, 37, 70), bool), (0, 5, 0))]
    for name, solid, origin in grids:
        caster = dense.RayCaster(dv, dev(solid), origin=origin)
        o, d = R.extreme_rays(rng, solid, origin, 20000)
        o2, d2 = R.ray_set(rng, solid, origin, 6000, far=20, limit=2)
        o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
        want = R.cast(solid, origin, o, d)
        for walk in (False, True):
            no_skip(walk)
            compare(cast(caster, o, d), want[:2], (name, "no skip" if walk else "skip"), o, d)
        no_skip(False)
        finite_t_max(caster, solid, origin, o, d, rng, name)
        print(f"{name}: {len(o)} rays, hit and miss shares {R.shares(want[0])}", flush=True)
    # one solid voxel in 512^3: 10^5 rays at its centre, at the middles of its edges and at its corners (ties on two and three axes)
    n, G = 100000, 512
    v = np.array([301, 77, 433])
    grid = torch.zeros((G, G, G), dtype=torch.bool, device=DEV)
    grid[v[2], v[1], v[0]] = True
    caster = dense.RayCaster(dv, grid)
    kind = rng.integers(0, 4, n)                     # how many coordinates of the target lie on the voxel's planes
    on = np.argsort(rng.random((n, 3)), axis=1) < np.where(kind == 1, 0, kind)[:, None]
    target = np.where(on, v + rng.integers(0, 2, (n, 3)), v + 0.5)
    o = np.clip(v + (rng.random((n, 3)) - 0.5) * 300, 0, G)      # (within 150 cells: the reference walks every one)
    o = np.where(rng.random((n, 1)) < 0.5, o, np.floor(o) + rng.integers(0, 2, (n, 3)) * 0.5)
    d = target - o
    d = np.where(rng.random((n, 1)) < 0.3, d, d * np.exp(rng.uniform(-3, 3, (n, 1))))
    o, d = o.astype(F), d.astype(F)
    solid = np.zeros((G, G, G), bool)
    solid[v[2], v[1], v[0]] = True
    t0 = time.time()
    want = R.cast_lockstep(solid, (0, 0, 0), o, d)
    got = cast(caster, o, d)
    compare(got, want[:2], "single voxel", o, d)
    no_skip(True)
    try:
        compare(cast(caster, o, d), want[:2], "single voxel, no skip", o, d)
    finally:
        no_skip(False)
    faces = np.bincount(want[0][:, 3] + 2, minlength=8)
    print("single voxel:", n, "rays, faces -2 .. 5:", faces.tolist(), f"reference {time.time() - t0:.1f} s; times", dv.raycast_times())
    assert (faces[2:] > 0).all() and faces[1] > 0        # every face is entered, and some rays pass a corner or an edge and miss


def case_snapshot():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(5)
    solid = R.random_solid(rng, (90, 60, 50), 0.004)
    origin = (2, 3, 4)
    o, d = R.ray_set(rng, solid, origin, 20000, far=20, limit=0)
    want = R.cast(solid, origin, o, d)
    grid = dev(solid.astype(np.uint8))
    first = dense.RayCaster(dv, grid, origin=origin)
    grid.copy_(torch.randint(0, 2, grid.shape, dtype=torch.uint8, device=DEV))    # noise over the grid, then gone
    torch.cuda.synchronize()
    del grid
    torch.cuda.empty_cache()
    junk = torch.randint(0, 255, (50 * 60 * 90 * 4,), dtype=torch.uint8, device=DEV)   # (its memory, very likely, written again)
    compare(cast(first, o, d), want[:2], "after the grid changed and was freed", o, d)
    compare(cast(first, o[:100], d[:100], 5.0), R.cast(solid, origin, o[:100], d[:100], 5.0)[:2], "repeated")
    # another grid: the old caster is refused, the new one is right
    other = R.random_solid(rng, (33, 80, 21), 0.01)
    second = dense.RayCaster(dv, dev(other), origin=(0, 0, 0))
    try:
        first.cast(dev(o), dev(d))
        raise AssertionError("a replaced RayCaster was accepted")
    except RuntimeError as e:
        assert "replaced" in str(e), str(e)
    o2, d2 = R.ray_set(rng, other, (0, 0, 0), 20000, far=20, limit=0)
    compare(cast(second, o2, d2), R.cast(other, (0, 0, 0), o2, d2)[:2], "the new caster", o2, d2)
    # shapes [..., 3] and the one-shot form
    hit, t = dense.raycast(dv, dev(other), dev(o2[:600]).reshape(20, 30, 3), dev(d2[:600]).reshape(20, 30, 3))
    assert tuple(hit.shape) == (20, 30, 4) and tuple(t.shape) == (20, 30)
    compare((hit.reshape(-1, 4).cpu().numpy(), t.reshape(-1).cpu().numpy()), R.cast(other, (0, 0, 0), o2[:600], d2[:600])[:2], "one-shot")
    assert dv.raycast_scratch_bytes((33, 80, 21)) == 8 * (9 * 20 * 6 + 3 * 5 * 2 + 1 * 2 * 1) and len(junk)
    print("compared; times", dv.raycast_times())


def case_pipeline():
    """mesh -> voxels, bits and TSDF on the device, the same rays through all three; a depth image of the bench mesh."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(9)
    res = 96
    verts = fill_ref.weld(meshes.uv_sphere(24))
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dense.set_mesh(dv, dev(positions.view(F)), dev(faces.reshape(-1, 3).astype(np.int32)))
    room = np.array([-1.3, -1.3, -1.3, 1.3, 1.3, 1.3], F)
    occ, origin = dense.voxelize_dense(dv, res, fill=True, bounds=room)
    labels, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True, bounds=room)
    bits, _ = dense.voxelize_dense(dv, res, fmt="bits", fill=True, bounds=room)
    tsdf, _ = dense.mesh_distance(dv, res, band=3.0, bounds=room)
    solid = occ.cpu().numpy()
    assert np.array_equal(R.solid_bits(bits.cpu().numpy(), res), solid) and np.array_equal(labels.cpu().numpy() != 0, solid) and solid.sum() > 10000
    below = R.solid_f32(tsdf.cpu().numpy(), 0.0)
    o, d = R.ray_set(rng, solid, origin, 20000, far=20, limit=0)
    want, want_f = R.cast(solid, origin, o, d), R.cast(below, origin, o, d)
    for name, grid in (("occupancy", occ), ("labels", labels), ("bits", bits)):
        compare(cast(dense.RayCaster(dv, grid, origin=origin), o, d), want[:2], name, o, d)
    got_f = cast(dense.RayCaster(dv, tsdf, level=0.0, origin=origin), o, d)
    compare(got_f, want_f[:2], "tsdf < 0", o, d)
    agree = (want[0] == want_f[0]).all(axis=1) & (want[1].view(np.uint32) == want_f[1].view(np.uint32))
    compare((got_f[0][agree], got_f[1][agree]), (want[0][agree], want[1][agree]), "tsdf < 0 against labels != 0 where the sets agree")
    print("pipeline:", len(o), "rays;", int((solid != below).sum()), "voxels differ between labels != 0 and tsdf < 0;", int(agree.sum()), "rays agree")
    # a depth image of scan_like at 512
    res = 512
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dense.set_mesh(dv, dev(positions.view(F)), dev(faces.reshape(-1, 3).astype(np.int32)))
    grid, origin = dense.voxelize_dense(dv, res, fill=True)
    caster = dense.RayCaster(dv, grid, origin=origin)
    ro, rd = dense.camera_rays(512, 512, (-300.0, -520.0, 700.0), (256.0, 256.0, 256.0), (0.0, 0.0, 1.0), 45.0, DEV)
    hit, depth = caster.cast(ro, rd)
    assert tuple(hit.shape) == (512, 512, 4) and tuple(depth.shape) == (512, 512)
    pix = rng.choice(512 * 512, 4096, replace=False)
    o, d = ro.reshape(-1, 3)[pix].cpu().numpy(), rd.reshape(-1, 3)[pix].cpu().numpy()
    want = R.cast_lockstep(grid.cpu().numpy(), origin, o, d)
    compare((hit.reshape(-1, 4)[pix].cpu().numpy(), depth.reshape(-1)[pix].cpu().numpy()), want[:2], "depth image", o, d)
    seen = float(torch.isfinite(depth).float().mean())
    print("depth image: 512 x 512,", f"{seen:.3f} of the pixels see the model; 4096 compared,", want[2], "fine steps; times", dv.raycast_times())
    assert 0.05 < seen < 0.95


def expect_code(code, fn, what):
    try:
        fn()
    except hip.DeviceError as e:
        assert f"code {code}" in str(e), (what, str(e))
        return str(e)
    raise AssertionError(what + " was accepted")


def case_refusals():
    """Every refusal of the header's list, made before any launch; the context stays usable.  (This child runs with torch's
    caching allocator off: each tensor is an allocation of its own, so a short one is short.)"""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(1)
    N = 160                                    # a U8 grid of 4 MB; its short twin is half of it
    solid = R.random_solid(rng, (N, N, N), 0.001)
    grid = dev(solid.astype(np.uint8))
    half = torch.zeros((N // 2, N, N), dtype=torch.uint8, device=DEV)
    field = torch.ones((N, N, N), dtype=torch.float32, device=DEV)
    words = torch.zeros((N, N, N // 32), dtype=torch.int32, device=DEV)
    host = np.zeros((N, N, N), np.uint8)
    n = 1 << 19                                # rays: 6 MiB of origins, 8 MiB of hits, 2 MiB of t
    o, d = R.ray_set(rng, solid, (0, 0, 0), n, far=0, limit=0)
    o, d = dev(o[:n]), dev(d[:n])
    hit = torch.full((n, 4), 7, dtype=torch.int32, device=DEV)
    t = torch.full((n,), 7.0, device=DEV)
    short = torch.full((n // 4,), 7.0, device=DEV)   # 512 KiB: at most half of any of the four arrays, and 1 MiB below it
    both = torch.full((n * 5,), 7, dtype=torch.int32, device=DEV)
    host_rays = np.zeros((n, 4), F)
    torch.cuda.synchronize()
    st, dims = (1, N, N * N), (N, N, N)

    def build(ptr=grid.data_ptr(), fmt=hip.RAY_GRID_U8, strides=st, d=dims, level=0.0, origin=(0, 0, 0)):
        return lambda: dv.raycast_build(ptr, fmt, strides, d, level, origin)

    def run(op=o.data_ptr(), dp=d.data_ptr(), m=n, t_max=INF, hp=hit.data_ptr(), tp=t.data_ptr()):
        return lambda: dv.raycast(op, dp, m, t_max, hp, tp)
    msgs = [expect_code3(run(), "cast without a build")]
    assert "no o2v_hip_raycast_build" in msgs[0]
    generation = dv.raycast_generation()
    msgs += [
        expect_code3(build(ptr=None), "null grid"),
        expect_code3(build(d=(N, 0, N)), "zero dims"),
        expect_code3(build(fmt=3), "unknown format"),
        expect_code3(build(ptr=words.data_ptr(), fmt=hip.RAY_GRID_BITS, strides=(2, N // 32, N * N // 32)), "bits with an x stride of 2"),
        expect_code3(build(ptr=field.data_ptr(), fmt=hip.RAY_GRID_F32_BELOW, level=float("nan")), "level nan"),
        expect_code3(build(ptr=field.data_ptr(), fmt=hip.RAY_GRID_F32_BELOW, level=float("inf")), "level inf"),
        expect_code3(build(ptr=host.ctypes.data), "host grid"),
        expect_code3(build(ptr=half.data_ptr()), "short grid"),
        expect_code3(build(ptr=grid.data_ptr(), fmt=hip.RAY_GRID_F32_BELOW), "short grid (f32)"),
        expect_code3(build(ptr=words.data_ptr(), fmt=hip.RAY_GRID_BITS, strides=(1, N // 32, N * N // 32), d=(N, N, 8 * N)), "short bits"),
        expect_code(5, build(origin=(65536 - N + 1, 0, 0)), "origin + dims above 65 536"),
        expect_code(5, build(d=(N, N, 65537), strides=(1, N, 0)), "dims above 65 536"),
        # the snapshot of 65 536^3 voxels (every voxel the one element: the grid is only read) is 35 TB
        expect_code(4, build(d=(65536, 65536, 65536), strides=(0, 0, 0)), "scratch that cannot be allocated"),
    ]
    assert dv.raycast_generation() == generation + len(msgs) - 1        # a refused build counts
    msgs.append(expect_code3(run(), "cast after refused builds"))
    # a level that is not finite is ignored where the format has none
    build(level=float("nan"))()
    build(ptr=words.data_ptr(), fmt=hip.RAY_GRID_BITS, strides=(1, N // 32, N * N // 32), level=float("inf"))()
    caster = dense.RayCaster(dv, grid)
    msgs += [
        expect_code3(run(t_max=float("nan")), "t_max nan"),
        expect_code3(run(t_max=-1.0), "t_max negative"),
        expect_code3(run(t_max=-INF), "t_max -inf"),
        expect_code(5, run(m=1 << 31), "2^31 rays"),
        expect_code3(run(op=None), "null origins"),
        expect_code3(run(dp=None), "null directions"),
        expect_code3(run(hp=None), "null hit"),
        expect_code3(run(tp=None), "null t"),
        expect_code3(run(op=host_rays.ctypes.data), "host origins"),
        expect_code3(run(hp=host_rays.ctypes.data), "host hit"),
        expect_code3(run(op=short.data_ptr()), "short origins"),
        expect_code3(run(dp=short.data_ptr()), "short directions"),
        expect_code3(run(hp=short.data_ptr()), "short hit"),
        expect_code3(run(tp=short.data_ptr()), "short t"),
        expect_code3(run(hp=both.data_ptr(), tp=both.data_ptr() + n * 16 - 4), "hit and t overlap"),
        expect_code3(run(hp=o.data_ptr()), "hit in the origins"),
        expect_code3(run(tp=d.data_ptr() + 64), "t in the directions"),
        expect_code3(run(hp=both.data_ptr(), dp=both.data_ptr() + n * 8), "hit over the directions"),
    ]
    torch.cuda.synchronize()
    assert bool((hit == 7).all()) and bool((t == 7).all()) and bool((both == 7).all()) and bool((short == 7).all())
    # the context still works, the last build is still the snapshot; side by side in one allocation is accepted; n = 0 is nothing
    k = 20000                                  # (the reference for the first rays of the set)
    ho, hd = o[:k].cpu().numpy(), d[:k].cpu().numpy()
    want = R.cast(solid, (0, 0, 0), ho, hd)
    run()()
    run(hp=both.data_ptr(), tp=both.data_ptr() + n * 16)()
    run(m=0, op=None, dp=None, hp=None, tp=None)()
    torch.cuda.synchronize()
    compare((hit[:k].cpu().numpy(), t[:k].cpu().numpy()), want[:2], "after the refusals")
    compare((both[:k * 4].view(k, 4).cpu().numpy(), both[n * 4:n * 4 + k].view(torch.float32).cpu().numpy()), want[:2], "side by side")
    assert torch.equal(both[:n * 4].view(n, 4), hit) and torch.equal(both[n * 4:].view(torch.float32).view(torch.int32), t.view(torch.int32))
    compare(cast(caster, ho, hd, 9.0), R.cast(solid, (0, 0, 0), ho, hd, 9.0)[:2], "t_max")
    assert len(dv.raycast_times()) == 2 and all(ms > 0 for ms in dv.raycast_times())
    print("\n".join(msgs))
    print("ok refusals")


CASES = {"formats_and_shapes": case_formats_and_shapes, "no_skip_ab": case_no_skip_ab, "extremes": case_extremes, "snapshot": case_snapshot,
         "pipeline": case_pipeline, "refusals": case_refusals}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
