"""The GPU cases of tests/test_gpu_components.py, each run in a child process of its own: `python -m tests.components_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison with the reference
(tests/components_ref.py) is np.array_equal on int32 labels / uint8 floods, the counts included.  A case prints what it covered
and "ok" last when everything held."""
import os
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import components_ref as CR
from tests import fill_ref
from tests import raycast_ref
from tests.dense_cases import expect_code3
from tests.raycast_cases import dev, expect_code, formats, layouts

DEV = torch.device("cuda", 0)
F = np.float32


def no_tiles(on):
    """O2V_CC_NO_TILES for the calls that follow (the library reads its switches at every call)."""
    if on:
        os.environ["O2V_CC_NO_TILES"] = "1"
    else:
        os.environ.pop("O2V_CC_NO_TILES", None)


def check_labels(dv, t, S, connectivity, background=False, level=None, out=None, want=None, what=""):
    """dense.components of the tensor t against the reference on the set S (a bool array [z, y, x])."""
    labels, n = dense.components(dv, t, level=level, connectivity=connectivity, background=background, out=out)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == S.shape and (out is None or labels is out)
    want = CR.label(~S if background else S, connectivity) if want is None else want
    got = labels.cpu().numpy()
    assert n == want[1], (what, connectivity, background, n, want[1])
    assert np.array_equal(got, want[0]), (what, connectivity, background, int((got != want[0]).sum()), "labels differ")
    return want


def check_flood(dv, t, S, connectivity, seeds=None, border=False, background=False, values=(1, 0, 0), level=None, out=None, what="", labelled=None):
    got = dense.flood(dv, t, seeds=None if seeds is None else dev(np.asarray(seeds, np.int32)), border=border, level=level, connectivity=connectivity,
                      background=background, values=values, out=out)
    want, reached = CR.flood(~S if background else S, connectivity, () if seeds is None else seeds, border, values, labelled)
    g = got.view(torch.uint8).cpu().numpy() if got.dtype == torch.bool else got.cpu().numpy()
    assert np.array_equal(g, want), (what, connectivity, border, background, values, int((g != want).sum()), "floods differ")
    return reached


def set_of(fmt, t, level):
    """The solid set a tensor holds, by the reference's readers."""
    a = t.cpu().numpy()
    return CR.solid_bits(a) if fmt == "bits" else CR.solid_f32(a, level) if fmt == "f32" else CR.solid_u8(a)


# ---- formats_and_layouts ---------------------------------------------------------------------------------------------------------------

SHAPES = [(70, 50, 40), (65, 9, 9), (64, 8, 8), (63, 20, 18), (130, 70, 67), (1, 37, 29), (40, 1, 30), (33, 29, 1), (200, 3, 5)]


def case_formats_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2025)
    n = 0
    for dims in SHAPES:
        solid = CR.random_grid(rng, dims, 0.3)
        for fmt, t, level in formats(solid, rng):
            S = set_of(fmt, t, level)                       # (bits: 32 voxels per word, the padding is empty)
            assert fmt == "bits" or np.array_equal(S, solid)
            wants = {(c, b): check_labels(dv, t, S, c, b, level, what=(dims, fmt)) for c in (6, 26) for b in (False, True)}
            check_flood(dv, t, S, 18, border=True, background=True, values=(0, 2, 1), level=level, what=(dims, fmt))
            n += 5
            if dims in ((65, 9, 9), (130, 70, 67), (70, 50, 40)):
                for layout, v in layouts(fmt, t):
                    check_labels(dv, v, S, 26, False, level, want=wants[26, False], what=(dims, fmt, layout))
                    check_labels(dv, v, S, 6, True, level, want=wants[6, True], what=(dims, fmt, layout))
                    n += 2
        # out= with strides: a slice of a batch, every second element along x, axes swapped in memory
        nz, ny, nx = solid.shape
        t = dev(solid)
        want = CR.label(solid, 18)
        batch = torch.full((3, nz, ny, nx), -7, dtype=torch.int32, device=DEV)
        check_labels(dv, t, solid, 18, out=batch[1], want=want, what=(dims, "out in a batch"))
        assert bool((batch[0] == -7).all()) and bool((batch[2] == -7).all())
        wide = torch.full((nz, ny, 2 * nx), -7, dtype=torch.int32, device=DEV)
        check_labels(dv, t, solid, 18, out=wide[:, :, ::2], want=want, what=(dims, "out with an x stride of 2"))
        assert bool((wide[:, :, 1::2] == -7).all())
        swapped = torch.empty((nx, ny, nz), dtype=torch.int32, device=DEV).permute(2, 1, 0)
        check_labels(dv, t, solid, 18, out=swapped, want=want, what=(dims, "out with x and z swapped in memory"))
        fl = torch.full((nz, ny, 2 * nx), 9, dtype=torch.uint8, device=DEV)
        check_flood(dv, t, solid, 6, seeds=[(0, 0, 0), (nx // 2, ny // 2, nz // 2)], border=False, values=(5, 6, 7), out=fl[:, :, ::2])
        assert bool((fl[:, :, 1::2] == 9).all())
        n += 4
    # voxels that share elements: a layer expanded along z, a plane expanded along x
    layer = CR.random_grid(rng, (50, 40, 1), 0.45)
    for name, S, t in (("expanded z", np.broadcast_to(layer, (30, 40, 50)), dev(layer).expand(30, -1, -1)),
                       ("expanded x", np.broadcast_to(layer[0][:, :1], (30, 40, 50)), dev(layer[0][:, :1].copy()).unsqueeze(0).expand(30, -1, 50))):
        assert 0 in t.stride()
        for c in CR.CONNECTIVITIES:
            check_labels(dv, t, S, c, what=name)
        f32 = torch.where(t, -1.0, 1.0)
        check_labels(dv, f32, S, 6, level=0.0, what=name + " f32")
        n += 4
    print("compared", n, "calls; times", dv.components_times())


# ---- connectivity_and_polarity, no_tiles_ab ----------------------------------------------------------------------------------------------

def connectivity_inputs():
    rng = np.random.default_rng(31)
    for density in (0.05, 0.3, 0.6, 0.95):
        yield f"random {density}", CR.random_grid(rng, (160, 150, 140), density)
    # the touching pairs on a tile's corner, on its edges, on its faces and inside it (tiles are 64 x 8 x 8)
    for kind in ("edge", "corner"):
        for corner in ((64, 8, 8), (128, 16, 24), (64, 8, 12), (64, 12, 8), (70, 8, 8), (64, 12, 12), (70, 8, 12), (70, 12, 8), (70, 12, 12)):
            yield f"{kind} pair at {corner}", CR.touching_pair((200, 40, 40), corner, kind)


def run_connectivity(dv, both_modes):
    n = 0
    for name, S in connectivity_inputs():
        t = dev(S)
        counts = []
        for c in CR.CONNECTIVITIES:
            for background in (False, True):
                if background and "pair" in name:
                    continue
                t0 = time.time()
                want = CR.label(~S if background else S, c)
                ref = time.time() - t0
                ms = []
                for mode in ((False, True) if both_modes else (False,)):
                    no_tiles(mode)
                    check_labels(dv, t, S, c, background, want=want, what=(name, "no tiles" if mode else "tiles"))
                    ms.append(dv.components_times())
                no_tiles(False)
                if not background:
                    counts.append(want[1])
                n += 1
                if "random" in name:
                    print(f"{name} conn {c} background {background}: {want[1]} components, reference {ref:.1f} s; ms " +
                          "; ".join(("no tiles " if i else "tiles ") + " ".join(f"{v:.3f}" for v in m) for i, m in enumerate(ms)), flush=True)
        if "pair" in name:
            assert tuple(counts) == ((2, 1, 1) if name.startswith("edge") else (2, 2, 1)), (name, counts)
    return n


def case_connectivity_and_polarity():
    dv = hip.DeviceVoxelizer(0)
    assert "O2V_CC_NO_TILES" not in os.environ
    print("compared", run_connectivity(dv, False), "sets")


def case_no_tiles_ab():
    """The inputs of connectivity_and_polarity and two of formats_and_layouts with O2V_CC_NO_TILES=1 (the child's environment has
    it) and without: both equal the reference, so each other."""
    assert os.environ.get("O2V_CC_NO_TILES") == "1"
    dv = hip.DeviceVoxelizer(0)
    n = run_connectivity(dv, True)
    rng = np.random.default_rng(2025)
    for dims in ((65, 9, 9), (130, 70, 67)):
        solid = CR.random_grid(rng, dims, 0.3)
        for fmt, t, level in formats(solid, rng):
            S = set_of(fmt, t, level)
            for mode in (True, False):
                no_tiles(mode)
                check_labels(dv, t, S, 26, False, level, what=(dims, fmt, mode))
                check_flood(dv, t, S, 6, border=True, background=True, values=(0, 2, 1), level=level, what=(dims, fmt, mode))
            n += 2
    no_tiles(True)
    print("compared", n, "sets with and without the tile pass")


# ---- extremes -------------------------------------------------------------------------------------------------------------------------------

def case_extremes():
    dv = hip.DeviceVoxelizer(0)
    dims = (150, 90, 70)
    empty, full = np.zeros(dims[::-1], bool), np.ones(dims[::-1], bool)
    single = empty.copy()
    single[33, 44, 77] = True
    for name, S in (("empty", empty), ("full", full), ("single voxel", single)):
        for c in CR.CONNECTIVITIES:
            for background in (False, True):
                want = check_labels(dv, dev(S), S, c, background, what=name)
        print(f"{name}: {want[1]} background components", flush=True)
    assert dense.components(dv, dev(empty))[1] == 0 and dense.components(dv, dev(full))[1] == 1 and dense.components(dv, dev(single), background=True)[1] == 1
    board = CR.checkerboard((128, 128, 128))
    t = dev(board)
    n6 = check_labels(dv, t, board, 6, what="checkerboard")[1]
    n18 = check_labels(dv, t, board, 18, what="checkerboard")[1]
    n26 = check_labels(dv, t, board, 26, what="checkerboard")[1]
    assert (n6, n18, n26) == (2 ** 20, 1, 1)
    print("checkerboard: 128^3,", n6, "components at 6,", n26, "at 26; times", dv.components_times(), flush=True)
    for name, S in (("serpentine", CR.serpentine((256, 256, 256))), ("comb", CR.comb((512, 128, 64))), ("spiral", CR.spiral((300, 200, 9)))):
        t = dev(S)
        wants = {c: CR.label(S, c) for c in (6, 26)}
        for mode in (False, True):
            no_tiles(mode)
            tmp = torch.empty(S.shape, dtype=torch.int32, device=DEV)
            dv_flags = dv.components_dense(t.data_ptr(), hip.GRID_U8, dense._strides(t), S.shape[::-1], 0.0, 6, hip.FLAG_STAGE_TIMES,
                                           tmp.data_ptr(), dense._strides(tmp))
            counters, ms = dv.components_counters(), dv.components_times()
            for c in (6, 26):
                assert check_labels(dv, t, S, c, want=wants[c], what=(name, mode))[1] == 1
            print(f"{name}{' (no tiles)' if mode else ''}: {int(S.sum())} voxels, {dv_flags} component, seam unions {counters[0]}, retries {counters[1]}; ms "
                  + " ".join(f"{v:.3f}" for v in ms), flush=True)
        no_tiles(False)
        check_flood(dv, t, S, 6, seeds=[(0, 0, 0)], values=(3, 4, 5), what=name, labelled=wants[6])


# ---- flood -----------------------------------------------------------------------------------------------------------------------------------

def case_flood():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(17)
    n = 0
    for dims, density in (((130, 70, 67), 0.2), ((130, 70, 67), 0.32), ((65, 40, 33), 0.5), ((200, 60, 50), 0.75), ((1, 50, 60), 0.6)):
        S = CR.random_grid(rng, dims, density)
        t = dev(S)
        inside = rng.integers(0, dims, (40, 3))
        seeds = np.concatenate([inside, rng.integers(-3, 0, (5, 3)), inside[:5] + np.array(dims), [[dims[0], 0, 0], [0, -1, 0], [2 ** 31 - 1, 0, 0]]])
        in_set = S[inside[:, 2], inside[:, 1], inside[:, 0]]
        assert in_set.any() and not in_set.all()           # seeds in the set and seeds that are not
        for c in CR.CONNECTIVITIES:
            for background in (False, True):
                labelled = CR.label(~S if background else S, c)
                for border, sd in ((True, None), (False, seeds), (True, seeds), (False, None), (False, seeds[-8:])):
                    for values in ((1, 0, 0), (0, 2, 1), (200, 100, 50)):
                        want_reached = check_flood(dv, t, S, c, sd, border, background, values, what=dims, labelled=labelled)
                        sd32, tmp = None if sd is None else dev(sd.astype(np.int32)), torch.empty(S.shape, dtype=torch.uint8, device=DEV)
                        torch.cuda.synchronize()
                        reached = dv.flood_dense(t.data_ptr(), hip.GRID_U8, dense._strides(t), dims, 0.0, c,
                                                 (hip.CC_INVERT if background else 0) | (hip.CC_SEED_BORDER if border else 0),
                                                 None if sd is None else sd32.data_ptr(), 0 if sd is None else len(sd), values, tmp.data_ptr(),
                                                 dense._strides(tmp))
                        assert reached == want_reached, (dims, c, background, border, reached, want_reached)
                        n += 1
        # int64 seeds and a sequence; exterior and solidify; a bool out
        check = dense.flood(dv, t, seeds=dev(seeds.astype(np.int64)), connectivity=18).cpu().numpy()
        assert np.array_equal(check, CR.flood(S, 18, seeds)[0])
        assert np.array_equal(dense.flood(dv, t, seeds=[tuple(int(v) for v in s) for s in inside], connectivity=6).cpu().numpy(), CR.flood(S, 6, inside)[0])
        for c in (6, 26):
            ext = dense.exterior(dv, t, connectivity=c)
            assert ext.dtype == torch.bool and np.array_equal(ext.cpu().numpy(), CR.flood(~S, c, border=True)[0].astype(bool))
            sol = dense.solidify(dv, t, connectivity=c)
            assert sol.dtype == torch.uint8 and np.array_equal(sol.cpu().numpy(), CR.solidify(S, c))
        mask = torch.zeros(S.shape, dtype=torch.bool, device=DEV)
        assert dense.flood(dv, t, border=True, out=mask) is mask and np.array_equal(mask.cpu().numpy(), CR.flood(S, 6, border=True)[0].astype(bool))
    print("compared", n, "floods; times", dv.components_times())


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------------

def indexed(verts):
    positions, faces = np.unique(np.asarray(verts, F).reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    return dev(positions.view(F)), dev(faces.reshape(-1, 3).astype(np.int32))


def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    # two closed cubes pushed into each other: the parity rule hollows the overlap out, the flood keeps it
    c = meshes.unit_cube().reshape(-1, 9)
    dense.set_mesh(dv, *indexed(np.concatenate([c * 16 + 4.03, c * 16 + 10.07])))
    surface, origin = dense.voxelize_dense(dv, 40, fmt="labels")
    parity, _ = dense.voxelize_dense(dv, 40, fmt="labels", fill=True)
    solid = dense.solidify(dv, surface)
    s = surface.cpu().numpy()
    assert origin == (0, 0, 0) and np.array_equal(solid.cpu().numpy(), CR.solidify(s != 0))
    inside, hollowed = (solid == 2).cpu().numpy(), (parity == 2).cpu().numpy()
    assert int(hollowed.sum()) == 29540 and int(inside.sum()) == 33636 and not (hollowed & ~inside).any()
    assert int(parity[15, 15, 15]) == 0 and int(solid[15, 15, 15]) == 2
    sdf = dense.distance_transform(dv, solid, "sdf")
    assert float(sdf[15, 15, 15]) < 0 < float(dense.distance_transform(dv, parity, "sdf")[15, 15, 15])
    caster = dense.RayCaster(dv, solid)
    o, d = np.array([[-5.0, 15.5, 15.5], [45.0, 44.0, 15.5]], F), np.array([[1.0, 0.0, 0.0], [-1.0, -1.0, 0.0]], F)
    hit, t = caster.cast(dev(o), dev(d))
    want_hit, want_t = raycast_ref.cast(solid.cpu().numpy() != 0, origin, o, d)[:2]
    assert np.array_equal(hit.cpu().numpy(), want_hit) and np.array_equal(t.cpu().numpy(), want_t) and (want_hit[:, 3] >= 0).all()
    print("pipeline: two cubes at 40:", int(inside.sum()), "interior voxels by the flood,", int(hollowed.sum()), "by parity; sdf at the overlap's centre",
          float(sdf[15, 15, 15]), flush=True)
    # one closed body: the two fills are the same grid
    dense.set_mesh(dv, *indexed(fill_ref.weld(meshes.uv_sphere(14))))
    surface, _ = dense.voxelize_dense(dv, 256, fmt="labels")
    parity, _ = dense.voxelize_dense(dv, 256, fmt="labels", fill=True)
    assert torch.equal(dense.solidify(dv, surface), parity) and int((parity == 2).sum()) > 10 ** 6
    print("sphere at 256: solidify equals fill=True;", int((parity == 2).sum()), "interior voxels; times", dv.components_times(), flush=True)
    # the islands of a scan's TSDF
    dense.set_mesh(dv, *indexed(meshes.scan_like()))
    tsdf, _ = dense.mesh_distance(dv, 512, band=3.0)
    labels, n = dense.components(dv, tsdf, level=0.0, connectivity=6)
    ms = dv.components_times()
    t0 = time.time()
    S = CR.solid_f32(tsdf.cpu().numpy(), 0.0)
    want, count = CR.label(S, 6)
    ref = time.time() - t0
    assert n == count and np.array_equal(labels.cpu().numpy(), want)
    sizes = dense.component_sizes(labels, n).cpu().numpy()
    want_sizes = np.bincount(want.reshape(-1), minlength=count + 1)
    assert sizes.dtype == np.int64 and np.array_equal(sizes, want_sizes)
    kept = dense.remove_small(dv, tsdf, 50, level=0.0, connectivity=6)
    assert kept.dtype == torch.bool and np.array_equal(kept.cpu().numpy(), (want_sizes >= 50)[want] & S)
    print(f"scan_like at 512: {n} components of tsdf < 0, the largest {int(sizes[1:].max())} voxels, {int((sizes[1:] < 50).sum())} below 50 voxels; "
          f"reference {ref:.1f} s; ms " + " ".join(f"{v:.3f}" for v in ms), flush=True)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list, made before any launch, the outputs untouched; the context stays usable.  (This child
    runs with torch's caching allocator off: each tensor is an allocation of its own, so a short one is short.)  One is not
    here: a failed scratch allocation.  Under the limit of 2^31 - 1 voxels the scratch is at most 9 GB, which a device of 288 GB
    only refuses once the test has taken the rest of its memory - from everyone else on it.  The allocation goes through
    grow_scratch, whose failure path the ray-casting refusals exercise."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(1)
    N = 160
    S = CR.random_grid(rng, (N, N, N), 0.3)
    grid = dev(S.astype(np.uint8))
    half = torch.zeros((N // 2, N, N), dtype=torch.uint8, device=DEV)
    field = torch.ones((N, N, N), dtype=torch.float32, device=DEV)
    words = torch.zeros((N, N, N // 32), dtype=torch.int32, device=DEV)
    labels = torch.full((N, N, N), 7, dtype=torch.int32, device=DEV)
    out = torch.full((N, N, N), 7, dtype=torch.uint8, device=DEV)
    short = torch.full((N * N * N // 4,), 7, dtype=torch.uint8, device=DEV)      # a quarter of out, a sixteenth of labels
    seeds = dev(np.array([[1, 2, 3], [4, 5, 6]], np.int32))
    host = np.zeros((N, N, N), np.int32)
    one = torch.zeros((1,), dtype=torch.uint8, device=DEV)
    both = torch.zeros((2 * N * N * N,), dtype=torch.uint8, device=DEV)      # the grid, and room for an out beside it
    both[:N * N * N] = grid.reshape(-1)
    torch.cuda.synchronize()
    st, dims = (1, N, N * N), (N, N, N)
    wst = (1, N // 32, N * N // 32)

    def comp(ptr=grid.data_ptr(), fmt=hip.GRID_U8, strides=st, d=dims, level=0.0, conn=6, flags=0, lp=labels.data_ptr(), ls=st):
        return lambda: dv.components_dense(ptr, fmt, strides, d, level, conn, flags, lp, ls)

    def fl(ptr=grid.data_ptr(), fmt=hip.GRID_U8, strides=st, d=dims, level=0.0, conn=6, flags=0, sp=seeds.data_ptr(), n=2, values=(1, 0, 0),
           op=out.data_ptr(), os_=st):
        return lambda: dv.flood_dense(ptr, fmt, strides, d, level, conn, flags, sp, n, values, op, os_)
    msgs = []
    for call, name in ((comp, "components"), (fl, "flood")):
        dst = dict(lp=None) if call is comp else dict(op=None)
        msgs += [
            expect_code3(call(ptr=None), name + ": null grid"), expect_code3(call(**dst), name + ": null output"),
            expect_code3(call(d=(N, 0, N)), name + ": zero dims"), expect_code3(call(fmt=3), name + ": unknown format"),
            expect_code3(call(conn=8), name + ": connectivity 8"), expect_code3(call(conn=0), name + ": connectivity 0"),
            expect_code3(call(flags=64), name + ": unknown flag bits"), expect_code3(call(flags=1), name + ": a flag of o2v_hip_voxelize"),
            expect_code3(call(ptr=words.data_ptr(), fmt=hip.GRID_BITS, strides=(2,) + wst[1:]), name + ": bits with an x stride of 2"),
            expect_code3(call(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("nan")), name + ": level nan"),
            expect_code3(call(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("-inf")), name + ": level -inf"),
            expect_code3(call(ptr=host.ctypes.data), name + ": host grid"), expect_code3(call(ptr=half.data_ptr()), name + ": short grid"),
            expect_code3(call(ptr=grid.data_ptr(), fmt=hip.GRID_F32_BELOW), name + ": short grid (f32)"),
            expect_code3(call(ptr=words.data_ptr(), fmt=hip.GRID_BITS, strides=wst, d=(N, N, 8 * N)), name + ": short bits"),
            expect_code(5, call(d=(N, N, 65537), strides=(1, N, 0)), name + ": a dim above 65 536"),
            # 2^31 voxels of an expanded grid (every voxel the one element: the grid is only read); the output pointer is never reached
            expect_code(5, call(ptr=one.data_ptr(), d=(1024, 1024, 2048), strides=(0, 0, 0), **({"lp": one.data_ptr()} if call is comp else {"op": one.data_ptr()})),
                        name + ": 2^31 voxels"),
        ]
        assert "2147483648 voxels" in msgs[-1]
    msgs += [
        expect_code3(comp(flags=hip.CC_SEED_BORDER), "components: the border flag"),
        expect_code3(comp(lp=host.ctypes.data), "host labels"), expect_code3(comp(lp=short.data_ptr()), "short labels"),
        expect_code3(comp(lp=out.data_ptr()), "short labels (a uint8 tensor)"),
        expect_code3(comp(ls=(1, N, 0)), "label strides that map two voxels to one element"), expect_code3(comp(ls=(1, 1, N * N)), "label strides (x, y)"),
        expect_code3(comp(ptr=labels.data_ptr(), fmt=hip.GRID_F32_BELOW), "labels in the grid"),
        expect_code3(comp(ptr=labels.data_ptr() + 64, fmt=hip.GRID_U8), "labels over the grid"),
        expect_code3(fl(op=host.ctypes.data), "host out"), expect_code3(fl(op=short.data_ptr()), "short out"),
        expect_code3(fl(os_=(0, N, N * N)), "out strides that map two voxels to one element"),
        expect_code3(fl(op=grid.data_ptr()), "out in the grid"), expect_code3(fl(ptr=both.data_ptr(), op=both.data_ptr() + N * N * N - 1), "out on the grid's last byte"),
        expect_code3(fl(sp=None), "null seeds"), expect_code3(fl(sp=host.ctypes.data), "host seeds"), expect_code3(fl(n=1 << 20), "short seeds"),
        expect_code(5, fl(n=1 << 31), "2^31 seeds"),
        expect_code3(fl(op=seeds.data_ptr(), d=(4, 1, 1), os_=(1, 4, 4)), "out over the seeds"),
        expect_code3(lambda: dv.flood_dense(grid.data_ptr(), hip.GRID_U8, st, dims, 0.0, 6, 0, None, 0, (1, 0, 0), None, st), "null out without seeds"),
    ]
    torch.cuda.synchronize()
    assert bool((labels == 7).all()) and bool((out == 7).all()) and bool((short == 7).all()) and bool((grid == dev(S.astype(np.uint8))).all())
    # a level that is not finite is ignored where the format has none; no seeds: the pointer is not read
    comp(level=float("nan"))()
    fl(sp=None, n=0, level=float("inf"))()
    # the context still works
    want = CR.label(S, 26)
    assert comp(conn=26)() == want[1] and np.array_equal(labels.cpu().numpy(), want[0])
    wf = CR.flood(S, 18, [(1, 2, 3), (4, 5, 6)], True, (9, 8, 7))
    assert fl(conn=18, flags=hip.CC_SEED_BORDER, values=(9, 8, 7))() == wf[1] and np.array_equal(out.cpu().numpy(), wf[0])
    # out and labels beside the grid in one allocation are accepted
    assert bool((both[N * N * N:] == 0).all())
    assert fl(ptr=both.data_ptr(), op=both.data_ptr() + N * N * N, conn=18, flags=hip.CC_SEED_BORDER, values=(9, 8, 7))() == wf[1]
    assert np.array_equal(both[N * N * N:].reshape(N, N, N).cpu().numpy(), wf[0])
    assert len(dv.components_times()) == 5 and all(ms > 0 for ms in dv.components_times())
    print("\n".join(msgs))
    print("ok refusals")


CASES = {"formats_and_layouts": case_formats_and_layouts, "connectivity_and_polarity": case_connectivity_and_polarity, "no_tiles_ab": case_no_tiles_ab,
         "extremes": case_extremes, "flood": case_flood, "pipeline": case_pipeline, "refusals": case_refusals}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
