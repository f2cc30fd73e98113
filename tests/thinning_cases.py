"""The GPU cases of tests/test_gpu_thinning.py, each run in a child process of its own: `python -m tests.thinning_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison with the reference
(tests/thinning_ref.py) is np.array_equal on the skeleton's bits or its degree grid, and every call is made with
O2V_HIP_FLAG_STAGE_TIMES so that the counters are compared too: iterations and removed voxels must be the reference's, the
launches nine per iteration.  The shapes are the smallest at which the passes can go wrong - rows of more than one word, more
than one tile along every axis, sizes that are no multiple of a word or a tile -, not workload sizes; a reference is computed
once per (set, mode, keep, cap) and shared.  A case prints what it covered and "ok" last when everything held."""
import os
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import thinning_ref as TR
from tests.components_cases import indexed, set_of
from tests.dense_cases import expect_code3
from tests.raycast_cases import dev, expect_code, formats, layouts

DEV = torch.device("cuda", 0)
MODES = {TR.ULTIMATE: "ultimate", TR.CURVE: "curve"}


def no_tiles(on):
    """O2V_THIN_NO_TILES for the calls that follow (the library reads its switches at every call)."""
    if on:
        os.environ["O2V_THIN_NO_TILES"] = "1"
    else:
        os.environ.pop("O2V_THIN_NO_TILES", None)


class Ref:
    """The reference's results of one set, each computed once: (skeleton, iterations, removed) per (mode, keep, cap)."""

    def __init__(self, S):
        self.S, self.memo = np.asarray(S, bool), {}

    def get(self, mode, keep=None, cap=0, key=None):
        k = (mode, key if keep is not None else None, cap)
        if k not in self.memo:
            self.memo[k] = TR.thin(self.S, mode, keep, cap)
        return self.memo[k]


def raw(dv, t, level, mode, flags, cap, keep, out, dst_format):
    """One o2v_hip_thin_dense call on tensors, with O2V_HIP_FLAG_STAGE_TIMES; the counters."""
    _, fmt, lvl, dims = dense._set_grid(dv, t, level, dense._limit_voxels)
    torch.cuda.synchronize()
    dv.thin_dense(t.data_ptr(), fmt, dense._strides(t), dims, 0.0 if lvl is None else lvl, flags | hip.FLAG_STAGE_TIMES, mode, cap,
                  None if keep is None else keep.data_ptr(), None if keep is None else dense._strides(keep), out.data_ptr(), dense._strides(out), dst_format)
    return dv.thin_counters()


def check(dv, t, ref, mode, level=None, invert=False, keep=None, keep_np=None, keep_key=None, cap=0, degree=False, out=None, what=""):
    """One call against the reference of the set (ref: a Ref of S, or of its complement with invert): the bits or the degree
    grid, and the counters."""
    if out is None:
        out = torch.full(ref.S.shape, 7, dtype=torch.uint8, device=DEV)
    counters = raw(dv, t, level, mode, hip.CC_INVERT if invert else 0, cap, keep, out, hip.THIN_DST_DEGREE if degree else hip.THIN_DST_MASK)
    K, iterations, removed = ref.get(mode, keep_np, cap, keep_key)
    got = out.cpu().numpy()
    want = TR.degree(K) if degree else K.astype(np.uint8)
    assert np.array_equal(got, want), (what, MODES[mode], invert, cap, degree, int((got != want).sum()), "voxels differ")
    assert (counters[0], counters[3]) == (iterations, removed) and counters[1] == 9 * iterations, (what, MODES[mode], counters, iterations, removed)
    return out, counters


# ---- formats_and_layouts ---------------------------------------------------------------------------------------------------------------

def case_formats_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2026)
    n = 0
    for density in (0.3, 0.6):
        solid = TR.random_grid(rng, (70, 19, 21), density)
        refs = {}
        for fmt, t, level in formats(solid, rng):
            S = set_of(fmt, t, level)                       # (bits: 32 voxels per word, the padding is empty - and set under INVERT)
            for invert in (False, True):
                ref = refs.setdefault((S.shape, invert), Ref(~S if invert else S))
                for mode in MODES:
                    for degree in (False, True):
                        check(dv, t, ref, mode, level, invert, degree=degree, what=(fmt, density))
                        n += 1
            ref = refs[S.shape, False]
            for layout, view in layouts(fmt, t):
                check(dv, view, ref, TR.CURVE, level, what=(fmt, layout))
                n += 1
            # out= views: every second element along x, a slice of a batch, y and z swapped in memory
            wide = torch.full(S.shape[:2] + (2 * S.shape[2],), 9, dtype=torch.uint8, device=DEV)
            check(dv, t, ref, TR.CURVE, level, degree=True, out=wide[:, :, ::2], what=(fmt, "strided out"))
            assert bool((wide[:, :, 1::2] == 9).all())
            batch = torch.full((3,) + S.shape, 9, dtype=torch.uint8, device=DEV)
            check(dv, t, ref, TR.ULTIMATE, level, out=batch[1], what=(fmt, "out in a batch"))
            assert bool((batch[0] == 9).all()) and bool((batch[2] == 9).all())
            swapped = torch.full((S.shape[1], S.shape[0], S.shape[2]), 9, dtype=torch.uint8, device=DEV).permute(1, 0, 2)
            check(dv, t, ref, TR.CURVE, level, out=swapped, what=(fmt, "swapped out"))
            n += 3
        # in place: dst is the grid itself, contiguous and as a view; through dense.skeletonize with out=grid as well
        S = solid
        ref = refs[S.shape, False]
        own = dev(S.astype(np.uint8) * 200)
        check(dv, own, ref, TR.CURVE, out=own, what="in place")
        wide = torch.full(S.shape[:2] + (2 * S.shape[2],), 9, dtype=torch.uint8, device=DEV)
        wide[:, :, ::2] = dev(S.astype(np.uint8))
        check(dv, wide[:, :, ::2], ref, TR.ULTIMATE, degree=True, out=wide[:, :, ::2], what="in place, strided")
        assert bool((wide[:, :, 1::2] == 9).all())
        grid = dev(S)
        assert dense.skeletonize(dv, grid, out=grid) is grid and np.array_equal(grid.cpu().numpy(), ref.get(TR.CURVE)[0])
        n += 3
    # the torch layer: dtypes, the background, the float grid with a level
    S = solid
    K = dense.skeletonize(dv, dev(S), mode="ultimate", background=True)
    assert K.dtype == torch.bool and K.is_contiguous() and np.array_equal(K.cpu().numpy(), TR.thin(~S, TR.ULTIMATE)[0])
    field = dev(np.where(S, -1.0, 1.0).astype(np.float32))
    D = dense.skeletonize(dv, field, level=0.0, fmt="degree")
    assert D.dtype == torch.uint8 and np.array_equal(D.cpu().numpy(), TR.degree(TR.thin(S, TR.CURVE)[0]))
    assert dv.thin_counters() == (0, 0, 0, 0) and len(dv.thin_times()) == 3                       # (counted only on request)
    print(f"{n} calls compared with the reference, bit for bit")


# ---- known_shapes ----------------------------------------------------------------------------------------------------------------------

def case_known_shapes():
    """The pinned results of the definition, on the device."""
    dv = hip.DeviceVoxelizer(0)

    def thin(S, mode, degree=False):
        out, counters = check(dv, dev(S.astype(np.uint8)), Ref(S), mode, degree=degree, what="known shape")
        return out.cpu().numpy(), counters[0]
    K, it = thin(TR.box(), TR.ULTIMATE)
    assert (int(K.sum()), it) == (1, 5)
    D, it = thin(TR.box(), TR.CURVE, True)
    assert int((D > 0).sum()) == 25 and int((D == 2).sum()) == 8
    K, it = thin(TR.ball(), TR.ULTIMATE)
    assert (int(K.sum()), it) == (1, 13)
    for mode in MODES:
        K, it = thin(TR.shell(), mode)
        assert (int(K.sum()), it) == (1142, 3)
        labels, n = dense.components(dv, dev(K), background=True, connectivity=6)
        assert n == 2                                                                   # the cavity stays closed
    D, it = thin(TR.torus(), TR.ULTIMATE, True)
    assert int((D > 0).sum()) == 56 and set(D[D > 0].tolist()) == {3}                   # a closed loop
    for S in (TR.line("x", 130), TR.line("x", 130, 1)):
        K, it = thin(S, TR.ULTIMATE)
        assert np.argwhere(K).tolist() == [[1, 1, 65]] and it == 34
    K, it = thin(TR.line("x", 130), TR.CURVE)
    assert np.array_equal(K != 0, TR.line("x", 130)) and it == 1
    for axis, at in (("y", [1, 10, 1]), ("z", [10, 1, 1])):
        K, it = thin(TR.line(axis, 20), TR.ULTIMATE)
        assert np.argwhere(K).tolist() == [at] and it == 6
    S = np.ones((5, 5, 21), bool)
    for mode in MODES:
        a, b = thin(S, mode), thin(np.pad(S, 2), mode)
        assert np.array_equal(a[0], b[0][2:-2, 2:-2, 2:-2]) and a[1] == b[1]            # outside the box is background
    print("box, ball, shell, torus, lines and the unpadded box: the pinned results")


# ---- tile_borders ----------------------------------------------------------------------------------------------------------------------

def case_tile_borders():
    """What crosses tile borders, with the tile pass and with O2V_THIN_NO_TILES=1, each twice: the same bits, the reference's."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(31)
    sets = [("line 130", TR.line("x", 130)), ("line 129", TR.line("x", 130, 1)), ("line y", TR.line("y", 20)), ("line z", TR.line("z", 20)),
            ("staircase", TR.staircase())] + [(f"random {d}", TR.random_grid(rng, (130, 19, 17), d)) for d in (0.3, 0.6)]
    for name, S in sets:
        ref, t = Ref(S), dev(S.astype(np.uint8))
        for mode in ((TR.ULTIMATE,) if "line" in name or name == "staircase" else tuple(MODES)):
            turns = {}
            for off in (False, True):
                no_tiles(off)
                a, counters = check(dv, t, ref, mode, what=(name, off))
                b, again = check(dv, t, ref, mode, what=(name, off, "again"))
                assert torch.equal(a, b) and counters[:2] == again[:2] and counters[3] == again[3]
                turns[off] = counters[2]
                if name == "staircase":
                    assert np.argwhere(a.cpu().numpy()).tolist() == [[9, 9, 65]] and counters[0] == 34
            no_tiles(False)
            K, it, removed = ref.get(mode)
            print(f"{name} ({MODES[mode]}): {int(S.sum())} -> {int(K.sum())} voxels in {it} iterations; tile turns {turns[False]}, without the tile rule {turns[True]}")
            assert turns[False] <= turns[True]
    print("with and without the tile pass: the same bits")


# ---- keep_and_caps ---------------------------------------------------------------------------------------------------------------------

def case_keep_and_caps():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(41)
    S = TR.random_grid(rng, (70, 19, 21), 0.7)
    S[4:17, 3:16, 5:60] = True
    ref, t = Ref(S), dev(S.astype(np.uint8))
    keep_np = rng.random(S.shape) < 0.02
    # keep as a strided view, and as a bool tensor through the torch layer
    wide = torch.zeros(S.shape[:2] + (2 * S.shape[2],), dtype=torch.uint8, device=DEV)
    wide[:, :, 1::2] = 1
    wide[:, :, ::2] = dev(keep_np.astype(np.uint8) * 3)
    for mode in MODES:
        out, _ = check(dv, t, ref, mode, keep=wide[:, :, ::2], keep_np=keep_np, keep_key="k", what="keep")
        assert bool(out[dev(keep_np & S)].all())
        K = dense.skeletonize(dv, dev(S), mode=MODES[mode], keep=dev(keep_np))
        assert np.array_equal(K.cpu().numpy(), ref.get(mode, keep_np, 0, "k")[0])
    assert not np.array_equal(ref.get(TR.ULTIMATE, keep_np, 0, "k")[0], ref.get(TR.ULTIMATE)[0])
    # max_iterations 1, 2, 3: each result holds the next, and the counters stop there
    last = S
    for cap in (1, 2, 3):
        out, counters = check(dv, t, ref, TR.ULTIMATE, cap=cap, what=("cap", cap))
        K = out.cpu().numpy() != 0
        assert counters[0] == cap and not (K & ~last).any() and K.sum() < last.sum()
        last = K
        assert np.array_equal(dense.skeletonize(dv, dev(S), mode="ultimate", max_iterations=cap).cpu().numpy(), K)
    check(dv, dev(TR.box().astype(np.uint8)), Ref(TR.box()), TR.ULTIMATE, cap=1, what="the box, one iteration")
    check(dv, dev(TR.box().astype(np.uint8)), Ref(TR.box()), TR.CURVE, cap=1, what="the box, one iteration")
    print("keep (strided, bool) and max_iterations 1, 2, 3")


# ---- degree ----------------------------------------------------------------------------------------------------------------------------

def case_degree():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(51)
    for S in (TR.random_grid(rng, (70, 19, 21), 0.5), TR.cross(), np.ones((3, 5, 70), bool)):
        for mode in MODES:
            check(dv, dev(S.astype(np.uint8)), Ref(S), mode, degree=True, what="degree")
    # the degree grid is a convolution of the result: also where nothing is removed (a full box, capped)
    full = np.ones((9, 9, 70), bool)
    check(dv, dev(full), Ref(full), TR.CURVE, cap=1, degree=True, what="degree of a nearly full box")
    deg = dense.skeletonize(dv, dev(TR.cross()), fmt="degree")
    ends, junctions = dense.skeleton_nodes(deg)
    want = TR.nodes(TR.degree(TR.thin(TR.cross(), TR.CURVE)[0]))
    assert ends.dtype == junctions.dtype == torch.int32 and ends.device == deg.device
    assert np.array_equal(ends.cpu().numpy(), want[0]) and np.array_equal(junctions.cpu().numpy(), want[1])
    assert len(want[0]) == 24 and [16, 16, 16] in want[1].tolist()                      # four spurs per bar end; the centre is a junction
    print(f"degree grids; the cross: {len(want[0])} end points, {len(want[1])} junction voxels")


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------

def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, *indexed(meshes.scan_like()))
    solid, _ = dense.voxelize_dense(dv, 64, fill=True)
    S = solid.cpu().numpy().astype(bool)
    assert S.sum() > 1000
    for background in (False, True):
        t0 = time.time()
        K = dense.skeletonize(dv, solid, background=background)
        ms = (time.time() - t0) * 1e3
        want = TR.thin(~S if background else S, TR.CURVE)
        assert K.dtype == torch.bool and np.array_equal(K.cpu().numpy(), want[0])
        # (objects are 26-connected: the thinned set - the solid, or the empty space - before and after)
        before26 = dense.components(dv, solid, connectivity=26, background=background)[1]
        after26 = dense.components(dv, K, connectivity=26)[1]
        assert after26 == before26 >= 1
        print(f"pipeline: scan_like at 64, {'background' if background else 'solid'}: {int((~S if background else S).sum())} -> {int(K.sum())} voxels in "
              f"{want[1]} iterations, {after26} components, {ms:.1f} ms")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list, by code and words, made before any launch, the outputs untouched; the context stays
    usable.  (This child runs with torch's caching allocator off: each tensor is an allocation of its own, so a short one is
    short.)  One is not here: a failed scratch allocation, for K12's reason (tests/components_cases.py)."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(1)
    N = 64
    S = TR.random_grid(rng, (N, N, N), 0.5)
    grid = dev(S.astype(np.uint8))
    half = torch.zeros((N // 2, N, N), dtype=torch.uint8, device=DEV)
    field = torch.ones((N, N, N), dtype=torch.float32, device=DEV)
    words = torch.zeros((N, N, N // 32), dtype=torch.int32, device=DEV)
    dst = torch.full((N, N, N), 7, dtype=torch.uint8, device=DEV)
    keep = torch.zeros((N, N, N), dtype=torch.uint8, device=DEV)
    big = torch.full((2 * N, N, N), 7, dtype=torch.uint8, device=DEV)
    host = np.zeros((N, N, N), np.uint8)
    one = torch.zeros((1,), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    st, dims = (1, N, N * N), (N, N, N)
    wst = (1, N // 32, N * N // 32)

    def th(ptr=grid.data_ptr(), fmt=hip.GRID_U8, strides=st, d=dims, level=0.0, flags=0, mode=hip.THIN_CURVE, cap=0, kp=keep.data_ptr(), ks=st, op=dst.data_ptr(),
           os_=st, df=hip.THIN_DST_MASK):
        return lambda: dv.thin_dense(ptr, fmt, strides, d, level, flags, mode, cap, kp, ks, op, os_, df)

    def words_of(m, what, *parts):
        assert all(p in m for p in parts), (what, m)
        return m
    msgs = [
        words_of(expect_code3(th(ptr=None), "null grid"), "null grid", "null argument"), words_of(expect_code3(th(op=None), "null dst"), "null dst", "null argument"),
        words_of(expect_code3(th(os_=None), "null dst strides"), "null dst strides", "null argument"),
        words_of(expect_code3(th(ks=None), "keep without strides"), "keep strides", "null argument"),
        words_of(expect_code3(th(d=(N, 0, N)), "zero dims"), "zero dims", "zero dims"), words_of(expect_code3(th(fmt=3), "unknown format"), "format", "unknown format 3"),
        words_of(expect_code3(th(ptr=words.data_ptr(), fmt=hip.GRID_BITS, strides=(2,) + wst[1:]), "bits with an x stride of 2"), "bits", "strides[0] == 1"),
        words_of(expect_code3(th(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("nan")), "level nan"), "level", "level must be finite"),
        expect_code3(th(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("inf")), "level inf"),
        expect_code3(th(ptr=host.ctypes.data), "host grid"), expect_code3(th(ptr=half.data_ptr()), "short grid"),
        expect_code3(th(ptr=grid.data_ptr(), fmt=hip.GRID_F32_BELOW), "short grid (f32)"),
        words_of(expect_code3(th(mode=2), "unknown mode"), "mode", "unknown mode 2"), words_of(expect_code3(th(df=2), "unknown dst_format"), "dst_format", "unknown dst_format 2"),
        words_of(expect_code3(th(flags=256), "unknown flag bits"), "flags", "unknown flag bits in 256"), expect_code3(th(flags=hip.CC_SEED_BORDER), "a flag of flood"),
        words_of(expect_code(5, th(ptr=one.data_ptr(), d=(65537, 1, 1), strides=(0, 0, 0)), "an axis of 65 537"), "axis", "more than 65 536 voxels along an axis"),
        words_of(expect_code(5, th(ptr=one.data_ptr(), d=(1024, 1024, 2048), strides=(0, 0, 0)), "2^31 voxels"), "voxels", "2147483648 voxels do not fit an int32 index"),
        expect_code3(th(op=host.ctypes.data), "host dst"), expect_code3(th(op=half.data_ptr()), "short dst"),
        words_of(expect_code3(th(kp=host.ctypes.data), "host keep"), "host keep", "keep"), words_of(expect_code3(th(kp=half.data_ptr()), "short keep"), "short keep", "keep"),
        words_of(expect_code3(th(os_=(1, N, 0)), "dst strides that map two voxels to one element"), "dst strides", "dst: strides map two voxels"),
        words_of(expect_code3(th(op=grid.data_ptr(), os_=(N, 1, N * N)), "dst in the grid, other strides"), "overlap", "dst and grid overlap"),
        words_of(expect_code3(th(ptr=big.data_ptr(), op=big.data_ptr() + N), "dst a row into the grid"), "overlap", "dst and grid overlap"),
        words_of(expect_code3(th(ptr=dst.data_ptr(), fmt=hip.GRID_BITS, strides=wst), "dst in a bits grid"), "overlap", "dst and grid overlap"),
        words_of(expect_code3(th(op=keep.data_ptr()), "dst in keep"), "overlap", "dst and keep overlap"),
    ]
    assert all("o2v_hip_thin_dense: " in m for m in msgs)
    torch.cuda.synchronize()
    assert bool((dst == 7).all()) and bool((big == 7).all()) and bool((keep == 0).all()) and bool((half == 0).all())
    assert bool((grid == dev(S.astype(np.uint8))).all())
    # a level that is not finite is ignored where the format has none; keep strides without a keep are not read; grid and keep
    # may share memory (both are only read)
    th(level=float("nan"))()
    th(kp=None, ks=None)()
    th(kp=grid.data_ptr(), cap=1)()
    assert np.array_equal(dst.cpu().numpy(), S.astype(np.uint8))                                   # everything kept
    # the order: the set grid's checks before the mode, the mode before the flags, the flags before the sizes, the sizes before the outputs
    assert "unknown format" in expect_code3(th(fmt=3, mode=5, flags=256), "format before mode")
    assert "unknown mode" in expect_code3(th(mode=5, df=9, flags=256), "mode before dst_format")
    assert "unknown dst_format" in expect_code3(th(df=9, flags=256), "dst_format before flags")
    assert "along an axis" in expect_code(5, th(ptr=one.data_ptr(), d=(65537, 1, 1), strides=(0, 0, 0), op=host.ctypes.data), "the sizes before the outputs")
    # the context still works
    r = Ref(S)
    th(kp=None, ks=None, flags=hip.FLAG_STAGE_TIMES)()
    K, iterations, removed = r.get(TR.CURVE)
    assert np.array_equal(dst.cpu().numpy(), K.astype(np.uint8)) and dv.thin_counters()[0] == iterations and dv.thin_counters()[3] == removed
    th(kp=None, ks=None)()
    assert dv.thin_counters() == (0, 0, 0, 0)                                                      # (counted only on request)
    assert len(dv.thin_times()) == 3 and all(ms >= 0 for ms in dv.thin_times()) and sum(dv.thin_times()) > 0
    print("\n".join(msgs))
    print("ok refusals")


CASES = {"formats_and_layouts": case_formats_and_layouts, "known_shapes": case_known_shapes, "tile_borders": case_tile_borders,
         "keep_and_caps": case_keep_and_caps, "degree": case_degree, "pipeline": case_pipeline, "refusals": case_refusals}

if __name__ == "__main__":
    t0 = time.time()
    CASES[sys.argv[1]]()
    print(f"wall time {time.time() - t0:.1f} s")
    print("ok")
