"""The GPU cases of tests/test_gpu_thickness.py, each run in a child process of its own: `python -m tests.thickness_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison with the reference
(tests/thickness_ref.py) is np.array_equal - int32 squared radii and depths, the bits of the float32 thickness, bool grids - and
every thickness call is made with O2V_HIP_FLAG_STAGE_TIMES where the counters are compared: candidates, kept centres and visited
ball voxels must be the reference's, which is how a case knows it went through the list and the ball stage (or around them).
The shapes are the smallest at which the passes can go wrong, not workload sizes; a reference is computed once per set and
shared.  A case prints what it covered and "ok" last when everything held."""
import math
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import components_ref as CR
from tests import distance_ref as DR
from tests import thickness_ref as TR
from tests.components_cases import SHAPES, indexed, set_of
from tests.dense_cases import expect_code3
from tests.raycast_cases import dev, expect_code, formats, layouts

DEV = torch.device("cuda", 0)
CAPS = (1, 2, 5, 17, 65)   # r^2 + 1 for r = 0, 1, 2, 4, 8


def radius_of(cap):
    """A max_radius that dense.local_thickness turns into this cap: floor(r^2) + 1 == cap."""
    return math.sqrt(cap - 0.5)


class Ref:
    """The reference's grids of one set, each computed once: depth2 per border, T / OPEN_ONLY / counters per (cap, border)."""

    def __init__(self, S):
        self.S, self.d2, self.memo = np.asarray(S, bool), {}, {}

    def depth2(self, border):
        if border not in self.d2:
            self.d2[border] = TR.depth2(self.S, border)
        return self.d2[border]

    def get(self, what, cap, border):
        key = (what, cap, border)
        if key not in self.memo:
            d2 = self.depth2(border)
            if what == "T":
                self.memo[key] = TR.thickness(self.S, cap, border, d2)
            elif what == "open":
                self.memo[key] = TR.open_only(self.S, cap, border, d2)
            else:
                cand, kept = TR.kept_centres(self.S, cap, border, hip.thickness_cover_table(cap), d2)
                self.memo[key] = (int(cand.sum()), int(kept.sum()))
        return self.memo[key]


def raw(dv, t, level, cap, border, background, flags, out, depth2):
    """One o2v_hip_thickness_dense call on tensors, with O2V_HIP_FLAG_STAGE_TIMES."""
    _, fmt, lvl, dims = dense._set_grid(dv, t, level, dense._limit_thickness)
    flags |= hip.FLAG_STAGE_TIMES | (hip.THICK_BORDER if border else 0) | (hip.THICK_BACKGROUND if background else 0)
    torch.cuda.synchronize()
    dv.thickness_dense(t.data_ptr(), fmt, dense._strides(t), dims, 0.0 if lvl is None else lvl, flags, cap, out.data_ptr(), dense._strides(out),
                       None if depth2 is None else depth2.data_ptr(), None if depth2 is None else dense._strides(depth2))


def check(dv, t, ref, cap, border=True, background=False, level=None, kind="r2", out=None, depth2=True, what=""):
    """One call against the reference of the set (ref: a Ref of S, or of its complement with background): T (kind "r2"), its
    float32 form ("thickness") or the OPEN_ONLY grid ("open"); depth2 if asked for; the counters."""
    shape = ref.S.shape
    if out is None:
        out = torch.full(shape, -3, dtype=torch.float32 if kind == "thickness" else torch.int32, device=DEV)
    if depth2 is True:
        depth2 = torch.full(shape, -3, dtype=torch.int32, device=DEV)
    flags = {"r2": 0, "thickness": hip.THICK_F32, "open": hip.THICK_OPEN_ONLY}[kind]
    raw(dv, t, level, cap, border, background, flags, out, depth2)
    want = ref.get("open" if kind == "open" else "T", cap, border)
    got = out.cpu().numpy()
    if kind == "thickness":
        assert np.array_equal(got.view(np.uint32), TR.as_float(want).view(np.uint32)), (what, cap, border, background, kind, "the float bits differ")
    else:
        assert np.array_equal(got, want), (what, cap, border, background, kind, int((got != want).sum()), "voxels differ")
    if depth2 is not None:
        assert np.array_equal(depth2.cpu().numpy(), ref.depth2(border)), (what, cap, border, background, "depth2 differs")
    cand, kept, visited = dv.thickness_counters()
    if kind == "open":
        assert (cand, kept, visited) == (0, 0, 0), (what, cand, kept, visited)
    else:
        assert (cand, kept) == ref.get("centres", cap, border), (what, cap, border, (cand, kept), ref.get("centres", cap, border))
        assert (visited > 0) == (kept > 0)
    return out


def blobs(rng, dims, n=5, rmax=9.0, noise=0.02, holes=0.001):
    """A set with thin and thick parts: a few balls, some through the faces of the box, a little noise added and a few holes cut."""
    nx, ny, nz = dims
    S = rng.random(dims[::-1]) < noise
    for _ in range(n):
        c = (rng.integers(0, nx), rng.integers(0, ny), rng.integers(0, nz))
        S |= TR.digital_ball(dims, c, rng.uniform(1.5, rmax))
    return S & ~(rng.random(dims[::-1]) < holes)


# ---- formats_and_layouts ---------------------------------------------------------------------------------------------------------------

def case_formats_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2027)
    n, seen = 0, set()
    t0 = time.time()
    for i, dims in enumerate(SHAPES):
        solid = blobs(rng, dims)
        big = dims == (130, 70, 67)
        # (cap, border, background, kind): every shape takes two caps in turn, so all five meet every kind of shape
        combos = [(CAPS[(2 * i) % 5], True, False, "r2"), (CAPS[(2 * i + 1) % 5], False, bool(i % 2), "r2")]
        if not big:
            combos += [(CAPS[(2 * i + 2) % 5], bool(i % 2), True, "thickness"), (CAPS[(2 * i + 3) % 5], not i % 2, False, "open")]
        refs = {}

        def ref(S, background):
            T = ~S if background else S
            key = T.tobytes()
            if key not in refs:
                refs[key] = Ref(T)
            return refs[key]
        for fmt, t, level in formats(solid, rng):
            S = set_of(fmt, t, level)                          # (bits: 32 voxels per word, the padding is empty)
            assert fmt == "bits" or np.array_equal(S, solid)
            for cap, border, background, kind in (combos[:1] if fmt == "bits" else combos):
                check(dv, t, ref(S, background), cap, border, background, level, kind, what=(dims, fmt))
                seen.add((cap, border, background, kind))
                n += 1
            if dims in ((65, 9, 9), (70, 50, 40), (33, 29, 1)):
                cap, border, background, kind = combos[0]
                for layout, v in layouts(fmt, t):
                    check(dv, v, ref(S, background), cap, border, background, level, kind, what=(dims, fmt, layout))
                    n += 1
        # dst and depth2 with strides: a slice of a batch, every second element along x, axes swapped in memory; what lies
        # between stays; and no depth2 at all (the depth grid in the context)
        nz, ny, nx = solid.shape
        t = dev(solid)
        cap, border, _, _ = combos[1]
        r = ref(solid, False)
        batch = torch.full((4, nz, ny, nx), -7, dtype=torch.int32, device=DEV)
        check(dv, t, r, cap, border, out=batch[1], depth2=batch[3], what=(dims, "dst and depth2 in a batch"))
        assert bool((batch[0] == -7).all()) and bool((batch[2] == -7).all())
        wide = torch.full((nz, ny, 2 * nx), -7, dtype=torch.int32, device=DEV)
        deep = torch.full((nz, 3 * ny, nx), -7, dtype=torch.int32, device=DEV)
        check(dv, t, r, cap, border, out=wide[:, :, ::2], depth2=deep[:, 1::3, :], what=(dims, "dst with an x stride of 2, depth2 with a y stride of 3 rows"))
        assert bool((wide[:, :, 1::2] == -7).all()) and bool((deep[:, 0::3, :] == -7).all()) and bool((deep[:, 2::3, :] == -7).all())
        swapped = torch.empty((nx, ny, nz), dtype=torch.int32, device=DEV).permute(2, 1, 0)
        swapped_f = torch.empty((ny, nz, nx), dtype=torch.float32, device=DEV).permute(1, 0, 2)
        check(dv, t, r, cap, border, out=swapped, depth2=None, what=(dims, "dst with x and z swapped in memory, no depth2"))
        check(dv, t, r, cap, border, kind="thickness", out=swapped_f, depth2=swapped, what=(dims, "float dst with y and z swapped, depth2 with x and z swapped"))
        n += 4
    # the row scan's box at cap 1, where the core is the set itself: both of K21's scans on its six rows
    for fmt, t, level in formats(DR.scan_rows(), rng):
        S = set_of(fmt, t, level)
        for border, background in ((False, False), (True, True)):
            check(dv, t, Ref(~S if background else S), 1, border, background, level, "r2", what=("scan rows", fmt))
            n += 1
    assert {c[0] for c in seen} == set(CAPS) and {c[3] for c in seen} == {"r2", "thickness", "open"} and {c[1:3] for c in seen} == {(a, b) for a in (False, True) for b in (False, True)}
    print("compared", n, "calls in", f"{time.time() - t0:.1f} s; times", dv.thickness_times())


# ---- large_radii -----------------------------------------------------------------------------------------------------------------------

def case_large_radii():
    dv = hip.DeviceVoxelizer(0)
    # a disc of radius 100 in one layer, border off (with the border the single layer would give every voxel depth 1): balls of up
    # to 201 voxels across, rows longer than a wave, the table near its end
    cap = hip.THICK_MAX_RADIUS2
    S = TR.digital_ball((210, 210, 1), (105, 105, 0), 100.0)
    r = Ref(S)
    t0 = time.time()
    out = check(dv, dev(S), r, cap, border=False, what="disc")
    top = int(out.max())
    assert 99 * 99 < top <= 100 * 100 and top < cap and bool((out[0, 105, 105] == top))
    print(f"disc of radius 100 at cap 2^14: T.max() {top}, centres {r.get('centres', cap, False)}, {dv.thickness_counters()[2]} ball voxels; "
          f"{time.time() - t0:.1f} s; times {dv.thickness_times()}", flush=True)
    S = TR.digital_ball((40, 40, 40), (20, 20, 20), 17.0)
    r = Ref(S)
    t0 = time.time()
    for border in (True, False):
        out = check(dv, dev(S), r, 400, border=border, what="ball")
        assert 16 * 16 < int(out.max()) <= 17 * 17
    check(dv, dev(S), r, 400, kind="thickness", what="ball")
    print(f"ball of radius 17 at cap 400: T.max() {int(out.max())}, centres {r.get('centres', 400, True)}; {time.time() - t0:.1f} s; times {dv.thickness_times()}")


# ---- many_centres ----------------------------------------------------------------------------------------------------------------------

def case_many_centres():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(98)
    S = CR.random_grid(rng, (96, 64, 64), 0.98)
    r, t = Ref(S), dev(S)
    cand, kept = r.get("centres", 5, True)
    # more centres than waves are resident (256 CUs x 8 workgroups x 4 waves), and the last block of the list is not full
    assert kept > 256 * 8 * 4 and kept % 256 != 0 and cand > kept, (cand, kept)
    a = check(dv, t, r, 5, what="noise")
    visited = dv.thickness_counters()[2]
    assert visited == TR.visited(S, 5, True, hip.thickness_cover_table(5)), visited
    b = check(dv, t, r, 5, what="noise again")
    assert torch.equal(a, b) and dv.thickness_counters()[2] == visited
    print(f"0.98-dense noise at 96 x 64 x 64, cap 5: {cand} candidates, {kept} kept, {visited} ball voxels, twice the same bits; times {dv.thickness_times()}")
    # nothing to list: a full grid without the border (no voxel outside S: depth2 0x7FFFFFFF, everything in the core), an empty one
    full, empty = np.ones((9, 20, 33), bool), np.zeros((9, 20, 33), bool)
    for border in (False, True):
        out = check(dv, dev(full), Ref(full), 17, border=border, what="full")
        assert (dv.thickness_counters()[1] == 0) == (not border)
        out = check(dv, dev(empty), Ref(empty), 17, border=border, what="empty")
        assert dv.thickness_counters() == (0, 0, 0) and bool((out == 0).all())
    out = torch.full(full.shape, -3, dtype=torch.int32, device=DEV)
    d2 = torch.full(full.shape, -3, dtype=torch.int32, device=DEV)
    raw(dv, dev(full), None, 17, False, False, 0, out, d2)
    assert bool((out == 17).all()) and bool((d2 == 0x7FFFFFFF).all())
    print("a full grid with the border off is the cap everywhere with no centre listed; an empty grid is 0")


# ---- clipping --------------------------------------------------------------------------------------------------------------------------

def case_clipping():
    dv = hip.DeviceVoxelizer(0)
    dims = (23, 14, 9)
    nx, ny, nz = dims
    S = np.zeros(dims[::-1], bool)
    for c, rad in (((0, 0, 0), 6.5), ((22, 13, 8), 5.0), ((11, 0, 8), 4.5), ((22, 7, 4), 6.0), ((0, 13, 4), 3.0), ((11, 7, 0), 4.0), ((12, 6, 4), 2.5)):
        S |= TR.digital_ball(dims, c, rad)   # through corners, edges and faces of the box, and one inside
    r, rb = Ref(S), Ref(~S)
    n = 0
    for cap in (5, 30, 200, 1000, hip.THICK_MAX_RADIUS2):   # (the last three above the box's (nx-1)^2 + (ny-1)^2 + (nz-1)^2 = 717 or near it)
        for kind in ("r2", "open"):
            check(dv, dev(S), r, cap, border=False, kind=kind, what="bodies through the box")
            check(dv, dev(S), rb, cap, border=False, background=True, kind=kind, what="their background")
            n += 2
    # with the border off a body through a face is as thick as if it went on outside: deeper than with it on
    assert int(r.get("T", 200, False).max()) > int(r.get("T", 200, True).max())
    check(dv, dev(S), r, 200, border=True, what="the same bodies, border on")
    # the whole box: border off the cap everywhere (no centre), border on the inscribed balls of the box itself
    full = np.ones(dims[::-1], bool)
    rf = Ref(full)
    out = check(dv, dev(full), rf, 1000, border=True, what="the whole box")
    assert int(out.max()) == 25 and int(out.min()) >= 1   # ((nz + 1) // 2)^2: the mid layer is 5 from the outside
    check(dv, dev(full), rf, 1000, border=False, what="the whole box, border off")
    print("compared", n + 3, "calls on bodies through faces, edges and corners; caps up to 2^14 on a", dims, "box")


# ---- morphology ------------------------------------------------------------------------------------------------------------------------

def subset(a, b):
    return not bool((a & ~b).any())


def around(dv, value):
    """value, once the call that made it is seen to have gone round the list and the ball stage (OPEN_ONLY: all three counters 0)."""
    assert dv.thickness_counters() == (0, 0, 0), dv.thickness_counters()
    return value


def case_morphology():
    dv = hip.DeviceVoxelizer(0)
    # (a full call first, so that the zeros below are the morphology calls' own and not a fresh context's)
    probe = dev(TR.digital_ball((20, 20, 20), (10, 10, 10), 7.0))
    dense.local_thickness(dv, probe, 3)
    assert dv.thickness_counters()[1] > 0
    c = meshes.unit_cube().reshape(-1, 9)
    models = {"sphere": meshes.uv_sphere(12), "two cubes": np.concatenate([c * 16 + 4.03, c * 16 + 10.07])}
    for name, verts in models.items():
        dense.set_mesh(dv, *indexed(verts))
        solid, _ = dense.voxelize_dense(dv, 48, fill=True)
        S = solid.cpu().numpy().astype(bool)
        assert S.shape == (48, 48, 48) and 1000 < S.sum() < S.size
        for radius in (1, 2.5, 4):
            er, di = around(dv, dense.erode(dv, solid, radius)), around(dv, dense.dilate(dv, solid, radius))
            op, cl = around(dv, dense.opening(dv, solid, radius)), around(dv, dense.closing(dv, solid, radius))
            for got, want, what in ((er, TR.erode(S, radius), "erode"), (di, TR.dilate(S, radius), "dilate"), (op, TR.opening(S, radius), "opening"),
                                    (cl, TR.closing(S, radius), "closing")):
                assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want), (name, radius, what)
            assert subset(er, op) and subset(op, solid) and subset(solid, cl) and subset(cl, di)
            assert np.array_equal(around(dv, dense.erode(dv, solid, radius, border=False)).cpu().numpy(), TR.erode(S, radius, False))
            dense.local_thickness(dv, probe, 3)   # (the counters leave 0 between the radii)
            assert dv.thickness_counters()[1] > 0
        depth = around(dv, dense.inner_distance(dv, solid))
        assert depth.dtype == torch.int32 and np.array_equal(depth.cpu().numpy(), TR.depth2(S, True))
        assert np.array_equal(around(dv, dense.inner_distance(dv, solid, background=True, border=False)).cpu().numpy(), TR.depth2(~S, False))
        for t in (1, 3, 6, 9.5):
            thin = around(dv, dense.thin_regions(dv, solid, t))
            assert thin.dtype == torch.bool and np.array_equal(thin.cpu().numpy(), TR.thin_regions(S, t)), (name, t)
        # nothing is thinner than one voxel, or than two: the ball of radius 0 or 1 / 2 is one voxel, the opening the set itself.
        # At 3 the ball is the 7-voxel cross, which the edges of a cube and the poles of a digital sphere do not lie in.
        n3 = int(dense.thin_regions(dv, solid, 3).sum())
        assert not bool(dense.thin_regions(dv, solid, 1).any()) and not bool(dense.thin_regions(dv, solid, 2).any())
        print(f"{name} at 48: {int(S.sum())} voxels, {n3} thinner than 3, {int(dense.thin_regions(dv, solid, 9.5).sum())} thinner than 9.5; "
              f"erode / opening / closing / dilate by 2.5: {int(dense.erode(dv, solid, 2.5).sum())} / {int(dense.opening(dv, solid, 2.5).sum())} / "
              f"{int(dense.closing(dv, solid, 2.5).sum())} / {int(dense.dilate(dv, solid, 2.5).sum())}", flush=True)


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------

def case_pipeline():
    """A thin-walled shell: two concentric spheres, the parity fill keeps what lies between them."""
    dv = hip.DeviceVoxelizer(0)
    shell = np.concatenate([meshes.uv_sphere(16), meshes.uv_sphere(16, radius=0.84, center=(0.02, 0.0, 0.03))])
    dense.set_mesh(dv, *indexed(shell))
    solid, _ = dense.voxelize_dense(dv, 64, fill=True)
    S = solid.cpu().numpy().astype(bool)
    assert not S[32, 32, 32] and S.sum() > 10000
    cap = TR.cap_of(6)
    t, d2 = dense.local_thickness(dv, solid, 6, fmt="thickness", depth2=True)
    counters, times = dv.thickness_counters(), dv.thickness_times()
    want = TR.thickness(S, cap, True)
    assert t.dtype == torch.float32 and np.array_equal(t.cpu().numpy().view(np.uint32), TR.as_float(want).view(np.uint32))
    assert np.array_equal(d2.cpu().numpy(), TR.depth2(S, True))
    # the call went through the list and the ball stage: the reference's candidates and kept centres, the ball voxels not counted
    # (no O2V_HIP_FLAG_STAGE_TIMES) ...
    cand, kept = TR.kept_centres(S, cap, True, hip.thickness_cover_table(cap))
    assert counters == (int(cand.sum()), int(kept.sum()), 0) and counters[1] > 0, (counters, int(cand.sum()), int(kept.sum()))
    r2 = dense.local_thickness(dv, solid, 6)
    assert r2.dtype == torch.int32 and np.array_equal(r2.cpu().numpy(), want) and dv.thickness_counters() == counters
    # ... and counted on request: the voxels of the kept centres' balls
    raw(dv, solid, None, cap, True, False, 0, r2, None)
    visited = dv.thickness_counters()[2]
    assert dv.thickness_counters()[:2] == counters[:2] and visited == TR.visited(S, cap, True, hip.thickness_cover_table(cap)) and np.array_equal(r2.cpu().numpy(), want)
    inside = t[solid]
    thinnest, thickest = float(inside.min()), float(inside.max())
    # the wall is 0.16 * 32 = 5 voxels where the spheres are closest to concentric: nowhere at the cap of 13
    assert 1.0 <= thinnest < thickest < 2 * 6 + 1 and bool((t[~solid] == 0).all())
    thin = dense.thin_regions(dv, solid, 5)
    assert dv.thickness_counters() == (0, 0, 0)   # (OPEN_ONLY: round the ball stage)
    assert np.array_equal(thin.cpu().numpy(), TR.thin_regions(S, 5)) and bool(thin.any()) and not bool(thin.all())
    print(f"pipeline: a shell at 64: {int(S.sum())} voxels, thickness {thinnest:.2f} .. {thickest:.2f} voxels (cap 13), {int(thin.sum())} voxels thinner than 5; "
          f"local_thickness: {counters[0]} candidates, {counters[1]} kept, {visited} ball voxels; times {times}")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list, by code and words, made before any launch, the outputs untouched; the context stays
    usable.  (This child runs with torch's caching allocator off: each tensor is an allocation of its own, so a short one is
    short.)  One is not here: a failed scratch allocation, for K12's reason (tests/components_cases.py)."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(1)
    N = 64
    S = blobs(rng, (N, N, N), 8, 12.0)
    grid = dev(S.astype(np.uint8))
    half = torch.zeros((N // 2, N, N), dtype=torch.uint8, device=DEV)
    field = torch.ones((N, N, N), dtype=torch.float32, device=DEV)
    words = torch.zeros((N, N, N // 32), dtype=torch.int32, device=DEV)
    dst = torch.full((N, N, N), 7, dtype=torch.int32, device=DEV)
    dep = torch.full((N, N, N), 7, dtype=torch.int32, device=DEV)
    short = torch.full((N * N * N // 4,), 7, dtype=torch.int32, device=DEV)
    host = np.zeros((N, N, N), np.int32)
    one = torch.zeros((1,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st, dims = (1, N, N * N), (N, N, N)
    wst = (1, N // 32, N * N // 32)

    def th(ptr=grid.data_ptr(), fmt=hip.GRID_U8, strides=st, d=dims, level=0.0, flags=hip.THICK_BORDER, cap=17, op=dst.data_ptr(), os_=st, dp=dep.data_ptr(), ds=st):
        return lambda: dv.thickness_dense(ptr, fmt, strides, d, level, flags, cap, op, os_, dp, ds)

    def words_of(fn, what, *parts):
        m = fn
        assert all(p in m for p in parts), (what, m)
        return m
    msgs = [
        words_of(expect_code3(th(ptr=None), "null grid"), "null grid", "null argument"), words_of(expect_code3(th(op=None), "null dst"), "null dst", "null argument"),
        words_of(expect_code3(th(ds=None), "depth2 without strides"), "depth2 strides", "null argument"),
        words_of(expect_code3(th(d=(N, 0, N)), "zero dims"), "zero dims", "zero dims"), words_of(expect_code3(th(fmt=3), "unknown format"), "format", "unknown format 3"),
        words_of(expect_code3(th(ptr=words.data_ptr(), fmt=hip.GRID_BITS, strides=(2,) + wst[1:]), "bits with an x stride of 2"), "bits", "strides[0] == 1"),
        words_of(expect_code3(th(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("nan")), "level nan"), "level", "level must be finite"),
        expect_code3(th(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("-inf")), "level -inf"),
        expect_code3(th(ptr=host.ctypes.data), "host grid"), expect_code3(th(ptr=half.data_ptr()), "short grid"),
        expect_code3(th(ptr=grid.data_ptr(), fmt=hip.GRID_F32_BELOW), "short grid (f32)"),
        words_of(expect_code3(th(flags=256), "unknown flag bits"), "flags", "unknown flag bits in 256"), expect_code3(th(flags=1), "a flag of o2v_hip_voxelize"),
        words_of(expect_code3(th(cap=0), "a cap of 0"), "cap 0", "max_radius2 must be at least 1"),
        words_of(expect_code(5, th(cap=(1 << 14) + 1), "a cap of 2^14 + 1"), "cap", "is above 2^14"), expect_code(5, th(cap=2 ** 32 - 1), "a cap of 2^32 - 1"),
        words_of(expect_code(5, th(ptr=one.data_ptr(), d=(1024, 1024, 2048), strides=(0, 0, 0)), "2^31 voxels"), "voxels", "1024 x 1024 x 2048 voxels do not fit an int32 index"),
        words_of(expect_code(5, th(ptr=one.data_ptr(), d=(46342, 1, 1), strides=(0, 0, 0)), "an axis of 46 342"), "dist2", "does not fit below 2^31 - 1"),
        expect_code3(th(op=host.ctypes.data), "host dst"), expect_code3(th(op=short.data_ptr()), "short dst"), expect_code3(th(dp=short.data_ptr()), "short depth2"),
        words_of(expect_code3(th(os_=(1, N, 0)), "dst strides that map two voxels to one element"), "dst strides", "dst: strides map two voxels"),
        words_of(expect_code3(th(ds=(1, 1, N * N)), "depth2 strides (x, y)"), "depth2 strides", "depth2: strides map two voxels"),
        words_of(expect_code3(th(dp=dst.data_ptr()), "depth2 in dst"), "overlap", "dst and depth2 overlap"),
        words_of(expect_code3(th(ptr=dst.data_ptr(), fmt=hip.GRID_F32_BELOW), "dst in the grid"), "overlap", "dst and grid overlap"),
        words_of(expect_code3(th(ptr=dep.data_ptr(), fmt=hip.GRID_F32_BELOW), "depth2 in the grid"), "overlap", "depth2 and grid overlap"),
    ]
    assert all("o2v_hip_thickness_dense: " in m for m in msgs)
    torch.cuda.synchronize()
    assert bool((dst == 7).all()) and bool((dep == 7).all()) and bool((short == 7).all())
    assert bool((grid == dev(S.astype(np.uint8))).all())
    # a level that is not finite is ignored where the format has none; depth2 strides without a depth2 are not read
    th(level=float("nan"))()
    th(dp=None, ds=None)()
    # the order: the set grid's checks before the flags, the flags before the cap, the cap before the sizes, the sizes before the outputs
    assert "unknown format" in expect_code3(th(fmt=3, flags=256, cap=0), "format before flags")
    assert "unknown flag bits" in expect_code3(th(flags=256, cap=0), "flags before the cap")
    assert "max_radius2" in expect_code(5, th(cap=1 << 15, op=host.ctypes.data), "the cap before the outputs")
    assert "int32 index" in expect_code(5, th(ptr=one.data_ptr(), d=(65536, 65536, 1), strides=(0, 0, 0)), "the voxels before dist2_limit")
    # the context still works, and the cover table needs no context: both answer
    r = Ref(S)
    th(flags=hip.THICK_BORDER | hip.FLAG_STAGE_TIMES)()
    assert np.array_equal(dst.cpu().numpy(), r.get("T", 17, True)) and np.array_equal(dep.cpu().numpy(), r.depth2(True))
    assert dv.thickness_counters()[:2] == r.get("centres", 17, True) and dv.thickness_counters()[2] > 0
    th()()
    assert dv.thickness_counters()[:2] == r.get("centres", 17, True) and dv.thickness_counters()[2] == 0   # (counted only on request)
    assert len(dv.thickness_times()) == 5 and all(ms >= 0 for ms in dv.thickness_times()) and sum(dv.thickness_times()[:3]) > 0
    print("\n".join(msgs))
    print("ok refusals")


CASES = {"formats_and_layouts": case_formats_and_layouts, "large_radii": case_large_radii, "many_centres": case_many_centres, "clipping": case_clipping,
         "morphology": case_morphology, "pipeline": case_pipeline, "refusals": case_refusals}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
