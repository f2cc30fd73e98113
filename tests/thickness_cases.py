"""The GPU cases of tests/test_gpu_thickness.py, each run in a child process of its own: `python -m tests.thickness_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison with the reference
(tests/thickness_ref.py) is np.array_equal - int32 squared radii and depths, the bits of the float32 thickness, bool grids - and
every thickness call is made with O2V_HIP_FLAG_STAGE_TIMES where the counters are compared: candidates, kept centres and visited
ball voxels must be the reference's, which is how a case knows it went through the list and the ball stage (or around them).
The shapes are the smallest at which the passes can go wrong, not workload sizes; a reference is computed once per set and
shared; the cases at the limits the call documents (the last four) are as large as the limit they are about.  A case prints what it
covered and "ok" last when everything held."""
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
            elif what == "visited":
                self.memo[key] = TR.visited(self.S, cap, border, hip.thickness_cover_table(cap))
            else:
                cand, kept = TR.kept_centres(self.S, cap, border, hip.thickness_cover_table(cap), d2)
                self.memo[key] = (int(cand.sum()), int(kept.sum()))
        return self.memo[key]


def raw(dv, t, level, cap, border, background, flags, out, depth2, nx=None):
    """One o2v_hip_thickness_dense call on tensors, with O2V_HIP_FLAG_STAGE_TIMES.  nx: the voxels along x of a bits grid whose last
    word is part padding (else 32 per word)."""
    _, fmt, lvl, dims = dense._set_grid(dv, t, level, dense._limit_thickness)
    if nx is not None:
        assert fmt == hip.GRID_BITS and dims[0] - 32 < nx <= dims[0]
        dims = (nx,) + dims[1:]
    flags |= hip.FLAG_STAGE_TIMES | (hip.THICK_BORDER if border else 0) | (hip.THICK_BACKGROUND if background else 0)
    torch.cuda.synchronize()
    dv.thickness_dense(t.data_ptr(), fmt, dense._strides(t), dims, 0.0 if lvl is None else lvl, flags, cap, out.data_ptr(), dense._strides(out),
                       None if depth2 is None else depth2.data_ptr(), None if depth2 is None else dense._strides(depth2))


def check(dv, t, ref, cap, border=True, background=False, level=None, kind="r2", out=None, depth2=True, what="", nx=None, visited=False):
    """One call against the reference of the set (ref: a Ref of S, or of its complement with background): T (kind "r2"), its
    float32 form ("thickness") or the OPEN_ONLY grid ("open"); depth2 if asked for; the counters - the ball voxels too with
    visited=True (the reference walks every kept centre's ball: for sets where that is affordable)."""
    shape = ref.S.shape
    if out is None:
        out = torch.full(shape, -3, dtype=torch.float32 if kind == "thickness" else torch.int32, device=DEV)
    if depth2 is True:
        depth2 = torch.full(shape, -3, dtype=torch.int32, device=DEV)
    flags = {"r2": 0, "thickness": hip.THICK_F32, "open": hip.THICK_OPEN_ONLY}[kind]
    raw(dv, t, level, cap, border, background, flags, out, depth2, nx)
    want = ref.get("open" if kind == "open" else "T", cap, border)
    got = out.cpu().numpy()
    if kind == "thickness":
        assert np.array_equal(got.view(np.uint32), TR.as_float(want).view(np.uint32)), (what, cap, border, background, kind, "the float bits differ")
    else:
        assert np.array_equal(got, want), (what, cap, border, background, kind, int((got != want).sum()), "voxels differ")
    if depth2 is not None:
        assert np.array_equal(depth2.cpu().numpy(), ref.depth2(border)), (what, cap, border, background, "depth2 differs")
    cand, kept, balls = dv.thickness_counters()
    if kind == "open":
        assert (cand, kept, balls) == (0, 0, 0), (what, cand, kept, balls)
    else:
        assert (cand, kept) == ref.get("centres", cap, border), (what, cap, border, (cand, kept), ref.get("centres", cap, border))
        assert (balls > 0) == (kept > 0)
        if visited:
            assert balls == ref.get("visited", cap, border), (what, cap, border, "ball voxels", balls, ref.get("visited", cap, border))
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


# ---- at the limits the call documents --------------------------------------------------------------------------------------------------
#
# The two large boxes are repetitions of a tile whose outer voxel layer is empty, so that the tile's reference, repeated, is the
# box's (tests/thickness_ref.py, held against the literal reference by tests/test_host_thickness.py); the longest axes carry sets
# that are constant over the cross-section, which reduce to a line (the same two files).

SMALL_TILE = ((33, 19, 27), (((9, 9, 13), 6.0), ((22, 8, 8), 3.0), ((27, 12, 20), 2.0)))                       # dims (x, y, z), balls
LARGE_TILE = ((43, 30, 30), (((12, 12, 14), 9.0), ((30, 10, 9), 5.0), ((33, 22, 20), 3.5), ((20, 24, 24), 2.0)))


def timed(dv, *args):
    """raw(dv, *args): (the counters, the wall time in ms, the stage times)."""
    t0 = time.time()
    raw(dv, *args)
    return dv.thickness_counters(), round((time.time() - t0) * 1e3, 1), [round(ms, 1) for ms in dv.thickness_times()]


def slabs_equal(got, tile_grid, reps, what):
    """got [z, y, x] on the device against the tile's grid repeated: one tile-thick slab of z at a time, every voxel."""
    tz = tile_grid.shape[0]
    slab = torch.from_numpy(np.ascontiguousarray(tile_grid)).to(DEV).repeat(1, reps[1], reps[2])
    assert got.dtype == slab.dtype and got.shape[0] == tz * reps[0] and got.shape[1:] == slab.shape[1:], what
    for k in range(reps[0]):
        assert torch.equal(got[k * tz:(k + 1) * tz], slab), (what, "slab", k, int((got[k * tz:(k + 1) * tz] != slab).sum()), "voxels differ")


def repeated(tile_spec, reps, cap, seed):
    """(the tile's repetition uint8 [z, y, x] built on the device, what it must give (TR.tiled), dims (x, y, z))."""
    dims, balls = tile_spec
    table = hip.thickness_cover_table(cap)
    P = TR.tile(dims, cap, seed, balls, table=table)
    want = TR.tiled(P, reps, cap, table)
    grid = torch.from_numpy(P.astype(np.uint8)).to(DEV).repeat(*reps)
    return grid, want, tuple(n * r for n, r in zip(dims, reps[::-1]))


def case_block_turns():
    """Just past 2^28 voxels: k_thick_init and k_thick_list take a second turn of 3 072 blocks, the last of them one voxel short, the block
    offsets go through 4 108 rounds of the one-workgroup scan, both envelope passes have more lines than lanes on the context's
    depth grid and on a dst / depth2 whose axes are swapped in memory.

    It bites: with the turns dropped (`for (b = blockIdx.x; b < n_blocks; b += gridDim.x)` of k_thick_init and k_thick_list made
    `if (b < n_blocks)`, the skipped blocks' sums zeroed so that the list stays one), the case failed at its first call with
    ('counters', (18703943, 5138684, 250617392), (18717831, 5152572, 250631280)) - the 13 888 centres of the last 3 072 blocks
    were never counted or listed."""
    dv = hip.DeviceVoxelizer(0)
    cap, reps = 17, (19, 27, 31)
    grid, want, (nx, ny, nz) = repeated(SMALL_TILE, reps, cap, seed=1)
    voxels = nx * ny * nz
    blocks = -(-voxels // 256)
    assert (nx, ny, nz) == (1023, 513, 513) and voxels == 269221887 and voxels > 1 << 28 and voxels % 256 != 0
    assert blocks == 1051648 and blocks - (1 << 20) == 3072 and voxels % 256 == 255 and nx * nz > 1 << 17 and nx * ny > 1 << 17
    assert want["last"] > 1 << 28 and want["last"] // 256 >= 1 << 20      # (a centre listed in the second turn)
    counters = (want["candidates"], want["kept"], want["visited"])
    shape = tuple(grid.shape)
    a = torch.full(shape, -3, dtype=torch.int32, device=DEV)
    got = timed(dv, grid, None, cap, False, False, 0, a, None)            # (the depth grid is the context's)
    assert got[0] == counters, ("counters", got[0], counters)
    slabs_equal(a, want["T"], reps, "r2, the context's depth grid")
    b = torch.full(shape, -3, dtype=torch.int32, device=DEV)
    again = timed(dv, grid, None, cap, False, False, 0, b, None)
    assert again[0] == counters and torch.equal(a, b), "the second run differs"
    # dst with y and z swapped in memory, depth2 with x and z swapped: more lines than lanes on strided grids
    del b
    b = torch.full((ny, nz, nx), -3, dtype=torch.int32, device=DEV).permute(1, 0, 2)
    d2 = torch.full((nx, ny, nz), -3, dtype=torch.int32, device=DEV).permute(2, 1, 0)
    assert tuple(b.shape) == tuple(d2.shape) == shape and not b.is_contiguous() and d2.stride(2) == ny * nz
    with_d2 = timed(dv, grid, None, cap, True, False, 0, b, d2)
    assert with_d2[0] == counters, ("counters, border on", with_d2[0], counters)
    slabs_equal(b, want["T"], reps, "r2 with depth2, border on")
    slabs_equal(d2, want["depth2"], reps, "depth2, border on")
    low = timed(dv, grid, None, cap, True, False, hip.THICK_OPEN_ONLY, b, d2)
    assert low[0] == (0, 0, 0), low[0]
    slabs_equal(b, want["open"], reps, "open")
    slabs_equal(d2, want["depth2"], reps, "depth2 of open")
    print(f"block_turns {nx} x {ny} x {nz}: voxels {voxels}, blocks {blocks} = 2^20 + {blocks - (1 << 20)} in a second turn, lines per envelope pass {nx * nz} and "
          f"{nx * ny}; candidates, kept, ball voxels {counters}, largest centre index {want['last']}, twice the same bits; "
          f"ms (wall, stages): r2 {got[1:]}, r2 with a strided dst and depth2 {with_d2[1:]}, open on the same {low[1:]}")


def case_largest_box():
    """1290^3 = 2 146 689 000 voxels, the largest cube under 2^31 - 1 (K15's): the centre list's int32 indices, c / nx in the ball
    stage, k_thick_convert's grid stride and byte offsets above 2^33 in dst and depth2, 8 385 504 blocks in eight turns.  One call in
    the float format with depth2 and the border on, one r2 call on the context's depth grid.

    No kept centre can lie within 2^20 of 2^31: the tile's empty outer layer puts the last content at z = 1288, and a z layer is
    1290^2 > 2^20 voxels.  The largest listed index is that of the last voxel inside the outer layer, (1288, 1288, 1288) =
    2 145 023 608 = 2^31 - 2 460 040, which is asserted exactly.

    Measured on the MI355X (50 588 640 kept centres, 3 578 036 880 ball voxels; ms, wall and then the stages depth2 / core /
    list / balls / convert): the float call with depth2 355.8 (67.1 / 31.9 / 216.0 / 31.3 / 6.4), the r2 call 342.6 (62.1 / 32.1 /
    215.3 / 31.0 / 0); the case with its comparisons 0.9 s, its child 3.7 s.  The ball stage is a tenth of the call; counting and
    listing the centres (the keep test twice over 2^31 voxels) is two thirds.

    It bites: with the centre index held in 30 bits (`list[...] = (int32_t) (i & 0x3fffffff)` in k_thick_list) the case failed at
    its first call with ('counters', (196252860, 50588640, 1825923900), (196252860, 50588640, 3578036880)): the balls of the
    centres past 2^30 were drawn around other voxels."""
    dv = hip.DeviceVoxelizer(0)
    cap, reps = 17, (43, 43, 30)
    t0 = time.time()
    grid, want, (nx, ny, nz) = repeated(LARGE_TILE, reps, cap, seed=2)
    voxels = nx * ny * nz
    assert (nx, ny, nz) == (1290, 1290, 1290) and voxels == 2146689000 and voxels <= 2 ** 31 - 1 < 1291 ** 3
    assert want["last"] == 1288 * (1290 * 1290 + 1290 + 1) == 2145023608 and want["last"] > 2 ** 31 - 2 ** 22
    counters = (want["candidates"], want["kept"], want["visited"])
    shape = tuple(grid.shape)
    out = torch.full(shape, -3.0, dtype=torch.float32, device=DEV)
    d2 = torch.full(shape, -3, dtype=torch.int32, device=DEV)
    as_float = timed(dv, grid, None, cap, True, False, hip.THICK_F32, out, d2)
    assert as_float[0] == counters, ("counters", as_float[0], counters)
    slabs_equal(out.view(torch.int32), TR.as_float(want["T"]).view(np.int32), reps, "the float bits")
    slabs_equal(d2, want["depth2"], reps, "depth2")
    del d2
    out = out.view(torch.int32).fill_(-3)
    r2 = timed(dv, grid, None, cap, False, False, 0, out, None)
    assert r2[0] == counters, ("counters, r2", r2[0], counters)
    slabs_equal(out, want["T"], reps, "r2, the context's depth grid")
    print(f"largest_box {nx} x {ny} x {nz}: voxels {voxels}, blocks {-(-voxels // 256)}; candidates, kept, ball voxels {counters}, largest centre index {want['last']} "
          f"= 2^31 - {2 ** 31 - want['last']}; ms (wall, stages): float with depth2 {as_float[1:]}, r2 {r2[1:]}; the case {time.time() - t0:.1f} s")


def case_long_axes():
    """46 341 voxels, the longest axis accepted, along x, y and z: 725 chunks per row in K21's two row scans, envelope lines whose
    stack entries use all 16 bits.  Sets constant over the cross-section, border off: T, depth2, OPEN_ONLY and the centres are
    TR.line_reduction's; with the border on depth2' is at most 4, the balls are small and the literal scatter is affordable.

    It bites: with thick_border skipped in the look-ahead of k_thick_core_x (`return erow[x] >= cap` when ahead) the case failed
    at the call with the border on: ((3, 5, 46341), 'T with the border').  (With the border off thick_border changes nothing.)"""
    dv = hip.DeviceVoxelizer(0)
    top = hip.THICK_MAX_RADIUS2
    tables = {cap: hip.thickness_cover_table(cap) for cap in (top, 401)}
    past = 1 << 15
    for axis, shape in zip((2, 1, 0), TR.LONG_SHAPES):
        assert max(shape) == shape[axis] == TR.LONG and sum((n - 1) ** 2 for n in shape) <= 2 ** 31 - 2, shape
        line = TR.runs_line(TR.LONG, seed=31 + axis)
        cross = tuple(n for a, n in enumerate(shape) if a != axis)
        S = TR.along(line, shape, axis)
        t = dev(S)
        spread = lambda v: dev(TR.along(v, shape, axis))   # noqa: E731
        out = torch.full(shape, -3, dtype=torch.int32, device=DEV)
        d2 = torch.full(shape, -3, dtype=torch.int32, device=DEV)
        # cap 2^14, border off
        red = TR.line_reduction(line, top, tables[top])
        raw(dv, t, None, top, False, False, 0, out, d2)
        assert torch.equal(out, spread(red["T"])), (shape, "T", int((out != spread(red["T"])).sum()), "voxels differ")
        assert torch.equal(d2, spread(red["depth2"])), (shape, "depth2")
        n = cross[0] * cross[1]
        counters = (n * int(red["candidates"].sum()), n * int(red["kept"].sum()), TR.line_visited(red, cross))
        assert dv.thickness_counters() == counters, (shape, dv.thickness_counters(), counters)
        mid = (red["T"] > 1) & (red["T"] < top)
        assert (red["T"] == top).any() and mid[past + 1:].any() and red["kept"][past + 1:].any()
        # cap 401, OPEN_ONLY
        low = TR.line_reduction(line, 401, tables[401])
        raw(dv, t, None, 401, False, False, hip.THICK_OPEN_ONLY, out, d2)
        assert torch.equal(out, spread(low["open"])) and torch.equal(d2, spread(low["depth2"])) and dv.thickness_counters() == (0, 0, 0), (shape, "open")
        assert (low["open"] == 401).any() and ((low["open"] > 0) & (low["open"] < 401)).any()
        # cap 2^14, border on: depth2' = min(the line's depth2, the border term) <= 4
        d2b = np.where(S, np.minimum(TR.along(red["depth2"], shape, axis), TR.border_term(shape)), 0).astype(np.int32)
        assert int(d2b.max()) == 4
        cand, kept = TR.kept_centres(S, top, True, tables[top], d2b)
        raw(dv, t, None, top, True, False, 0, out, d2)
        assert torch.equal(d2, dev(d2b)), (shape, "depth2 with the border")
        assert torch.equal(out, dev(TR.thickness(S, top, True, d2b))), (shape, "T with the border")
        with_border = (int(cand.sum()), int(kept.sum()), TR.visited_small(d2b, kept))
        assert dv.thickness_counters() == with_border, (shape, dv.thickness_counters(), with_border)
        print(f"long_axes {shape}: {int(line.sum())} of {TR.LONG} positions in {int((np.diff(line.astype(np.int8)) == 1).sum()) + 1} runs, T reaches the cap 2^14 at "
              f"{int((red['T'] == top).sum())}; taken past 2^15 along axis {'zyx'[axis]}: {int(red['kept'][past + 1:].sum())} kept centres per cross-section "
              f"position, {int(mid[past + 1:].sum())} positions with 1 < T < cap; counters {counters}, with the border {with_border}; times {dv.thickness_times()}", flush=True)


def case_border_core():
    """Full boxes with the border on: depth2 is 0x7FFFFFFF everywhere and the core {depth2' >= cap} exists through thick_border
    alone, which k_thick_core_x evaluates once in the look-ahead (no write) and once in the chunk's own turn.  Rows of 200 and 131
    voxels: four and three chunks.  One empty voxel at the far end of the middle row is the row's only voxel outside S, which the
    depth scan's look-ahead has to find two chunks on - but in the two small boxes the border's min (m <= 4, m <= 2) hides what the
    depth scan gave everywhere but within a few voxels of the hole, so a look-ahead that missed it from chunks 0 - 2 would go
    unnoticed there.  Only the 131 x 129 x 129 box below shows it: with the hole, depth2 at x = 66 .. 127 of its middle rows
    is (130 - x)^2 from the look-ahead into chunk 2.  That box is not to be trimmed.

    m = min(x + 1, nx - x, y + 1, ny - y, z + 1, nz - z) is at most 4 in the 200 x 9 x 7 box (its rows y = 4, z = 3) and at most 2
    in the 131 x 70 x 3 box (z = 1): the core is empty at cap 17 in the first and from cap 5 on in the second, and where it is
    not empty it starts at x = 1 or 2.  A core that starts past the first chunk needs m >= 65: the 131 x 129 x 129 box at cap
    65^2 = 4225, whose core is the three voxels x = 64 .. 66 of its middle row y = 64, z = 64 alone (two with the empty voxel).  There depth2 and OPEN_ONLY are
    compared against the reference, and T of the full box - balls of up to 129 voxels across in three dimensions - against its closed
    form by levels (TR.full_box_thickness: the literal scatter of two million centres is out of reach).

    It bites: with thick_border skipped in the look-ahead of k_thick_core_x (`return erow[x] >= cap` when ahead) the case failed
    at its first call: (((200, 9, 7), False, 'u8'), 2, True, False, 'r2', 12, 'voxels differ')."""
    dv = hip.DeviceVoxelizer(0)
    n, empty_cores, late = 0, 0, None
    for dims, caps in (((200, 9, 7), (2, 5, 17)), ((131, 70, 3), (2, 5, 17, 1000))):
        nx, ny, nz = dims
        for hole in (False, True):
            S = np.ones(dims[::-1], bool)
            if hole:
                S[nz // 2, ny // 2, nx - 1] = False      # the only voxel outside S, in the last chunk of the middle row
            r = Ref(S)
            for fmt, t, width in (("u8", dev(S.astype(np.uint8)), None), ("bits", dev(pack_padded(S)), nx)):
                for cap in caps:
                    for kind in ("r2", "open"):
                        check(dv, t, r, cap, border=True, kind=kind, what=(dims, hole, fmt), nx=width, visited=True)
                        n += 1
                    core = r.depth2(True) >= cap
                    empty_cores += not core.any()
                    assert core.any() == (cap <= ((min(dims) + 1) // 2) ** 2), (dims, cap)
    assert empty_cores > 0
    dims, cap = (131, 129, 129), 65 * 65
    nx, ny, nz = dims
    for hole in (False, True):
        S = np.ones(dims[::-1], bool)
        if hole:
            S[nz // 2, ny // 2, nx - 1] = False
        r = Ref(S)
        core = np.argwhere(r.depth2(True) >= cap)
        # (z, y, x): found by the look-ahead of chunk 0 in chunk 1; the empty voxel at x = 130 is 64 from x = 66, which leaves the core
        assert core.tolist() == [[64, 64, x] for x in ((64, 65) if hole else (64, 65, 66))], core
        late = int(core[0][2])
        check(dv, dev(S), r, cap, border=True, kind="open", what=(dims, hole))
        n += 1
        if not hole:   # T of the full box by levels in closed form (held against the scatter by tests/test_host_thickness.py)
            r.memo["T", cap, True] = TR.full_box_thickness(dims, cap)
            check(dv, dev(S), r, cap, border=True, kind="r2", what=(dims, "the full box"))
            # the ball voxels per radius class: depth2' = m^2 puts the centre m - 1 voxels or more from every face and its ball
            # {|q|^2 < m^2} reaches m - 1, so no ball of the full box is clipped and each holds the whole digital ball of its radius
            _, kept = TR.kept_centres(S, cap, True, hip.thickness_cover_table(cap), r.depth2(True))
            radii, counts = np.unique(r.depth2(True)[kept], return_counts=True)
            balls = sum(int(c) * int(TR.ball(int(R))[0].sum()) for R, c in zip(radii, counts))
            assert int(radii.max()) == 64 * 64 and dv.thickness_counters()[2] == balls, ("ball voxels of the full box", dv.thickness_counters()[2], balls)
            big = (r.get("centres", cap, True), balls, [round(ms, 1) for ms in dv.thickness_times()])
            assert big[0][1] > 0
            n += 1
    assert late >= 64
    print(f"border_core: compared {n} calls on full boxes with the border on, u8 and bits, with and without one empty voxel at the far end of the middle row; "
          f"{empty_cores} of the 28 boxes / formats / caps without a core; in the 131 x 129 x 129 box at cap 4225 the core starts at x = {late} of the row y = 64, z = 64; its full box: candidates and kept {big[0]}, {big[1]} ball voxels, ms {big[2]}")


def pack_padded(S):
    """int32 [z, y, ceil(nx / 32)]: bit x % 32 of word x / 32, the padding of the last word set (it is not part of the box)."""
    nz, ny, nx = S.shape
    words = (nx + 31) // 32
    padded = np.ones((nz, ny, words * 32), np.uint64)
    padded[:, :, :nx] = S
    w = (padded.reshape(nz, ny, words, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32).view(np.int32)


CASES = {"formats_and_layouts": case_formats_and_layouts, "large_radii": case_large_radii, "many_centres": case_many_centres, "clipping": case_clipping,
         "morphology": case_morphology, "pipeline": case_pipeline, "refusals": case_refusals, "block_turns": case_block_turns, "largest_box": case_largest_box,
         "long_axes": case_long_axes, "border_core": case_border_core}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
