"""The GPU cases of tests/test_gpu_nearest.py, each run in a child process of its own: `python -m tests.nearest_cases <case>`.

torch is imported before the library is loaded (the grids are torch tensors; see tests/dense_cases.py).  Every comparison is
np.array_equal on int32 against the numpy references of tests/nearest_ref.py (or a closed form), never against the code under
test.  A case prints what it covered and "ok" last when everything held."""
import os
import sys
import tempfile

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import distance_ref as R
from tests import gather_ref as GR
from tests import nearest_ref as N
from tests.dense_cases import torus

DEV = torch.device("cuda", 0)
NO_LIMIT = 0x7FFFFFFF


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def check(dv, seed, want=None, what="", **kw):
    """nearest and dist2 of the device for the seeds `seed` (a bool array, or labels with surface_only=True in kw) against
    `want` = (nearest, d2) (the separable reference unless given), and dist2 against K8's on the device for the same seeds."""
    seed = np.asarray(seed)
    is_seed = seed == 1 if kw.get("surface_only") else seed != 0
    want_near, want_d2 = N.separable_nearest(is_seed) if want is None else want
    near, d2 = dense.nearest_voxel(dv, dev(seed), dist2=True, **kw)
    near, d2 = host(near), host(d2)
    assert near.dtype == np.int32 and near.shape == seed.shape, (what, near.dtype, near.shape)
    assert np.array_equal(near, want_near), (what, seed.shape, int((near != want_near).sum()), "nearest differ")
    assert d2.dtype == np.int32 and np.array_equal(d2, want_d2), (what, seed.shape, int((d2 != want_d2).sum()), "dist2 differ")
    k8 = host(dense.distance_transform(dv, dev(is_seed.astype(np.uint8)), "dist2"))
    assert np.array_equal(d2, k8), (what, seed.shape, "dist2 differs from distance_transform's")
    alone = host(dense.nearest_voxel(dv, dev(seed), **kw))      # (without dist2: the z pass with a null dist2)
    assert np.array_equal(alone, want_near), (what, seed.shape, "nearest without dist2")
    return want_near, want_d2


def case_random():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(15)
    n = 0
    shapes = [(1, 1, 1), (2, 2, 2), (1, 1, 257), (257, 1, 1), (1, 257, 1), (63, 63, 63), (64, 64, 64), (65, 65, 65),
              (129, 7, 300), (5, 3, 257), (3, 70, 129)]
    for shape in shapes:
        for density in (0.0005, 0.01, 0.3):
            check(dv, rng.random(shape) < density, what=f"density {density}")
            n += 1
    seed = rng.random((9, 10, 11)) < 0.05
    check(dv, seed, N.brute_nearest(seed), "brute")
    for shape in ((1, 1, 1), (7, 9, 130), (65, 65, 65)):
        seed = np.zeros(shape, bool)
        near, d2 = check(dv, seed, what="no seeds")
        assert (near == -1).all() and (d2 == NO_LIMIT).all()
        seed[tuple(s // 3 for s in shape)] = True
        near, _ = check(dv, seed, what="one seed")
        assert len(np.unique(near)) == 1 and near.flat[0] >= 0
        near, d2 = check(dv, np.ones(shape, bool), what="all seeds")
        assert np.array_equal(near.ravel(), np.arange(near.size)) and not d2.any()
        n += 3
    # rows, columns and planes without seeds
    seed = rng.random((64, 65, 257)) < 0.01
    seed[:, 10:20, :] = False
    seed[5:30, :, :] = False
    seed[:, :, 100:230] = False
    check(dv, seed, what="empty rows and planes")
    seed = np.zeros((65, 64, 200), bool)
    seed[:, :, 199] = True     # one seed per row, at its far end: the look-ahead crosses every chunk
    seed[3, 5, 0] = True
    check(dv, seed, what="far seeds")
    print("compared", n + 3)


def case_ties():
    dv = hip.DeviceVoxelizer(0)
    for name, seed in N.tie_grids().items():
        share = N.tie_share(seed)
        check(dv, seed, N.brute_nearest(seed), name)
        print("ties", name, seed.shape, "seeds", int(seed.sum()), "voxels with more than one nearest seed", round(share * seed.size), "of", seed.size)
        assert (share == 0.0) == (name in N.NO_TIES), name
        if name == "lattice":
            assert share >= 0.25, share
            print("lattice share", round(share, 4))


def pack_bits(seed):
    """int32 [z, y, ceil(nx / 32)]: bit x % 32 of word x / 32."""
    nz, ny, nx = seed.shape
    words = (nx + 31) // 32
    padded = np.zeros((nz, ny, words * 32), np.uint64)
    padded[:, :, :nx] = seed
    w = (padded.reshape(nz, ny, words, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32).view(np.int32)


def case_formats():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(16)
    shape = (7, 9, 70)     # nx a multiple of neither 32 nor 64: the last word of a row is part empty
    shapes = []
    for density in (0.004, 0.1, None):
        seed = R.scan_rows() if density is None else rng.random(shape) < density
        shapes.append(seed.shape)
        nz, ny, nx = seed.shape
        words = (nx + 31) // 32
        assert seed.any()
        want = N.separable_nearest(seed)
        check(dv, seed, want, "bool")
        labels = np.where(seed, 1, np.where(rng.random(seed.shape) < 0.4, 2, 0)).astype(np.uint8)
        assert (labels == 2).any()
        check(dv, labels, want, "labels, surface_only", surface_only=True)
        check(dv, labels, None, "labels, every non-zero voxel a seed")
        level = 0.25
        field = np.where(seed, level - rng.random(seed.shape) - 1e-3, level + rng.random(seed.shape)).astype(np.float32)
        field[~seed & (rng.random(seed.shape) < 0.2)] = level           # (at the level: not below it)
        near, d2 = dense.nearest_voxel(dv, dev(field), level=level, dist2=True)
        assert np.array_equal(host(near), want[0]) and np.array_equal(host(d2), want[1]), "float32 with a level"
        # bits at the C level: dims of nx voxels over rows of whole words (70 voxels: 3 words)
        bits = dev(pack_bits(seed))
        assert tuple(bits.shape) == (nz, ny, words)
        near = torch.full(seed.shape, -5, dtype=torch.int32, device=DEV)
        d2 = torch.full(seed.shape, -5, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        dv.nearest_dense(bits.data_ptr(), hip.GRID_BITS, (1, words, words * ny), (nx, ny, nz), 0.0, 0, near.data_ptr(), (1, nx, nx * ny),
                         d2.data_ptr(), (1, nx, nx * ny))
        assert np.array_equal(host(near), want[0]) and np.array_equal(host(d2), want[1]), ("bits", nx, "voxels")
        # ... and through dense: 32 voxels per word, the box as wide as its words (70 voxels: 96) and its last columns without seeds
        padded = np.zeros((nz, ny, 32 * words), bool)
        padded[:, :, :nx] = seed
        want_padded = N.separable_nearest(padded)
        near, d2 = dense.nearest_voxel(dv, bits, dist2=True)
        assert tuple(near.shape) == padded.shape and np.array_equal(host(near), want_padded[0]) and np.array_equal(host(d2), want_padded[1]), ("bits", 32 * words, "voxels")
    print("formats", shapes, "bool, labels, float32, bits at nx voxels and at whole words")


def case_strided():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(17)
    shape = nz, ny, nx = (33, 20, 70)
    batch_np = np.stack([R.random_labels(rng, shape, d) for d in (0.002, 0.05)])
    batch = dev(batch_np)
    for i in range(2):
        lab = batch_np[i]
        want_near, want_d2 = N.separable_nearest(lab == 1)
        colors = rng.integers(-2 ** 31, 2 ** 31, shape).astype(np.int32)
        painted = colors.ravel()[want_near]
        # nearest: a slice of a batch; dist2: stored [x][z][y] inside a larger buffer; values: every second element along x
        out = torch.full((2,) + shape, 7, dtype=torch.int32, device=DEV)
        dbuf = torch.full((nx + 2, nz, ny), 7, dtype=torch.int32, device=DEV)
        d2 = dbuf[1:-1].permute(1, 2, 0)
        got, got_d2 = dense.nearest_voxel(dv, batch[i], surface_only=True, out=out[1 - i], dist2=d2)
        assert got.data_ptr() == out[1 - i].data_ptr() and got_d2.data_ptr() == d2.data_ptr()
        assert np.array_equal(host(out[1 - i]), want_near) and np.array_equal(host(d2), want_d2), i
        assert bool((out[i] == 7).all()) and bool((dbuf[0] == 7).all()) and bool((dbuf[-1] == 7).all()), "a write outside the views"
        vbuf = torch.full((nz, ny, 2 * nx), 7, dtype=torch.int32, device=DEV)
        values = vbuf[:, :, ::2]
        got = dense.spread_colors(dv, batch[i], dev(colors), surface_only=True, out=values)
        assert got.data_ptr() == values.data_ptr() and np.array_equal(host(values), painted), i
        assert bool((vbuf[:, :, 1::2] == 7).all()), "a write between the values"
        # everything permuted: seeds stored [y][x][z], nearest [x][z][y], values [x][y][z] painted in place
        lab_p = batch[i].permute(1, 2, 0).contiguous().permute(2, 0, 1)
        out_p = torch.zeros((nx, nz, ny), dtype=torch.int32, device=DEV).permute(1, 2, 0)
        dense.nearest_voxel(dv, lab_p, surface_only=True, out=out_p)
        assert np.array_equal(host(out_p), want_near), (i, "permuted")
        col_p = dev(colors).permute(2, 1, 0).contiguous().permute(2, 1, 0)
        assert col_p.stride() == (1, nz, nz * ny)
        dense.spread_colors(dv, lab_p, col_p, surface_only=True, out=col_p)
        assert np.array_equal(host(col_p), painted), (i, "permuted, in place")
    print("strided", shape)


def case_values():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(18)
    shape = (33, 20, 70)
    labels = R.random_labels(rng, shape, 0.001, interior=0.4)
    seed = labels == 1
    near, d2 = N.separable_nearest(seed)
    colors = rng.integers(-2 ** 31, 2 ** 31, shape).astype(np.int32)
    assert (colors < 0).any() and (colors >= 0).any() and seed.sum() > 10 and (labels == 2).any() and (labels == 0).any()
    gathered = colors.ravel()[near]
    assert np.array_equal(gathered[seed], colors[seed])           # (a seed is its own nearest)
    lab_d = dev(labels)

    # in place, no limit: every voxel holds its nearest seed's colour; the seeds kept theirs
    c = dev(colors)
    assert dense.spread_colors(dv, lab_d, c, surface_only=True, out=c) is c
    assert np.array_equal(host(c), gathered)
    # every non-zero voxel a seed (no surface_only): the same through the other seed test
    near_all = N.separable_nearest(labels != 0)[0]
    assert np.array_equal(host(dense.spread_colors(dv, lab_d, dev(colors))), colors.ravel()[near_all])
    # inside_only: only the 2s change
    got = host(dense.spread_colors(dv, lab_d, dev(colors), surface_only=True, inside_only=True))
    assert np.array_equal(got, np.where(labels == 2, gathered, colors))
    assert (got != colors).any() and np.array_equal(got[labels != 2], colors[labels != 2])
    # max_distance: d2 == max_dist2 is painted, max_dist2 + 1 is not
    for r, m in ((0, 0), (1, 1), (3, 9), (4.5, 20)):
        at, past = d2 == m, d2 == m + 1
        assert at.any() and past.any(), (r, int(at.sum()), int(past.sum()))
        got = host(dense.spread_colors(dv, lab_d, dev(colors), surface_only=True, max_distance=r))
        assert np.array_equal(got, np.where(d2 <= m, gathered, colors)), r
        assert np.array_equal(got[at], gathered[at]) and np.array_equal(got[past], colors[past])
        assert r == 0 or (gathered[at] != colors[at]).any()
        assert (gathered[past] != colors[past]).any()
        both = host(dense.spread_colors(dv, lab_d, dev(colors), surface_only=True, inside_only=True, max_distance=r))
        assert np.array_equal(both, np.where((d2 <= m) & (labels == 2), gathered, colors)), (r, "inside_only")
        print("max_distance", r, "max_dist2", m, "voxels at it", int(at.sum()), "one past it", int(past.sum()))
    # no seeds: nothing changes
    for kw in (dict(), dict(surface_only=True), dict(surface_only=True, inside_only=True)):
        none = np.where(labels == 1, 2 if kw else 0, labels if kw else 0).astype(np.uint8)
        assert np.array_equal(host(dense.spread_colors(dv, dev(none), dev(colors), **kw)), colors), kw
    # the three out modes agree, and the first leaves colors alone
    c = dev(colors)
    clone = dense.spread_colors(dv, lab_d, c, surface_only=True, max_distance=3)
    assert clone.data_ptr() != c.data_ptr() and np.array_equal(host(c), colors)
    other = torch.full(shape, 7, dtype=torch.int32, device=DEV)
    assert dense.spread_colors(dv, lab_d, c, surface_only=True, max_distance=3, out=other) is other and np.array_equal(host(c), colors)
    dense.spread_colors(dv, lab_d, c, surface_only=True, max_distance=3, out=c)
    assert torch.equal(clone, other) and torch.equal(clone, c) and not np.array_equal(host(c), colors)
    # one run equals another bit for bit
    assert torch.equal(dense.spread_colors(dv, lab_d, dev(colors), surface_only=True), dense.spread_colors(dv, lab_d, dev(colors), surface_only=True))
    print("values", shape, "seeds", int(seed.sum()), "interior", int((labels == 2).sum()))


# ---- at the limits the call documents -----------------------------------------------------------------------------------

def case_lane_cap():
    """More lines than the 2^17 lanes in both envelope passes, every voxel compared: a lane's second and later lines, and a
    plane without seeds, whose lines along y carry no payload."""
    dv = hip.DeviceVoxelizer(0)
    for shape in R.LANE_CAP_SHAPES:
        nz, ny, nx = shape
        ly, lz = R.pass_lines(shape)
        assert ly > R.LANE_CAP and lz > R.LANE_CAP, shape
        for density, empty_plane in ((0.01, None), (3e-6, 2)):
            lab = R.lane_cap_labels(shape, density, seed=17, empty_plane=empty_plane)
            dark = nx * int((~(lab == 1).any(axis=(1, 2))).sum())      # lines along y of the planes without a seed
            assert (lab == 1).any() and (lab == 2).any() and (empty_plane is None or dark > 0), (shape, density)
            near, _ = check(dv, lab, None, f"lane cap, density {density}", surface_only=True)
            print("lane_cap", shape, "lines y", ly, "z", lz, "cap", R.LANE_CAP, "last turn", ly % R.LANE_CAP, lz % R.LANE_CAP, "density", density,
                  "seeds", int((lab == 1).sum()), "y lines without a payload", dark, "largest index", int(near.max()))
    assert all(n % R.LANE_CAP and n % 256 for n in R.pass_lines(R.LANE_CAP_SHAPES[1]))


def case_long_lines():
    """Lines of 46 341 voxels, the longest accepted, along z, y and x, with seeds at both ends and past position 2^15: fx, fy
    and the s and t of a stack entry use their upper bit.  (No accepted box with such an axis has 2^22 voxels at these widths:
    the largest index here is past 2^21.)"""
    dv = hip.DeviceVoxelizer(0)
    top = 0
    for shape in R.LONG_SHAPES:
        assert max(shape) == R.LONG and sum((n - 1) ** 2 for n in shape) <= R.D2_LIMIT, shape
        lab = R.long_line_labels(shape, seed=29)
        axis = int(np.argmax(shape))
        near, d2 = check(dv, lab, None, "long lines", surface_only=True)
        coords = np.stack(np.unravel_index(near.ravel().astype(np.int64), shape))      # (z, y, x) of the seeds taken
        along = coords[axis]
        assert int(along.max()) == R.LONG - 1 and int((np.unique(along) > 1 << 15).sum()) >= 6, shape
        top = max(top, int(near.max()))
        print("long_lines", shape, "seeds", int((lab == 1).sum()), "taken past 2^15 along axis", "zyx"[axis], int((np.unique(along) > 1 << 15).sum()),
              "largest index", int(near.max()), "largest d2", int(d2.max()))
    assert top > 1 << 21, top


def deep_stack_closed_form():
    """(nearest, d2) [1024, 2100] of R.deep_stack_labels: the last column and the last row are seeds."""
    y, x = np.indices((1024, 2100))
    near = np.where((2099 - x) ** 2 <= (1023 - y) ** 2, y * 2100 + 2099, 1023 * 2100 + x).astype(np.int32)
    return near, np.minimum((2099 - x) ** 2, (1023 - y) ** 2).astype(np.int32)


def case_deep_stacks():
    """An envelope a thousand entries deep that empties at one position, in the y pass and in the z pass, against the closed
    form (tests/test_host_nearest.py holds it against the reference): of the seed in the voxel's row and the seed in its column
    the nearer, the row's (the smaller index) on a tie."""
    dv = hip.DeviceVoxelizer(0)
    y, x = np.indices((1024, 2100))
    closed, closed_d2 = deep_stack_closed_form()
    for along_z, interior in ((False, 41), (True, 43)):
        lab = R.deep_stack_labels(along_z, interior)
        assert (lab == 2).any()
        stats = []
        R.separable_d2(lab, stats)
        depth, pops, _ = stats[1 if along_z else 0]
        deep, long_runs = int((depth >= 1000).sum()), int((pops >= 1000).sum())
        assert deep > 0 and long_runs > 0, (deep, long_runs)
        want = (closed.reshape(lab.shape), closed_d2.reshape(lab.shape))
        check(dv, lab, want, "deep stacks", surface_only=True)
        ties = int(((2099 - x) ** 2 == (1023 - y) ** 2).sum())
        print("deep_stacks", lab.shape, "lines", len(depth), "depth >= 1000 on", deep, "largest", int(depth.max()), ">= 1000 pops at one position on",
              long_runs, "voxels as far from their row's seed as from their column's", ties)


def case_largest_box():
    """1290^3 = 2 146 689 000 voxels, the largest cube under the limit of 2^31 - 1: element offsets and linear indices next to
    2^31, more lines than lanes in both passes.  Seeds at the first and the last voxel; a voxel is nearer to the first where
    x + y + z < 3 * 1289 / 2 (the sum is never equal to it), so everything has a closed form, compared plane by plane on the device."""
    dv = hip.DeviceVoxelizer(0)
    n = 1290
    m, last = n - 1, n ** 3 - 1
    assert 2 ** 31 - 2 ** 20 < last < 2 ** 31 - 1 and (n + 1) ** 3 > 2 ** 31 - 1
    seeds = torch.zeros((n, n, n), dtype=torch.uint8, device=DEV)
    colors = torch.full((n, n, n), 5, dtype=torch.int32, device=DEV)
    seeds[0, 0, 0] = seeds[m, m, m] = 1
    c0, c1 = -1234567, 0x7654321
    colors[0, 0, 0], colors[m, m, m] = c0, c1
    near, d2 = dense.nearest_voxel(dv, seeds, dist2=True)
    assert dense.spread_colors(dv, seeds, colors, out=colors) is colors
    a = torch.arange(n, dtype=torch.int32, device=DEV)
    y, x = a[None, :, None], a[None, None, :]
    scalar = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)   # noqa: E731
    for z0 in range(0, n, 64):
        z = a[z0:z0 + 64, None, None]
        first = (x + y + z) * 2 < 3 * m
        d0, d1 = x * x + y * y + z * z, (m - x) ** 2 + (m - y) ** 2 + (m - z) ** 2
        assert torch.equal(near[z0:z0 + 64], torch.where(first, scalar(0), scalar(last))), ("nearest", z0)
        assert torch.equal(d2[z0:z0 + 64], torch.where(first, d0, d1)), ("dist2", z0)
        assert torch.equal(colors[z0:z0 + 64], torch.where(first, scalar(c0), scalar(c1))), ("values", z0)
    print("largest_box", (n, n, n), "voxels", n ** 3, "largest index", int(near.max()), "largest d2", int(d2.max()), "times", dv.nearest_times())


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def expect_code(code, fn, what):
    try:
        fn()
    except hip.DeviceError as e:
        assert f"code {code}" in str(e) and "o2v_hip_nearest_dense" in str(e), (what, str(e))
        return what + ": " + str(e)
    raise AssertionError(what + " was accepted")


def case_refusals():
    dv = hip.DeviceVoxelizer(0)
    n = 24
    shape, dims, st = (n, n, n), (n, n, n), (1, n, n * n)
    rng = np.random.default_rng(19)
    seed_np = rng.random(shape) < 0.01
    want = N.separable_nearest(seed_np)
    colors_np = rng.integers(-2 ** 31, 2 ** 31, shape).astype(np.int32)
    lab = dev(seed_np.astype(np.uint8))
    f32 = dev(np.where(seed_np, -1.0, 1.0).astype(np.float32))
    bits = dev(pack_bits(seed_np))
    near = torch.full(shape, 7, dtype=torch.int32, device=DEV)
    d2 = torch.full(shape, 7, dtype=torch.int32, device=DEV)
    val = dev(colors_np)
    short = torch.full((n // 2, n, n), 7, dtype=torch.int32, device=DEV)
    line = torch.full((n,), 7, dtype=torch.int32, device=DEV)
    shared = torch.full((3 * n ** 3,), 7, dtype=torch.int32, device=DEV)      # several grids in one allocation
    host_i32 = np.zeros(shape, np.int32)
    host_u8 = seed_np.astype(np.uint8)
    torch.cuda.synchronize()
    U8, BITS, F32 = hip.GRID_U8, hip.GRID_BITS, hip.GRID_F32_BELOW
    one, inside = hip.NEAREST_SEED_ONE, hip.NEAREST_VALUES_INSIDE
    L, P, D, V, S = lab.data_ptr(), near.data_ptr(), d2.data_ptr(), val.data_ptr(), shared.data_ptr()
    bst = (1, 1, n)     # one word per row

    def good():
        """After a refusal the context still works, and the refusal wrote nothing."""
        assert bool((near == 7).all()) and bool((d2 == 7).all()) and np.array_equal(host(val), colors_np)
        assert bool((short == 7).all()) and bool((line == 7).all()) and bool((shared == 7).all())
        a, b = dense.nearest_voxel(dv, lab, dist2=True)
        assert np.array_equal(host(a), want[0]) and np.array_equal(host(b), want[1])

    call = dv.nearest_dense
    refusals = [
        (5, lambda: call(L, U8, (1, 1291, 1291 * 1291), (1291, 1291, 1291), 0.0, 0, P, (1, 1291, 1291 * 1291)), "1291^3 voxels"),
        (5, lambda: call(L, U8, (1, 46342, 46342), (46342, 1, 1), 0.0, 0, P, (1, 46342, 46342)), "46342 x 1 x 1"),
        (5, lambda: call(L, U8, (1, 1, 1), (1, 1, 46342), 0.0, 0, P, (1, 1, 1)), "1 x 1 x 46342"),
        (3, lambda: call(L, U8, st, (n, 0, n), 0.0, 0, P, st), "zero dims"),
        (3, lambda: call(None, U8, st, dims, 0.0, 0, P, st), "null grid"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, None, st), "null nearest"),
        (3, lambda: call(L, U8, None, dims, 0.0, 0, P, st), "null strides"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, P, None), "null nearest strides"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, P, st, D, None), "dist2 without strides"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, P, st, None, None, V, None), "values without strides"),
        (3, lambda: call(L, 3, st, dims, 0.0, 0, P, st), "unknown format"),
        (3, lambda: call(L, U8, st, dims, 0.0, 4, P, st), "unknown flag"),
        (3, lambda: call(f32.data_ptr(), F32, st, dims, float("nan"), 0, P, st), "level nan"),
        (3, lambda: call(f32.data_ptr(), F32, st, dims, float("inf"), 0, P, st), "level inf"),
        (3, lambda: call(bits.data_ptr(), BITS, (2, 1, n), dims, 0.0, 0, P, st), "bits with an x stride of 2"),
        (3, lambda: call(bits.data_ptr(), BITS, bst, dims, 0.0, one, P, st), "SEED_ONE on bits"),
        (3, lambda: call(f32.data_ptr(), F32, st, dims, 0.0, one, P, st), "SEED_ONE on float32"),
        (3, lambda: call(f32.data_ptr(), F32, st, dims, 0.0, inside, P, st, None, None, V, st), "VALUES_INSIDE on float32"),
        (3, lambda: call(bits.data_ptr(), BITS, bst, dims, 0.0, inside, P, st, None, None, V, st), "VALUES_INSIDE on bits"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, line.data_ptr(), (1, 0, 0)), "nearest with strides of 0"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, P, (1, n // 2, n * n)), "nearest with y inside x"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, P, st, line.data_ptr(), (1, 0, 0)), "dist2 with strides of 0"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, P, st, None, None, line.data_ptr(), (0, 1, 0)), "values with strides of 0"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, short.data_ptr(), st), "short nearest"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, P, st, short.data_ptr(), st), "short dist2"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, P, st, None, None, short.data_ptr(), st), "short values"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, host_i32.ctypes.data, st), "host nearest"),
        (3, lambda: call(host_u8.ctypes.data, U8, st, dims, 0.0, 0, P, st), "host grid"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, P, st, host_i32.ctypes.data, st), "host dist2"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, P, st, None, None, host_i32.ctypes.data, st), "host values"),
        # overlaps: the last element of one range is the first of the next
        (3, lambda: call(S, U8, st, dims, 0.0, 0, S + n ** 3 - 4, st), "grid and nearest overlap"),
        (3, lambda: call(S, F32, st, dims, 0.0, 0, S + 4 * (n ** 3 - 1), st), "float32 grid and nearest overlap"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, S, st, S + 4 * (n ** 3 - 1), st), "nearest and dist2 overlap"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, S, st, None, None, S + 4 * (n ** 3 - 1), st), "nearest and values overlap"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, P, st, S, st, S + 4 * (n ** 3 - 1), st), "dist2 and values overlap"),
        (3, lambda: call(S, U8, st, dims, 0.0, 0, P, st, None, None, S + n ** 3 - 4, st), "grid and values overlap"),
        (3, lambda: call(S, U8, st, dims, 0.0, 0, P, st, S + n ** 3 - 4, st), "grid and dist2 overlap"),
        (3, lambda: call(L, U8, st, dims, 0.0, 0, P, st, P, st), "nearest is dist2"),
    ]
    msgs = []
    for code, fn, what in refusals:
        msgs.append(expect_code(code, fn, what))
        good()
    assert all("one element" in m for m in msgs if "strides of 0" in m or "y inside x" in m), msgs
    assert all("overlap" in m.split(": ", 1)[1] for m in msgs if "overlap" in m.split(":")[0] or "nearest is dist2" in m), msgs
    # through dense: an expand()ed out
    try:
        dense.nearest_voxel(dv, lab, out=line.view(1, 1, n).expand(n, n, n))
        raise AssertionError("an expanded out was accepted")
    except hip.DeviceError as e:
        assert "code 3" in str(e), str(e)
    good()
    # next to each other in one allocation: accepted
    shared.zero_()
    shared[:n ** 3 // 4] = dev(host_u8.ravel().view(np.int32))
    torch.cuda.synchronize()
    call(S, U8, st, dims, 0.0, 0, S + n ** 3, st, S + n ** 3 + 4 * n ** 3, st)
    got = host(shared)
    assert np.array_equal(got[n ** 3 // 4:n ** 3 // 4 + n ** 3].reshape(shape), want[0])
    assert np.array_equal(got[n ** 3 // 4 + n ** 3:n ** 3 // 4 + 2 * n ** 3].reshape(shape), want[1])
    assert dv.nearest_scratch_bytes(dims) == dv.distance_scratch_bytes(dims, hip.DIST_SQ_I32) > 0 and all(t >= 0 for t in dv.nearest_times())
    print("\n".join(msgs))
    print("refused", len(msgs) + 1)


# ---- the flow of the README ------------------------------------------------------------------------------------------------------

def case_mesh():
    dv = hip.DeviceVoxelizer(0)
    verts = torus()
    T = len(verts)
    types = np.full(T, hip.TRI_UNTEXTURED, np.uint32)
    dense.set_mesh(dv, dev(verts), types=dev(types.view(np.int32)), colors=dev(meshes.triangle_colors(T)))
    res, fill = 48, 0xFFFFFFFF
    labels, origin = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
    argb, _ = dense.voxelize_dense(dv, res, fmt="argb", fill=True)
    lab, before = host(labels), host(argb)
    interior, surface = lab == 2, lab == 1
    assert interior.sum() > 1000 and surface.sum() > 1000 and (before[interior].view(np.uint32) == fill).all()
    assert len(np.unique(before[surface])) > 100
    near, _ = N.separable_nearest(surface)
    want = np.where(interior, before.ravel()[near], before)
    got = dense.spread_colors(dv, labels, argb, surface_only=True, inside_only=True, out=argb)
    assert got is argb
    after = host(argb)
    assert np.array_equal(after, want), int((after != want).sum())
    assert np.array_equal(after[~interior], before[~interior]), "a surface or exterior voxel changed"
    assert (after[interior].view(np.uint32) != fill).all() and len(np.unique(after[interior])) > 50
    # the records and the file carry those colours
    records = GR.records(lab, GR.U8, origin=origin, colors=want)
    rec = dense.to_voxels(dv, labels, origin=origin, colors=argb)
    assert np.array_equal(host(rec).view(np.uint32), records)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "solid.vl32")
        assert dense.save_voxels(dv, labels, path, origin=origin, colors=argb, resolution=res) == len(records)
        assert np.array_equal(GR.parse_vl32(open(path, "rb").read()), records)
    # a shell of two voxels inwards, and nearest_coords of the same seeds
    shell = host(dense.spread_colors(dv, labels, dev(before), surface_only=True, inside_only=True, max_distance=2))
    d2 = N.d2_of(near)
    assert np.array_equal(shell, np.where(interior & (d2 <= 4), before.ravel()[near], before)) and (interior & (d2 > 4)).any()
    xyz = host(dense.nearest_coords(dense.nearest_voxel(dv, labels, surface_only=True)))
    assert np.array_equal(xyz, np.stack([near % res, near // res % res, near // (res * res)], axis=-1).astype(np.int32))
    print("mesh: torus at", res, "surface", int(surface.sum()), "interior", int(interior.sum()), "colours inside", len(np.unique(after[interior])))


CASES = {"random": case_random, "ties": case_ties, "formats": case_formats, "strided": case_strided, "values": case_values,
         "lane_cap": case_lane_cap, "long_lines": case_long_lines, "deep_stacks": case_deep_stacks, "largest_box": case_largest_box,
         "refusals": case_refusals, "mesh": case_mesh}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
