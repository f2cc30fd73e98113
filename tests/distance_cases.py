"""The GPU cases of tests/test_gpu_distance.py, each run in a child process of its own: `python -m tests.distance_cases <case>`.

torch is imported before the library is loaded (the grids are torch tensors; see tests/dense_cases.py).  Every comparison is
bit for bit: DIST2 as int32, SDF as the int32 bits of its float32.  A case prints "ok" last when everything held."""
import sys

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import distance_ref as R
from tests import fill_ref
from tests.dense_cases import expect_code3, torus

DEV = torch.device("cuda", 0)


def run(dv, labels_np, fmt):
    lab = torch.from_numpy(np.ascontiguousarray(labels_np)).to(DEV)
    return dense.distance_transform(dv, lab, fmt).cpu().numpy()


def check(dv, labels, d2=None, what=""):
    """Both formats of the device transform of `labels` against the reference (separable unless d2 is given)."""
    want = R.separable_d2(labels) if d2 is None else d2
    got = run(dv, labels, "dist2")
    assert got.dtype == np.int32 and np.array_equal(got, want), (what, labels.shape, int((got != want).sum()))
    got = run(dv, labels, "sdf")
    want_sdf = R.sdf(labels, want)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want_sdf.view(np.int32)), (what, labels.shape)


def case_random():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(11)
    n = 0
    # [z, y, x] shapes: dims 1, 2, 63, 64, 65, 257 and non-cubes
    shapes = [(1, 1, 1), (2, 2, 2), (1, 1, 257), (257, 1, 1), (1, 257, 1), (63, 63, 63), (64, 64, 64), (65, 65, 65),
              (129, 7, 300), (5, 3, 257), (3, 70, 129), (40, 33, 1000)]
    for shape in shapes:
        for density in (0.0005, 0.01, 0.3):
            check(dv, R.random_labels(rng, shape, density), what=f"density {density}")
            n += 1
    small = (9, 10, 11)
    brute = lambda lab: R.brute_d2(lab)   # noqa: E731
    lab = R.random_labels(rng, small, 0.05)
    check(dv, lab, brute(lab), "brute")
    for shape in ((1, 1, 1), (7, 9, 130), (65, 65, 65)):
        lab = np.zeros(shape, np.uint8)
        lab[rng.random(shape) < 0.4] = 2
        check(dv, lab, what="no seeds")                                  # INF / +-inf everywhere
        lab[tuple(s // 3 for s in shape)] = 1
        check(dv, lab, what="one seed")
        check(dv, np.ones(shape, np.uint8), what="all seeds")
        n += 3
    # rows, columns and planes without seeds
    lab = R.random_labels(rng, (64, 65, 257), 0.01)
    lab[:, 10:20, :] = 0
    lab[5:30, :, :] = 0
    lab[:, :, 100:230] = 0
    check(dv, lab, what="empty rows and planes")
    lab = np.zeros((65, 64, 200), np.uint8)
    lab[:, :, 199] = 1     # one seed per row, at its far end: the look-ahead crosses every chunk
    lab[3, 5, 0] = 1
    check(dv, lab, what="far seeds")
    lab = np.where(R.scan_rows(), 1, np.where(rng.random((3, 2, 193)) < 0.3, 2, 0)).astype(np.uint8)
    check(dv, lab, what="scan rows")
    print("compared", n + 5)


def case_strided():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(5)
    batch_np = np.stack([R.random_labels(rng, (33, 70, 129), d) for d in (0.002, 0.05)])
    batch = torch.from_numpy(batch_np).to(DEV)
    for fmt, dtype in (("dist2", torch.int32), ("sdf", torch.float32)):
        for i in range(2):
            want = R.separable_d2(batch_np[i])
            want = want if fmt == "dist2" else R.sdf(batch_np[i], want).view(np.int32)
            out = torch.full((2, 33, 70, 129), 7, dtype=dtype, device=DEV)
            got = dense.distance_transform(dv, batch[i], fmt, out=out[1 - i])
            assert got.data_ptr() == out[1 - i].data_ptr()
            assert np.array_equal(out[1 - i].cpu().numpy().view(np.int32), want), (fmt, i)
            assert bool((out[i] == 7).all()), "a write outside the slice"
            # permuted views: labels stored [y][x][z], out stored [x][z][y], both looked at as [z, y, x]
            lab_p = batch[i].permute(1, 2, 0).contiguous().permute(2, 0, 1)
            out_p = torch.zeros((129, 33, 70), dtype=dtype, device=DEV).permute(1, 2, 0)
            dense.distance_transform(dv, lab_p, fmt, out=out_p)
            assert np.array_equal(out_p.cpu().numpy().view(np.int32), want), (fmt, i, "permuted")
    print("ok strided")


def case_corner():
    """A plane with one corner seed: d2 = x^2 + y^2, past 2^24, for the rounding of the sqrt."""
    dv = hip.DeviceVoxelizer(0)
    n = 4096
    lab = torch.zeros((1, n, n), dtype=torch.uint8, device=DEV)
    lab[0, 0, 0] = 1
    lab[0, n // 2:, :] = torch.where(lab[0, n // 2:, :] == 0, 2, 1).to(torch.uint8)
    i = np.arange(n, dtype=np.int64)
    d2 = (i[None, :] ** 2 + i[:, None] ** 2)[None]
    lab_np = lab.cpu().numpy()
    got = dense.distance_transform(dv, lab, "dist2").cpu().numpy()
    assert np.array_equal(got, d2.astype(np.int32))
    got = dense.distance_transform(dv, lab, "sdf").cpu().numpy()
    assert np.array_equal(got.view(np.int32), R.sdf(lab_np, d2.astype(np.int32)).view(np.int32))
    # the same along z and y: the envelope passes carry the distances
    lab = torch.zeros((n, 2, 1), dtype=torch.uint8, device=DEV)
    lab[0, 0, 0] = 1
    want = (np.arange(n, dtype=np.int64)[:, None] ** 2 + np.arange(2)[None, :] ** 2)[:, :, None].astype(np.int32)
    assert np.array_equal(dense.distance_transform(dv, lab, "dist2").cpu().numpy(), want)
    print("ok corner")


def case_refusals():
    dv = hip.DeviceVoxelizer(0)
    big = 46342   # (big - 1)^2 > 2^31 - 2
    lab = torch.zeros((1, 1, big), dtype=torch.uint8, device=DEV)
    out = torch.zeros((1, 1, big), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    try:
        dv.distance_dense(lab.data_ptr(), (1, big, big), out.data_ptr(), hip.DIST_SQ_I32, (1, big, big), (big, 1, 1))
        raise AssertionError("the d2 limit was not enforced")
    except hip.DeviceError as e:
        assert "code 5" in str(e), str(e)
    ok = big - 1   # (ok - 1)^2 fits: accepted
    dv.distance_dense(lab.data_ptr(), (1, ok, ok), out.data_ptr(), hip.DIST_SQ_I32, (1, ok, ok), (ok, 1, 1))
    assert int(out[0, 0, 0]) == 0x7FFFFFFF
    R_ = 96
    lab = torch.zeros((R_, R_, R_), dtype=torch.uint8, device=DEV)
    lab[R_ // 2, R_ // 2, R_ // 2] = 1
    full = torch.full((R_, R_, R_), 7, dtype=torch.int32, device=DEV)
    short = torch.full((R_ // 2, R_, R_), 7, dtype=torch.int32, device=DEV)
    host = np.zeros((R_, R_, R_), np.int32)
    host_lab = lab.cpu().numpy()
    shared = torch.zeros(R_ ** 3 * 5, dtype=torch.uint8, device=DEV)   # labels and dst in one allocation
    torch.cuda.synchronize()
    st, dims = (1, R_, R_ * R_), (R_, R_, R_)
    st4 = st   # (the same element strides for the int32 dst)
    msgs = [
        expect_code3(lambda: dv.distance_dense(lab.data_ptr(), st, short.data_ptr(), hip.DIST_SQ_I32, st4, dims), "short dst"),
        expect_code3(lambda: dv.distance_dense(lab.data_ptr(), st, host.ctypes.data, hip.DIST_SQ_I32, st4, dims), "host dst"),
        expect_code3(lambda: dv.distance_dense(host_lab.ctypes.data, st, full.data_ptr(), hip.DIST_SDF_F32, st4, dims),
                     "host labels"),
        expect_code3(lambda: dv.distance_dense(shared.data_ptr(), st, shared.data_ptr() + R_ ** 3 - 4, hip.DIST_SQ_I32, st4, dims),
                     "overlap"),
        expect_code3(lambda: dv.distance_dense(lab.data_ptr(), st, full.data_ptr(), 2, st4, dims), "format"),
        expect_code3(lambda: dv.distance_dense(lab.data_ptr(), st, full.data_ptr(), hip.DIST_SQ_I32, st4, (R_, 0, R_)), "zero dims"),
    ]
    # dst strides under which voxels share an element: an expand()ed tensor, and y overlapping x
    line = torch.full((R_,), 7, dtype=torch.int32, device=DEV)
    wide = torch.full((R_ ** 3,), 7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    aliased = [
        expect_code3(lambda: dv.distance_dense(lab.data_ptr(), st, line.data_ptr(), hip.DIST_SQ_I32, (1, 0, 0), dims), "stride 0"),
        expect_code3(lambda: dv.distance_dense(lab.data_ptr(), st, wide.data_ptr(), hip.DIST_SQ_I32, (1, R_ // 2, R_ * R_), dims),
                     "aliasing strides"),
    ]
    assert all("one element" in m for m in aliased), aliased
    msgs += aliased
    try:
        dense.distance_transform(dv, lab, "dist2", out=line.view(1, 1, R_).expand(R_, R_, R_))
        raise AssertionError("an expanded out was accepted")
    except hip.DeviceError as e:
        assert "code 3" in str(e), str(e)
    assert bool((line == 7).all()) and bool((wide == 7).all())
    assert bool((full == 7).all()) and bool((short == 7).all()) and not bool(shared.any())
    # next to each other in one allocation: accepted
    dv.distance_dense(shared.data_ptr(), st, shared.data_ptr() + R_ ** 3, hip.DIST_SQ_I32, st4, dims)
    dv.distance_dense(lab.data_ptr(), st, full.data_ptr(), hip.DIST_SQ_I32, st4, dims)
    assert int(full.min()) == 0 and int(full.max()) == 3 * (R_ // 2) ** 2
    assert dv.distance_scratch_bytes(dims, hip.DIST_SQ_I32) > 0 and all(t >= 0 for t in dv.distance_times())
    print("\n".join(msgs))
    print("ok refusals")


def _mesh_case(dv, verts, res, **kw):
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(DEV),
                   torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(DEV))
    lab, origin = dense.voxelize_dense(dv, res, fmt="labels", fill=True, **kw)
    lab_np = lab.cpu().numpy()
    assert (lab_np == 2).any() and (lab_np == 1).any()
    want = R.separable_d2(lab_np)
    sdf, o2 = dense.voxelize_dense(dv, res, fmt="sdf", fill=True, **kw)
    assert o2 == origin and sdf.dtype == torch.float32 and tuple(sdf.shape) == lab_np.shape
    assert np.array_equal(sdf.cpu().numpy().view(np.int32), R.sdf(lab_np, want).view(np.int32)), kw
    d2, _ = dense.voxelize_dense(dv, res, fmt="dist2", fill=True, **kw)
    assert np.array_equal(d2.cpu().numpy(), want), kw
    return lab_np.shape


def case_mesh():
    dv = hip.DeviceVoxelizer(0)
    sphere = fill_ref.weld(meshes.uv_sphere(24))
    shapes = [_mesh_case(dv, sphere, 96), _mesh_case(dv, sphere, 96, box="tight"), _mesh_case(dv, sphere, 96, max_layers=24),
              _mesh_case(dv, torus(), 128), _mesh_case(dv, torus(), 128, box="tight", max_layers=16)]
    # an SDF without a sign is refused; out= of the box's shape
    try:
        dense.voxelize_dense(dv, 64, fmt="sdf")
        raise AssertionError("sdf without fill was accepted")
    except ValueError as e:
        assert "fill" in str(e)
    out = torch.zeros((2, 128, 128, 128), dtype=torch.float32, device=DEV)
    g, _ = dense.voxelize_dense(dv, 128, fmt="sdf", fill=True, out=out[1])
    ref, _ = dense.voxelize_dense(dv, 128, fmt="sdf", fill=True)
    assert g.data_ptr() == out[1].data_ptr() and torch.equal(out[1], ref) and not bool(out[0].any())
    print("shapes", shapes)


def case_bench_mesh():
    """The bench mesh at 1024 with the fill: the SDF on sampled voxels against an int64 brute force over every surface voxel."""
    dv = hip.DeviceVoxelizer(0)
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(DEV),
                   torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(DEV))
    res = 1024
    lab, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
    sdf = dense.distance_transform(dv, lab, "sdf")
    d2 = dense.distance_transform(dv, lab, "dist2")
    seeds = torch.nonzero(lab == 1).to(torch.int64)      # [k, 3] as z, y, x
    assert len(seeds) > 0 and bool((lab == 2).any())
    g = torch.Generator(device="cpu").manual_seed(3)
    pts = torch.randint(0, res, (4096, 3), generator=g).to(DEV)
    pts[:1024] = seeds[torch.randint(0, len(seeds), (1024,), generator=g).to(DEV)] + torch.randint(-3, 4, (1024, 3), generator=g).to(DEV)
    pts = pts.clamp(0, res - 1)
    best = torch.empty(len(pts), dtype=torch.int64, device=DEV)
    for i in range(0, len(pts), 16):
        diff = pts[i:i + 16, None, :] - seeds[None, :, :]
        best[i:i + 16] = (diff * diff).sum(-1).min(1).values
    z, y, x = pts.T
    got_d2 = d2[z, y, x].to(torch.int64)
    assert torch.equal(got_d2, best), int((got_d2 != best).sum())
    want = np.sqrt(best.cpu().numpy().astype(np.float64)).astype(np.float32)
    want = np.where(lab[z, y, x].cpu().numpy() == 2, -want, want)
    assert np.array_equal(sdf[z, y, x].cpu().numpy().view(np.int32), want.view(np.int32))
    print("sampled", len(pts), "surface voxels", len(seeds), "interior", int((lab == 2).sum()))


# ---- at the limits the call documents -----------------------------------------------------------------------------------

def _largest(d2):
    finite = d2[d2 != R.INF]
    return int(finite.max()) if finite.size else None


def case_lane_cap():
    """More lines than the 2^17 lanes in both envelope passes, every voxel compared: a lane's second and later lines, and the
    few lines of a count that is no multiple of the cap or of a workgroup."""
    dv = hip.DeviceVoxelizer(0)
    for shape in R.LANE_CAP_SHAPES:
        nz, ny, nx = shape
        ly, lz = R.pass_lines(shape)
        assert nx * nz > 2 ** 17 and nx * ny > 2 ** 17 and ny >= 5 and nz >= 5, shape
        for density, empty_plane in ((0.01, None), (3e-6, 2)):
            lab = R.lane_cap_labels(shape, density, seed=17, empty_plane=empty_plane)
            dark = nx * int((~(lab == 1).any(axis=(1, 2))).sum())      # lines along y of the planes without a seed
            assert (lab == 1).any() and (lab == 2).any() and (empty_plane is None or dark > 0), (shape, density)
            want = R.separable_d2(lab)
            check(dv, lab, want, f"lane cap, density {density}")
            print("lane_cap", shape, "lines y", ly, "z", lz, "cap", R.LANE_CAP, "last turn", ly % R.LANE_CAP, lz % R.LANE_CAP,
                  "density", density, "seeds", int((lab == 1).sum()), "y lines without a value", dark, "largest d2", _largest(want))
    assert all(n % R.LANE_CAP and n % 256 for n in R.pass_lines(R.LANE_CAP_SHAPES[1]))
    # labels stored [y][x][z], out stored [x][z][y], both looked at as [z, y, x]: x * d0 is a stride, the SDF reads l0, l1, l2
    nz, ny, nx = shape = R.LANE_CAP_SHAPES[0]
    lab = R.lane_cap_labels(shape, 0.002, seed=23)
    want = R.separable_d2(lab)
    lab_p = torch.from_numpy(lab).to(DEV).permute(1, 2, 0).contiguous().permute(2, 0, 1)
    for fmt, dtype, w in (("dist2", torch.int32, want), ("sdf", torch.float32, R.sdf(lab, want).view(np.int32))):
        out_p = torch.zeros((nx, nz, ny), dtype=dtype, device=DEV).permute(1, 2, 0)
        dense.distance_transform(dv, lab_p, fmt, out=out_p)
        got = out_p.cpu().numpy().view(np.int32)
        assert np.array_equal(got, w), (fmt, "permuted", int((got != w).sum()))
    print("lane_cap permuted", shape, "strides", tuple(lab_p.stride()), tuple(out_p.stride()))


def case_long_lines():
    """Lines of 46 341 voxels, the longest accepted, along z, y and x, with seeds at both ends and past position 2^15: s and t
    of a stack entry above 2^15, through the scratch and back."""
    dv = hip.DeviceVoxelizer(0)
    for shape in R.LONG_SHAPES:
        assert max(shape) == R.LONG and sum((n - 1) ** 2 for n in shape) <= R.D2_LIMIT, shape
        lab = R.long_line_labels(shape, seed=29)
        v = np.moveaxis(lab, int(np.argmax(shape)), 0)
        assert v[0, 0, 0] == 1 and v[-1, 0, 0] == 1 and (lab == 2).any()
        stats = []
        want = R.separable_d2(lab, stats)
        if shape[2] != R.LONG:   # a long envelope pass: its stacks, from the reference
            depth, pops, stacks = stats[1 if shape[0] == R.LONG else 0]
            # entries below the top two of the final stack (stored, and loaded again by the backward sweep) with s, t > 2^15
            stacks = [R.final_stack(*stacks, line) for line in range(len(depth))]
            high = [sum(1 for s, t in st[:-2] if s > 1 << 15 and t > 1 << 15) for st in stacks]
            past = int((v[(1 << 15) + 1:] == 1).any(axis=(1, 2)).sum())
            assert max(high) >= 6 and past >= 6, (shape, high, past)
            print("long_lines", shape, "stack depth", depth.tolist(), "entries from the scratch with s, t > 2^15", high,
                  "largest t", max(t for st in stacks for _, t in st))
        check(dv, lab, want, "long lines")
        print("long_lines", shape, "seeds", int((lab == 1).sum()), "largest d2", _largest(want))


def case_value_limit():
    """One seed in a corner of a box at the d2 limit: d2 = x^2 + y^2 + z^2 up to 2 147 483 216 of the 2 147 483 646 accepted,
    the SDF against the float64 sqrt rounded to float32; with the long axis along x and along z."""
    dv = hip.DeviceVoxelizer(0)
    a, b = np.arange(R.LONG, dtype=np.int64), np.arange(297, dtype=np.int64)
    for shape in ((1, 297, R.LONG), (R.LONG, 297, 1)):
        lab = np.zeros(shape, np.uint8)
        d2 = (b[None, :, None] ** 2 + a[None, None, :] ** 2) if shape[0] == 1 else (a[:, None, None] ** 2 + b[None, :, None] ** 2)
        lab[d2 > 1 << 30] = 2                                    # the far part inside: the sign at the largest values
        lab[(d2 % 7 == 3) & (d2 > 0)] = 2
        lab[0, 0, 0] = 1
        assert int(d2.max()) == 46340 ** 2 + 296 ** 2 == 2147483216 <= R.D2_LIMIT and (lab == 1).sum() == 1
        check(dv, lab, d2.astype(np.int32), "value limit")
        got = run(dv, lab, "sdf")
        far = got[-1, -1, -1]
        assert far == -np.float32(np.sqrt(np.float64(2147483216))), far
        print("value_limit", shape, "largest d2", int(d2.max()), "limit", R.D2_LIMIT, "sdf there", float(far))


def case_deep_stacks():
    """An envelope a thousand entries deep that empties at one position, in the y pass and in the z pass."""
    dv = hip.DeviceVoxelizer(0)
    for along_z, interior in ((False, None), (True, None), (False, 41), (True, 43)):
        lab = R.deep_stack_labels(along_z, interior)
        stats = []
        want = R.separable_d2(lab, stats)
        depth, pops, _ = stats[1 if along_z else 0]
        deep, long_runs, short_runs = int((depth >= 1000).sum()), int((pops >= 1000).sum()), int(((pops >= 1) & (pops <= 100)).sum())
        assert deep > 0 and long_runs > 0 and short_runs > 0, (deep, long_runs, short_runs)
        assert interior is None or (lab == 2).any()
        check(dv, lab, want, "deep stacks")
        print("deep_stacks", lab.shape, "interior", interior, "lines", len(depth), "depth >= 1000 on", deep, "largest", int(depth.max()),
              ">= 1000 pops at one position on", long_runs, "1 to 100 pops on", short_runs, "largest d2", _largest(want))


CASES = {"random": case_random, "strided": case_strided, "corner": case_corner, "refusals": case_refusals, "mesh": case_mesh,
         "bench_mesh": case_bench_mesh, "lane_cap": case_lane_cap, "long_lines": case_long_lines, "value_limit": case_value_limit,
         "deep_stacks": case_deep_stacks}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
