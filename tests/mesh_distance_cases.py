"""The GPU cases of tests/test_gpu_mesh_distance.py, each run in a child process of its own:
`python -m tests.mesh_distance_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison is bit for bit: the distances as
the int32 bits of their float32, closest exactly.  The reference (tests/mesh_distance_ref.py) takes its sample-space vertices
from the transform o2v_hip_voxelize reports for the same params.  A case prints "ok" last when everything held."""
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import fill_ref
from tests import mesh_distance_ref as R
from tests.dense_cases import expect_code3, torus

DEV = torch.device("cuda", 0)
PERMUTE_FLIP = np.array([[0, 0, -1], [1, 0, 0], [0, -1, 0]], np.int32)


def upload(dv, verts):
    v = torch.from_numpy(np.ascontiguousarray(verts, np.float32).reshape(-1, 9)).to(DEV)
    dense.set_mesh(dv, v)


def xform(dv, res, **kw):
    """The transform o2v_hip_voxelize computes for these params (needs a mesh with finite vertices in the context)."""
    dv.voxelize(res, read=False, **kw)
    return dv.transform()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        a, b = a.view(np.int32), b.view(np.int32)
    return a.shape == b.shape and np.array_equal(a, b)


def check(dv, verts, res, band, signed, xf=None, what="", **kw):
    """One call of the whole grid against the reference; returns the device result."""
    ss = kw.get("supersampling", 1)
    if xf is None:
        xf = xform(dv, res, **kw)
    sv = fill_ref.sample_vertices(verts, xf)
    got, idx, _ = dense.mesh_distance(dv, res, band=band, signed=signed, closest=True, **kw)
    vals, want_idx = R.mesh_distance(sv, res, ss, band, signed)
    got, idx = got.cpu().numpy(), idx.cpu().numpy()
    bad = int((got.view(np.int32) != vals.view(np.int32)).sum())
    assert bad == 0, (what, res, band, signed, kw, bad, got[got.view(np.int32) != vals.view(np.int32)][:5],
                      vals[got.view(np.int32) != vals.view(np.int32)][:5])
    assert np.array_equal(idx, want_idx), (what, res, band, signed, kw, int((idx != want_idx).sum()))
    assert (got < band).any(), (what, "nothing inside the band")
    return got, idx


def degenerate_mix():
    v = meshes.uv_sphere(8).reshape(-1, 3, 3).copy()
    v[5, 1] = v[5, 0]                       # two equal vertices
    v[9, 1] = v[9, 2] = v[9, 0]             # all equal
    v[13, 2] = v[13, 0] + 2 * (v[13, 1] - v[13, 0])   # collinear
    v[17, 0, 1] = np.nan                    # non-finite: ignored
    v[21, 2, 0] = np.inf
    return v.reshape(-1, 9)


def case_shapes():
    dv = hip.DeviceVoxelizer(0)
    n = 0
    sphere = fill_ref.weld(meshes.uv_sphere(24))
    upload(dv, sphere)
    for band in (0.5, 1.0, 2.5, 8.0):
        check(dv, sphere, 96, band, True, what="sphere")
        n += 1
    check(dv, sphere, 96, 2.5, True, what="sphere ss2", supersampling=2)
    check(dv, sphere, 96, 1.0, False, what="sphere permuted", unit_transform=PERMUTE_FLIP, supersampling=2)
    check(dv, sphere, 80, 2.5, True, what="sphere bounds", bounds=np.array([-1.5, -1.2, -1, 1.1, 1.3, 1.6], np.float32))
    t = torus()
    upload(dv, t)
    check(dv, t, 128, 2.5, True, what="torus")
    check(dv, t, 128, 8.0, True, what="torus permuted", unit_transform=PERMUTE_FLIP)
    cube = meshes.unit_cube()
    upload(dv, cube)
    for band, ss in ((0.5, 1), (2.5, 2), (8.0, 1)):
        check(dv, cube, 64, band, True, what="cube", supersampling=ss)
    tri = meshes.single_triangle()
    upload(dv, tri)
    check(dv, tri, 32, 2.5, True, what="triangle")
    check(dv, tri, 32, 1.0, False, what="triangle", supersampling=2)
    planes = meshes.three_planes()
    upload(dv, planes)
    for signed in (True, False):
        check(dv, planes, 48, 2.5, signed, what="three planes")
        check(dv, planes, 48, 1.0, signed, what="three planes ss2", supersampling=2, unit_transform=PERMUTE_FLIP)
    soup = meshes.random_soup(2000, seed=3)
    upload(dv, soup)
    check(dv, soup, 64, 2.5, False, what="soup")
    check(dv, soup, 64, 0.5, False, what="soup ss2", supersampling=2)
    # degenerate and non-finite triangles: the transform of explicit bounds (taken from the finite sphere it was made from)
    mix = degenerate_mix()
    bounds = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    upload(dv, meshes.uv_sphere(8))
    xf = xform(dv, 48, bounds=bounds)
    upload(dv, mix)
    for signed in (True, False):
        check(dv, mix, 48, 2.5, signed, xf=xf, what="degenerate mix", bounds=bounds)
    print("compared", n + 22)


def case_boxes():
    dv = hip.DeviceVoxelizer(0)
    t = torus()
    upload(dv, t)
    res, band = 128, 2.5
    full, fidx, _ = dense.mesh_distance(dv, res, band=band, closest=True)
    full_np, fidx_np = full.cpu().numpy(), fidx.cpu().numpy()
    # a box with a non-zero origin
    out = torch.full((37, 29, 45), 7.0, device=DEV)
    got, idx, origin = dense.mesh_distance(dv, res, band=band, out=out, closest=True, origin=(11, 50, 3))
    assert origin == (11, 50, 3) and same(got.cpu(), full_np[3:40, 50:79, 11:56]) and same(idx.cpu(), fidx_np[3:40, 50:79, 11:56])
    # a box away from the mesh: the band everywhere
    far, fi, _ = dense.mesh_distance(dv, res, band=band, closest=True, out=torch.empty((4, 5, 6), device=DEV), origin=(0, 0, 0))
    assert bool((far == band).all()) and bool((fi == -1).all()), "far box"
    # out as a slice of a batch with permuted strides, closest with strides of its own
    batch = torch.full((3, res, res, res), 5.0, device=DEV)
    o = batch[1].permute(2, 0, 1)          # [z, y, x] view whose x stride is res * res
    cbuf = torch.full((res, res, res), 9, dtype=torch.int32, device=DEV)
    c = cbuf.permute(1, 2, 0)
    g, ci, _ = dense.mesh_distance(dv, res, band=band, out=o, closest=c)
    assert same(g.cpu(), full_np) and same(ci.cpu(), fidx_np)
    assert bool((batch[0] == 5).all()) and bool((batch[2] == 5).all())
    # z ranges: the bits of one call
    for layers in (1, 7, 40):
        out = torch.empty((res, res, res), device=DEV)
        ci = torch.empty((res, res, res), dtype=torch.int32, device=DEV)
        dense.mesh_distance(dv, res, band=band, out=out, closest=ci, max_layers=layers)
        assert same(out.cpu(), full_np) and same(ci.cpu(), fidx_np), layers
    for signed in (True, False):
        a, _ = dense.mesh_distance(dv, res, band=8.0, signed=signed, supersampling=2)
        b, _ = dense.mesh_distance(dv, res, band=8.0, signed=signed, supersampling=2, max_layers=13)
        assert same(a.cpu(), b.cpu().numpy())
    print("ok boxes")


def case_fill_agree():
    dv = hip.DeviceVoxelizer(0)
    for verts, res in ((fill_ref.weld(meshes.uv_sphere(24)), 96), (torus(), 128), (meshes.unit_cube(), 64)):
        upload(dv, verts)
        for ss in (1, 2):
            lab, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True, supersampling=ss)
            sv = fill_ref.sample_vertices(verts, dv.transform())
            d, _ = dense.mesh_distance(dv, res, band=3.0, supersampling=ss)
            lab, neg = lab.cpu().numpy(), np.signbit(d.cpu().numpy())
            assert (lab == 2).any() and neg[lab == 2].all() and not neg[lab == 0].any(), res
            keys = fill_ref.parity_keys(sv, res, ss)
            z, y, x = np.nonzero(neg)
            assert np.array_equal(np.sort((x.astype(np.int64) * res + y) * res + z), keys), res
    print("ok fill_agree")


def case_transform():
    dv = hip.DeviceVoxelizer(0)
    verts = meshes.uv_sphere(16, center=(0.3, -2.0, 5.0), radius=3.0)
    upload(dv, verts)
    for kw in (dict(), dict(bounds=np.array([-4, -6, 1, 4, 2, 9], np.float32)), dict(unit_transform=PERMUTE_FLIP, supersampling=2)):
        xf = xform(dv, 72, **kw)
        check(dv, verts, 72, 2.5, True, xf=xf, what="transform", **kw)
        # the same call after another voxelize call of other params: the transform is the call's own
        dv.voxelize(50, read=False)
        check(dv, verts, 72, 2.5, True, xf=xf, what="transform again", **kw)
    print("ok transform")


def case_crowded():
    """A fan of 20 000 thin triangles around one point inside one tile, and a few far triangles."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(1)
    n = 20000
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    c = np.array([0.52, 0.47, 0.5])
    tip = c + 0.06 * np.stack([np.cos(ang), np.sin(ang), rng.uniform(-0.3, 0.3, n)], 1)
    side = tip + 0.002 * rng.normal(size=(n, 3))
    fan = np.stack([np.broadcast_to(c, (n, 3)), tip, side], 1)
    far = rng.uniform(0, 1, (8, 3, 3)) * 0.1 + np.array([0.85, 0.05, 0.9])
    corners = np.array([[[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]], [[1, 1, 1], [1, 1 - 1e-3, 1], [1 - 1e-3, 1, 1]]])
    verts = np.concatenate([fan, far, corners]).astype(np.float32).reshape(-1, 9)
    upload(dv, verts)
    res = 64
    xf = xform(dv, res)
    t0 = time.perf_counter()
    got, idx, _ = dense.mesh_distance(dv, res, band=2.5, signed=False, closest=True)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    sv = fill_ref.sample_vertices(verts, xf)
    vals, want_idx = R.mesh_distance(sv, res, 1, 2.5, False)
    assert same(got.cpu(), vals) and np.array_equal(idx.cpu().numpy(), want_idx)
    print("crowded call ms", round(ms, 2), "stage ms", dv.mesh_distance_times())


def case_empty():
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.zeros((0, 9), dtype=torch.float32, device=DEV))
    for signed in (True, False):
        d, idx, _ = dense.mesh_distance(dv, 40, band=1.5, signed=signed, closest=True, supersampling=2)
        assert same(d.cpu(), np.full((40, 40, 40), 1.5, np.float32)) and bool((idx == -1).all())
    print("ok empty")


def case_refusals():
    dv = hip.DeviceVoxelizer(0)
    upload(dv, meshes.unit_cube())
    R_ = 40
    dims, st = (R_, R_, R_), (1, R_, R_ * R_)
    full = torch.full((R_, R_, R_), 7.0, device=DEV)
    cl = torch.full((R_, R_, R_), 7, dtype=torch.int32, device=DEV)
    short = torch.full((R_ // 2, R_, R_), 7.0, device=DEV)
    host = np.zeros((R_, R_, R_), np.float32)
    shared = torch.zeros(R_ ** 3 * 2, dtype=torch.float32, device=DEV)
    wide = torch.full((R_ ** 3,), 7.0, device=DEV)
    torch.cuda.synchronize()
    S = hip.MESH_DIST_SIGNED_F32

    def call(dst, band=2.0, fmt=S, origin=(0, 0, 0), d=dims, strides=st, closest=None, cst=None, res=R_, **kw):
        return lambda: dv.mesh_distance_dense(res, band, fmt, origin, d, dst, strides, closest, cst, **kw)
    msgs = [
        expect_code3(call(short.data_ptr()), "short dst"),
        expect_code3(call(host.ctypes.data), "host dst"),
        expect_code3(call(full.data_ptr(), closest=host.ctypes.data, cst=st), "host closest"),
        expect_code3(call(shared.data_ptr(), closest=shared.data_ptr() + R_ ** 3 * 4 - 4, cst=st), "dst and closest overlap"),
        expect_code3(call(full.data_ptr(), band=0.0), "band 0"),
        expect_code3(call(full.data_ptr(), band=float("nan")), "band nan"),
        expect_code3(call(full.data_ptr(), band=32.5), "band above 32"),
        expect_code3(call(full.data_ptr(), band=float("inf")), "band inf"),
        expect_code3(call(full.data_ptr(), fmt=2), "format"),
        expect_code3(call(full.data_ptr(), d=(R_, 0, R_)), "zero dims"),
        expect_code3(call(full.data_ptr(), origin=(1, 0, 0)), "box past the grid"),
        expect_code3(call(full.data_ptr(), supersampling=3), "supersampling"),
        expect_code3(call(wide.data_ptr(), strides=(1, R_ // 2, R_ * R_)), "aliasing strides"),
        expect_code3(call(full.data_ptr(), closest=cl.data_ptr(), cst=(1, 0, R_ * R_)), "aliasing closest strides"),
    ]
    # the slab and tile fields of params must be 0
    p = dv._params(R_, 1, 0, None, None, (0, 8))
    rc = dv._L.o2v_hip_mesh_distance_dense(dv._ctx, hip.C.byref(p), 2.0, S, (hip.C.c_uint32 * 3)(0, 0, 0), (hip.C.c_uint32 * 3)(*dims),
                                           full.data_ptr(), (hip.C.c_uint64 * 3)(*st), None, None)
    assert rc == 3, rc
    # a box of more than 65 535 voxels along x: O2V_HIP_ERR_LIMIT
    line = torch.full((65536,), 7.0, device=DEV)
    torch.cuda.synchronize()
    try:
        dv.mesh_distance_dense(70000, 2.0, S, (0, 0, 0), (65536, 1, 1), line.data_ptr(), (1, 65536, 65536))
        raise AssertionError("a box of 65 536 voxels was accepted")
    except hip.DeviceError as e:
        assert "code 5" in str(e), str(e)
    assert bool((full == 7).all()) and bool((cl == 7).all()) and bool((short == 7).all()) and bool((line == 7).all())
    assert bool((wide == 7).all()) and not bool(shared.any())
    # the context is still usable; next to each other in one allocation is accepted
    dv.mesh_distance_dense(R_, 2.0, S, (0, 0, 0), dims, shared.data_ptr(), st, shared.data_ptr() + R_ ** 3 * 4, st)
    dv.mesh_distance_dense(R_, 2.0, S, (0, 0, 0), dims, full.data_ptr(), st, cl.data_ptr(), st)
    torch.cuda.synchronize()
    assert bool((full < 0).any()) and bool((full.abs() == 2.0).any()) and bool((cl >= 0).any())   # (the cube fills the grid)
    assert torch.equal(shared[:R_ ** 3].view(R_, R_, R_), full)
    assert all(t >= 0 for t in dv.mesh_distance_times())
    print("\n".join(msgs))
    print("ok refusals")


def case_bench_mesh():
    """scan_like at 1024 with band 3: 2 048 sampled voxels against the reference over their AABB-candidate triangles, and
    |signed| equal to unsigned bitwise on the whole grid."""
    dv = hip.DeviceVoxelizer(0)
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(DEV),
                   torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(DEV))
    welded = positions.view(np.float32)[faces.reshape(-1, 3)].reshape(-1, 9)
    res, band = 1024, 3.0
    xf = xform(dv, res)
    uns, idx, _ = dense.mesh_distance(dv, res, band=band, signed=False, closest=True)
    sgn, _ = dense.mesh_distance(dv, res, band=band, signed=True)
    assert torch.equal(sgn.abs().view(torch.int32), uns.view(torch.int32)), "|signed| != unsigned"
    assert bool((sgn < 0).any())
    g = torch.Generator(device="cpu").manual_seed(5)
    near = torch.nonzero(uns < band)
    assert len(near) > 0
    pts = torch.randint(0, res, (2048, 3), generator=g).to(DEV)
    pts[:1024] = near[torch.randint(0, len(near), (1024,), generator=g).to(DEV)]
    z, y, x = pts.T
    got, got_idx = uns[z, y, x].cpu().numpy(), idx[z, y, x].cpu().numpy()
    sv = fill_ref.sample_vertices(welded, xf)
    want, want_idx = R.point_distance(np.stack([x.cpu().numpy(), y.cpu().numpy(), z.cpu().numpy()], 1), sv, 1, band)
    assert same(got, want), int((got.view(np.int32) != want.view(np.int32)).sum())
    assert np.array_equal(got_idx, want_idx), int((got_idx != want_idx).sum())
    print("sampled", len(pts), "in band", int((got < band).sum()), "times", dv.mesh_distance_times())


CASES = {"shapes": case_shapes, "boxes": case_boxes, "fill_agree": case_fill_agree, "transform": case_transform,
         "crowded": case_crowded, "empty": case_empty, "refusals": case_refusals, "bench_mesh": case_bench_mesh}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
