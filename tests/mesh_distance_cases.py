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


def check(dv, verts, res, band, signed, xf=None, what="", box=None, inside=True, want=None, **kw):
    """One call of the whole grid, or of the box (origin, dims) in x, y, z, against the reference; returns the device result.
    inside=False: for a band so narrow that no centre of the case lies in it.  want: the reference's (values, closest) if the
    caller has them."""
    ss = kw.get("supersampling", 1)
    if xf is None:
        xf = xform(dv, res, **kw)
    sv = fill_ref.sample_vertices(verts, xf)
    origin, dims = box if box else ((0, 0, 0), (res, res, res))
    out = torch.empty(tuple(dims[::-1]), device=DEV) if box else None
    got, idx, o = dense.mesh_distance(dv, res, band=band, signed=signed, closest=True, out=out, origin=origin, **kw)
    assert o == tuple(origin)
    vals, want_idx = want if want is not None else R.mesh_distance(sv, res, ss, band, signed, origin, dims)
    got, idx = got.cpu().numpy(), idx.cpu().numpy()
    bad = int((got.view(np.int32) != vals.view(np.int32)).sum())
    assert bad == 0, (what, res, band, signed, kw, bad, got[got.view(np.int32) != vals.view(np.int32)][:5],
                      vals[got.view(np.int32) != vals.view(np.int32)][:5])
    assert np.array_equal(idx, want_idx), (what, res, band, signed, kw, int((idx != want_idx).sum()))
    assert (np.abs(got) < np.float32(band)).any() or not inside, (what, "nothing inside the band")
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
        expect_code3(call(full.data_ptr(), band=1e-46), "band 0 as a float"),
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


# ---- at the limits the call documents -----------------------------------------------------------------------------------

UNIT = np.array([0, 0, 0, 1, 1, 1], np.float32)


def _through_centre(xf, voxel, ss):
    """A model-space triangle around the centre of `voxel` (x, y, z), in the plane of constant model z through it, for a
    transform that only scales and shifts: after the float32 rounding the centre lies within 1e-4 sample of it."""
    m, t = np.asarray(xf, np.float64)[:9].reshape(3, 3), np.asarray(xf, np.float64)[9:]
    assert np.count_nonzero(m - np.diag(np.diag(m))) == 0
    c = np.linalg.solve(m, (np.asarray(voxel, np.float64) + 0.5) * ss - t)
    return np.concatenate([c + [-0.03, -0.02, 0], c + [0.04, -0.01, 0], c + [-0.01, 0.05, 0]]).astype(np.float32)


def case_bands():
    """The widest band (32, with ss 1 and 2: every box dilated by up to 66 samples), bands that are no float32 (31.9, 2.6, 0.1)
    and one of a thousandth of a voxel, on a closed sphere (signed and unsigned) and a soup, whole grid with closest."""
    dv = hip.DeviceVoxelizer(0)
    res = 48
    sphere = fill_ref.weld(meshes.uv_sphere(7))
    soup = meshes.random_soup(150, seed=3)
    upload(dv, soup)
    xf_soup = xform(dv, res, bounds=UNIT)
    soup = np.concatenate([soup, _through_centre(xf_soup, (20, 31, 9), 1)[None]])
    bands = ((32.0, 1), (32.0, 2), (31.9, 1), (0.1, 1), (2.6, 2), (1e-3, 1))
    n = 0
    for band, ss in bands:
        assert 0 < band <= 32
        upload(dv, sphere)
        xf = xform(dv, res, supersampling=ss)
        sv = fill_ref.sample_vertices(sphere, xf)
        vals, idx = R.mesh_distance(sv, res, ss, band, True)     # (unsigned: the same without the sign, by R.finish)
        got, _ = check(dv, sphere, res, band, True, xf=xf, what="sphere", inside=band > 1e-3, want=(vals, idx), supersampling=ss)
        check(dv, sphere, res, band, False, xf=xf, what="sphere", inside=band > 1e-3, want=(np.abs(vals), idx), supersampling=ss)
        print("bands sphere", len(sphere), "triangles, band", band, "ss", ss, "in band", int((idx >= 0).sum()), "of", idx.size,
              "negative", int((got < 0).sum()))
        upload(dv, soup)
        xf = xform(dv, res, supersampling=ss, bounds=UNIT)
        got, idx = check(dv, soup, res, band, False, xf=xf, what="soup", supersampling=ss, bounds=UNIT)
        assert band < 32 or (idx >= 0).all()     # (at 32 voxels of a grid of 48 every centre is in some triangle's band)
        print("bands soup", len(soup), "triangles, band", band, "ss", ss, "in band", int((idx >= 0).sum()), "of", idx.size)
        n += 3
    print("compared", n)


def case_band_threshold():
    """The in-band test to one float32 step of the band: a voxel v* whose D lies between the float32 and the double square
    of a float32 f is inside band f (Bs2 is squared in double) and exactly at the float32 below f."""
    dv = hip.DeviceVoxelizer(0)
    res = 32
    sphere = fill_ref.weld(meshes.uv_sphere(10))
    upload(dv, sphere)
    xf = xform(dv, res)
    sv = fill_ref.sample_vertices(sphere, xf)
    D, best_id = R.best_d2(sv, res, 1, 8.0)
    found = None
    count = 0
    for z, y, x in np.argwhere((D >= 0.25 ** 2) & (D < 7.9 ** 2)):
        f, narrow = R.threshold_band(D[z, y, x])
        if narrow and 0.25 <= f <= 8:
            count += 1
            found = found or ((int(z), int(y), int(x)), f)
    assert found, "no voxel whose band threshold tells a float32 square from a double one"
    (z, y, x), f = found
    g = np.nextafter(f, np.float32(0))
    d = D[z, y, x]
    assert np.float64(f) * np.float64(f) > d >= np.float64(np.float32(f * f)) and np.float64(g) * np.float64(g) <= d
    got, idx = check(dv, sphere, res, float(f), True, xf=xf, what="band f")
    # (inside the band: its own distance and triangle.  The distance may round to f itself; closest tells the two apart)
    assert abs(got[z, y, x]) == np.float32(np.sqrt(d)) and idx[z, y, x] == best_id[z, y, x] >= 0, (got[z, y, x], idx[z, y, x])
    assert (idx == -1).any() and (np.abs(got[idx == -1]) == f).all()
    got_g, idx_g = check(dv, sphere, res, float(g), True, xf=xf, what="the float32 below f")
    assert abs(got_g[z, y, x]) == g and idx_g[z, y, x] == -1, (got_g[z, y, x], idx_g[z, y, x])
    print("band_threshold v* (z, y, x)", (z, y, x), "D", repr(float(d)), "f", repr(float(f)), "below", repr(float(g)), "float32 f*f",
          repr(float(np.float32(f * f))), "voxels with such an f", count, "of", D.size, "value at f", float(got[z, y, x]),
          "closest", int(idx[z, y, x]), "in band", int((idx >= 0).sum()), "and", int((idx_g >= 0).sum()))


def case_cropped():
    """bounds= strictly inside the mesh: triangles that stick out of the grid on both sides of every axis or lie wholly
    outside it, within and beyond the margin; and two triangles with sample coordinates near 1e18."""
    dv = hip.DeviceVoxelizer(0)
    res = 48
    sphere = fill_ref.weld(meshes.uv_sphere(16))
    inner = np.array([-0.62, -0.6, -0.64, 0.6, 0.63, 0.61], np.float32)   # (the corners reach past the sphere of radius 1)
    upload(dv, sphere)
    n = 0
    for ss in (1, 2):
        xf = xform(dv, res, supersampling=ss, bounds=inner)
        sv = fill_ref.sample_vertices(sphere, xf)
        lo, hi = sv.min(axis=1), sv.max(axis=1)
        S = res * ss
        sticks = [(int(((lo[:, a] < 0) & (hi[:, a] > 0)).sum()), int(((lo[:, a] < S) & (hi[:, a] > S)).sum())) for a in range(3)]
        outside = (hi < 0).any(axis=1) | (lo > S).any(axis=1)
        gap = np.maximum(np.maximum(-hi, lo - S), 0).max(axis=1)           # samples between the grid and the triangle's box
        assert all(a > 0 and b > 0 for a, b in sticks) and (outside & (gap < ss)).any() and (outside & (gap > 10 * ss)).any()
        for band in (1.0, 8.0):
            got, idx = check(dv, sphere, res, band, True, xf=xf, what="cropped sphere", supersampling=ss, bounds=inner)
            assert (got < 0).any() and (got > 0).any() and (idx == -1).any()
            n += 1
        # a box with an origin: the clamps against o and o + n - 1 are not those against the grid
        box = ((5, 9, 3), (30, 21, 40))
        check(dv, sphere, res, 8.0, True, xf=xf, what="cropped sphere, box", box=box, supersampling=ss, bounds=inner)
        n += 1
        print("cropped sphere ss", ss, "triangles across the low / high side per axis", sticks, "wholly outside", int(outside.sum()))
    soup = meshes.random_soup(600, seed=8)
    inner = np.array([0.2, 0.25, 0.3, 0.8, 0.75, 0.7], np.float32)
    far = np.float32(1e16)
    huge = np.array([[-far, -far, 0.52, far, -far, 0.52, 0, 2 * far, 0.52],                       # spans the grid in x and y
                     [far, far, far, far * 1.5, far, far, far, far * 1.5, far * 1.25]], np.float32)   # wholly outside
    both = np.concatenate([soup, huge])
    for ss in (1, 2):
        upload(dv, soup)
        xf = xform(dv, res, supersampling=ss, bounds=inner)      # (of the bounds alone; voxelize never sees the huge triangles)
        sv = fill_ref.sample_vertices(both, xf)
        assert np.isfinite(sv).all() and (np.abs(sv[-2:]).max(axis=(1, 2)) > 1e17).all(), sv[-2:]
        upload(dv, both)
        for band in (1.0, 8.0):
            got, idx = check(dv, both, res, band, False, xf=xf, what="cropped soup", supersampling=ss, bounds=inner)
            assert (idx == len(both) - 2).any() and not (idx == len(both) - 1).any()
            n += 1
        check(dv, both, res, 8.0, False, xf=xf, what="cropped soup, box", box=((7, 2, 11), (33, 40, 20)), supersampling=ss, bounds=inner)
        n += 1
        print("cropped soup ss", ss, "huge sample coordinates", float(np.abs(sv[-2:]).max()), "closest to the spanning triangle",
              int((idx == len(both) - 2).sum()))
    print("compared", n)


def _line_mesh(axis):
    """A sliver along `axis` of the unit cube and three small triangles beside it."""
    small = np.zeros((3, 3, 3))
    for k, t in enumerate((0.1, 0.5, 0.93)):
        c = np.full(3, 2e-5)
        c[axis] = t
        small[k] = c + 1e-5 * np.array([[0, 0, 0], [3, 1, 0.5], [0.5, 2, 3]])
    return np.concatenate([meshes.sliver(axis), small.reshape(-1, 9).astype(np.float32)])


def case_longest_box():
    """A box of 65 535 voxels, the most accepted, along x, then y, then z, at resolution 65 535 and, with origin 4 000, at
    70 000.  Every voxel of the box against R.mesh_distance, and R.point_distance at 8 192 sampled voxels of it (both ends
    and the 64 either side of each small triangle among them).  Beside it, 65 536 is refused."""
    dv = hip.DeviceVoxelizer(0)
    n_long, band = 65535, 2.0
    rng = np.random.default_rng(65535)
    for axis in range(3):
        verts = _line_mesh(axis)
        upload(dv, verts)
        for res, o_long in ((65535, 0), (70000, 4000)):
            # the transform, from a voxelize call of a thin range along the axis
            tile = {("xtile", "ytile", "zslab")[axis]: (0, 256)}
            dv.voxelize(res, read=False, bounds=UNIT, **tile)
            xf = dv.transform()
            origin, dims = [0, 0, 0], [2, 2, 2]
            origin[axis], dims[axis], dims[(axis + 2) % 3] = o_long, n_long, 1
            got, idx = check(dv, verts, res, band, False, xf=xf, what="longest box", box=(tuple(origin), tuple(dims)), bounds=UNIT)
            sv = fill_ref.sample_vertices(verts, xf)
            along = np.concatenate([[0, n_long - 1], rng.choice(n_long, 8192, replace=False)] +
                                   [np.arange(c - 64, c + 65) for c in np.floor(sv[2:, :, axis].mean(axis=1)).astype(np.int64) - o_long])
            along = np.unique(np.clip(along, 0, n_long - 1))
            assert len(along) >= 8192
            pts = np.zeros((len(along), 3), np.int64)
            pts[:, axis] = along
            pts[:, (axis + 1) % 3] = rng.integers(0, dims[(axis + 1) % 3], len(along))
            want, want_idx = R.point_distance(pts + np.array(origin), sv, 1, band)
            z, y, x = pts[:, 2], pts[:, 1], pts[:, 0]
            assert same(got[z, y, x], want) and np.array_equal(idx[z, y, x], want_idx)
            ends = [bool(idx.reshape(-1)[0] >= 0), bool(idx.reshape(-1)[-1] >= 0)]
            assert (idx >= 2).any() and (idx == -1).any() and (idx[(idx >= 0)] < 2).any()
            print("longest_box axis", axis, "res", res, "origin", tuple(origin), "dims", tuple(dims), "in band", int((idx >= 0).sum()), "of",
                  idx.size, "closest to a small triangle", int((idx >= 2).sum()), "ends in band", ends, "sampled", len(along))
    line = torch.full((65536,), 7.0, device=DEV)
    torch.cuda.synchronize()
    try:
        dv.mesh_distance_dense(70000, band, hip.MESH_DIST_UNSIGNED_F32, (0, 0, 0), (65536, 1, 1), line.data_ptr(), (1, 65536, 65536), bounds=UNIT)
        raise AssertionError("a box of 65 536 voxels was accepted")
    except hip.DeviceError as e:
        assert "code 5" in str(e), str(e)
    assert bool((line == 7).all())
    print("ok longest_box")


CASES = {"shapes": case_shapes, "boxes": case_boxes, "fill_agree": case_fill_agree, "transform": case_transform,
         "crowded": case_crowded, "empty": case_empty, "refusals": case_refusals, "bench_mesh": case_bench_mesh,
         "bands": case_bands, "band_threshold": case_band_threshold, "cropped": case_cropped, "longest_box": case_longest_box}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
