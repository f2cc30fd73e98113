"""The GPU cases of tests/test_gpu_dense.py, each run in a child process of its own: `python -m tests.dense_cases <case>`.

torch is imported before the library is loaded (the library must use the HIP runtime torch loaded), which a pytest process
that has already voxelized in another test module cannot promise.  A case prints "ok" last when everything held."""
import sys

if __name__ == "__main__" and sys.argv[1:] == ["lib_first"]:
    # the library loaded before torch: obj2voxel_amd.dense must refuse (before it touches the GPU)
    from obj2voxel_amd import _lib
    _lib.lib()
    import torch
    from obj2voxel_amd import dense

    class _Stub:
        device = 0
    for call in (lambda: dense.set_mesh(_Stub(), None), lambda: dense.voxelize_dense(_Stub(), 64)):
        try:
            call()
            raise AssertionError("dense worked with the library loaded before torch")
        except RuntimeError as e:
            assert "before torch" in str(e), str(e)
    print("ok")
    sys.exit(0)

import torch  # first

import numpy as np

from obj2voxel_amd import hip, meshes
from tests import fill_ref


def index_mesh(verts, index_dtype=np.int32):
    """(positions [V, 3], faces [T, 3]) of a flat [T, 9] mesh: bit-identical vertices shared, so gathering gives verts back."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    _, first, inverse = np.unique(v.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    positions = v[first]
    faces = inverse.reshape(-1, 3).astype(index_dtype)
    assert np.array_equal(positions[faces].reshape(-1, 9).view(np.uint32), np.asarray(verts, np.float32).reshape(-1, 9).view(np.uint32))
    return positions, faces


def torus():
    from tests.test_gpu_fill import _torus
    return _torus()


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_upload(dv, verts, mat, indexed=True, index_dtype=np.int32):
    """dv.set_triangles_device from torch tensors; the tensors are returned (they must outlive nothing but the call)."""
    T = len(verts)
    keep = {k: cuda(mat[k]) for k in ("uvs", "types", "colors", "texids") if k in mat}
    if indexed:
        positions, faces = index_mesh(verts, index_dtype)
        p, f = cuda(positions), cuda(faces)
        torch.cuda.synchronize()
        dv.set_triangles_device(p.data_ptr(), len(positions), f.data_ptr(), f.element_size(), T,
                                *[keep[k].data_ptr() if k in keep else None for k in ("uvs", "types", "colors", "texids")])
    else:
        p = cuda(np.asarray(verts, np.float32).reshape(-1, 9))
        torch.cuda.synchronize()
        dv.set_triangles_device(p.data_ptr(), 0, None, 0, T,
                                *[keep[k].data_ptr() if k in keep else None for k in ("uvs", "types", "colors", "texids")])


def materials(kind, T, uvs=None):
    if kind == "none":
        return {}
    if kind == "coloured":
        return dict(types=np.full(T, hip.TRI_UNTEXTURED, np.uint32), colors=meshes.triangle_colors(T))
    # textured: only the last triangle is TEXTURED - the device must find it to take the uv path
    types = np.full(T, hip.TRI_UNTEXTURED, np.uint32)
    types[-1] = hip.TRI_TEXTURED
    types[::3] = hip.TRI_TEXTURED
    return dict(types=types, colors=meshes.triangle_colors(T), uvs=uvs, texids=np.zeros(T, np.int32))


def case_upload():
    dv = hip.DeviceVoxelizer(0)
    sphere, sphere_uv = meshes.uv_sphere(24, with_uv=True)
    sphere = fill_ref.weld(sphere)
    runs = [("sphere", sphere, "none", 96), ("sphere", sphere, "coloured", 96), ("sphere", sphere, "textured", 96),
            ("torus", torus(), "coloured", 128), ("scan", meshes.scan_like(50_000), "none", 192)]
    dv.set_textures([(meshes.checker_texture(64, 8), 1)])
    n_cmp = 0
    for name, verts, kind, res in runs:
        mat = materials(kind, len(verts), sphere_uv if kind == "textured" else None)
        for ss in (1, 2):
            for strategy in (hip.STRATEGY_MAX, hip.STRATEGY_BLEND):
                dv.set_triangles(verts, **mat)
                want = meshes.sorted_voxels(dv.voxelize(res, supersampling=ss, strategy=strategy))
                assert len(want) > 0
                for indexed, idt in ((True, np.int32), (True, np.int64), (False, None)):
                    device_upload(dv, verts, mat, indexed, idt)
                    assert dv.n_tris == len(verts)
                    got = meshes.sorted_voxels(dv.voxelize(res, supersampling=ss, strategy=strategy))
                    assert got.shape == want.shape and np.array_equal(got, want), (name, kind, ss, strategy, indexed, idt)
                    n_cmp += 1
    print("compared", n_cmp)


def case_bad_index():
    dv = hip.DeviceVoxelizer(0)
    verts = fill_ref.weld(meshes.uv_sphere(16))
    dv.set_triangles(verts)
    want = meshes.sorted_voxels(dv.voxelize(64))
    positions, faces = index_mesh(verts)
    for idt in (np.int32, np.int64):
        for bad in (len(positions), -1):
            f = faces.astype(idt)
            f[len(f) // 2, 1] = bad
            p, fd = cuda(positions), cuda(f)
            torch.cuda.synchronize()
            try:
                dv.set_triangles_device(p.data_ptr(), len(positions), fd.data_ptr(), fd.element_size(), len(f))
            except hip.DeviceError as e:
                assert "face index" in str(e) and "code 3" in str(e), str(e)
            else:
                raise AssertionError("an out-of-range face index was accepted")
            assert dv.n_tris == 0
            assert dv.voxelize(64, read=False) == 0
            device_upload(dv, verts, {}, True, idt)
            got = meshes.sorted_voxels(dv.voxelize(64))
            assert np.array_equal(got, want)
    # an int64 index of 2^32 + i is refused, not wrapped onto i
    f = faces.astype(np.int64)
    f[0, 0] += 1 << 32
    p, fd = cuda(positions), cuda(f)
    torch.cuda.synchronize()
    try:
        dv.set_triangles_device(p.data_ptr(), len(positions), fd.data_ptr(), 8, len(f))
        raise AssertionError("an index above 2^32 was accepted")
    except hip.DeviceError as e:
        assert "face index" in str(e)
    print("ok refusals")


def expect_code3(fn, what):
    try:
        fn()
    except hip.DeviceError as e:
        assert "code 3" in str(e), (what, str(e))
        return str(e)
    raise AssertionError(what + " was accepted")


def case_pointers():
    """Every refusal happens before a launch.  The short allocations are at most half of what the call would read, and at
    least 1 MiB below it, so that an allocation granularity of the runtime cannot hide them."""
    dv = hip.DeviceVoxelizer(0)
    verts = fill_ref.weld(meshes.uv_sphere(12))
    positions, faces = index_mesh(verts)
    dv.set_triangles(verts)
    want = meshes.sorted_voxels(dv.voxelize(48))
    T, V = len(faces), len(positions)
    hp, hf = np.ascontiguousarray(positions), np.ascontiguousarray(faces)
    p, f = cuda(positions), cuda(faces)
    # (this child runs with torch's caching allocator off: each tensor is an allocation of its own)
    MiB, big = 1 << 20, 1 << 20   # big: a claimed count whose arrays are 4 - 36 MiB
    one_mib_f32 = torch.empty(MiB // 4, dtype=torch.float32, device="cuda")
    one_mib_i32 = torch.empty(MiB // 4, dtype=torch.int32, device="cuda")
    flat = torch.zeros((big, 9), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    msgs = [
        expect_code3(lambda: dv.set_triangles_device(hp.ctypes.data, V, f.data_ptr(), 4, T), "host positions"),
        expect_code3(lambda: dv.set_triangles_device(p.data_ptr(), V, hf.ctypes.data, 4, T), "host faces"),
        expect_code3(lambda: dv.set_triangles_device(one_mib_f32.data_ptr(), big, f.data_ptr(), 4, T), "short positions"),
        expect_code3(lambda: dv.set_triangles_device(p.data_ptr(), V, one_mib_i32.data_ptr(), 4, big), "short faces"),
        expect_code3(lambda: dv.set_triangles_device(one_mib_f32.data_ptr(), 0, None, 0, big), "short flat positions"),
        expect_code3(lambda: dv.set_triangles_device(flat.data_ptr(), 0, None, 0, big, types_ptr=one_mib_i32.data_ptr()), "short types"),
        expect_code3(lambda: dv.set_triangles_device(flat.data_ptr(), 0, None, 0, big, colors_ptr=one_mib_f32.data_ptr()), "short colors"),
        expect_code3(lambda: dv.set_triangles_device(p.data_ptr(), 0, f.data_ptr(), 4, T), "no positions"),
        expect_code3(lambda: dv.set_triangles_device(p.data_ptr(), V, f.data_ptr(), 2, T), "index bytes"),
    ]
    # refused before anything was launched: the triangles of before are still there
    assert dv.n_tris == T
    assert np.array_equal(meshes.sorted_voxels(dv.voxelize(48)), want)
    n = dv.count
    R = 160   # dst grids of 160^3: U8 4 MB
    grid = torch.zeros((R, R, R), dtype=torch.uint8, device="cuda")
    host = np.zeros((R, R, R), np.uint8)
    half = torch.zeros((R // 2, R, R), dtype=torch.uint8, device="cuda")
    bits = torch.zeros((R, R, R // 32), dtype=torch.int32, device="cuda")   # 512 kB
    torch.cuda.synchronize()
    full = ((0, 0, 0), (R, R, R), (1, R, R * R))
    msgs += [
        expect_code3(lambda: dv.write_dense(host.ctypes.data, hip.DENSE_U8, *full), "host dst"),
        expect_code3(lambda: dv.write_dense(half.data_ptr(), hip.DENSE_U8, *full), "short dst"),
        expect_code3(lambda: dv.write_dense(grid.data_ptr(), hip.DENSE_ARGB32, *full), "short dst (argb)"),
        expect_code3(lambda: dv.write_dense(grid.data_ptr(), hip.DENSE_U8, (0, 0, 0), (R, 0, R), (1, R, R * R)), "zero dims"),
        expect_code3(lambda: dv.write_dense(bits.data_ptr(), hip.DENSE_BITS, (0, 0, 0), (R, R, R), (2, 5, 5 * R)), "bits stride"),
        expect_code3(lambda: dv.write_dense(bits.data_ptr(), hip.DENSE_BITS, (0, 0, 0), (R, R, 8 * R), (1, 5, 5 * R)), "short bits"),
        expect_code3(lambda: dv.write_dense(grid.data_ptr(), 7, *full), "format"),
    ]
    assert not grid.any() and not half.any() and not bits.any()
    assert dv.write_dense(grid.data_ptr(), hip.DENSE_U8, *full) == 0
    assert int(grid.sum()) == n
    print("\n".join(msgs))
    print("ok pointers")


def scatter_ref(vox, n_surf, fmt, origin, dims, layout="zyx"):
    """numpy: the dense grid [z, y, x] (bits: [z, y, words]) of records `vox` in the box, and the number outside it."""
    o, d = np.array(origin, np.int64), np.array(dims, np.int64)
    rel = vox[:, :3].astype(np.int64) - o
    inside = np.all((rel >= 0) & (rel < d), axis=1)
    x, y, z = rel[inside].T
    if fmt == hip.DENSE_BITS:
        g = np.zeros((d[2], d[1], (d[0] + 31) // 32), np.uint32)
        np.bitwise_or.at(g, (z, y, x // 32), (np.uint32(1) << (x % 32).astype(np.uint32)))
        return g.view(np.int32), int((~inside).sum())
    if fmt == hip.DENSE_U8:
        g = np.zeros((d[2], d[1], d[0]), np.uint8)
        g[z, y, x] = np.where(np.arange(len(vox)) < n_surf, 1, 2)[inside]
        return g, int((~inside).sum())
    g = np.zeros((d[2], d[1], d[0]), np.uint32)
    g[z, y, x] = vox[inside, 3]
    return g.view(np.int32), int((~inside).sum())


def dense_dtype(fmt):
    return torch.uint8 if fmt == hip.DENSE_U8 else torch.int32


def write_and_compare(dv, vox, n_surf, fmt, origin, dims, permuted=False):
    dx, dy, dz = dims
    wx = (dx + 31) // 32 if fmt == hip.DENSE_BITS else dx
    if permuted:   # storage [y][x][z] (bits: [y][z][words]), looked at as [z, y, x]
        if fmt == hip.DENSE_BITS:
            t = torch.zeros((dy, dz, wx), dtype=dense_dtype(fmt), device="cuda").permute(1, 0, 2)
        else:
            t = torch.zeros((dy, wx, dz), dtype=dense_dtype(fmt), device="cuda").permute(2, 0, 1)
    else:
        t = torch.zeros((dz, dy, wx), dtype=dense_dtype(fmt), device="cuda")
    torch.cuda.synchronize()
    outside = dv.write_dense(t.data_ptr(), fmt, origin, dims, (t.stride(2), t.stride(1), t.stride(0)))
    want, want_out = scatter_ref(vox, n_surf, fmt, origin, dims)
    got = t.cpu().numpy()
    assert outside == want_out, (fmt, origin, dims, outside, want_out)
    assert np.array_equal(got, want), (fmt, origin, dims, permuted, int((got != want).sum()))


def case_write_dense():
    dv = hip.DeviceVoxelizer(0)
    verts = meshes.scan_like(50_000)
    T = len(verts)
    dv.set_triangles(verts, types=np.full(T, hip.TRI_UNTEXTURED, np.uint32), colors=meshes.triangle_colors(T))
    res = 160
    vox = dv.voxelize(res)
    n = len(vox)
    lo, hi = vox[:, :3].min(0), vox[:, :3].max(0) + 1
    boxes = [((0, 0, 0), (res, res, res)), ((int(lo[0]), int(lo[1]), int(lo[2])), tuple(int(v) for v in hi - lo)),
             ((20, 30, 40), (70, 50, 60)), ((3, 0, 5), (res - 3, res, res - 5))]
    for fmt in (hip.DENSE_U8, hip.DENSE_ARGB32, hip.DENSE_BITS):
        for origin, dims in boxes:
            write_and_compare(dv, vox, n, fmt, origin, dims)
        write_and_compare(dv, vox, n, fmt, (0, 0, 0), (res, res, res), permuted=True)
        write_and_compare(dv, vox, n, fmt, (10, 7, 0), (100, 120, res), permuted=True)
    # solid fill of a closed torus: labels 1 and 2 count the surface and the interior
    dv.set_triangles(torus(), types=None)
    vox = dv.voxelize(128, fill=True, fill_argb=0xFF102030)
    st = dv.stats()
    assert st["interior_voxels"] > 0
    n_surf = st["voxels"] - st["interior_voxels"]
    for fmt in (hip.DENSE_U8, hip.DENSE_ARGB32, hip.DENSE_BITS):
        write_and_compare(dv, vox, n_surf, fmt, (0, 0, 0), (128, 128, 128))
        write_and_compare(dv, vox, n_surf, fmt, (16, 16, 16), (64, 64, 64))
    t = torch.zeros((128, 128, 128), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert dv.write_dense(t.data_ptr(), hip.DENSE_U8, (0, 0, 0), (128, 128, 128), (1, 128, 128 * 128)) == 0
    assert int((t == 1).sum()) == n_surf and int((t == 2).sum()) == st["interior_voxels"]
    print("ok write_dense", n, n_surf)


def case_voxels_box():
    dv = hip.DeviceVoxelizer(0)
    for verts, res, kw in ((meshes.scan_like(50_000), 200, {}), (torus(), 96, dict(fill=True)),
                           (fill_ref.weld(meshes.uv_sphere(16, radius=0.3, center=(0.5, -0.2, 0.1))), 64, {})):
        dv.set_triangles(verts)
        vox = dv.voxelize(res, **kw)
        lo, hi = dv.voxels_box()
        assert lo == tuple(int(v) for v in vox[:, :3].min(0)) and hi == tuple(int(v) + 1 for v in vox[:, :3].max(0)), (lo, hi)
        # a z-slab: the box of its records only
        vox = dv.voxelize(res, zslab=(res // 4, res // 2), **kw)
        lo, hi = dv.voxels_box()
        assert lo == tuple(int(v) for v in vox[:, :3].min(0)) and hi == tuple(int(v) + 1 for v in vox[:, :3].max(0)), (lo, hi)
    # an empty result: a slab above the mesh
    dv.set_triangles(np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32))
    assert dv.voxelize(64, zslab=(32, 64), read=False) == 0
    assert dv.voxels_box() == ((0, 0, 0), (0, 0, 0))
    print("ok voxels_box")


def case_torch():
    from obj2voxel_amd import dense
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    # positions computed by torch ops right before set_mesh, no explicit synchronisation here
    sphere = fill_ref.weld(meshes.uv_sphere(24))
    positions, faces = index_mesh(sphere, np.int64)
    p = (torch.from_numpy(positions).to(dev) * 2.0 + 1.0) * 0.5   # = positions + 0.5 exactly, on torch's stream
    f = torch.from_numpy(faces).to(dev)
    dense.set_mesh(dv, p, f)
    ref_verts = (positions * 2.0 + 1.0) * 0.5
    ref = hip.DeviceVoxelizer(0)
    T = len(faces)
    cols = meshes.triangle_colors(T)
    types = np.full(T, hip.TRI_UNTEXTURED, np.uint32)

    def ref_vox(res, **kw):
        ref.set_triangles(ref_verts.astype(np.float32)[faces].reshape(-1, 9), types=types, colors=cols)
        return ref.voxelize(res, **kw)

    dense.set_mesh(dv, p, f, types=torch.from_numpy(types.view(np.int32)).to(dev), colors=torch.from_numpy(cols).to(dev))
    res = 96
    vox = ref_vox(res)
    n = len(vox)
    for name, code in (("occupancy", hip.DENSE_U8), ("labels", hip.DENSE_U8), ("argb", hip.DENSE_ARGB32), ("bits", hip.DENSE_BITS)):
        g, origin = dense.voxelize_dense(dv, res, fmt=name)
        want, _ = scatter_ref(vox, n, code, (0, 0, 0), (res,) * 3)
        assert origin == (0, 0, 0) and g.dtype == dense.FORMATS[name][1] and g.is_contiguous()
        got = g.cpu().numpy()
        if name == "occupancy":
            want = want.astype(bool)
        assert got.shape == want.shape and np.array_equal(got, want), name
        # the tight box
        g, origin = dense.voxelize_dense(dv, res, fmt=name, box="tight")
        lo = vox[:, :3].min(0)
        dims = tuple(int(v) for v in vox[:, :3].max(0) + 1 - lo)
        want, _ = scatter_ref(vox, n, code, tuple(int(v) for v in lo), dims)
        assert origin == tuple(int(v) for v in lo), origin
        assert np.array_equal(g.cpu().numpy(), want.astype(bool) if name == "occupancy" else want), name + " tight"
        # max_layers: several z-slabs into one tensor
        g3, _ = dense.voxelize_dense(dv, res, fmt=name, max_layers=24)
        g1, _ = dense.voxelize_dense(dv, res, fmt=name)
        assert torch.equal(g3, g1), name + " slabs"
    # out= slices of a batch: two meshes, one a permuted view
    batch = torch.zeros((2, res, res, res), dtype=torch.bool, device=dev)
    other = meshes.scan_like(20_000)
    dense.voxelize_dense(dv, res, out=batch[0])
    dense.set_mesh(dv, torch.from_numpy(other).to(dev))
    perm = torch.zeros((res, res, res), dtype=torch.bool, device=dev)
    dense.voxelize_dense(dv, res, out=perm.permute(2, 0, 1))
    dense.voxelize_dense(dv, res, out=batch[1])
    ref.set_triangles(other)
    want1, _ = scatter_ref(ref.voxelize(res), 0, hip.DENSE_U8, (0, 0, 0), (res,) * 3)
    want0, _ = scatter_ref(vox, n, hip.DENSE_U8, (0, 0, 0), (res,) * 3)
    assert np.array_equal(batch[0].cpu().numpy(), want0.astype(bool))
    assert np.array_equal(batch[1].cpu().numpy(), want1.astype(bool))
    assert np.array_equal(perm.permute(2, 0, 1).cpu().numpy(), want1.astype(bool))
    # solid fill occupancy, in slabs too
    tp, tf = index_mesh(torus())
    dense.set_mesh(dv, torch.from_numpy(tp).to(dev), torch.from_numpy(tf).to(dev))
    ref.set_triangles(torus())
    fv = ref.voxelize(128, fill=True)
    st = ref.stats()
    want, _ = scatter_ref(fv, st["voxels"] - st["interior_voxels"], hip.DENSE_U8, (0, 0, 0), (128,) * 3)
    g, _ = dense.voxelize_dense(dv, 128, fill=True)
    assert g.dtype == torch.bool and np.array_equal(g.cpu().numpy(), want.astype(bool))
    lab, _ = dense.voxelize_dense(dv, 128, fmt="labels", fill=True, max_layers=40)
    assert np.array_equal(lab.cpu().numpy(), want)
    assert int((lab == 2).sum()) == st["interior_voxels"]
    # a box that does not hold every voxel raises
    try:
        dense.voxelize_dense(dv, 128, out=torch.zeros((128, 128, 64), dtype=torch.bool, device=dev))   # (the torus spans x)
        raise AssertionError("voxels outside the tensor were not reported")
    except ValueError as e:
        assert "outside" in str(e)
    print("ok torch")


CASES = {"upload": case_upload, "bad_index": case_bad_index, "pointers": case_pointers, "write_dense": case_write_dense,
         "voxels_box": case_voxels_box, "torch": case_torch}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
