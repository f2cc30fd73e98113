"""The calls of tests/test_gpu_upload_bounds.py that run twice: in the test process with the shortcut (occupancy only: bounds
from the upload, transform from the host, no k_bounds and no k_setup) and, as `python -m tests.upload_bounds_cases ab` with
O2V_ALL_LAUNCHES=1, in a child process with both launches.  The child leaves its results in the .npz file that
O2V_TEST_UPLOAD_BOUNDS_OUT names.  Case `device_upload`: the bounds-follow-the-upload sequence through
o2v_hip_set_triangles_device (torch imported before the library is loaded).  A case prints "ok" last when everything held."""
import os
import re
import sys

if __name__ == "__main__" and sys.argv[1:] == ["device_upload"]:
    import torch  # first

import numpy as np

from obj2voxel_amd import hip, meshes

PERMUTE = (0, -1, 0, 0, 0, 1, -1, 0, 0)   # a unit transform that permutes the axes and negates two of them


def affine(v, scale, shift):
    """The mesh v scaled and shifted per axis, rounded once to float32."""
    p = np.asarray(v, np.float64).reshape(-1, 3) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    return p.astype(np.float32).reshape(-1, 9)


def bounds_of(v):
    p = np.asarray(v, np.float32).reshape(-1, 3)
    return np.concatenate([p.min(axis=0), p.max(axis=0)]).astype(np.float32)


def sphere():
    return meshes.uv_sphere(60)


def awkward():
    """name -> (mesh, resolution): boxes whose transform has little to spare in float32"""
    s = meshes.uv_sphere(24)
    return {
        "far": (affine(s, (0.53, 0.47, 0.5), (10000.123, 10003.456, -9999.789)), 128),   # offset about 1e4, extent about 1
        "flat": (affine(s, (1.0, 1.0, 1.0e-3), (0.0, 0.0, 0.0)), 128),              # one axis 1e-3 of the others
        "npot": (affine(s, (1.37, 0.9, 0.61), (0.3, -0.2, 0.1)), 300),              # longest axis 2.74, no power of two
    }


def nan_mesh():
    v = meshes.uv_sphere(20).copy()
    v[len(v) // 2, 4] = np.nan
    return v


def follow_meshes():
    """v, w (every other triangle of v, half the size, shifted: other bounds), v"""
    v = meshes.uv_sphere(40)
    w = affine(v[::2], (0.5, 0.5, 0.5), (0.25, -0.125, 0.375))
    return [v, w, v]


def _call(d, res, **kw):
    """(transform, sorted records, kernel names, return code) of one voxelize call; the second of two equal calls is the one
    with kernel_times"""
    try:
        d.voxelize(res, read=False, **kw)
        vox = meshes.sorted_voxels(d.voxelize(res, kernel_times=True, **kw))
        return d.transform(), vox, sorted(d.kernel_times()), 0
    except hip.DeviceError as e:
        return np.zeros(12, np.float32), np.zeros((0, 4), np.uint32), [], int(re.search(r"code (-?\d+)", str(e)).group(1))


def ab_calls():
    """name -> (transform, sorted records, kernel names, return code) of every call that is compared between the two processes"""
    out = {}
    d = hip.DeviceVoxelizer(0)
    try:
        d.set_triangles(sphere())
        for res in (128, 256):       # on one context
            out[f"sphere_{res}"] = _call(d, res)
            out[f"sphere_{res}_permuted"] = _call(d, res, unit_transform=PERMUTE)
        for name, (v, res) in awkward().items():
            d.set_triangles(v)
            out[name] = _call(d, res)
        d.set_triangles(nan_mesh())
        out["nan"] = _call(d, 64)
    finally:
        d.close()
    return out


def pack(calls):
    flat = {}
    for name, (xf, vox, kernels, rc) in calls.items():
        flat[name + ".xf"], flat[name + ".vox"], flat[name + ".rc"] = xf, vox, np.int64(rc)
        flat[name + ".kernels"] = np.array(kernels, dtype="U64")
    return flat


def unpack(npz):
    names = sorted({k.rsplit(".", 1)[0] for k in npz.files})
    return {n: (npz[n + ".xf"], npz[n + ".vox"], [str(k) for k in npz[n + ".kernels"]], int(npz[n + ".rc"])) for n in names}


def device_upload():
    from oracle import oracle
    from tests.dense_cases import device_upload as upload
    oracle.build()
    d = hip.DeviceVoxelizer(0)
    try:
        for i, (m, indexed) in enumerate(zip(follow_meshes(), (False, True, False))):
            upload(d, m, {}, indexed=indexed)
            got = meshes.sorted_voxels(d.voxelize(128, kernel_times=True))
            assert "k_bounds" not in d.kernel_times() and "k_voxelize_occ" in d.kernel_times(), d.kernel_times()
            assert np.array_equal(d.transform(), oracle.mesh_transform(bounds_of(m), 128)), i
            assert np.array_equal(got, meshes.sorted_voxels(oracle.voxelize(m, 128))), i
    finally:
        d.close()


if __name__ == "__main__":
    if sys.argv[1] == "ab":
        assert os.environ.get("O2V_ALL_LAUNCHES") == "1"
        np.savez(os.environ["O2V_TEST_UPLOAD_BOUNDS_OUT"], **pack(ab_calls()))
    else:
        {"device_upload": device_upload}[sys.argv[1]]()
    print("ok")
