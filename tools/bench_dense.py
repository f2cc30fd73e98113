#!/usr/bin/env python3
"""Device-resident input and dense output on the bench headline mesh (meshes.scan_like(), welded into positions + faces) at
1024: the host flat upload against the device indexed upload, the voxelize call, o2v_hip_write_dense per format, clearing each grid with torch, and o2v_hip_read_voxels to host for
comparison; the same with the solid fill and U8.  Wall times of the synchronous calls, median of --reps, in ms.  One JSON
object on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import torch  # first: the library binds to the HIP runtime torch loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from obj2voxel_amd import hip, meshes  # noqa: E402


def median_ms(fn, reps):
    fn()   # (warm-up)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    res, reps = args.resolution, args.reps
    verts = meshes.scan_like()
    v = verts.reshape(-1, 3)
    _, first, inverse = np.unique(v.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    positions, faces = v[first], inverse.reshape(-1, 3).astype(np.int32)
    T, V = len(faces), len(positions)
    dev = torch.device("cuda", 0)
    p, f = torch.from_numpy(positions).to(dev), torch.from_numpy(faces).to(dev)
    torch.cuda.synchronize()
    dv = hip.DeviceVoxelizer(0)
    r = {"mesh": "scan_like", "triangles": T, "positions": V, "resolution": res}
    r["upload_host_flat_ms"] = median_ms(lambda: dv.set_triangles(verts), reps)
    r["upload_device_indexed_ms"] = median_ms(lambda: dv.set_triangles_device(p.data_ptr(), V, f.data_ptr(), 4, T), reps)
    r["voxelize_ms"] = median_ms(lambda: dv.voxelize(res, read=False), reps)
    n = dv.count
    r["voxels"] = n
    dims, box0 = (res, res, res), (0, 0, 0)

    def dense_leg(tag, n_records):
        words = (res + 31) // 32
        for name, code, shape, dtype in (("u8", hip.DENSE_U8, (res, res, res), torch.uint8),
                                          ("argb32", hip.DENSE_ARGB32, (res, res, res), torch.int32),
                                          ("bits", hip.DENSE_BITS, (res, res, words), torch.int32)):
            if tag and name != "u8":
                continue
            try:
                t = torch.zeros(shape, dtype=dtype, device=dev)
            except torch.OutOfMemoryError:
                r[f"{tag}write_{name}_ms"] = None
                continue
            torch.cuda.synchronize()
            strides = (t.stride(2), t.stride(1), t.stride(0))
            r[f"{tag}clear_{name}_ms"] = median_ms(lambda: t.zero_(), reps)
            r[f"{tag}write_{name}_ms"] = median_ms(lambda: dv.write_dense(t.data_ptr(), code, box0, dims, strides), reps)
            if name == "u8":
                r[f"{tag}write_u8_GBps"] = round(n_records * 16 / (r[f"{tag}write_u8_ms"] * 1e-3) / 1e9, 1)
            del t
            torch.cuda.empty_cache()
        m = min(n_records, 1 << 26)   # (at most 1 GiB of host memory: the fill's records are several GB)
        out = np.empty((m, 4), np.uint32)
        r[f"{tag}read_voxels_records"] = m
        r[f"{tag}read_voxels_ms"] = median_ms(lambda: dv._L.o2v_hip_read_voxels(dv._ctx, hip._ptr(out), 0, m), reps)
        r[f"{tag}box_ms"] = median_ms(dv.voxels_box, reps)

    dense_leg("", n)
    r["fill_voxelize_ms"] = median_ms(lambda: dv.voxelize(res, read=False, fill=True), reps)
    r["fill_voxels"], r["fill_interior_voxels"] = dv.count, dv.stats()["interior_voxels"]
    dense_leg("fill_", dv.count)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
