#!/usr/bin/env python3
"""The nearest-voxel transform (o2v_hip_nearest_dense) on the bench headline mesh (meshes.scan_like(), welded into positions +
faces) at 1024 with the solid fill: the labels and the argb grid from voxelize_dense(fill=True), then, with the surface voxels
as seeds, nearest alone, nearest with dist2, and nearest with the interior painted (values, VALUES_INSIDE).  In the same run
K8's DIST2 of the same labels (o2v_hip_distance_dense): the yardstick, the same passes without the payload.  Medians of --reps,
in ms: the wall time of each synchronous call, and each pass from the events around it (o2v_hip_nearest_times /
o2v_hip_distance_times).  Bytes are the grid traffic the passes must move at least, as tools/bench_distance.py counts it, plus
4 per voxel for dist2 and 8 per painted voxel (the gather and the write) in the z pass.  One JSON object on stdout (DESIGN.md
section 18)."""
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

from obj2voxel_amd import dense, hip, meshes  # noqa: E402


def timed(reps, call, times):
    """(median wall ms, median ms per pass) of `call`, after one warm-up."""
    call()
    walls, passes = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        walls.append((time.perf_counter() - t0) * 1e3)
        passes.append(times())
    return statistics.median(walls), [statistics.median(p[i] for p in passes) for i in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    res, reps = args.resolution, args.reps
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    lab, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
    argb, _ = dense.voxelize_dense(dv, res, fmt="argb", fill=True)
    n = lab.numel()
    interior = int((lab == 2).sum())
    r = {"mesh": "scan_like", "resolution": res, "fill": True, "surface_voxels": int((lab == 1).sum()), "interior_voxels": interior,
         "scratch_bytes": dv.nearest_scratch_bytes((res,) * 3)}
    shape = tuple(lab.shape)
    near = torch.empty(shape, dtype=torch.int32, device=dev)
    d2 = torch.empty(shape, dtype=torch.int32, device=dev)
    grid = dense._strides(lab), (res,) * 3, 0.0

    def report(name, wall, ms, z_extra):
        # grid bytes: x reads the seeds (up to twice: the look-ahead) and writes 4; y and z read and write 4
        b = [n * (1 + 4), n * 8, n * 8 + z_extra]
        r[name] = {"call_ms": round(wall, 3), "pass_ms": [round(v, 3) for v in ms], "passes_ms": round(sum(ms), 3),
                   "grid_GB": [round(v / 1e9, 2) for v in b], "grid_TBps": [round(v / (t * 1e-3) / 1e12, 2) for v, t in zip(b, ms)]}

    def k8():
        dv.distance_dense(lab.data_ptr(), grid[0], d2.data_ptr(), hip.DIST_SQ_I32, dense._strides(d2), grid[1])

    def k15(flags, dist2=None, values=None):
        dv.nearest_dense(lab.data_ptr(), hip.GRID_U8, *grid, flags, near.data_ptr(), dense._strides(near), dense._ptr(dist2),
                         None if dist2 is None else dense._strides(dist2), dense._ptr(values), None if values is None else dense._strides(values))

    one, inside = hip.NEAREST_SEED_ONE, hip.NEAREST_VALUES_INSIDE
    torch.cuda.synchronize()
    report("distance_dist2", *timed(reps, k8, dv.distance_times), 0)
    want = d2.clone()
    report("nearest", *timed(reps, lambda: k15(one), dv.nearest_times), 0)
    report("nearest_dist2", *timed(reps, lambda: k15(one, dist2=d2), dv.nearest_times), n * 4)
    r["dist2_equals_distance"] = bool(torch.equal(d2, want))
    # (painting is idempotent: a painted interior voxel takes the same seed's colour again)
    report("nearest_values_inside", *timed(reps, lambda: k15(one | inside, values=argb), dv.nearest_times), n + interior * 8)
    r["nearest_over_distance"] = round(r["nearest"]["passes_ms"] / r["distance_dist2"]["passes_ms"], 3)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
