#!/usr/bin/env python3
"""The distance transform (o2v_hip_distance_dense) on the bench headline mesh (meshes.scan_like(), welded into positions +
faces) at 1024 with the solid fill: the labels from voxelize_dense(fmt="labels", fill=True), then DIST2 and SDF of the whole
grid.  Medians of --reps, in ms: the wall time of each synchronous call, and each pass from the events around it
(o2v_hip_distance_times).  Bytes are what the passes must move at least (grid traffic, plus the envelope stacks at 16 bytes
per pushed entry counted as if every voxel were pushed: an upper bound); TB/s against the 6.0 - 6.3 TB/s of streaming.  One
JSON object on stdout."""
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
    n = lab.numel()
    r = {"mesh": "scan_like", "resolution": res, "fill": True, "surface_voxels": int((lab == 1).sum()),
         "interior_voxels": int((lab == 2).sum()), "scratch_bytes": dv.distance_scratch_bytes((res,) * 3, hip.DIST_SQ_I32)}
    for fmt in ("dist2", "sdf"):
        out = torch.empty(tuple(lab.shape), dtype=dense.DISTANCE_FORMATS[fmt][1], device=dev)
        dense.distance_transform(dv, lab, fmt, out=out)   # (warm-up, and the scratch is grown)
        walls, passes = [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dense.distance_transform(dv, lab, fmt, out=out)
            walls.append((time.perf_counter() - t0) * 1e3)
            passes.append(dv.distance_times())
        ms = [statistics.median(p[i] for p in passes) for i in range(3)]
        # grid bytes: x reads the labels (up to twice: the look-ahead) and writes 4; y and z read and write 4; SDF reads the
        # labels once more in z
        grid = [n * (1 + 4), n * 8, n * (8 + (1 if fmt == "sdf" else 0))]
        stack = [0, n * 16, n * 16]
        r[fmt] = {"call_ms": round(statistics.median(walls), 3), "pass_ms": [round(v, 3) for v in ms],
                  "grid_GB": [round(b / 1e9, 2) for b in grid],
                  "grid_TBps": [round(b / (t * 1e-3) / 1e12, 2) for b, t in zip(grid, ms)],
                  "grid_and_stack_TBps": [round((b + s) / (t * 1e-3) / 1e12, 2) for b, s, t in zip(grid, stack, ms)]}
        del out
        torch.cuda.empty_cache()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
