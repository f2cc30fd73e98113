#!/usr/bin/env python3
"""Surface extraction (o2v_hip_surface_count / _write, dense.extract_surface) on the band-3 signed TSDF of the bench headline
mesh (meshes.scan_like(), welded into positions + faces) at 1024: levels 0 and 1.5.  Medians of --reps, in ms: the wall time of
the two synchronous calls and of the whole extract_surface (count, two torch.empty, write), and the four stages from the
events around them (o2v_hip_surface_times: classify, count + scan, vertices, faces).  Beside each stage what it must at least
move, at the 6.29 TB/s of a streaming copy: the field once for the classify stage, the outputs (12 V + 12 T bytes) and eight
corner reads per vertex for the two emit stages.  One JSON object on stdout."""
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

STREAM_TBS = 6.29   # a streaming copy on one MI355X, TB/s


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
    tsdf, origin = dense.mesh_distance(dv, res, band=3.0)
    nz, ny, nx = tsdf.shape
    grid = (tsdf.data_ptr(), (tsdf.stride(2), tsdf.stride(1), tsdf.stride(0)), (nx, ny, nz))
    floor = lambda nbytes: nbytes / (STREAM_TBS * 1e12) * 1e3   # noqa: E731  (ms)
    r = {"mesh": "scan_like", "resolution": res, "band": 3.0, "field_bytes": tsdf.numel() * 4, "runs": []}
    for level in (0.0, 1.5):
        dense.extract_surface(dv, tsdf, level, origin=origin)   # (warm-up: the scratch is grown)
        count_ms, write_ms, whole_ms, stages = [], [], [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p, f = dense.extract_surface(dv, tsdf, level, origin=origin)
            whole_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            v, t = dv.surface_count(*grid, level)
            t1 = time.perf_counter()
            dv.surface_write(*grid, level, origin, p.data_ptr(), v, f.data_ptr(), t)
            t2 = time.perf_counter()
            count_ms.append((t1 - t0) * 1e3)
            write_ms.append((t2 - t1) * 1e3)
            stages.append(dv.surface_times())
        ms = [statistics.median(s[i] for s in stages) for i in range(4)]
        floors = [floor(tsdf.numel() * 4), None, floor(12 * v + 32 * v), floor(12 * t)]
        r["runs"].append({"level": level, "vertices": v, "triangles": t, "count_call_ms": round(statistics.median(count_ms), 3),
                          "write_call_ms": round(statistics.median(write_ms), 3), "extract_surface_ms": round(statistics.median(whole_ms), 3),
                          "stage_ms": [round(x, 3) for x in ms], "floor_ms": [None if x is None else round(x, 4) for x in floors],
                          "ratio_to_floor": [None if x is None else round(m / x, 2) for m, x in zip(ms, floors)],
                          "emit_over_classify": round((ms[2] + ms[3]) / ms[0], 2)})
    r["host_copy_ms_at_56GBs"] = round(tsdf.numel() * 4 / 56e9 * 1e3, 1)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
