#!/usr/bin/env python3
"""Signed crossing numbers (o2v_hip_crossings_dense) on the bench headline mesh (meshes.scan_like(), welded into positions +
faces) at 1024^3.  Per axis: the device time from the events around its kernels (o2v_hip_crossings_times), median of --reps
after a warm-up, with min and max - each axis asked for alone (its sums are stored) and the three in one call (y and z are added
to what x stored); the bytes the axis must move at least - the int32 delta grid cleared, then read, and the output written
(and read, where it is added to) - over that time, and as a share of the 6.3 TB/s a device copy reaches on the MI355X; the
x : z and y : z ratios, and the x rays again without the LDS-staged tile (O2V_CROSS_NO_TILE=1).  Beside it, on the same mesh:
the time of K6's parity bitmap (the parity stage of o2v_hip_mesh_distance_times) and the wall times of
voxelize_dense(fmt="labels") + solidify, of fill=True's labels and of winding_fill as a whole.  One JSON object on stdout
(DESIGN.md section 21)."""
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

COPY_TBPS = 6.3   # the measured device copy of the MI355X


def stats(ms, nbytes):
    t = statistics.median(ms)
    tbps = nbytes / (t * 1e-3) / 1e12
    return {"device_ms": round(t, 3), "device_ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "GB": round(nbytes / 1e9, 2),
            "TBps": round(tbps, 3), "share_of_copy": round(tbps / COPY_TBPS, 3)}


def wall(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        del out
    return {"wall_ms": round(statistics.median(ms), 2), "wall_ms_min_max": [round(min(ms), 2), round(max(ms), 2)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    res, reps = args.resolution, args.reps
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    n = res ** 3
    r = {"mesh": "scan_like", "triangles": int(len(verts)), "resolution": res, "copy_TBps": COPY_TBPS}
    S = torch.empty((res, res, res), dtype=torch.int32, device=dev)
    # each axis alone: delta cleared + read + the output written
    for i, a in enumerate("xyz"):
        dense.crossing_numbers(dv, res, axes=a, out=S)
        ms = []
        for _ in range(reps):
            dense.crossing_numbers(dv, res, axes=a, out=S)
            ms.append(dv.crossings_times()[i])
        r["alone_" + a] = stats(ms, 12 * n)
    # A/B: the x rays without the LDS-staged tile, a lane per line storing 4 bytes into a row of its own
    os.environ["O2V_CROSS_NO_TILE"] = "1"
    dense.crossing_numbers(dv, res, axes="x", out=S)
    ms = []
    for _ in range(reps):
        dense.crossing_numbers(dv, res, axes="x", out=S)
        ms.append(dv.crossings_times()[0])
    del os.environ["O2V_CROSS_NO_TILE"]
    r["alone_x_no_tile"] = stats(ms, 12 * n)
    # the three in one call: y and z also read the output
    dense.crossing_numbers(dv, res, out=S)
    ms = [[], [], []]
    for _ in range(reps):
        dense.crossing_numbers(dv, res, out=S)
        for i, t in enumerate(dv.crossings_times()):
            ms[i].append(t)
    for i, a in enumerate("xyz"):
        r["xyz_" + a] = stats(ms[i], (12 if i == 0 else 16) * n)
    r["xyz_total_ms"] = round(sum(r["xyz_" + a]["device_ms"] for a in "xyz"), 3)
    r["x_no_tile_to_z_alone"] = round(r["alone_x_no_tile"]["device_ms"] / r["alone_z"]["device_ms"], 2)
    for a in "xy":
        r[a + "_to_z_alone"] = round(r["alone_" + a]["device_ms"] / r["alone_z"]["device_ms"], 2)
    r["inside_voxels"] = int((S.abs() >= 4).sum())
    r["values"] = [int(v) for v in torch.unique(S).tolist()][:16]
    del S
    # K6's parity bitmap of the same box
    out = torch.empty((res, res, res), dtype=torch.float32, device=dev)
    dense.mesh_distance(dv, res, band=1.0, out=out)
    ms = []
    for _ in range(reps):
        dense.mesh_distance(dv, res, band=1.0, out=out)
        ms.append(dv.mesh_distance_times()[1])
    r["k6_parity_ms"] = {"device_ms": round(statistics.median(ms), 3), "device_ms_min_max": [round(min(ms), 3), round(max(ms), 3)]}
    del out
    # the two fills as a user calls them
    dense.solidify(dv, dense.voxelize_dense(dv, res, fmt="labels")[0])
    r["labels_plus_solidify"] = wall(lambda: dense.solidify(dv, dense.voxelize_dense(dv, res, fmt="labels")[0]), max(1, reps // 3))
    r["fill_true_labels"] = wall(lambda: dense.voxelize_dense(dv, res, fmt="labels", fill=True)[0], max(1, reps // 3))
    dense.winding_fill(dv, res)
    r["winding_fill"] = wall(lambda: dense.winding_fill(dv, res)[0], max(1, reps // 3))
    print(json.dumps(r))


if __name__ == "__main__":
    main()
