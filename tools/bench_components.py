#!/usr/bin/env python3
"""Connected components and flood fill (o2v_hip_components_dense / o2v_hip_flood_dense, dense.components / solidify) of the filled
occupancy grid of the bench headline mesh (meshes.scan_like(), fmt="occupancy", fill=True) at 1024^3, and of a serpentine of the
same size.  Medians of --reps, in ms, from the events around the stages (o2v_hip_components_times: classify, tile pass, seams,
flatten, write): components at connectivities 6 and 26 of the solid and of the background, solidify, each with the tile pass and
with O2V_CC_NO_TILES=1; beside them the floor of a call - its bytes read and written at the 6.1 TB/s of a streaming copy - and the
seam unions and atomicMin retries of one more call made with the counters on.  One JSON object on stdout."""
import argparse
import json
import os
import statistics
import sys

import torch  # first: the library binds to the HIP runtime torch loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from obj2voxel_amd import dense, hip, meshes  # noqa: E402
from tests import components_ref  # noqa: E402

STREAM_TBS = 6.1   # a streaming copy on one MI355X, TB/s (the guide's 6.0 - 6.2)
STAGES = ("classify", "tiles", "seams", "flatten", "write")


def measure(dv, call, reps):
    call()   # (warm-up: the scratch is grown)
    ms = []
    for _ in range(reps):
        call()
        ms.append(dv.components_times())
    stages = [statistics.median(m[i] for m in ms) for i in range(5)]
    return {"ms": round(sum(stages), 4), "stages_ms": dict(zip(STAGES, (round(v, 4) for v in stages)))}


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
    grid, _ = dense.voxelize_dense(dv, res, fill=True)
    surface, _ = dense.voxelize_dense(dv, res, fmt="labels")
    serpentine = torch.from_numpy(components_ref.serpentine((res, res, res))).to(dev)
    voxels = grid.numel()
    labels = torch.empty((res, res, res), dtype=torch.int32, device=dev)
    out = torch.empty((res, res, res), dtype=torch.uint8, device=dev)
    # a call's traffic per voxel: the grid (1), the bits written and read by four passes (5/8), then
    #   labels: parents written by the tile pass (4), read and written by the flatten (8), read and the labels written (8)
    #   flood: the same parents (12), read again (4), out written (1)
    floors = {"components": voxels * (1 + 5 / 8 + 20) / (STREAM_TBS * 1e12) * 1e3, "solidify": voxels * (1 + 5 / 8 + 17) / (STREAM_TBS * 1e12) * 1e3}
    r = {"mesh": "scan_like", "resolution": res, "solid_voxels": int(grid.sum()), "floor_ms": {k: round(v, 3) for k, v in floors.items()},
         "scratch_bytes": {"labels": dv.components_scratch_bytes((res,) * 3), "flood": dv.components_scratch_bytes((res,) * 3, hip.CC_SCRATCH_FLOOD)},
         "runs": []}
    calls = [(f"components {c} {'background' if b else 'solid'}", g, c, b) for g in (grid,) for c in (6, 26) for b in (False, True)]
    calls.append(("components 6 serpentine", serpentine, 6, False))
    for mode in ("tiles", "no_tiles"):
        if mode == "no_tiles":
            os.environ["O2V_CC_NO_TILES"] = "1"
        try:
            for name, g, c, b in calls:
                run = {"name": name, "mode": mode}
                run.update(measure(dv, lambda: dense.components(dv, g, connectivity=c, background=b, out=labels), reps))
                run["components"] = dense.components(dv, g, connectivity=c, background=b, out=labels)[1]
                dv.components_dense(g.data_ptr(), hip.GRID_U8, dense._strides(g), (res,) * 3, 0.0, c, (hip.CC_INVERT if b else 0) | hip.FLAG_STAGE_TIMES,
                                    labels.data_ptr(), dense._strides(labels))
                run["seam_unions"], run["atomic_min_retries"] = dv.components_counters()
                run["ratio_to_floor"] = round(run["ms"] / floors["components"], 2)
                r["runs"].append(run)
            run = {"name": "solidify", "mode": mode}
            run.update(measure(dv, lambda: dense.solidify(dv, surface, out=out), reps))
            run["interior_voxels"] = int((out == 2).sum())
            run["ratio_to_floor"] = round(run["ms"] / floors["solidify"], 2)
            r["runs"].append(run)
        finally:
            os.environ.pop("O2V_CC_NO_TILES", None)
    r["host_copy_ms_of_a_float_grid_measured_by_k10"] = 77
    print(json.dumps(r))


if __name__ == "__main__":
    main()
