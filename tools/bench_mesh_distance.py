#!/usr/bin/env python3
"""The narrow-band distance to the triangles (o2v_hip_mesh_distance_dense) on the bench headline mesh (meshes.scan_like(),
welded into positions + faces) at 1024: bands 1, 3 and 8, signed and unsigned, the whole grid into one float32 tensor.
Medians of --reps, in ms: the wall time of each synchronous call and its three stages from the events around them
(o2v_hip_mesh_distance_times: binning, parity, distance).  Pairs are the (voxel, triangle) pairs the distance stage evaluates
(tile lists x the voxels of the tile) and those that pass the per-voxel dilated-AABB cut, counted on the host from the mesh.
For comparison, section 11's voxel SDF of the same mesh (labels with the fill, then distance_transform).  One JSON object on
stdout."""
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
from tests import fill_ref  # noqa: E402

TILE = 8


def pair_counts(sv, res, band):
    """(pairs in the tile lists x 512, pairs inside the dilated AABB) of the whole grid, ss = 1."""
    sv = sv[np.all(np.isfinite(sv), axis=(1, 2))]
    m = band + 1.0
    lo, hi = sv.min(axis=1).astype(np.float64) - m, sv.max(axis=1).astype(np.float64) + m
    ilo = np.clip(np.floor(lo - 0.5) - 1, 0, res - 1)
    ihi = np.clip(np.floor(hi - 0.5) + 1, 0, res - 1)
    tiles = np.prod(ihi // TILE - ilo // TILE + 1, axis=1)
    # voxels whose centre i + 0.5 lies in [lo, hi]
    clo = np.clip(np.ceil(lo - 0.5), 0, res)
    chi = np.clip(np.floor(hi - 0.5), -1, res - 1)
    inside = np.prod(np.maximum(chi - clo + 1, 0), axis=1)
    return int(tiles.sum()) * TILE ** 3, int(inside.sum())


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
    dv.voxelize(res, read=False)
    sv = fill_ref.sample_vertices(positions.view(np.float32)[faces.reshape(-1, 3)].reshape(-1, 9), dv.transform())
    out = torch.empty((res, res, res), dtype=torch.float32, device=dev)
    r = {"mesh": "scan_like", "triangles": int(len(sv)), "resolution": res, "tile": TILE, "runs": []}
    for band in (1.0, 3.0, 8.0):
        listed, inside = pair_counts(sv, res, band)
        for signed in (True, False):
            dense.mesh_distance(dv, res, band=band, signed=signed, out=out)   # (warm-up: the scratch is grown)
            walls, stages = [], []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dense.mesh_distance(dv, res, band=band, signed=signed, out=out)
                walls.append((time.perf_counter() - t0) * 1e3)
                stages.append(dv.mesh_distance_times())
            ms = [statistics.median(s[i] for s in stages) for i in range(3)]
            r["runs"].append({"band": band, "signed": signed, "call_ms": round(statistics.median(walls), 3),
                              "stage_ms": [round(v, 3) for v in ms], "pairs_listed": listed, "pairs_in_aabb": inside,
                              "Gpairs_per_s_listed": round(listed / (ms[2] * 1e-3) / 1e9, 1),
                              "Gpairs_per_s_in_aabb": round(inside / (ms[2] * 1e-3) / 1e9, 1),
                              "in_band": int((out.abs() < band).sum())})
    del out
    torch.cuda.empty_cache()
    # section 11: the voxel SDF (labels with the fill, then the exact transform)
    walls = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g, _ = dense.voxelize_dense(dv, res, fmt="sdf", fill=True)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        del g
    r["voxel_sdf_call_ms"] = round(statistics.median(walls[1:]), 3)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
