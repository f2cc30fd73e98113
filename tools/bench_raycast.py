#!/usr/bin/env python3
"""Ray casting (o2v_hip_raycast_build / o2v_hip_raycast, dense.RayCaster) through the filled occupancy grid of the bench
headline mesh (meshes.scan_like(), fmt="occupancy", fill=True) at 1024^3.  Medians of --reps, in ms, from the events around
the kernels (o2v_hip_raycast_times): the build beside one streaming read of the grid at the 6.29 TB/s of a streaming copy; the
cast of a 2048 x 2048 dense.camera_rays image and of 2^22 rays from seeded random points of a sphere around the box to random
targets inside it, each with the hierarchy and with O2V_RAY_NO_SKIP=1 on the same build: Mrays/s, the ratio of the two, and ps
per fine cell, the fine cells per ray taken from the reference (tests/raycast_ref.py) on a seeded sample of 4 096 rays.  One
JSON object on stdout."""
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
from tests import raycast_ref  # noqa: E402

STREAM_TBS = 6.29   # a streaming copy on one MI355X, TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--image", type=int, default=2048)
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--sample", type=int, default=4096)
    args = ap.parse_args()
    res, reps = args.resolution, args.reps
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    grid, origin = dense.voxelize_dense(dv, res, fill=True)
    r = {"mesh": "scan_like", "resolution": res, "grid_bytes": grid.numel(), "solid_voxels": int(grid.sum()),
         "snapshot_bytes": dv.raycast_scratch_bytes((res, res, res))}
    caster = dense.RayCaster(dv, grid, origin=origin)   # (warm-up: the scratch is grown)
    build_ms = []
    for _ in range(reps):
        caster = dense.RayCaster(dv, grid, origin=origin)
        build_ms.append(dv.raycast_times()[0])
    floor = grid.numel() / (STREAM_TBS * 1e12) * 1e3
    r["build_ms"] = round(statistics.median(build_ms), 4)
    r["build_floor_ms"] = round(floor, 4)
    r["build_ratio_to_floor"] = round(statistics.median(build_ms) / floor, 2)

    gen = torch.Generator(device="cpu").manual_seed(1024)
    c = res / 2.0
    eye = (c - 1.1 * res, c - 1.9 * res, c + 1.2 * res)
    cam = dense.camera_rays(args.image, args.image, eye, (c, c, c), (0.0, 0.0, 1.0), 35.0, dev)
    u = torch.randn((args.rays, 3), generator=gen, dtype=torch.float64)
    start = c + u / u.norm(dim=1, keepdim=True) * (1.2 * res)
    target = torch.rand((args.rays, 3), generator=gen, dtype=torch.float64) * res
    sphere = (start.to(torch.float32).to(dev), (target - start).to(torch.float32).to(dev))
    host = grid.cpu().numpy()
    r["casts"] = []
    for name, (o, d) in (("camera", cam), ("sphere", sphere)):
        o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        n = o.shape[0]
        pick = torch.randperm(n, generator=gen)[:args.sample].to(dev)
        want_hit, want_t, steps = raycast_ref.cast_lockstep(host, origin, o[pick].cpu().numpy(), d[pick].cpu().numpy())
        cells_per_ray = steps / args.sample
        run = {"rays": n, "name": name, "hit_share_of_sample": round(float((want_hit[:, 0] >= 0).mean()), 4),
               "fine_cells_per_ray": round(cells_per_ray, 1)}
        for key, walk in (("skip", False), ("no_skip", True)):
            if walk:
                os.environ["O2V_RAY_NO_SKIP"] = "1"
            try:
                hit, t = caster.cast(o, d)
                ms = []
                for _ in range(reps):
                    hit, t = caster.cast(o, d)
                    ms.append(dv.raycast_times()[1])
            finally:
                os.environ.pop("O2V_RAY_NO_SKIP", None)
            same = bool((hit[pick].cpu().numpy() == want_hit).all()) and bool((t[pick].cpu().numpy().view(np.uint32) == want_t.view(np.uint32)).all())
            m = statistics.median(ms)
            run[key] = {"ms": round(m, 4), "mrays_per_s": round(n / m / 1e3, 1), "ps_per_fine_cell": float("%.4g" % (m * 1e9 / (n * cells_per_ray))),
                        "sample_equals_reference": same}
        run["no_skip_over_skip"] = round(run["no_skip"]["ms"] / run["skip"]["ms"], 2)
        r["casts"].append(run)
    r["host_copy_ms_at_56GBs"] = round(grid.numel() / 56e9 * 1e3, 1)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
