#!/usr/bin/env python3
"""Sky visibility (o2v_hip_openness) on the filled bench headline mesh (meshes.scan_like(), welded into positions + faces) at every
--resolutions.  For each grid, surface targets: 26 and 98 directions, max_distance 16 and unlimited, with and without
O2V_OPEN_NO_SKIP=1 - the device times of the stages build, targets and walk from the events around them (o2v_hip_openness_times),
median of --reps after a warm-up (the fine walk, O2V_OPEN_NO_SKIP=1, once after a warm-up of the skipping one), the rays per second
of the walk (targets x directions / walk time) and of the whole call, and the results of the two walks asserted equal.  The
yardstick, measured in the same run: RayCaster.cast on a sample of 2^24 of the same rays - origins at the centres of every k-th
target, the same directions as floats, t_max = inf - by o2v_hip_raycast_times.  One JSON object on stdout."""
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

CAST_RAYS = 2 ** 24


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def med(v):
    return round(statistics.median(v), 4)


def open_ms(dv, solid, n_dirs, max_distance, reps, no_skip):
    """(medians of build, targets, walk), the counts of the last call"""
    if no_skip:
        os.environ["O2V_OPEN_NO_SKIP"] = "1"
    else:
        os.environ.pop("O2V_OPEN_NO_SKIP", None)
    ms = []
    for i in range(reps + (0 if no_skip else 1)):
        count = dense.openness(dv, solid, directions=n_dirs, max_distance=max_distance)
        if i or no_skip:
            ms.append(dv.openness_times())
    os.environ.pop("O2V_OPEN_NO_SKIP", None)
    return [med(m[k] for m in ms) for k in range(3)], count


def cast_ms(dv, solid, count, n_dirs, reps):
    """RayCaster.cast on CAST_RAYS rays of the openness call: every k-th target x all directions; (ms, rays, open fraction)"""
    dev = solid.device
    cells = (count != 255).nonzero()                         # (z, y, x), in the order of the grid
    per = max(1, CAST_RAYS // n_dirs)
    cells = cells[::max(1, len(cells) // per)][:per]
    d = dense.direction_set(n_dirs).to(dev).to(torch.float32)
    origins = (cells.flip(1).to(torch.float32) + 0.5)[:, None, :].expand(-1, n_dirs, -1).reshape(-1, 3).contiguous()
    directions = d[None, :, :].expand(len(cells), -1, -1).reshape(-1, 3).contiguous()
    del cells
    caster = dense.RayCaster(dv, solid)
    ms = []
    for i in range(reps + 1):
        hit, _ = caster.cast(origins, directions)
        if i:
            ms.append(dv.raycast_times()[1])
    # (a ray from a voxel's centre starts inside it: face -1 at t = 0 - cast cannot leave the start cell out, so its rays end at
    # once; the yardstick that walks is the same rays started one step outside: origins moved by a direction's length)
    moved = origins + directions
    ms_moved = []
    for i in range(reps + 1):
        hit, _ = caster.cast(moved, directions)
        if i:
            ms_moved.append(dv.raycast_times()[1])
    miss = float((hit[:, 0] < 0).float().mean())   # (a hit has box coordinates, a miss -1)
    return med(ms), med(ms_moved), len(origins), round(miss, 4)


def bench_grid(dv, res, solid, reps):
    r = {"shape": list(solid.shape), "solid_voxels": int(dense.count_voxels(dv, solid))}
    say(f"solid at {res}", r)
    for n_dirs in (26, 98):
        for max_distance in (16, None):
            name = f"{n_dirs}_directions_max_distance_{max_distance}"
            (t_b, t_t, t_w), count = open_ms(dv, solid, n_dirs, max_distance, reps, False)
            targets = int((count != 255).sum())
            rays = targets * n_dirs
            q = {"targets": targets, "rays": rays, "mean_open_fraction": round(float(count[count != 255].float().mean()) / n_dirs, 4),
                 "build_ms": t_b, "targets_ms": t_t, "walk_ms": t_w, "call_ms": round(t_b + t_t + t_w, 4), "walk_Grays_per_s": round(rays / t_w / 1e6, 3),
                 "call_Grays_per_s": round(rays / (t_b + t_t + t_w) / 1e6, 3)}
            say(" ", name, q)
            (_, _, t_f), fine = open_ms(dv, solid, n_dirs, max_distance, 1, True)
            assert torch.equal(fine, count), "the fine walk and the skipping walk differ"
            q["no_skip_walk_ms"], q["no_skip_walk_Grays_per_s"], q["skip_speedup"] = t_f, round(rays / t_f / 1e6, 3), round(t_f / t_w, 2)
            del fine
            if max_distance is None:
                t_c, t_cm, n_cast, miss = cast_ms(dv, solid, count, n_dirs, reps)
                q["cast"] = {"rays": n_cast, "from_centre_ms": t_c, "from_centre_Grays_per_s": round(n_cast / t_c / 1e6, 3), "one_step_out_ms": t_cm,
                             "one_step_out_Grays_per_s": round(n_cast / t_cm / 1e6, 3), "one_step_out_miss_fraction": miss,
                             "walk_over_cast_per_ray": round((rays / t_w) / (n_cast / t_cm), 2)}
            say(" ", name, q)
            r[name] = q
            del count
            torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    r = {"mesh": "scan_like", "reps": args.reps, "grids": {}}
    for res in args.resolutions:
        solid, _ = dense.voxelize_dense(dv, res, fmt="occupancy", fill=True)
        r["grids"][f"fill_occupancy_{res}"] = bench_grid(dv, res, solid, args.reps)
        del solid
        torch.cuda.empty_cache()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
