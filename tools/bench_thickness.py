#!/usr/bin/env python3
"""Local thickness and ball morphology (o2v_hip_thickness_dense) on the filled bench mesh (meshes.scan_like(), welded into
positions + faces, voxelize_dense(fill=True)) at --resolutions (512 and 1024): local_thickness at max_radius 2, 4, 8 and 16 with
the time of each stage from the events around it (o2v_hip_thickness_times: depth, opening, list, balls, convert), the counters
(candidate centres, centres kept, ball voxels visited; the last from one extra call with O2V_HIP_FLAG_STAGE_TIMES), the atomics
issued per second in the ball stage at most (a visited voxel issues one only where its stored value is smaller) and the ball
stage over the two transforms; thin_regions and the four morphology calls as wall times; and for scale dense.distance_transform
(K8, "dist2") of the same grid's labels from the same session.  First the 96^3 digital ball of DESIGN.md section 24 through the
counters.  Medians of --reps, in ms.  One JSON object on stdout, progress on stderr."""
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


def wall_ms(reps, call):
    call()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 3)


def thickness(dv, solid, cap, reps, dst, depth):
    """Stage times and counters of o2v_hip_thickness_dense at this cap (border on, int32 out, the caller's depth2)."""
    dims = tuple(solid.shape[::-1])
    args = (solid.data_ptr(), hip.GRID_U8, dense._strides(solid), dims, 0.0)
    outs = (dst.data_ptr(), dense._strides(dst), depth.data_ptr(), dense._strides(depth))
    torch.cuda.synchronize()
    dv.thickness_dense(*args, hip.THICK_BORDER | hip.FLAG_STAGE_TIMES, cap, *outs)   # warm-up, and the visited voxels
    counters = dv.thickness_counters()
    stages, walls = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        dv.thickness_dense(*args, hip.THICK_BORDER, cap, *outs)
        walls.append((time.perf_counter() - t0) * 1e3)
        stages.append(dv.thickness_times())
    ms = [statistics.median(s[i] for s in stages) for i in range(5)]
    two = ms[0] + ms[1]
    return {"cap": cap, "call_ms": round(statistics.median(walls), 3), "stage_ms": dict(zip(("depth", "opening", "list", "balls", "convert"), (round(v, 3) for v in ms))),
            "candidates": counters[0], "kept": counters[1], "ball_voxels": counters[2], "voxels_per_centre": round(counters[2] / max(counters[1], 1), 1),
            "ball_voxels_per_s": round(counters[2] / (ms[3] * 1e-3)) if ms[3] > 0 and counters[2] else 0, "balls_over_two_transforms": round(ms[3] / two, 2),
            "thinner_than_cap": int(((dst > 0) & (dst < cap)).sum()), "scratch_bytes": dv.thickness_scratch_bytes(dims, cap, True) + 4 * counters[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--radii", type=float, nargs="+", default=[2, 4, 8, 16])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    r = {"mesh": "scan_like", "fill": True}
    # the digital ball of the issue: 78 298 candidates and 15 584 kept at cap 16, 151 574 and 17 660 at cap 64
    z, y, x = np.meshgrid(*(np.arange(96),) * 3, indexing="ij")
    ball = torch.from_numpy((x - 48) ** 2 + (y - 48) ** 2 + (z - 48) ** 2 < 43.2 ** 2).to(dev)
    dst, depth = torch.empty((96,) * 3, dtype=torch.int32, device=dev), torch.empty((96,) * 3, dtype=torch.int32, device=dev)
    r["ball_96"] = [{k: v for k, v in thickness(dv, ball, cap, 1, dst, depth).items() if k in ("cap", "candidates", "kept", "ball_voxels", "stage_ms")} for cap in (16, 64)]
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    for res in args.resolutions:
        print(f"resolution {res} ...", file=sys.stderr, flush=True)
        solid, _ = dense.voxelize_dense(dv, res, fill=True)
        labels, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
        shape = tuple(solid.shape)
        dst, depth = torch.empty(shape, dtype=torch.int32, device=dev), torch.empty(shape, dtype=torch.int32, device=dev)
        e = {"solid_voxels": int(solid.sum()), "local_thickness": []}
        dense.distance_transform(dv, labels, "dist2", out=dst)
        walls, passes = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dense.distance_transform(dv, labels, "dist2", out=dst)
            walls.append((time.perf_counter() - t0) * 1e3)
            passes.append(sum(dv.distance_times()))
        e["distance_transform"] = {"call_ms": round(statistics.median(walls), 3), "passes_ms": round(statistics.median(passes), 3)}
        del labels
        for radius in args.radii:
            cap = int(radius * radius) + 1
            t = thickness(dv, solid, cap, args.reps, dst, depth)
            t["max_radius"] = radius
            e["local_thickness"].append(t)
            print(f"  max_radius {radius}: {t['stage_ms']}, kept {t['kept']}", file=sys.stderr, flush=True)
        del dst, depth
        e["thin_regions_5_ms"] = wall_ms(args.reps, lambda: dense.thin_regions(dv, solid, 5))
        e["thin_regions_17_ms"] = wall_ms(args.reps, lambda: dense.thin_regions(dv, solid, 17))
        for name in ("erode", "opening", "dilate", "closing"):
            e[name + "_4_ms"] = wall_ms(args.reps, lambda: getattr(dense, name)(dv, solid, 4))
        e["inner_distance_ms"] = wall_ms(args.reps, lambda: dense.inner_distance(dv, solid))
        e["local_thickness_f32_8_ms"] = wall_ms(args.reps, lambda: dense.local_thickness(dv, solid, 8, fmt="thickness"))
        r[str(res)] = e
        del solid
        torch.cuda.empty_cache()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
