#!/usr/bin/env python3
"""Geodesic distances (o2v_hip_geodesic_dense, dense.geodesic_distance) on one MI355X: (a) the empty space of the filled labels of
the bench headline mesh (meshes.scan_like(), fmt="labels", fill=True) at 1024^3, from the border, chamfer (3, 4, 5) - the drain
depth; (b) its solid from one seed, chamfer and hops at connectivity 6; (c) a serpentine at 256^3 from its first voxel, hops at 6 -
the round-count worst case.  Medians of --reps, in ms, from the events around the stages (o2v_hip_geodesic_times: classify, init +
seeds, propagation, write), with the tile pass and with O2V_GEO_NO_TILES=1, and the rounds, tile visits, in-tile sweeps and host
reads of one more call made with the counters on; beside them the floor of a call - the grid read once, the bits written and read,
the distances written once and read once, at the 6.1 TB/s of a streaming copy - and the torch route: torch.minimum over the
shifted views of a padded tensor, pass after pass to the fixed point, checked equal.  A run that would take minutes is cut off and
says so: the whole-grid sweeps and the torch route on (c) run under a max_distance / a pass limit, and their full time is the
stated lower bound passes x time per pass.  One JSON object on stdout."""
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
from tests import components_ref, geodesic_ref  # noqa: E402

STREAM_TBS = 6.1   # a streaming copy on one MI355X, TB/s (the guide's 6.0 - 6.2)
STAGES = ("classify", "init_seeds", "propagation", "write")


def measure(dv, call, reps):
    call()   # (warm-up: the scratch is grown)
    ms = []
    for _ in range(reps):
        call()
        ms.append(dv.geodesic_times())
    stages = [statistics.median(m[i] for m in ms) for i in range(4)]
    return {"ms": round(sum(stages), 4), "stages_ms": dict(zip(STAGES, (round(v, 4) for v in stages)))}


def torch_route(S, weights, seed_mask, limit_s, limit_passes):
    """(dist or None, passes, seconds, done): the relaxation with torch.minimum over up to 26 shifted views of a padded int32 tensor,
    a full-grid pass at a time, until nothing changes or a limit is reached."""
    big = 1 << 29
    nz, ny, nx = S.shape
    P = torch.full((nz + 2, ny + 2, nx + 2), big, dtype=torch.int32, device=S.device)
    core = P[1:-1, 1:-1, 1:-1]
    core[seed_mask] = 0
    offs = geodesic_ref.offsets(weights)
    floor = (~S).to(torch.int32) * big
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    passes, done = 0, False
    while not done and passes < limit_passes and time.perf_counter() - t0 < limit_s:
        new = core.clone()
        for dx, dy, dz, w in offs:
            new = torch.minimum(new, P[1 + dz:nz + 1 + dz, 1 + dy:ny + 1 + dy, 1 + dx:nx + 1 + dx] + w)
        new = torch.maximum(new, floor)
        done = bool(torch.equal(new, core))
        core.copy_(new)
        passes += 1
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    return (torch.where(core >= big, -1, core) if done else None), passes, seconds, done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--serpentine", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-seconds", type=float, default=60.0, help="the torch route of a set is cut off after this long")
    ap.add_argument("--sets", default="abc")
    args = ap.parse_args()
    res, reps = args.resolution, args.reps
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    r = {"mesh": "scan_like", "resolution": res, "serpentine": args.serpentine, "reps": reps, "runs": [],
         "scratch_bytes": {"contiguous": dv.geodesic_scratch_bytes((res,) * 3), "strided": dv.geodesic_scratch_bytes((res,) * 3, hip.GEO_SCRATCH_STRIDED)}}
    sets = []
    if "a" in args.sets or "b" in args.sets:
        verts = meshes.scan_like()
        positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
        dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
        labels, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
        layer = torch.nonzero(labels[res // 2])
        seed = [(int(layer[len(layer) // 2][1]), int(layer[len(layer) // 2][0]), res // 2)]
        r["solid_voxels"], r["seed"] = int((labels != 0).sum()), seed[0]
        if "a" in args.sets:
            sets.append(("a: the air from the border, chamfer", labels, (3, 4, 5), None, True, True, None))
        if "b" in args.sets:
            sets.append(("b: the solid from one seed, chamfer", labels, (3, 4, 5), seed, False, False, None))
            sets.append(("b: the solid from one seed, hops at 6", labels, (1, 0, 0), seed, False, False, None))
    if "c" in args.sets:
        n = args.serpentine
        serp = torch.from_numpy(components_ref.serpentine((n, n, n))).to(dev)
        sets.append(("c: the serpentine, hops at 6", serp, (1, 0, 0), [(0, 0, 0)], False, False, 2000))
    for name, grid, weights, seeds, border, background, sweep_cap in sets:
        shape = tuple(grid.shape)
        voxels = grid.numel()
        out = torch.empty(shape, dtype=torch.int32, device=dev)
        sd = None if seeds is None else torch.tensor(seeds, dtype=torch.int32, device=dev)
        floor = voxels * (1 + 2 / 8 + 4 + 4) / (STREAM_TBS * 1e12) * 1e3
        flags = (hip.CC_INVERT if background else 0) | (hip.CC_SEED_BORDER if border else 0) | hip.FLAG_STAGE_TIMES
        results = {}
        for mode in ("tiles", "no_tiles"):
            if mode == "no_tiles":
                os.environ["O2V_GEO_NO_TILES"] = "1"
            try:
                # the whole-grid sweeps need a sweep per voxel of a one-voxel path: under a cap, and extrapolated
                cap = sweep_cap if mode == "no_tiles" else None
                run = {"set": name, "mode": mode, "weights": weights, "voxels": voxels, "floor_ms": round(floor, 3)}
                run.update(measure(dv, lambda: dense.geodesic_distance(dv, grid, sd, border=border, weights=weights, background=background, max_distance=cap,
                                                                       out=out), 1 if cap else reps))
                torch.cuda.synchronize()
                run["reached"] = dv.geodesic_dense(grid.data_ptr(), hip.GRID_U8, dense._strides(grid), shape[::-1], 0.0, weights, flags,
                                                   sd.data_ptr() if sd is not None else None, 0 if sd is None else len(sd),
                                                   hip.GEO_MAX_DISTANCE if cap is None else cap, out.data_ptr(), dense._strides(out))
                run["rounds"], run["tile_visits"], run["tile_sweeps"], run["host_reads"] = dv.geodesic_counters()
                run["max_distance"] = int(out.max())
                run["ratio_to_floor"] = round(run["ms"] / floor, 1)
                if cap:
                    full = results["tiles"]["max_distance"] + 1      # a sweep per voxel of the path
                    run["cut_off_at_max_distance"] = cap
                    run["lower_bound_ms_of_the_full_run"] = round(run["stages_ms"]["propagation"] / run["rounds"] * full, 0)
                else:
                    results[mode + " dist"] = out.clone()
                results[mode] = run
                r["runs"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
            finally:
                os.environ.pop("O2V_GEO_NO_TILES", None)
        if "no_tiles dist" in results:
            assert torch.equal(results["tiles dist"], results["no_tiles dist"]), name
        # the torch route
        S = (grid == 0) if background else (grid != 0)
        seed_mask = torch.zeros(shape, dtype=torch.bool, device=dev)
        if seeds is not None:
            for x, y, z in seeds:
                seed_mask[z, y, x] = True
        if border:
            seed_mask[[0, -1]] = True
            seed_mask[:, [0, -1]] = True
            seed_mask[:, :, [0, -1]] = True
        seed_mask &= S
        dist, passes, seconds, done = torch_route(S, weights, seed_mask, args.torch_seconds, 400 if sweep_cap else 1 << 30)
        run = {"set": name, "mode": "torch", "passes": passes, "ms": round(seconds * 1e3, 1), "ms_per_pass": round(seconds * 1e3 / max(passes, 1), 2), "fixed_point": done}
        if done:
            run["equal"] = bool(torch.equal(dist, results["tiles dist"]))
            assert run["equal"], name
        else:
            full = results["tiles"]["max_distance"] // max(weights) + 1      # at least a pass per step of the longest path
            run["lower_bound_ms_of_the_full_run"] = round(run["ms_per_pass"] * full, 0)
        r["runs"].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)
        del dist, S, seed_mask, results, out
    r["host_copy_ms_of_a_float_grid_measured_by_k10"] = 77
    print(json.dumps(r))


if __name__ == "__main__":
    main()
