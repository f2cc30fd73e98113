#!/usr/bin/env python3
"""Blocky meshes with merge="rects" beside "none" and "runs" (o2v_hip_faces_count / _write), in one
process: the grids of tools/bench_faces.py - the surface labels, the fill=True labels and the band-3 TSDF at level 0 of the
bench headline mesh (meshes.scan_like()) at --resolution, with a constant colour and a colour grid - and two grids that have
walls at --walls: the all-solid box and the README's two cubes through solidify.  Medians of --reps, in ms: the count and write
calls on the host clock, the three stages from the events around them (o2v_hip_faces_times: classify + colour comparison, count +
scan, write), the quads and the faces per quad, the scratch bound of the mode, and for "rects" the ratio of its count + write to
those of "runs" on the same grid in the same run.  One JSON object per grid set on stdout, a line each."""
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

STAGES = ("classify", "count_scan", "write")
MERGES = (("none", hip.FACES_MERGE_NONE), ("runs", hip.FACES_MERGE_RUNS), ("rects", hip.FACES_MERGE_RECTS))


def wall(fn, reps):
    """(median wall ms of fn, the spread max - min, its last result); fn ends synchronised."""
    ms, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), max(ms) - min(ms), out


def rows(dv, name, grid, level, cname, cgrid, reps):
    """A row per merge mode of one grid and colour source."""
    dev = grid.device
    dims = (grid.shape[2] * (32 if grid.dtype == torch.int32 else 1), grid.shape[1], grid.shape[0])
    mode = hip.GATHER_COLOR_CONSTANT if cgrid is None else hip.GATHER_COLOR_GRID
    out, by_merge = [], {}
    for merge, m in MERGES:
        run = {"grid": name, "colour": cname, "merge": merge, "scratch_bytes": dv.faces_scratch_bytes(dims, mode, m)}
        kw = dict(level=level, merge=merge, colors=cgrid)
        try:
            dense.count_faces(dv, grid, **kw)   # (warm-up: the scratch is grown)
            count_ms, count_spread, n = wall(lambda: dense.count_faces(dv, grid, **kw), reps)
            count_stages = dv.faces_times()
            _, fargs, origin = dense._faces_args(dv, grid, level, (0, 0, 0), merge, 0xFFFFFFFF, cgrid, None)
            p = torch.empty((4 * n, 3), dtype=torch.float32, device=dev)
            f = torch.empty((2 * n, 3), dtype=torch.int32, device=dev)
            q = torch.empty((n,), dtype=torch.int32, device=dev)
            write_ms, write_spread, _ = wall(lambda: dv.faces_write(*fargs, origin, p.data_ptr(), f.data_ptr(), q.data_ptr(), n), reps)
            stages = dv.faces_times()
            del p, f, q
            run.update({"quads": n, "count_call_ms": round(count_ms, 3), "count_spread_ms": round(count_spread, 3),
                        "write_call_ms": round(write_ms, 3), "write_spread_ms": round(write_spread, 3),
                        "stages_ms": dict(zip(STAGES, (round(v, 4) for v in (count_stages[0], count_stages[1], stages[2]))))})
            by_merge[merge] = run
            if merge != "none" and "none" in by_merge:
                run["faces_per_quad"] = round(by_merge["none"]["quads"] / max(n, 1), 2)
            if merge == "rects" and "runs" in by_merge:
                runs = by_merge["runs"]
                run["quads_over_runs"] = round(n / max(runs["quads"], 1), 4)
                run["count_plus_write_over_runs"] = round((count_ms + write_ms) / (runs["count_call_ms"] + runs["write_call_ms"]), 2)
        except (torch.OutOfMemoryError, hip.DeviceError) as e:
            run["device_error"] = str(e)[:200]
        torch.cuda.empty_cache()
        out.append(run)
    return out


def scan_grids(dv, res):
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    surface, _ = dense.voxelize_dense(dv, res, fmt="labels")
    yield "surface labels", surface, None
    del surface
    filled, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
    yield "filled labels", filled, None
    del filled
    tsdf, _ = dense.mesh_distance(dv, res, band=3.0, signed=True)
    yield "tsdf band 3 at level 0", tsdf, 0.0


def wall_grids(dv, res):
    dev = torch.device("cuda", 0)
    yield "all-solid box", torch.ones((res, res, res), dtype=torch.uint8, device=dev), None
    c = meshes.unit_cube().reshape(-1, 9)
    s = res / 40.0                                               # the README's two cubes at 40, scaled
    dense.set_mesh(dv, torch.from_numpy(np.concatenate([c * 16 * s + 4.03 * s, c * 16 * s + 10.07 * s]).astype(np.float32)).to(dev))
    surface, _ = dense.voxelize_dense(dv, res, fmt="labels")
    yield "two cubes, solidified", dense.solidify(dv, surface), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, nargs="*", default=[1024], help="of the scan_like grids")
    ap.add_argument("--walls", type=int, nargs="*", default=[1024], help="resolution of the two grids with walls")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="only the grid of this name")
    args = ap.parse_args()
    dv = hip.DeviceVoxelizer(0)
    for kind, sizes, grids in (("scan_like", args.resolution, scan_grids), ("walls", args.walls, wall_grids)):
        for res in sizes:
            r = {"set": kind, "resolution": res, "runs": []}
            colors = torch.arange(res ** 3, dtype=torch.int32, device=torch.device("cuda", 0)).reshape(res, res, res) >> 12   # 4096 voxels a colour
            for name, grid, level in grids(dv, res):
                if args.only and name != args.only:
                    continue
                for cname, cgrid in (("constant", None), ("grid", colors)):
                    r["runs"] += rows(dv, name, grid, level, cname, cgrid, args.reps)
                del grid
                torch.cuda.empty_cache()
            del colors
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
