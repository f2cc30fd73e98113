#!/usr/bin/env python3
"""Dense grids as voxel lists and voxel files (o2v_hip_gather_count / _write / _save, dense.to_voxels / save_voxels) on grids of
the bench headline mesh (meshes.scan_like()) at --resolution: the surface labels, the fill=True labels and the band-3 TSDF at
level 0, with a constant colour and with a colour grid.  Medians of --reps, in ms: the count and write calls on the host clock, the
three stages from the events around them (o2v_hip_gather_times: classify, count + scan, write), classify against one read of the
grid at 6.29 TB/s and the write against 16 bytes per record.  Beside each the route a user takes without them, on the same tensors:

    idx = grid.nonzero()
    rec = torch.stack([idx[:, 2], idx[:, 1], idx[:, 0], colors[idx[:, 0], idx[:, 1], idx[:, 2]]], 1).to(torch.int32)

and save_voxels to VL32 against that route plus .cpu().numpy().astype(">u4").tofile(); the peak device memory of both routes.
A route that runs out of device memory is reported as such.  One JSON object on stdout."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch  # first: the library binds to the HIP runtime torch loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from obj2voxel_amd import dense, hip, meshes  # noqa: E402

HBM_TBS = 6.29   # the achievable HBM bandwidth of one MI355X, TB/s
STAGES = ("classify", "count_scan", "write")


def wall(fn, reps):
    """(median wall ms of fn, its last result); fn ends synchronised."""
    ms, out = [], None
    for _ in range(reps):
        out = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), out


def torch_route(grid, level, colors, argb):
    solid = grid < level if level is not None else grid
    idx = solid.nonzero()
    c = colors[idx[:, 0], idx[:, 1], idx[:, 2]] if colors is not None else torch.full((idx.shape[0],), argb, dtype=torch.int64, device=grid.device)
    return torch.stack([idx[:, 2], idx[:, 1], idx[:, 0], c], 1).to(torch.int32)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-save", action="store_true", help="leave the file comparison out")
    ap.add_argument("--no-lists", action="store_true", help="leave the list comparison out")
    args = ap.parse_args()
    res, reps = args.resolution, args.reps
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    surface, _ = dense.voxelize_dense(dv, res, fmt="labels")
    filled, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
    tsdf, _ = dense.mesh_distance(dv, res, band=3.0, signed=True)
    colors = torch.arange(res ** 3, dtype=torch.int32, device=dev).reshape(res, res, res)
    dims = (res,) * 3
    r = {"mesh": "scan_like", "resolution": res, "scratch_bytes": dv.gather_scratch_bytes(dims), "runs": []}
    for name, grid, level in () if args.no_lists else (("surface labels", surface, None), ("filled labels", filled, None), ("tsdf band 3 at level 0", tsdf, 0.0)):
        grid_bytes = grid.numel() * grid.element_size()
        for cname, cgrid in (("constant", None), ("grid", colors)):
            run = {"grid": name, "colour": cname}
            dense.to_voxels(dv, grid, level=level, colors=cgrid, first=0, count=0)   # (warm-up: the scratch is grown)
            count_ms, n = wall(lambda: dense.count_voxels(dv, grid, level=level), reps)
            args_, cargs = dense._gather_args(dv, grid, level, (0, 0, 0), 0xFFFFFFFF, cgrid, None)[1:]
            try:
                rec = torch.empty((n, 4), dtype=torch.int32, device=dev)
                write_ms, _ = wall(lambda: dv.gather_write(*args_, *cargs, 0, n, rec.data_ptr()), reps)
                stages = dv.gather_times()
                run.update({"records": n, "count_call_ms": round(count_ms, 3), "write_call_ms": round(write_ms, 3),
                            "stages_ms": dict(zip(STAGES, (round(v, 4) for v in stages))),
                            "classify_floor_ms": round(grid_bytes / (HBM_TBS * 1e12) * 1e3, 4),
                            "write_floor_ms": round(16 * n / (HBM_TBS * 1e12) * 1e3, 4)})
                run["classify_to_floor"] = round(stages[0] / max(run["classify_floor_ms"], 1e-9), 2)
                run["write_to_floor"] = round(stages[2] / max(run["write_floor_ms"], 1e-9), 2)
                del rec
                run["device_peak_bytes"] = peak_of(lambda: dense.to_voxels(dv, grid, level=level, colors=cgrid))
            except (torch.OutOfMemoryError, hip.DeviceError) as e:
                run["device_error"] = str(e)[:200]
            torch.cuda.empty_cache()
            try:
                torch_ms, out = wall(lambda: torch_route(grid, level, cgrid, -1), reps)
                run["torch_ms"] = round(torch_ms, 3)
                if "write_call_ms" in run:
                    run["torch_over_device"] = round(torch_ms / (run["count_call_ms"] + run["write_call_ms"]), 2)
                del out
                run["torch_peak_bytes"] = peak_of(lambda: torch_route(grid, level, cgrid, -1))
            except torch.OutOfMemoryError as e:
                run["torch_error"] = "out of device memory: " + str(e)[:120]
            torch.cuda.empty_cache()
            r["runs"].append(run)
    if not args.no_save:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "a.vl32")
            for name, grid in (("surface labels", surface), ("filled labels", filled)):
                run = {"grid": name, "file": "vl32", "colour": "grid"}
                n = dense.count_voxels(dv, grid)
                file_reps = 1 if n > 10 ** 8 else reps
                # (a voxelizer of its own: what the device holds for it afterwards is the scratch and the two record buffers)
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                free0 = torch.cuda.mem_get_info()[0]
                dv2 = hip.DeviceVoxelizer(0)
                free1 = torch.cuda.mem_get_info()[0]
                assert dense.save_voxels(dv2, grid, path, colors=colors) == n
                run["context_bytes"], run["save_device_bytes"] = free0 - free1, free1 - torch.cuda.mem_get_info()[0]
                ms, _ = wall(lambda: dense.save_voxels(dv2, grid, path, colors=colors), file_reps)
                run.update({"records": n, "save_voxels_ms": round(ms, 1), "file_bytes": os.path.getsize(path)})
                dv2.close()
                os.remove(path)
                try:
                    ms, _ = wall(lambda: torch_route(grid, None, colors, -1).cpu().numpy().astype(">u4").tofile(path), file_reps)
                    run["torch_and_numpy_ms"] = round(ms, 1)
                    run["torch_over_device"] = round(ms / run["save_voxels_ms"], 2)
                    os.remove(path)
                except (torch.OutOfMemoryError, MemoryError, OSError) as e:
                    run["torch_error"] = type(e).__name__ + ": " + str(e)[:120]
                r["runs"].append(run)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
