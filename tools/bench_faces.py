#!/usr/bin/env python3
"""Blocky meshes (o2v_hip_faces_count / _write, dense.voxel_faces / count_faces) on grids of the bench headline mesh
(meshes.scan_like()) at --resolution: the surface labels, the fill=True labels and the band-3 TSDF at level 0, with both merge
modes, a constant colour and a colour grid.  Medians of --reps, in ms: the count and write calls on the host clock, the three
stages from the events around them (o2v_hip_faces_times: classify, count + scan, write), classify against one read of the grid
at 6.29 TB/s and the write against the 76 bytes per quad it stores.  Beside merge="none" the route a user takes without them, on
the same tensors: a padded grid, six shifted comparisons, nonzero, a sort into the contract's order, positions from a corner
table and colours by indexing - checked against the device's result -, and the peak device memory of both routes.  A route that
runs out of device memory is reported as such.  One JSON object per resolution on stdout, a line each; the table of DESIGN.md
section 17 is `bench_faces.py --resolution 512 1024`.  (The raw faces_write call is timed apart from the allocation of its
outputs, so its arguments come from dense._faces_args, the helper voxel_faces itself uses.)"""
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

HBM_TBS = 6.29   # the achievable HBM bandwidth of one MI355X, TB/s
STAGES = ("classify", "count_scan", "write")
STEP = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def corner_table(device):
    """[6, 4, 3]: the offsets of a unit face's four corners from its voxel, in the contract's order."""
    table = np.zeros((6, 4, 3), np.float32)
    for d in range(6):
        a, s = d >> 1, d & 1
        u, v = (a + 1) % 3, (a + 2) % 3
        for k, (cu, cv) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1)) if s else ((0, 0), (0, 1), (1, 1), (1, 0))):
            table[d, k, a], table[d, k, u], table[d, k, v] = s, cu, cv
    return torch.from_numpy(table).to(device)


def torch_route(grid, level, colors, argb, corners):
    """merge="none" in plain torch: (positions [4Q, 3], faces [2Q, 3], quad_argb [Q]) as voxel_faces returns them."""
    solid = grid < level if level is not None else grid != 0
    nz, ny, nx = solid.shape
    pad = torch.nn.functional.pad(solid, (1, 1, 1, 1, 1, 1))
    idx, dirs = [], []
    for d, (dx, dy, dz) in enumerate(STEP):
        i = (solid & ~pad[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]).nonzero()
        idx.append(i)
        dirs.append(torch.full((i.shape[0],), d, dtype=torch.int64, device=grid.device))
    idx, dirs = torch.cat(idx), torch.cat(dirs)
    order = torch.argsort(((idx[:, 0] * ny + idx[:, 1]) * 6 + dirs) * nx + idx[:, 2])
    idx, dirs = idx[order], dirs[order]
    positions = (idx.flip(1).to(torch.float32)[:, None, :] + corners[dirs]).reshape(-1, 3)
    base = 4 * torch.arange(idx.shape[0], dtype=torch.int32, device=grid.device)[:, None]
    faces = (base + torch.tensor([0, 1, 2, 0, 2, 3], dtype=torch.int32, device=grid.device)).reshape(-1, 3)
    c = colors[idx[:, 0], idx[:, 1], idx[:, 2]] if colors is not None else torch.full((idx.shape[0],), argb, dtype=torch.int32, device=grid.device)
    return positions, faces, c


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
    ap.add_argument("--resolution", type=int, nargs="+", default=[1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch route out")
    args = ap.parse_args()
    for res in args.resolution:
        print(json.dumps(bench(res, args.reps, args.no_torch)), flush=True)
        torch.cuda.empty_cache()


def bench(res, reps, no_torch):
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    surface, _ = dense.voxelize_dense(dv, res, fmt="labels")
    filled, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
    tsdf, _ = dense.mesh_distance(dv, res, band=3.0, signed=True)
    colors = (torch.arange(res ** 3, dtype=torch.int32, device=dev).reshape(res, res, res) >> 12)   # 4096 voxels along x a colour
    corners = corner_table(dev)
    dims = (res,) * 3
    r = {"mesh": "scan_like", "resolution": res, "scratch_bytes": {"constant": dv.faces_scratch_bytes(dims),
                                                                   "grid": dv.faces_scratch_bytes(dims, hip.GATHER_COLOR_GRID)}, "runs": []}
    for name, grid, level in (("surface labels", surface, None), ("filled labels", filled, None), ("tsdf band 3 at level 0", tsdf, 0.0)):
        grid_bytes = grid.numel() * grid.element_size()
        for cname, cgrid in (("constant", None), ("grid", colors)):
            quads = {}
            for merge in ("none", "runs"):
                run = {"grid": name, "colour": cname, "merge": merge}
                kw = dict(level=level, merge=merge, colors=cgrid)
                try:
                    dense.count_faces(dv, grid, **kw)   # (warm-up: the scratch is grown)
                    count_ms, n = wall(lambda: dense.count_faces(dv, grid, **kw), reps)
                    quads[merge] = n
                    _, fargs, origin = dense._faces_args(dv, grid, level, (0, 0, 0), merge, 0xFFFFFFFF, cgrid, None)
                    p = torch.empty((4 * n, 3), dtype=torch.float32, device=dev)
                    f = torch.empty((2 * n, 3), dtype=torch.int32, device=dev)
                    q = torch.empty((n,), dtype=torch.int32, device=dev)
                    write_ms, _ = wall(lambda: dv.faces_write(*fargs, origin, p.data_ptr(), f.data_ptr(), q.data_ptr(), n), reps)
                    stages = dv.faces_times()
                    run.update({"quads": n, "count_call_ms": round(count_ms, 3), "write_call_ms": round(write_ms, 3),
                                "stages_ms": dict(zip(STAGES, (round(v, 4) for v in stages))),
                                "classify_floor_ms": round((grid_bytes + (4 * grid.numel() if cgrid is not None and merge == "runs" else 0)) /
                                                           (HBM_TBS * 1e12) * 1e3, 4),
                                "write_floor_ms": round(76 * n / (HBM_TBS * 1e12) * 1e3, 4)})
                    run["classify_to_floor"] = round(stages[0] / max(run["classify_floor_ms"], 1e-9), 2)
                    run["write_to_floor"] = round(stages[2] / max(run["write_floor_ms"], 1e-9), 2)
                    if merge == "runs" and "none" in quads:
                        run["faces_per_quad"] = round(quads["none"] / max(n, 1), 2)
                    del p, f, q
                    run["device_peak_bytes"] = peak_of(lambda: dense.voxel_faces(dv, grid, **kw))
                except (torch.OutOfMemoryError, hip.DeviceError) as e:
                    run["device_error"] = str(e)[:200]
                torch.cuda.empty_cache()
                if merge == "none" and not no_torch:
                    try:
                        torch_ms, out = wall(lambda: torch_route(grid, level, cgrid, -1, corners), reps)
                        run["torch_ms"] = round(torch_ms, 3)
                        if "write_call_ms" in run:
                            run["torch_over_device"] = round(torch_ms / (run["count_call_ms"] + run["write_call_ms"]), 2)
                            mine = dense.voxel_faces(dv, grid, **kw)
                            run["torch_equals_device"] = all(bool(torch.equal(a, b)) for a, b in zip(out, mine))
                            del mine
                        del out
                        run["torch_peak_bytes"] = peak_of(lambda: torch_route(grid, level, cgrid, -1, corners))
                    except torch.OutOfMemoryError as e:
                        run["torch_error"] = "out of device memory: " + str(e)[:120]
                    torch.cuda.empty_cache()
                r["runs"].append(run)
    return r


if __name__ == "__main__":
    main()
