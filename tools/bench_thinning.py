#!/usr/bin/env python3
"""Skeletons by topological thinning (o2v_hip_thin_dense) on the filled bench mesh (meshes.scan_like(), welded into positions +
faces, voxelize_dense(fill=True)) and on its empty space (background=True) at --resolutions (512 and 1024), in both modes
("curve", "ultimate"): ms per call (wall, median of --reps), the stage times from the events around them (o2v_hip_thin_times:
classify, iterate, write), the counters of one extra call with O2V_HIP_FLAG_STAGE_TIMES (iterations, launches, tile turns, voxels
removed), ms per iteration - and the same with O2V_THIN_NO_TILES=1, every sub-step a whole-grid sweep.  For scale dense.erode by a
ball of radius 4 (K21: two distance transforms) on the same grid from the same session.  One JSON object on stdout, progress on
stderr."""
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

MODES = {"curve": hip.THIN_CURVE, "ultimate": hip.THIN_ULTIMATE}


def thinning(dv, solid, background, mode, reps, out):
    """Wall and stage times and the counters of o2v_hip_thin_dense on this grid (uint8 mask out)."""
    dims = tuple(solid.shape[::-1])
    args = (solid.data_ptr(), hip.GRID_U8, dense._strides(solid), dims, 0.0)
    tail = (MODES[mode], 0, None, None, out.data_ptr(), dense._strides(out), hip.THIN_DST_MASK)
    flags = hip.CC_INVERT if background else 0
    torch.cuda.synchronize()
    dv.thin_dense(*args, flags | hip.FLAG_STAGE_TIMES, *tail)   # warm-up, and the counters
    iterations, launches, turns, removed = dv.thin_counters()
    walls, stages = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        dv.thin_dense(*args, flags, *tail)
        walls.append((time.perf_counter() - t0) * 1e3)
        stages.append(dv.thin_times())
    ms = [statistics.median(s[i] for s in stages) for i in range(3)]
    call = statistics.median(walls)
    return {"call_ms": round(call, 3), "stage_ms": dict(zip(("classify", "iterate", "write"), (round(v, 3) for v in ms))), "iterations": iterations,
            "launches": launches, "tile_turns": turns, "removed": removed, "skeleton_voxels": int(out.sum()), "ms_per_iteration": round(ms[1] / max(iterations, 1), 4)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-no-tiles", action="store_true", help="leave out the O2V_THIN_NO_TILES=1 runs (minutes at 1024^3)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    r = {"mesh": "scan_like", "fill": True}
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    for res in args.resolutions:
        print(f"resolution {res} ...", file=sys.stderr, flush=True)
        solid, _ = dense.voxelize_dense(dv, res, fill=True)
        out = torch.empty(tuple(solid.shape), dtype=torch.uint8, device=dev)
        e = {"solid_voxels": int(solid.sum()), "voxels": solid.numel(), "scratch_bytes": dv.thin_scratch_bytes(tuple(solid.shape[::-1]))}
        for background in (False, True):
            which = "empty_space" if background else "solid"
            e[which] = {}
            for mode in MODES:
                os.environ.pop("O2V_THIN_NO_TILES", None)
                t = thinning(dv, solid, background, mode, args.reps, out)
                if not args.skip_no_tiles:
                    os.environ["O2V_THIN_NO_TILES"] = "1"
                    t["no_tiles"] = {k: v for k, v in thinning(dv, solid, background, mode, max(1, args.reps - 1), out).items()
                                     if k in ("call_ms", "stage_ms", "iterations", "tile_turns", "ms_per_iteration", "skeleton_voxels")}
                    os.environ.pop("O2V_THIN_NO_TILES", None)
                    assert t["no_tiles"]["skeleton_voxels"] == t["skeleton_voxels"] and t["no_tiles"]["iterations"] == t["iterations"]
                e[which][mode] = t
                print(f"  {which} {mode}: {t['call_ms']} ms, {t['iterations']} iterations, {t['tile_turns']} tile turns; no tiles "
                      f"{t.get('no_tiles', {}).get('call_ms')} ms", file=sys.stderr, flush=True)
            e[which]["erode_4_ms"] = wall_ms(args.reps, lambda: dense.erode(dv, solid, 4, background=background))
        r[str(res)] = e
        del solid, out
        torch.cuda.empty_cache()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
