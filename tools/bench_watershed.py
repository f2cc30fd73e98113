#!/usr/bin/env python3
"""Watershed parts (o2v_hip_watershed_dense) on the filled bench mesh (meshes.scan_like(), welded into positions + faces,
voxelize_dense(fill=True)) at --resolutions (512 and 1024): dense.split_parts as a whole (inner_distance, the scaled root, the
watershed) and dense.watershed on the stored relief, at min_depth 0 and two positive values and at 6 and 26 neighbours - ms per
call (wall, median of --reps), the stage times (o2v_hip_watershed_times: ascent, flatten, pairs, merge on the host, labels) and
the counters of one extra call with O2V_HIP_FLAG_STAGE_TIMES (peaks, boundary pairs seen, distinct adjacent pairs, table growths,
table bytes, survivors) - and the same with O2V_WS_NO_TILES=1, the ascent with its neighbours from global memory.  For scale, in
the same run: a device copy of an int32 grid of that size and dense.components on the solid.  One JSON object on stdout, progress
on stderr."""
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
from obj2voxel_amd import watershed as ws  # noqa: E402

STAGES = ("ascent", "flatten", "pairs", "merge_host", "labels")
COUNTERS = ("peaks", "boundary_pairs", "distinct_pairs", "table_growths", "table_bytes", "survivors")


def watershed(dv, relief, connectivity, steps, reps, out):
    """Wall and stage times and the counters of o2v_hip_watershed_dense on this relief."""
    dims = tuple(relief.shape[::-1])
    args = (relief.data_ptr(), dense._strides(relief), dims, connectivity, steps)
    tail = (out.data_ptr(), dense._strides(out))
    torch.cuda.synchronize()
    n = dv.watershed_dense(*args, hip.FLAG_STAGE_TIMES, *tail)   # warm-up, and the counters
    counters = dv.watershed_counters()
    walls, stages = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        dv.watershed_dense(*args, 0, *tail)
        walls.append((time.perf_counter() - t0) * 1e3)
        stages.append(dv.watershed_times())
    ms = [statistics.median(s[i] for s in stages) for i in range(5)]
    return {"call_ms": round(statistics.median(walls), 3), "stage_ms": dict(zip(STAGES, (round(v, 3) for v in ms))), "parts": n, **dict(zip(COUNTERS, counters))}


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
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--min-depths", type=float, nargs="+", default=[0.0, 1.0, 4.0], help="in voxels, as split_parts takes them")
    ap.add_argument("--skip-no-tiles", action="store_true", help="leave out the O2V_WS_NO_TILES=1 runs")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    r = {"mesh": "scan_like", "fill": True, "scale": args.scale}
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    for res in args.resolutions:
        print(f"resolution {res} ...", file=sys.stderr, flush=True)
        solid, _ = dense.voxelize_dense(dv, res, fill=True)
        relief = ws.scaled_root(dense.inner_distance(dv, solid), args.scale)
        out = torch.empty(tuple(relief.shape), dtype=torch.int32, device=dev)
        e = {"solid_voxels": int((solid != 0).sum()), "voxels": solid.numel(), "relief_max": int(relief.max()),
             "scratch_bytes": dv.watershed_scratch_bytes(tuple(solid.shape[::-1]))}
        e["copy_int32_ms"] = wall_ms(args.reps, lambda: out.copy_(relief))
        e["components_ms"] = wall_ms(args.reps, lambda: dense.components(dv, solid, connectivity=26, out=out))
        e["inner_distance_ms"] = wall_ms(args.reps, lambda: dense.inner_distance(dv, solid))
        e["scaled_root_ms"] = wall_ms(args.reps, lambda: ws.scaled_root(dense.inner_distance(dv, solid), args.scale)) - e["inner_distance_ms"]
        for connectivity in (6, 26):
            for min_depth in args.min_depths:
                steps = int(np.ceil(min_depth * args.scale))
                os.environ.pop("O2V_WS_NO_TILES", None)
                t = watershed(dv, relief, connectivity, steps, args.reps, out)
                parts = out.clone() if not args.skip_no_tiles else None
                t["split_parts_ms"] = wall_ms(args.reps, lambda: dense.split_parts(dv, solid, min_depth=min_depth, scale=args.scale, connectivity=connectivity))
                if not args.skip_no_tiles:
                    os.environ["O2V_WS_NO_TILES"] = "1"
                    t["no_tiles"] = {k: v for k, v in watershed(dv, relief, connectivity, steps, args.reps, out).items() if k in ("call_ms", "stage_ms", "parts")}
                    os.environ.pop("O2V_WS_NO_TILES", None)
                    assert torch.equal(parts, out) and t["no_tiles"]["parts"] == t["parts"]
                    del parts
                e[f"{connectivity} neighbours, min_depth {min_depth}"] = t
                print(f"  {connectivity} neighbours, min_depth {min_depth}: {t['call_ms']} ms {t['stage_ms']}, {t['peaks']} peaks, {t['distinct_pairs']} pairs, "
                      f"{t['parts']} parts; split_parts {t['split_parts_ms']} ms; no tiles {t.get('no_tiles', {}).get('call_ms')} ms "
                      f"(ascent {t.get('no_tiles', {}).get('stage_ms', {}).get('ascent')})", file=sys.stderr, flush=True)
        r[str(res)] = e
        del solid, relief, out
        torch.cuda.empty_cache()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
