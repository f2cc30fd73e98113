#!/usr/bin/env python3
"""Ray casting through sparse voxel octrees and DAGs (o2v_hip_octree_raycast / o2v_hip_octree_dag_raycast, dense.octree_raycast /
dense.dag_raycast) beside dense.RayCaster on the dense grid, in the same run: the filled occupancy grid of the bench headline mesh
(meshes.scan_like(), fill=True) at 512^3 and 1024^3, the two ray sets of tools/bench_raycast.py (a 2048 x 2048 dense.camera_rays
image; 2^22 rays from seeded random points of a sphere around the box to random targets inside it), the grid as tree and as DAG,
collapsed and not, each with the ancestor stack and with O2V_TREERAY_NO_STACK=1.  Device times from the events around the kernels
(o2v_hip_octree_raycast_times, o2v_hip_raycast_times), medians of --reps after a warm-up; Mrays/s, the ratio to RayCaster.cast,
the ratio of the two variants, and the bytes each route keeps resident (the tree's or the DAG's arrays; the grid and RayCaster's
snapshot).  Every cast's hit and t are asserted equal to RayCaster's, bit for bit.  One JSON object on stdout, a table on stderr
(DESIGN.md section 35)."""
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

NO_STACK = "O2V_TREERAY_NO_STACK"


def median_ms(reps, cast, time_of):
    out = cast()   # the warm-up
    ms = []
    for _ in range(reps):
        out = cast()
        ms.append(time_of())
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--image", type=int, default=2048)
    ap.add_argument("--rays", type=int, default=1 << 22)
    args = ap.parse_args()
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    result = {"mesh": "scan_like", "reps": args.reps, "runs": []}
    rows = []
    for res in args.resolutions:
        grid, origin = dense.voxelize_dense(dv, res, fill=True)
        caster = dense.RayCaster(dv, grid, origin=origin)
        dense_bytes = grid.numel() + dv.raycast_scratch_bytes(tuple(grid.shape[::-1]))
        gen = torch.Generator(device="cpu").manual_seed(1024)
        c = res / 2.0
        eye = (c - 1.1 * res, c - 1.9 * res, c + 1.2 * res)
        cam = dense.camera_rays(args.image, args.image, eye, (c, c, c), (0.0, 0.0, 1.0), 35.0, dev)
        u = torch.randn((args.rays, 3), generator=gen, dtype=torch.float64)
        start = c + u / u.norm(dim=1, keepdim=True) * (1.2 * res)
        target = torch.rand((args.rays, 3), generator=gen, dtype=torch.float64) * res
        sphere = (start.to(torch.float32).to(dev), (target - start).to(torch.float32).to(dev))
        sources = []
        for collapse in (True, False):
            tree = dense.build_octree(dv, grid, origin=origin, collapse=collapse)
            dag = dense.octree_dag(dv, tree)
            tag = "collapsed" if collapse else "plain"
            sources.append(("tree, " + tag, 6 * len(tree.valid), lambda o, d, tree=tree: dense.octree_raycast(dv, tree, o, d, voxel_index=True)))
            sources.append(("DAG, " + tag, dag.nbytes, lambda o, d, dag=dag: dense.dag_raycast(dv, dag, o, d, voxel_index=True)))
        run = {"resolution": res, "solid_voxels": int(grid.sum()), "grid_and_snapshot_bytes": dense_bytes, "casts": []}
        for name, (o, d) in (("camera", cam), ("sphere", sphere)):
            o, d = o.reshape(-1, 3), d.reshape(-1, 3)
            n = o.shape[0]
            base_ms, want = median_ms(args.reps, lambda: caster.cast(o, d), lambda: dv.raycast_times()[1])
            entry = {"name": name, "rays": n, "hit_share": round(float((want[0][:, 0] >= 0).float().mean()), 4),
                     "raycaster": {"ms": round(base_ms, 4), "mrays_per_s": round(n / base_ms / 1e3, 1)}, "sources": []}
            rows.append((res, name, "RayCaster (grid + snapshot)", dense_bytes, base_ms, n / base_ms / 1e3, 1.0, None))
            for what, nbytes, cast in sources:
                ms = {}
                for key, off in (("stack", False), ("no_stack", True)):
                    os.environ.pop(NO_STACK, None)
                    if off:
                        os.environ[NO_STACK] = "1"
                    try:
                        ms[key], got = median_ms(args.reps, lambda: cast(o, d), lambda: dv.octree_raycast_times()[0])
                    finally:
                        os.environ.pop(NO_STACK, None)
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (res, name, what, key)
                entry["sources"].append({"source": what, "bytes": nbytes, "stack_ms": round(ms["stack"], 4), "no_stack_ms": round(ms["no_stack"], 4),
                                         "stack_mrays_per_s": round(n / ms["stack"] / 1e3, 1), "no_stack_mrays_per_s": round(n / ms["no_stack"] / 1e3, 1),
                                         "stack_over_raycaster": round(ms["stack"] / base_ms, 2), "no_stack_over_stack": round(ms["no_stack"] / ms["stack"], 2),
                                         "equals_raycaster": True})
                rows.append((res, name, what, nbytes, ms["stack"], n / ms["stack"] / 1e3, ms["stack"] / base_ms, ms["no_stack"] / ms["stack"]))
                print("%d^3, %s, %s: %.3f ms, without the stack %.3f ms, RayCaster %.3f ms" % (res, name, what, ms["stack"], ms["no_stack"], base_ms), file=sys.stderr, flush=True)
            run["casts"].append(entry)
        result["runs"].append(run)
        del caster, sources, grid, cam, sphere
        torch.cuda.empty_cache()
    print("| grid | rays | route | resident bytes | ms | Mrays/s | time / RayCaster | no stack / stack |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|", file=sys.stderr)
    for res, name, what, nbytes, ms, mrays, ratio, ab in rows:
        print("| %d^3 | %s | %s | %s | %.3f | %.0f | %.2f | %s |" % (res, name, what, format(nbytes, ",").replace(",", " "), ms, mrays, ratio, "" if ab is None else "%.2f" % ab),
              file=sys.stderr)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
