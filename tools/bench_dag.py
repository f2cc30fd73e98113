#!/usr/bin/env python3
"""Sparse voxel DAGs (o2v_hip_octree_dag_build / _write / _lookup / _to_dense) on the octrees of the filled labels of the bench
headline mesh (meshes.scan_like(), welded into positions + faces) at every --resolutions, collapsed and not.  The method is
tools/bench_octree.py's: device times from the events around the stages (o2v_hip_octree_dag_times: the merge of level D - 1, the
merge of the levels above, the output, the write), medians of --reps after a warm-up; wall times around a synchronise for the
queries.  Per grid: the tree's nodes per level and bytes (6 per node) beside the DAG's nodes per level, pointers and bytes (6 per
node, 8 per pointer; 4 without skips); the merge as a ratio to build_octree, measured in the same run; dag_lookup and dag_to_dense
beside octree_lookup and octree_to_dense on the same points and boxes, their results asserted equal.  The all-solid 512^3 grid,
not collapsed, is the contended case: every key of a level is equal.  Comparator: the torch route - torch.unique(dim=0) over the
keys (valid, full, eight child ids), level by level, the classes reordered by their first index - with its wall time and the peak
memory torch allocated for it; its class counts are asserted equal to the build's.  One JSON object on stdout."""
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


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def med(v):
    return round(statistics.median(v), 4)


def wall_ms(fn, reps):
    ms = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i:
            ms.append((time.perf_counter() - t0) * 1e3)
    return med(ms), out


def tree_ms(dv, grid, origin, collapse, reps):
    """(the median of build_octree's device time: classify + pyramid + order + write), the last tree"""
    ms = []
    for i in range(reps + 1):
        tree = dense.build_octree(dv, grid, origin=origin, collapse=collapse)
        if i:
            ms.append(sum(dv.octree_times()))
    return med(ms), tree


def dag_ms(dv, tree, reps):
    """(medians of the merge of level D - 1, of the levels above, the output, the write, their sum), the last DAG"""
    ms = []
    for i in range(reps + 1):
        dag = dense.octree_dag(dv, tree)
        if i:
            ms.append(dv.octree_dag_times())
    return [med(m[k] for m in ms) for k in range(4)] + [med(sum(m) for m in ms)], dag


def torch_route(tree):
    """The classes per level by plain torch: torch.unique(dim=0) over the keys of a level, bottom up, the classes numbered by their
    first index (scatter_reduce amin, argsort)."""
    D, off, dev = tree.depth, tree.level_offsets, tree.valid.device
    shifts = torch.arange(8, device=dev)
    ids, counts = None, [0] * D
    for l in range(D - 1, -1, -1):   # noqa: E741
        a, b = off[l], off[l + 1]
        n = b - a
        if not n:
            ids = torch.zeros(0, dtype=torch.int64, device=dev)
            continue
        v, f = tree.valid[a:b].long(), tree.full[a:b].long()
        if l == D - 1:
            keys = v[:, None]
        else:
            m = v & ~f if tree.collapsed else v
            bits = (m[:, None] >> shifts) & 1
            child = tree.first_child[a:b].long()[:, None] + torch.cumsum(bits, 1) - bits - off[l + 1]
            below = ids[child.clamp_(0, max(len(ids) - 1, 0))] if len(ids) else torch.zeros_like(child)
            keys = torch.cat([v[:, None], f[:, None], torch.where(bits == 1, below, -1)], 1)
            del bits, child, below
        uniq, inverse = torch.unique(keys, dim=0, return_inverse=True)
        first = torch.full((len(uniq),), n, dtype=torch.int64, device=dev).scatter_reduce_(0, inverse, torch.arange(n, device=dev), "amin")
        rank = torch.empty_like(first)
        rank[torch.argsort(first)] = torch.arange(len(uniq), device=dev)
        ids, counts[l] = rank[inverse], len(uniq)
        del keys, uniq, inverse, first, rank
    return counts


def bench_tree(dv, name, grid, origin, collapse, reps, n_points, torch_nodes):
    dev = grid.device
    t_tree, tree = tree_ms(dv, grid, origin, collapse, reps)
    (t_leaf, t_up, t_out, t_wr, t_all), dag = dag_ms(dv, tree, reps)
    tree_counts = [b - a for a, b in zip(tree.level_offsets, tree.level_offsets[1:])]
    dag_counts = [b - a for a, b in zip(dag.level_offsets, dag.level_offsets[1:])]
    N, M, P = len(tree.valid), len(dag.valid), len(dag.child)
    q = {"depth": tree.depth, "tree_nodes_per_level": tree_counts, "tree_nodes": N, "tree_MB": round(6 * N / 1e6, 3), "dag_nodes_per_level": dag_counts,
         "dag_nodes": M, "dag_pointers": P, "dag_MB": round(dag.nbytes / 1e6, 3), "dag_MB_without_skips": round((dag.nbytes - 4 * P) / 1e6, 3),
         "dag_over_tree_bytes": round(dag.nbytes / (6 * N), 4), "voxels_listed": tree.voxels_listed,
         "merge_last_level_ms": t_leaf, "merge_levels_above_ms": t_up, "output_ms": t_out, "write_ms": t_wr, "dag_ms": t_all, "build_octree_ms": t_tree,
         "dag_over_build_octree": round(t_all / t_tree, 2), "scratch_MB": round(hip.octree_dag_scratch_bytes(tree_counts, tree.depth) / 1e6, 1),
         "dag_wall_ms": wall_ms(lambda: dense.octree_dag(dv, tree), reps)[0]}
    gen = torch.Generator(device=dev).manual_seed(30)
    pts = torch.randint(0, 2 ** tree.depth, (n_points, 3), dtype=torch.int32, device=dev, generator=gen)
    t_tl, of_tree = wall_ms(lambda: dense.octree_lookup(dv, tree, pts), reps)
    t_dl, of_dag = wall_ms(lambda: dense.dag_lookup(dv, dag, pts), reps)
    assert torch.equal(of_dag[:, [0, 1, 3]], of_tree[:, [0, 1, 3]]), "dag_lookup differs from octree_lookup"
    q["octree_lookup_ms"], q["dag_lookup_ms"], q["dag_lookup_Mpoints_per_s"] = t_tl, t_dl, round(n_points / t_dl / 1e3, 1)
    del pts, of_tree, of_dag
    shape = tuple(grid.shape)
    t_td, a = wall_ms(lambda: dense.octree_to_dense(dv, tree, shape, origin=origin), reps)
    t_dd, b = wall_ms(lambda: dense.dag_to_dense(dv, dag, shape, origin=origin), reps)
    assert torch.equal(a, b), "dag_to_dense differs from octree_to_dense"
    q["octree_to_dense_ms"], q["dag_to_dense_ms"] = t_td, t_dd
    del a, b
    if N <= torch_nodes:
        small = dense.build_octree(dv, torch.ones((8, 8, 8), dtype=torch.bool, device=dev), collapse=False)
        torch_route(small)   # (a small call first: it loads torch's kernels)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        counts = torch_route(tree)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        assert counts == dag_counts, ("the torch route's classes differ", counts, dag_counts)
        q["torch"] = {"wall_ms": round(wall, 2), "peak_GB": round((torch.cuda.max_memory_allocated() - base) / 1e9, 2), "counts_equal": True,
                      "times_the_dag": round(wall / q["dag_wall_ms"], 1)}
    del tree, dag
    torch.cuda.empty_cache()
    say(" ", name, q)
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=2 ** 24, help="random points of the root cube per lookup")
    ap.add_argument("--solid", type=int, default=512, help="the side of the all-solid grid of the contended case; 0: leave it out")
    ap.add_argument("--torch-nodes", type=int, default=2 ** 31, help="the torch route only for trees of at most this many nodes")
    args = ap.parse_args()
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    r = {"mesh": "scan_like", "reps": args.reps, "points": args.points, "grids": {}}
    for res in args.resolutions:
        lab, origin = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
        origin = tuple(int(v) for v in origin)
        g = {"shape": list(lab.shape), "origin": list(origin)}
        say(f"labels at {res}", g)
        for collapse in (True, False):
            name = "collapsed" if collapse else "not_collapsed"
            g[name] = bench_tree(dv, name, lab, origin, collapse, args.reps, args.points, args.torch_nodes)
        r["grids"][f"fill_labels_u8_{res}"] = g
        del lab
        torch.cuda.empty_cache()
    if args.solid:
        n = args.solid
        one = torch.ones((1, 1, 1), dtype=torch.uint8, device=dev).expand(n, n, n)   # (one byte, expanded: every read is a cache hit)
        say(f"all solid at {n}")
        r["all_solid_%d_not_collapsed" % n] = bench_tree(dv, "not_collapsed", one, (0, 0, 0), False, args.reps, args.points, args.torch_nodes)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
