#!/usr/bin/env python3
"""Sparse voxel octrees (o2v_hip_octree_build / _write / _lookup / _to_dense) on the filled labels of the bench headline mesh
(meshes.scan_like(), welded into positions + faces) at every --resolutions.  For each grid, collapsed and not: the device time of
the build by stage - classify, pyramid, order, and the write into the caller's tensors - from the events around them
(o2v_hip_octree_times), median of --reps after a warm-up; the nodes per level; the bytes of the tree (6 per node: valid, full,
first_child) beside the grid (1 per voxel), its bits (1/8) and the record list (16 per solid voxel); the lookup rate for 2^24
uniform random points of the root cube and for the coordinates of to_voxels; the time of octree_to_dense, whose result is asserted
equal to the set.  Comparators: dense.count_voxels on the same grid (it reads the same bytes: classify + count, from
o2v_hip_gather_times), a device copy of the grid, and the torch route - amax / amin over reshaped 2^3 blocks per level, nonzero,
Morton keys, sort, cumsum - with its wall time around a synchronise and the peak memory torch allocated for it; its arrays are
asserted equal to the build's.  One JSON object on stdout."""
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


def build_ms(dv, grid, origin, collapse, reps):
    """(medians of classify, pyramid, order, write, their sum), the last tree"""
    ms = []
    for i in range(reps + 1):
        tree = dense.build_octree(dv, grid, origin=origin, collapse=collapse)
        if i:
            ms.append(dv.octree_times())
    return [med(m[k] for m in ms) for k in range(4)] + [med(sum(m) for m in ms)], tree


def count_ms(dv, grid, reps):
    ms = []
    for i in range(reps + 1):
        n = dense.count_voxels(dv, grid)
        if i:
            ms.append(sum(dv.gather_times()[:2]))
    return med(ms), n


def copy_ms(grid, reps):
    ms = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        c = grid.clone()
        b.record()
        torch.cuda.synchronize()
        del c
        if i:
            ms.append(a.elapsed_time(b))
    return med(ms)


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


def morton(c):
    """int64 keys of int64 cell coordinates [n, 3] = (x, y, z), z the high bit"""
    key = torch.zeros(len(c), dtype=torch.int64, device=c.device)
    for b in range(17):
        key |= ((c[:, 0] >> b & 1) | (c[:, 1] >> b & 1) << 1 | (c[:, 2] >> b & 1) << 2) << (3 * b)
    return key


def torch_route(solid, origin, D, collapse):
    """(valid, full, first_child, level counts) by plain torch: bottom up amax / amin over 2^3 blocks of the touched cells padded to even
    alignment, then per level nonzero of the cells that are nodes, Morton keys, sort, and the prefix sums of the stored children."""
    bit = 1 << torch.arange(8, device=solid.device, dtype=torch.int32)
    c_any = c_all = solid.to(torch.uint8)
    lo = torch.tensor(origin[::-1])   # (z, y, x)
    levels = []
    for l in range(D - 1, -1, -1):   # noqa: E741
        hi = lo + torch.tensor(c_any.shape)
        pl, ph = lo & 1, hi & 1
        pad = (int(pl[2]), int(ph[2]), int(pl[1]), int(ph[1]), int(pl[0]), int(ph[0]))
        c_any, c_all = torch.nn.functional.pad(c_any, pad), torch.nn.functional.pad(c_all, pad)
        kz, ky, kx = (s // 2 for s in c_any.shape)
        blocks = lambda t: t.reshape(kz, 2, ky, 2, kx, 2).permute(0, 2, 4, 1, 3, 5).reshape(kz, ky, kx, 8)   # noqa: E731
        ba, bf = blocks(c_any), blocks(c_all)
        valid, full = (ba.int() * bit).sum(-1), (bf.int() * bit).sum(-1)
        lo = (lo - pl) // 2
        c_any, c_all = ba.amax(-1), bf.amin(-1)
        node = (valid != 0) & ~(full == 255) if collapse and l else valid != 0
        if l == 0:
            node = torch.ones_like(node)
        idx = node.nonzero()
        order = torch.sort(morton((idx + lo.to(idx.device)).flip(1))).indices
        idx = idx[order]
        levels.append((valid[idx[:, 0], idx[:, 1], idx[:, 2]], full[idx[:, 0], idx[:, 1], idx[:, 2]]))
        del ba, bf, valid, full, node, idx
    levels.reverse()
    counts = [len(v) for v, _ in levels]
    firsts, offset = [], 0
    for l, (v, f) in enumerate(levels):   # noqa: E741
        offset += counts[l]
        m = v if l == D - 1 or not collapse else v & ~f
        pc = sum((m >> b & 1) for b in range(8)).long()
        ex = torch.cumsum(pc, 0) - pc
        firsts.append(ex if l == D - 1 else torch.where(m != 0, offset + ex, -1))
    return (torch.cat([v for v, _ in levels]).to(torch.uint8), torch.cat([f for _, f in levels]).to(torch.uint8), torch.cat(firsts).to(torch.int32), counts)


def bench_grid(dv, res, labels, origin, reps, rec_lookup):
    dev = labels.device
    solid = labels != 0
    voxels = labels.numel()
    t_count, n_solid = count_ms(dv, labels, reps)
    r = {"shape": list(labels.shape), "origin": list(origin), "solid_voxels": n_solid, "count_voxels_ms": t_count, "copy_ms": copy_ms(labels, reps),
         "grid_MB": round(voxels / 1e6, 1), "bits_MB": round(voxels / 8e6, 1), "records_MB": round(16 * n_solid / 1e6, 1)}
    say(f"labels at {res}", r)
    gen = torch.Generator(device=dev).manual_seed(26)
    for collapse in (True, False):
        name = "collapsed" if collapse else "not_collapsed"
        (t_cl, t_py, t_or, t_wr, t_all), tree = build_ms(dv, labels, origin, collapse, reps)
        counts = [b - a for a, b in zip(tree.level_offsets, tree.level_offsets[1:])]
        nodes = len(tree.valid)
        q = {"depth": tree.depth, "nodes_per_level": counts, "nodes": nodes, "voxels_listed": tree.voxels_listed, "tree_MB": round(6 * nodes / 1e6, 2),
             "classify_ms": t_cl, "pyramid_ms": t_py, "order_ms": t_or, "write_ms": t_wr, "build_ms": t_all, "build_over_count_voxels": round(t_all / t_count, 2),
             "build_wall_ms": wall_ms(lambda: dense.build_octree(dv, labels, origin=origin, collapse=collapse), reps)[0]}
        pts = torch.randint(0, 2 ** tree.depth, (2 ** 24, 3), dtype=torch.int32, device=dev, generator=gen)
        t_lk, hit = wall_ms(lambda: dense.octree_lookup(dv, tree, pts), reps)
        o3 = torch.tensor(origin, dtype=torch.int32, device=dev)
        p = (pts - o3).long()
        inside = ((p >= 0) & (p < torch.tensor(labels.shape[::-1], device=dev))).all(1)
        want = torch.zeros(len(pts), dtype=torch.bool, device=dev)
        want[inside] = solid[p[inside, 2], p[inside, 1], p[inside, 0]]
        assert torch.equal(hit[:, 0] == 1, want), "lookup differs from the grid"
        q["lookup_random_2^24_ms"], q["lookup_random_Mpoints_per_s"] = t_lk, round(2 ** 24 / t_lk / 1e3, 1)
        del pts, hit, p, inside, want
        if rec_lookup:
            rec = dense.to_voxels(dv, labels, origin=origin)[:, :3].contiguous()
            t_rec, hit = wall_ms(lambda: dense.octree_lookup(dv, tree, rec), max(1, reps // 2))
            assert bool((hit[:, 0] == 1).all()), "a solid voxel is not solid in the tree"
            q["lookup_records_ms"], q["lookup_records_Mpoints_per_s"] = t_rec, round(len(rec) / t_rec / 1e3, 1)
            del rec, hit
        t_dense, back = wall_ms(lambda: dense.octree_to_dense(dv, tree, labels.shape, origin=origin), reps)
        assert torch.equal(back, solid), "to_dense differs from the set"
        q["to_dense_ms"] = t_dense
        del back
        torch_route(solid[:8, :8, :8].contiguous(), (0, 0, 0), 3, collapse)   # (a small call first: it loads torch's kernels)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        v, f, fc, tc = torch_route(solid, origin, tree.depth, collapse)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        assert tc == counts and torch.equal(v, tree.valid) and torch.equal(f, tree.full) and torch.equal(fc, tree.first_child), "the torch route's tree differs"
        q["torch"] = {"wall_ms": round(wall, 2), "peak_GB": round((torch.cuda.max_memory_allocated() - base) / 1e9, 2), "equal": True,
                      "times_the_build": round(wall / q["build_wall_ms"], 1)}
        del v, f, fc, tree
        torch.cuda.empty_cache()
        say(" ", name, q)
        r[name] = q
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-record-lookup", action="store_true", help="leave the lookup of the to_voxels coordinates out")
    args = ap.parse_args()
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    r = {"mesh": "scan_like", "reps": args.reps, "grids": {}}
    for res in args.resolutions:
        lab, origin = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
        r["grids"][f"fill_labels_u8_{res}"] = bench_grid(dv, res, lab, tuple(int(v) for v in origin), args.reps, not args.no_record_lookup)
        del lab
        torch.cuda.empty_cache()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
