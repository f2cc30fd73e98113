#!/usr/bin/env python3
"""Euler numbers (o2v_hip_euler_stats) on label grids of the bench headline mesh (meshes.scan_like(), welded into positions +
faces) at every --resolutions: the uint8 labels of fill=True - three hot rows -, the int32 labels of components(connectivity=6,
background=True) and the int32 labels of split_parts - thousands of labels, spatially coherent -, and a random label out of 2^20
per voxel at --random-resolution - no coherence, the regime that global atomics bound.  For each grid: the device time of the
table's initialisation and of the pass from the events around them (o2v_hip_euler_stats_times), median of --reps after a warm-up;
the same with O2V_EU_NO_TABLE=1 (every row straight to global memory, no table in LDS); label_stats(faces=True), the nearest
existing pass; a device copy of the grid; and the torch route - eight shifted views of the padded grid, a sort over the views that a
cell touches and a bincount per cell type, in slabs of --slab lattice planes so that its int64 stacks fit - with its wall time
around a synchronise and the peak memory torch allocated for it; its table is asserted equal to the call's.  The Betti numbers of
the filled mesh at the first resolution.  One JSON object on stdout."""
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

# (closed-in column, inner column or None, the window positions b = i + 2 j + 4 k that the cell touches): include/o2v_hip.h
WINDOW_CELLS = ((3, 6, 0xff), (2, 5, 0xaa), (2, 5, 0xcc), (2, 5, 0xf0), (1, 4, 0x88), (1, 4, 0xa0), (1, 4, 0xc0), (0, None, 0x80))


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def table_of(s):
    return torch.stack([s.voxels, s.faces, s.edges, s.vertices, s.inner_faces, s.inner_edges, s.inner_vertices], dim=1)


def device_ms(dv, labels, n, reps, no_table):
    """(median of init + pass, median init, median pass, min, max) of the call's device time after a warm-up; the last table."""
    if no_table:
        os.environ["O2V_EU_NO_TABLE"] = "1"
    else:
        os.environ.pop("O2V_EU_NO_TABLE", None)
    try:
        ms = []
        for i in range(reps + 1):
            st = dense.euler_stats(dv, labels, n)
            if i:
                ms.append(dv.euler_stats_times())
    finally:
        os.environ.pop("O2V_EU_NO_TABLE", None)
    total = [a + b for a, b in ms]
    return (statistics.median(total), statistics.median(m[0] for m in ms), statistics.median(m[1] for m in ms), min(total), max(total)), table_of(st)


def faces_ms(dv, labels, n, reps):
    ms = []
    for i in range(reps + 1):
        dense.label_stats(dv, labels, n, box=False, sums=False, faces=True)
        if i:
            ms.append(sum(dv.label_stats_times()))
    return statistics.median(ms)


def copy_ms(labels, reps):
    ms = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        c = labels.clone()
        b.record()
        torch.cuda.synchronize()
        del c
        if i:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def torch_route(labels, n, slab):
    """The table [n + 1, 7] by plain torch: the window form of the definition, a slab of lattice planes at a time."""
    nz, ny, nx = labels.shape
    table = torch.zeros((n + 1, 7), dtype=torch.int64, device=labels.device)
    for z0 in range(0, nz + 1, slab):
        z1 = min(nz + 1, z0 + slab)                                   # the lattice planes vz = z0 ... z1 - 1 see the voxel planes z0 - 1 ... z1 - 1
        v = labels[max(z0 - 1, 0):min(z1, nz)].to(torch.int64)
        v = torch.where((v < 0) | (v > n), -1, v)
        pad = torch.nn.functional.pad(v, (1, 1, 1, 1, 1 if z0 == 0 else 0, 1 if z1 == nz + 1 else 0), value=-1)
        planes = z1 - z0
        P = [pad[k:k + planes, j:j + ny + 1, i:i + nx + 1].reshape(-1) for k in (0, 1) for j in (0, 1) for i in (0, 1)]
        for closed, inner, mask in WINDOW_CELLS:
            s = torch.sort(torch.stack([P[b] for b in range(8) if mask >> b & 1]), dim=0).values
            first = torch.ones_like(s, dtype=torch.bool)
            first[1:] = s[1:] != s[:-1]
            first &= s >= 0
            table[:, closed] += torch.bincount(s[first], minlength=n + 1)
            if inner is not None:
                same = (s[0] == s[-1]) & (s[0] >= 0)
                table[:, inner] += torch.bincount(s[0][same], minlength=n + 1)
            del s, first
        del P, pad, v
    return table


def timed_torch(labels, n, slab):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    got = torch_route(labels, n, slab)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return got, wall, torch.cuda.max_memory_allocated() - base


def bench_grid(dv, name, labels, n, reps, slab):
    say(name, tuple(labels.shape), labels.dtype, "n =", n)
    nbytes = labels.numel() * labels.element_size()
    r = {"shape": list(labels.shape), "dtype": str(labels.dtype).replace("torch.", ""), "n_labels": n, "GB": round(nbytes / 1e9, 3)}
    (t, t_init, t_pass, lo, hi), table = device_ms(dv, labels, n, reps, False)
    (t0, _, _, lo0, hi0), table0 = device_ms(dv, labels, n, reps, True)
    r["euler_stats"] = {"device_ms": round(t, 4), "init_ms": round(t_init, 4), "pass_ms": round(t_pass, 4), "device_ms_min_max": [round(lo, 4), round(hi, 4)],
                        "TBps": round(nbytes / (t * 1e-3) / 1e12, 3), "no_table_ms": round(t0, 4), "no_table_ms_min_max": [round(lo0, 4), round(hi0, 4)],
                        "no_table_equal": bool(torch.equal(table, table0))}
    r["label_stats_faces_ms"] = round(faces_ms(dv, labels, n, reps), 4)
    r["ratio_to_label_stats_faces"] = round(t / r["label_stats_faces_ms"], 3)
    r["copy_ms"] = round(copy_ms(labels, reps), 4)
    r["labels_with_voxels"] = int((table[:, 0] > 0).sum())
    say(" ", {k: r[k] for k in ("euler_stats", "label_stats_faces_ms", "copy_ms")})
    torch_route(labels[:8, :8, :8].contiguous(), n, slab)   # (a small call first: it loads torch's kernels)
    got, wall, peak = timed_torch(labels, n, slab)
    assert torch.equal(got, table), name + ": the torch route's table differs from o2v_hip_euler_stats'"
    r["torch"] = {"slab": slab, "wall_ms": round(wall, 3), "peak_GB": round(peak / 1e9, 3), "equal": True, "times_the_pass": round(wall / t, 1)}
    say("  torch", r["torch"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--random-resolution", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slab", type=int, default=32)
    ap.add_argument("--no-parts", action="store_true", help="leave the split_parts grids out")
    args = ap.parse_args()
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    r = {"mesh": "scan_like", "reps": args.reps, "grids": {}}
    for res in args.resolutions:
        lab, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
        if "betti" not in r:
            t0 = time.perf_counter()
            r["betti"] = {"resolution": res, "b0_b1_b2_at_26": list(dense.betti_numbers(dv, lab)), "b0_b1_b2_at_6": list(dense.betti_numbers(dv, lab, connectivity=6))}
            torch.cuda.synchronize()
            r["betti"]["wall_ms_both"] = round((time.perf_counter() - t0) * 1e3, 1)
            say("betti", r["betti"])
        r["grids"][f"fill_labels_u8_{res}"] = bench_grid(dv, f"fill labels at {res}", lab, 2, args.reps, args.slab)
        cc, n = dense.components(dv, lab, connectivity=6, background=True)
        r["grids"][f"background_components_i32_{res}"] = bench_grid(dv, f"background components at {res}", cc, n, args.reps, args.slab)
        del cc
        if not args.no_parts:
            parts, n = dense.split_parts(dv, lab, min_depth=2)
            r["grids"][f"split_parts_i32_{res}"] = bench_grid(dv, f"split_parts at {res}", parts, n, args.reps, args.slab)
            del parts
        del lab
        torch.cuda.empty_cache()
    rr = args.random_resolution
    rnd = torch.randint(0, 2 ** 20, (rr, rr, rr), dtype=torch.int32, device=dev, generator=torch.Generator(device=dev).manual_seed(25))
    r["grids"][f"random_labels_i32_{rr}"] = bench_grid(dv, f"random labels at {rr}", rnd, 2 ** 20 - 1, args.reps, args.slab)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
