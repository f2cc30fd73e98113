#!/usr/bin/env python3
"""Region adjacency (o2v_hip_adjacency_count / _write) on the label grids of the bench headline mesh (meshes.scan_like(), welded
into positions + faces) at each of --resolutions: the uint8 labels of fill=True with the background as a label at connectivity 6 -
two or three hot pairs -, the int32 parts of split_parts at connectivity 26 with the depth as values, and the int32 labels of
components(connectivity=6, background=True) - thousands of labels, spatially coherent; and a random label out of 2^20 per voxel at
--random-resolution - no coherence: nearly three pairs a voxel, so the table's atomics, the list and the host's sort bound it.  For
each grid: the device times of the four stages (o2v_hip_adjacency_times: table initialisation, pass, list, sort on the host), median
of --reps after a warm-up; the same with O2V_ADJ_NO_TABLE=1 (every pending pair straight to global memory, no table in LDS); the
counters; the bytes of the grid over the pass's time.  Beside them label_stats(faces=True) on the same grid (its pass reads the
same kind of rows), a device copy of the grid, and the torch route - shifted views, int64 keys, unique - with its wall time around
a synchronise and the peak memory torch allocated for it, on the grid or on its first half per axis if that does not fit; its
pairs and contact counts are compared with the call's.  One JSON object on stdout."""
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
from obj2voxel_amd.watershed import scaled_root  # noqa: E402

OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)][:13]


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def device_ms(dv, labels, n, reps, no_table, **kw):
    """The medians of the four stage times after a warm-up, the counters of a counted call and the result of the last call."""
    if no_table:
        os.environ["O2V_ADJ_NO_TABLE"] = "1"
    else:
        os.environ.pop("O2V_ADJ_NO_TABLE", None)
    try:
        ms = []
        for i in range(reps + 1):
            adj = dense.label_adjacency(dv, labels, n, **kw)
            if i:
                ms.append(dv.adjacency_times())
        nz, ny, nx = labels.shape
        values = kw.get("values")
        dv.adjacency_count(labels.data_ptr(), hip.LABELS_I32 if labels.dtype == torch.int32 else hip.LABELS_U8, dense._strides(labels), (nx, ny, nz), n,
                           kw.get("connectivity", 6), hip.FLAG_STAGE_TIMES | (hip.ADJ_ZERO if kw.get("background") else 0),
                           None if values is None else values.data_ptr(), None if values is None else dense._strides(values))
        counters = dv.adjacency_counters()
    finally:
        os.environ.pop("O2V_ADJ_NO_TABLE", None)
    return [statistics.median(m[s] for m in ms) for s in range(4)], counters, adj


def torch_route(labels, n, connectivity, background):
    """(pairs int64 [m, 2], contacts int64 [m]) by plain torch: a shifted view per earlier neighbour, an int64 key per voxel pair,
    unique."""
    top = {6: 1, 18: 2, 26: 3}[connectivity]
    lo = 0 if background else 1
    L = labels.to(torch.int64) if labels.dtype != torch.int64 else labels
    keys = []
    nz, ny, nx = L.shape
    for dx, dy, dz in OFFSETS:
        if (dx != 0) + (dy != 0) + (dz != 0) > top:
            continue
        u = L[max(0, -dz):nz - max(0, dz), max(0, -dy):ny - max(0, dy), max(0, -dx):nx - max(0, dx)]
        v = L[max(0, dz):nz - max(0, -dz), max(0, dy):ny - max(0, -dy), max(0, dx):nx - max(0, -dx)]
        on = (u != v) & (u >= lo) & (u <= n) & (v >= lo) & (v <= n)
        a, b = u[on], v[on]
        keys.append(torch.minimum(a, b) << 32 | torch.maximum(a, b))
    key, counts = torch.unique(torch.cat(keys), return_counts=True)
    return torch.stack([key >> 32, key & 0xffffffff], 1), counts


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    got = fn()
    torch.cuda.synchronize()
    return got, (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated() - base


def copy_ms(t, reps):
    out = torch.empty_like(t)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(reps + 1):
        ev[0].record()
        out.copy_(t)
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            ms.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(ms)


def bench_grid(dv, name, labels, n, reps, **kw):
    say(name, tuple(labels.shape), labels.dtype, "n =", n, {k: v for k, v in kw.items() if k != "values"})
    nbytes = labels.numel() * labels.element_size()
    r = {"shape": list(labels.shape), "dtype": str(labels.dtype).replace("torch.", ""), "n_labels": n, "GB": round(nbytes / 1e9, 3),
         "connectivity": kw.get("connectivity", 6), "background": bool(kw.get("background")), "values": kw.get("values") is not None}
    ms, counters, adj = device_ms(dv, labels, n, reps, False, **kw)
    ms0, counters0, adj0 = device_ms(dv, labels, n, reps, True, **kw)
    equal = all(torch.equal(getattr(adj, f), getattr(adj0, f)) for f in ("pairs", "faces", "edges", "corners", "pass_high", "pass_low") if getattr(adj, f) is not None)
    r.update({"pairs": int(adj.pairs.shape[0]), "contacts": int(adj.contacts.sum()), "stage_ms": [round(v, 4) for v in ms], "pass_TBps": round(nbytes / (ms[1] * 1e-3) / 1e12, 3),
              "counters": dict(zip(("to_lds", "to_global", "growths", "table_bytes"), counters)), "no_table_stage_ms": [round(v, 4) for v in ms0],
              "no_table_counters": dict(zip(("to_lds", "to_global", "growths", "table_bytes"), counters0)), "no_table_equal": equal})
    say(" ", {k: r[k] for k in ("pairs", "contacts", "stage_ms", "pass_TBps", "counters", "no_table_stage_ms", "no_table_equal")})
    ls = []
    for i in range(reps + 1):
        dense.label_stats(dv, labels, n, faces=True)
        if i:
            ls.append(sum(dv.label_stats_times()))
    r["label_stats_faces_ms"], r["copy_ms"] = round(statistics.median(ls), 4), round(copy_ms(labels, reps), 4)
    # the torch route: a small call first (it loads torch's kernels), then the wall time and the peak of its allocations
    conn, background = kw.get("connectivity", 6), bool(kw.get("background"))
    torch_route(labels[:8, :8, :8].contiguous(), n, conn, background)
    part, crop = labels, 1
    while True:
        try:
            (pairs, counts), wall, peak = timed(lambda: torch_route(part, n, conn, background))
            break
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            crop *= 2
            part = labels[:labels.shape[0] // crop, :labels.shape[1] // crop, :labels.shape[2] // crop].contiguous()
    ours = adj if crop == 1 else dense.label_adjacency(dv, part, n, connectivity=conn, background=background)
    r["torch"] = {"first_nth_per_axis": crop, "wall_ms": round(wall, 3), "peak_GB": round(peak / 1e9, 3),
                  "equal": bool(torch.equal(pairs, ours.pairs.to(torch.int64)) and torch.equal(counts, ours.contacts))}
    say("  label_stats(faces)", r["label_stats_faces_ms"], "ms, copy", r["copy_ms"], "ms, torch", r["torch"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--random-resolution", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    r = {"mesh": "scan_like", "reps": args.reps}
    for res in args.resolutions:
        lab, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
        at = r[str(res)] = {}
        at["fill_labels_u8"] = bench_grid(dv, "fill labels", lab, 2, args.reps, connectivity=6, background=True)
        parts, n = dense.split_parts(dv, lab, min_depth=2)
        depth = scaled_root(dense.inner_distance(dv, lab), 4)
        at["split_parts_i32"] = bench_grid(dv, "split_parts", parts, n, args.reps, connectivity=26, values=depth)
        del parts, depth
        cc, n = dense.components(dv, lab, connectivity=6, background=True)
        del lab
        at["background_components_i32"] = bench_grid(dv, "background components", cc, n, args.reps, connectivity=6)
        del cc
        torch.cuda.empty_cache()
    rr = args.random_resolution
    rnd = torch.randint(0, 2 ** 20, (rr, rr, rr), dtype=torch.int32, device=dev, generator=torch.Generator(device=dev).manual_seed(24))
    r["random_labels_i32"] = bench_grid(dv, "random labels", rnd, 2 ** 20 - 1, min(args.reps, 3), connectivity=6)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
