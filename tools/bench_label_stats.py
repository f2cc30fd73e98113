#!/usr/bin/env python3
"""Per-label statistics (o2v_hip_label_stats) on three label grids: the int32 labels of components(connectivity=6,
background=True) of the bench headline mesh (meshes.scan_like(), welded into positions + faces) filled at --resolution - thousands
of labels, spatially coherent -, the uint8 labels of fill=True of the same mesh - three hot rows -, and a random label out of 2^20
per voxel at --random-resolution - no coherence, the regime that global atomics bound.  For each grid and for count + box + sums,
the same with moments and the same with faces: the device time from the events around the call's two launches
(o2v_hip_label_stats_times), median of --reps after a warm-up; the same with O2V_LS_NO_TABLE=1 (every run straight to global memory,
no table in LDS); the bytes of the grid over the time, and as a share of the 6.3 TB/s a device copy reaches on the MI355X.  And
the torch route to count, box and sums - bincount, scatter_reduce amin / amax over three int64 coordinate grids, bincount with
float64 weights - with its wall time around a synchronise and the peak memory torch allocated for it, at --resolution, or on every
second voxel per axis if that does not fit; its results are compared with the call's.  One JSON object on stdout (DESIGN.md
section 22)."""
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

COPY_TBPS = 6.3   # the measured device copy of the MI355X
REQUESTS = (("count_box_sums", {}), ("with_moments", dict(moments=True)), ("with_faces", dict(faces=True)))


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def device_ms(dv, labels, n, reps, no_table, **kw):
    """(median, min, max) of the call's device time, both launches, after a warm-up; the statistics of the last call."""
    if no_table:
        os.environ["O2V_LS_NO_TABLE"] = "1"
    else:
        os.environ.pop("O2V_LS_NO_TABLE", None)
    try:
        ms = []
        for i in range(reps + 1):
            st = dense.label_stats(dv, labels, n, **kw)
            if i:
                ms.append(sum(dv.label_stats_times()))
    finally:
        os.environ.pop("O2V_LS_NO_TABLE", None)
    return (statistics.median(ms), min(ms), max(ms)), st


def torch_route(labels, n):
    """(count, lo, hi exclusive, sums) as label_stats gives them, by plain torch."""
    nz, ny, nx = labels.shape
    idx = labels.reshape(-1).to(torch.int64)
    dev = labels.device
    z, y, x = torch.meshgrid(torch.arange(nz, device=dev), torch.arange(ny, device=dev), torch.arange(nx, device=dev), indexing="ij")
    count = torch.bincount(idx, minlength=n + 1)
    lo, hi, sums = [], [], []
    for c in (x, y, z):
        c = c.reshape(-1)
        lo.append(torch.full((n + 1,), 2 ** 31 - 1, dtype=torch.int64, device=dev).scatter_reduce(0, idx, c, "amin"))
        hi.append(torch.full((n + 1,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, idx, c, "amax"))
        sums.append(torch.bincount(idx, weights=c.to(torch.float64), minlength=n + 1))
    some = (count > 0)[:, None]
    return count, torch.where(some, torch.stack(lo, 1), 0), torch.where(some, torch.stack(hi, 1) + 1, 0), torch.stack(sums, 1)


def timed_torch(labels, n):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    got = torch_route(labels, n)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return got, wall, torch.cuda.max_memory_allocated() - base


def bench_grid(dv, name, labels, n, reps, torch_reps):
    say(name, tuple(labels.shape), labels.dtype, "n =", n)
    nbytes = labels.numel() * labels.element_size()
    r = {"shape": list(labels.shape), "dtype": str(labels.dtype).replace("torch.", ""), "n_labels": n, "GB": round(nbytes / 1e9, 3)}
    for what, kw in REQUESTS:
        (t, lo, hi), st = device_ms(dv, labels, n, reps, False, **kw)
        (t0, lo0, hi0), st0 = device_ms(dv, labels, n, reps, True, **kw)
        same = all(torch.equal(getattr(st, f), getattr(st0, f)) for f in ("count", "lo", "hi", "sum", "moment", "faces") if getattr(st, f) is not None)
        tbps = nbytes / (t * 1e-3) / 1e12
        r[what] = {"device_ms": round(t, 4), "device_ms_min_max": [round(lo, 4), round(hi, 4)], "TBps": round(tbps, 3),
                   "share_of_copy": round(tbps / COPY_TBPS, 3), "no_table_ms": round(t0, 4), "no_table_ms_min_max": [round(lo0, 4), round(hi0, 4)],
                   "no_table_equal": same}
        say(" ", what, r[what])
    r["labels_with_voxels"], r["outside"] = int((st.count > 0).sum()), st.outside
    # the torch route: a small call first (it loads torch's kernels), then the wall time and the peak of its allocations
    torch_route(labels[:8, :8, :8].contiguous(), n)
    st = dense.label_stats(dv, labels, n)
    sub = 1
    try:
        got, wall, peak = timed_torch(labels, n)
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        sub = 2
        labels = labels[::2, ::2, ::2].contiguous()
        st = dense.label_stats(dv, labels, n)
        got, wall, peak = timed_torch(labels, n)
    walls = [wall]
    for _ in range(torch_reps - 1):
        del got
        got, wall, peak = timed_torch(labels, n)
        walls.append(wall)
    equal = bool(torch.equal(got[0], st.count) and torch.equal(got[1], st.lo) and torch.equal(got[2], st.hi) and
                 torch.equal(got[3], st.sum.to(torch.float64)))
    r["torch"] = {"every_nth_voxel": sub, "wall_ms": round(statistics.median(walls), 3), "peak_GB": round(peak / 1e9, 3), "equal": equal}
    say("  torch", r["torch"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--random-resolution", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-reps", type=int, default=1)
    args = ap.parse_args()
    res, reps = args.resolution, args.reps
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    lab, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
    r = {"mesh": "scan_like", "resolution": res, "copy_TBps": COPY_TBPS, "reps": reps}
    r["fill_labels_u8"] = bench_grid(dv, "fill labels", lab, 2, reps, args.torch_reps)
    cc, n = dense.components(dv, lab, connectivity=6, background=True)
    del lab
    r["background_components_i32"] = bench_grid(dv, "background components", cc, n, reps, args.torch_reps)
    del cc
    torch.cuda.empty_cache()
    rr = args.random_resolution
    rnd = torch.randint(0, 2 ** 20, (rr, rr, rr), dtype=torch.int32, device=dev, generator=torch.Generator(device=dev).manual_seed(19))
    r["random_labels_i32"] = bench_grid(dv, "random labels", rnd, 2 ** 20 - 1, reps, args.torch_reps)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
