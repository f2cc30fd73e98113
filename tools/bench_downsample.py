#!/usr/bin/env python3
"""Downsampling (o2v_hip_downsample) on the bench headline mesh (meshes.scan_like(), welded into positions + faces) at 1024 with
the solid fill: the labels and the argb grid from voxelize_dense(fill=True), merged by 2, 4 and 3 (1024 -> 512, 256 and 342) into
occupancy alone, occupancy + count, and occupancy + mean colours.  For each: the device time of the one launch from the events
around it (o2v_hip_downsample_times), median of --reps after a warm-up; the bytes the call must move at least - the grid once,
the colours of the solid fine voxels once, every output once - over that time, and as a share of the 6.3 TB/s a device copy
reaches on the MI355X; and the same result by the torch route (the grid padded to the lattice, reshaped to blocks, amax / sum
per block, the colours a masked sum per channel), with its wall time around a synchronise and the peak memory torch allocated
for it.  The two routes' results are compared.  One JSON object on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import torch  # first: the library binds to the HIP runtime torch loaded
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from obj2voxel_amd import dense, hip, meshes  # noqa: E402

COPY_TBPS = 6.3   # the measured device copy of the MI355X


def blocks(t, f):
    """t [z, y, x] padded with zeros to multiples of f (the box starts at the lattice's origin) as [cz, f, cy, f, cx, f]."""
    nz, ny, nx = t.shape
    pad = [(-n) % f for n in (nx, ny, nz)]
    if any(pad):
        t = F.pad(t, (0, pad[0], 0, pad[1], 0, pad[2]))
    nz, ny, nx = t.shape
    return t.view(nz // f, f, ny // f, f, nx // f, f)


def torch_route(lab, argb, f, what):
    s = blocks((lab != 0).to(torch.uint8), f)
    if what == "solid":
        return (s.amax(dim=(1, 3, 5)) != 0,)
    n = s.sum(dim=(1, 3, 5), dtype=torch.int32)
    if what == "count":
        return n != 0, n.to(torch.int16)
    c = blocks(argb, f)
    mean = torch.zeros_like(n)
    safe = n.clamp(min=1)
    for shift in (0, 8, 16, 24):
        ch = (((c >> shift) & 0xff) * s).sum(dim=(1, 3, 5), dtype=torch.int32)
        mean |= ((2 * ch + safe) // (2 * safe)) << shift
    return n != 0, torch.where(n != 0, mean, torch.zeros_like(mean))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    res, reps = args.resolution, args.reps
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    lab, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
    argb, _ = dense.voxelize_dense(dv, res, fmt="argb", fill=True)
    n, solid_fine = lab.numel(), int((lab != 0).sum())
    r = {"mesh": "scan_like", "resolution": res, "fill": True, "solid_voxels": solid_fine, "copy_TBps": COPY_TBPS}
    for f in (2, 4, 3):
        _, cshape = dense.downsample_box((0, 0, 0), tuple(lab.shape), f)
        m = cshape[0] * cshape[1] * cshape[2]
        for what, kw, nbytes in (("solid", {}, n + m), ("count", dict(count=True), n + 3 * m),
                                 ("colors", dict(colors=argb), n + 4 * solid_fine + 5 * m)):
            outs = dense.downsample(dv, lab, f, **kw)[:-1]           # (warm-up; the outputs are written again below)
            names = ["out"] + (["out_count"] if what == "count" else ["out_colors"] if what == "colors" else [])
            again = dict(zip(names, outs))
            ms = []
            for _ in range(reps):
                dense.downsample(dv, lab, f, **kw, **again)
                ms.append(dv.downsample_times()[0])
            t = statistics.median(ms)
            # the torch route: one warm-up, then the wall time around a synchronise and the peak of its allocations
            want = torch_route(lab, argb, f, what)
            equal = all(bool(torch.equal(a, b)) for a, b in zip(outs, want))
            del want
            walls = []
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            for _ in range(max(1, reps // 2)):
                t0 = time.perf_counter()
                got = torch_route(lab, argb, f, what)
                torch.cuda.synchronize()
                walls.append((time.perf_counter() - t0) * 1e3)
                del got
            peak = torch.cuda.max_memory_allocated() - base
            tbps = nbytes / (t * 1e-3) / 1e12
            r[f"f{f}_{what}"] = {"coarse": list(cshape), "device_ms": round(t, 4), "device_ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                                 "GB": round(nbytes / 1e9, 3), "TBps": round(tbps, 3), "share_of_copy": round(tbps / COPY_TBPS, 3),
                                 "torch_ms": round(statistics.median(walls), 3), "torch_peak_GB": round(peak / 1e9, 3), "equal": equal}
            del outs, again
    print(json.dumps(r))


if __name__ == "__main__":
    main()
