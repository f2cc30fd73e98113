#!/usr/bin/env python3
"""Surface nets of label grids (o2v_hip_label_surface_count / _write / _relax) on label grids of the bench headline mesh
(meshes.scan_like(), welded into positions + faces) at every --resolutions: the uint8 labels of fill=True, the int32 parts of
split_parts and the int32 labels of components(connectivity=6, background=True).  For each grid, closed: the device times of the
five stages from the events around them (o2v_hip_label_surface_times), medians of --reps after a warm-up - classify, count + scan,
vertices, faces, and the relaxation per iteration (--iterations of them in one call) -, V and Q; beside them
  classify with O2V_LSF_NO_TILE=1 (no tile in LDS, the rows y + 1 and z + 1 re-read through L2);
  a device copy of the grid - the floor of classify;
  extract_surface's count and write (o2v_hip_surface_times) on the float32 field where(grid != 0, -1, 1), and the net of the binary
  grid grid != 0, open - the same V and Q, asserted;
  voxel_faces(merge="none") of the binary grid - the same Q as its closed net, asserted;
  the torch route - shifted comparisons of the padded grid and nonzero, for the cells and the quads' edges - with its wall time
  around a synchronise and the peak memory torch allocated for it; its counts are asserted equal to the call's.
One JSON object on stdout."""
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


def med(rows):
    return [round(statistics.median(c), 4) for c in zip(*rows)]


def net_ms(dv, labels, closed, reps, iterations):
    """(medians of the five stages, the relaxation per iteration; V, Q) of count + write + relax on the grid."""
    nz, ny, nx = labels.shape
    fmt = hip.LABELS_I32 if labels.dtype == torch.int32 else hip.LABELS_U8
    args = (labels.data_ptr(), fmt, (labels.stride(2), labels.stride(1), labels.stride(0)), (nx, ny, nz), hip.LABEL_SURFACE_CLOSED if closed else 0)
    torch.cuda.synchronize()
    V, Q = dv.label_surface_count(*args)
    dev = labels.device
    cells, links = torch.empty((V, 3), dtype=torch.int32, device=dev), torch.empty((V, 6), dtype=torch.int32, device=dev)
    faces, pairs = torch.empty((2 * Q, 3), dtype=torch.int32, device=dev), torch.empty((Q, 2), dtype=torch.int32, device=dev)
    positions = torch.empty((V, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rows = []
    for i in range(reps + 1):
        assert dv.label_surface_count(*args) == (V, Q)
        dv.label_surface_write(*args, cells.data_ptr(), links.data_ptr(), V, faces.data_ptr(), pairs.data_ptr(), Q)
        dv.label_surface_relax(cells.data_ptr(), links.data_ptr(), V, (0, 0, 0), iterations, 0.5, 0.5, positions.data_ptr())
        if i:
            rows.append(dv.label_surface_times())
    ms = med(rows)
    return ms[:4] + [round(ms[4] / iterations, 4)], V, Q


def k10_ms(dv, field, reps):
    nz, ny, nx = field.shape
    args = (field.data_ptr(), (field.stride(2), field.stride(1), field.stride(0)), (nx, ny, nz), 0.0)
    torch.cuda.synchronize()
    V, T = dv.surface_count(*args)
    positions = torch.empty((V, 3), dtype=torch.float32, device=field.device)
    faces = torch.empty((T, 3), dtype=torch.int32, device=field.device)
    torch.cuda.synchronize()
    rows = []
    for i in range(reps + 1):
        dv.surface_count(*args)
        dv.surface_write(*args, (0, 0, 0), positions.data_ptr(), V, faces.data_ptr(), T)
        if i:
            rows.append(dv.surface_times())
    return med(rows), V, T // 2


def event_ms(f, reps):
    ms = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = f()
        b.record()
        torch.cuda.synchronize()
        del out
        if i:
            ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4)


def torch_route(labels):
    """(cells [V, 3], the edges of the quads along x, y, z) of the closed net by plain torch."""
    pad = torch.nn.functional.pad(labels.to(torch.int32) if labels.dtype != torch.int32 else labels, (1, 1, 1, 1, 1, 1))
    dx, dy, dz = pad[:, :, 1:] != pad[:, :, :-1], pad[:, 1:] != pad[:, :-1], pad[1:] != pad[:-1]
    quads = [torch.nonzero(d) for d in (dx, dy, dz)]
    active = dx[:-1, :-1] | dx[1:, :-1] | dx[:-1, 1:] | dx[1:, 1:]
    active |= dy[:-1, :, :-1] | dy[1:, :, :-1] | dy[:-1, :, 1:] | dy[1:, :, 1:]
    active |= dz[:, :-1, :-1] | dz[:, 1:, :-1] | dz[:, :-1, 1:] | dz[:, 1:, 1:]
    return torch.nonzero(active), quads


def timed_torch(labels):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    cells, quads = torch_route(labels)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return cells.shape[0], sum(q.shape[0] for q in quads), wall, torch.cuda.max_memory_allocated() - base


def bench_grid(dv, name, labels, reps, iterations, with_torch):
    say(name, tuple(labels.shape), labels.dtype)
    nbytes = labels.numel() * labels.element_size()
    r = {"shape": list(labels.shape), "dtype": str(labels.dtype).replace("torch.", ""), "GB": round(nbytes / 1e9, 3)}
    ms, V, Q = net_ms(dv, labels, True, reps, iterations)
    r["label_surface"] = {"vertices": V, "quads": Q, "classify_ms": ms[0], "count_scan_ms": ms[1], "vertices_ms": ms[2], "faces_ms": ms[3],
                          "relax_ms_per_iteration": ms[4], "classify_TBps": round(nbytes / (ms[0] * 1e-3) / 1e12, 3),
                          "relax_ns_per_vertex": round(ms[4] * 1e6 / max(V, 1), 3)}
    os.environ["O2V_LSF_NO_TILE"] = "1"   # the A/B: classify without its tile in LDS, the rows y + 1 and z + 1 re-read through L2
    try:
        ms0, V0, Q0 = net_ms(dv, labels, True, reps, 1)
    finally:
        os.environ.pop("O2V_LSF_NO_TILE", None)
    assert (V0, Q0) == (V, Q)
    r["label_surface"]["classify_no_tile_ms"] = ms0[0]
    r["copy_ms"] = event_ms(labels.clone, reps)
    say(" ", r["label_surface"], "copy", r["copy_ms"])
    binary = labels != 0
    ms_b, Vb, Qb = net_ms(dv, binary, False, reps, 1)
    field = torch.where(binary, -1.0, 1.0).to(torch.float32)
    ms_k, Vk, Qk = k10_ms(dv, field, reps)
    assert (Vb, Qb) == (Vk, Qk), (name, Vb, Qb, Vk, Qk)
    r["binary_open"] = {"vertices": Vb, "quads": Qb, "label_surface_u8_ms": ms_b[:4], "extract_surface_f32_ms": ms_k}
    del field
    if labels.dtype == torch.int32:   # 4 bytes a sample on both sides: the labels against the float32 field of the same shape
        r["classify_count_i32_ms"] = round(ms[0] + ms[1], 4)
        r["extract_surface_classify_count_f32_ms"] = round(ms_k[0] + ms_k[1], 4)
    _, _, Qc = net_ms(dv, binary, True, 1, 1)
    n_faces = dense.count_faces(dv, binary, merge="none")
    assert n_faces == Qc, (name, n_faces, Qc)
    r["voxel_faces_none_ms"] = event_ms(lambda: dense.voxel_faces(dv, binary, merge="none"), max(2, reps // 2))
    r["binary_closed_quads"] = Qc
    say(" ", r["binary_open"], "voxel_faces", r["voxel_faces_none_ms"])
    del binary
    if with_torch:
        torch_route(labels[:8, :8, :8].contiguous())   # (a small call first: it loads torch's kernels)
        Vt, Qt, wall, peak = timed_torch(labels)
        assert (Vt, Qt) == (V, Q), (name, Vt, Qt, V, Q)
        r["torch"] = {"wall_ms": round(wall, 3), "peak_GB": round(peak / 1e9, 3), "equal_counts": True,
                      "times_count_and_write": round(wall / sum(ms[:4]), 1)}
        say("  torch", r["torch"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--no-parts", action="store_true", help="leave the split_parts grids out")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch route out")
    args = ap.parse_args()
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    r = {"mesh": "scan_like", "reps": args.reps, "iterations": args.iterations, "grids": {}}
    for res in args.resolutions:
        lab, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True)
        r["grids"][f"fill_labels_u8_{res}"] = bench_grid(dv, f"fill labels at {res}", lab, args.reps, args.iterations, not args.no_torch)
        if not args.no_parts:
            parts, n = dense.split_parts(dv, lab, min_depth=2)
            r["grids"][f"split_parts_i32_{res}"] = dict(bench_grid(dv, f"split_parts at {res}", parts, args.reps, args.iterations, not args.no_torch), n_labels=n)
            del parts
        cc, n = dense.components(dv, lab, connectivity=6, background=True)
        r["grids"][f"background_components_i32_{res}"] = dict(bench_grid(dv, f"background components at {res}", cc, args.reps, args.iterations, not args.no_torch),
                                                              n_labels=n)
        del cc, lab
        torch.cuda.empty_cache()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
