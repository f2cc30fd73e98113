#!/usr/bin/env python3
"""Seeded watershed (o2v_hip_grow_dense) on one MI355X.  On the filled bench mesh (meshes.scan_like(),
welded into positions + faces, voxelize_dense(fill=True)) at --resolutions (512 and 1024):
  flat    dense.grow_labels with 1, 64 and 4 096 seeds drawn with a fixed generator from the solid, beside dense.geodesic_distance
          on the same set and seeds in the same run (it computes a strict subset: the ticks), and the ratio of the two;
  relief  dense.seeded_watershed on split_parts' depth map with the peaks of dense.watershed(min_depth) as markers, beside
          dense.watershed with that min_depth in the same run;
both with the tile pass and (at the first resolution) with O2V_GROW_NO_TILES=1, checked equal; and the worst case by name, the
128 x 64 x 16 serpentine one voxel wide, in both modes.  Medians of --reps of the stage events (o2v_hip_grow_times: init, level
rounds, sources, tick rounds, tight, label rounds, write) in ms, and the counters of one more call made with
O2V_HIP_FLAG_STAGE_TIMES: per phase the rounds, tile visits and in-tile sweeps.  One JSON object on stdout, progress on stderr."""
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
from obj2voxel_amd import watershed as ws  # noqa: E402
from tests import components_ref  # noqa: E402

STAGES = ("init", "level_rounds", "sources", "tick_rounds", "tight", "label_rounds", "write")
PHASES = ("level", "ticks", "labels")


def no_tiles(on):
    if on:
        os.environ["O2V_GROW_NO_TILES"] = "1"
    else:
        os.environ.pop("O2V_GROW_NO_TILES", None)


def grow(dv, relief, markers, weights, reps, outs):
    """Stage medians and the counters of o2v_hip_grow_dense on this relief and these markers, into outs = (labels, level, ticks)."""
    dims = tuple(relief.shape[::-1])
    lab, lev, tic = outs

    def call(flags):
        return dv.grow_dense(relief.data_ptr(), dense._strides(relief), markers.data_ptr(), dense._strides(markers), dims, weights, flags, lab.data_ptr(),
                             dense._strides(lab), lev.data_ptr(), dense._strides(lev), tic.data_ptr(), dense._strides(tic))
    torch.cuda.synchronize()
    reached = call(hip.FLAG_STAGE_TIMES)     # warm-up (the scratch is grown), and the counters
    c = dv.grow_counters()
    ms = []
    for _ in range(reps):
        call(0)
        ms.append(dv.grow_times())
    stages = [statistics.median(m[i] for m in ms) for i in range(7)]
    return {"ms": round(sum(stages), 3), "stage_ms": dict(zip(STAGES, (round(v, 3) for v in stages))), "reached": reached,
            "counters": {p: dict(zip(("rounds", "tile_visits", "tile_sweeps"), c[3 * i:3 * i + 3])) for i, p in enumerate(PHASES)}}


def geodesic(dv, solid, seeds, weights, reps, out):
    def call():
        return dense.geodesic_distance(dv, solid, seeds, weights=weights, out=out)
    call()
    ms = []
    for _ in range(reps):
        call()
        ms.append(dv.geodesic_times())
    stages = [statistics.median(m[i] for m in ms) for i in range(4)]
    return {"ms": round(sum(stages), 3), "stage_ms": dict(zip(("classify", "init_seeds", "propagation", "write"), (round(v, 3) for v in stages)))}


def watershed_ms(dv, relief, steps, reps, out):
    torch.cuda.synchronize()   # (torch has finished writing the relief: the library reads it on a stream of its own)
    dv.watershed_dense(relief.data_ptr(), dense._strides(relief), tuple(relief.shape[::-1]), 26, steps, 0, out.data_ptr(), dense._strides(out))
    ms = []
    for _ in range(reps):
        n = dv.watershed_dense(relief.data_ptr(), dense._strides(relief), tuple(relief.shape[::-1]), 26, steps, 0, out.data_ptr(), dense._strides(out))
        ms.append(sum(dv.watershed_times()))
    return round(statistics.median(ms), 3), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 64, 4096])
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--min-depth", type=float, default=2.0, help="in voxels, as split_parts takes it (the README's setting)")
    ap.add_argument("--sets", default="frs", help="f: flat, r: relief, s: serpentine")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    dv = hip.DeviceVoxelizer(0)
    weights = (3, 4, 5)
    r = {"mesh": "scan_like", "fill": True, "reps": args.reps, "weights": weights}
    if "f" in args.sets or "r" in args.sets:
        verts = meshes.scan_like()
        positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
        dense.set_mesh(dv, torch.from_numpy(positions.view(np.float32)).to(dev), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(dev))
    for res in (args.resolutions if "f" in args.sets or "r" in args.sets else []):
        print(f"resolution {res} ...", file=sys.stderr, flush=True)
        solid, _ = dense.voxelize_dense(dv, res, fill=True)
        shape = tuple(solid.shape)
        outs = tuple(torch.empty(shape, dtype=torch.int32, device=dev) for _ in range(3))
        e = {"solid_voxels": int((solid != 0).sum()), "voxels": solid.numel(), "scratch_bytes": dv.grow_scratch_bytes(shape[::-1])}
        both = res == args.resolutions[0]
        if "f" in args.sets:
            flat = (solid != 0).to(torch.int32)
            # voxels of the box drawn with a fixed generator, those in the solid kept: the first n of them are the seeds
            drawn = torch.from_numpy(np.random.default_rng(28).integers(0, solid.numel(), 16 * max(args.seeds) + 64)).to(dev)
            drawn = drawn[solid.reshape(-1)[drawn] != 0]
            assert len(drawn) >= max(args.seeds)
            for n in args.seeds:
                at = drawn[:n]
                seeds = torch.stack([at % shape[2], at // shape[2] % shape[1], at // (shape[2] * shape[1])], 1).to(torch.int32).contiguous()
                markers = dense.markers_from_seeds(seeds, shape, device=dev)
                no_tiles(False)
                t = grow(dv, flat, markers, weights, args.reps, outs)
                keep = outs[0].clone() if both else None
                t["geodesic"] = geodesic(dv, solid, seeds, weights, args.reps, outs[1])
                assert torch.equal(outs[1], outs[2]), "ticks on a flat relief are the geodesic distance"
                t["ratio_to_geodesic"] = round(t["ms"] / t["geodesic"]["ms"], 2)
                g = t["geodesic"]["stage_ms"]["propagation"]
                t["phase_ratio_to_geodesic_propagation"] = {p: round(t["stage_ms"][stage] / g, 2)
                                                            for p, stage in zip(PHASES, ("level_rounds", "tick_rounds", "label_rounds"))}
                if both:
                    no_tiles(True)
                    t["no_tiles"] = grow(dv, flat, markers, weights, args.reps, outs)
                    no_tiles(False)
                    assert torch.equal(keep, outs[0])
                e[f"flat, {n} seeds"] = t
                print(f"  flat, {n} seeds: {t['ms']} ms {t['stage_ms']} {t['counters']}; geodesic {t['geodesic']['ms']} ms; x{t['ratio_to_geodesic']}; "
                      f"no tiles {t.get('no_tiles', {}).get('ms')}", file=sys.stderr, flush=True)
            del flat, drawn
        if "r" in args.sets:
            relief = ws.scaled_root(dense.inner_distance(dv, solid), args.scale)
            steps = int(np.ceil(args.min_depth * args.scale))
            no_tiles(False)
            w_ms, parts = watershed_ms(dv, relief, steps, args.reps, outs[0])
            peaks, _ = dense.watershed_peaks(outs[0], relief, parts)
            markers = dense.markers_from_seeds(peaks, shape, device=dev)
            t = grow(dv, relief, markers, weights, args.reps, outs)
            keep = outs[0].clone() if both else None
            t.update({"watershed_ms": w_ms, "parts": parts, "labels_found": int(len(torch.unique(outs[0])) - 1), "ratio_to_watershed": round(t["ms"] / w_ms, 2)})
            if both:
                no_tiles(True)
                t["no_tiles"] = grow(dv, relief, markers, weights, args.reps, outs)
                no_tiles(False)
                assert torch.equal(keep, outs[0])
            e[f"relief, min_depth {args.min_depth}"] = t
            print(f"  relief: {t['ms']} ms {t['stage_ms']} {t['counters']}; watershed {w_ms} ms, {parts} parts; no tiles {t.get('no_tiles', {}).get('ms')}",
                  file=sys.stderr, flush=True)
            del relief, markers
        r[str(res)] = e
        del solid, outs
        torch.cuda.empty_cache()
    if "s" in args.sets:
        S = components_ref.serpentine((128, 64, 16))
        relief = torch.from_numpy(S.astype(np.int32)).to(dev)
        markers = torch.zeros_like(relief)
        markers[0, 0, 0] = 1
        outs = tuple(torch.empty(tuple(relief.shape), dtype=torch.int32, device=dev) for _ in range(3))
        e = {"voxels": int(S.sum())}
        for mode in (False, True):
            no_tiles(mode)
            e["no_tiles" if mode else "tiles"] = grow(dv, relief, markers, (1, 0, 0), args.reps, outs)
            assert int(outs[2].max()) == int(S.sum()) - 1
        no_tiles(False)
        r["serpentine 128 x 64 x 16"] = e
        print(f"  serpentine: {e}", file=sys.stderr, flush=True)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
