"""Parts of dense grids - the watershed basins of a relief, merged by persistence - on the voxelizer's device
(o2v_hip_watershed_dense): the torch layer, which obj2voxel_amd.dense re-exports as dense.watershed,
dense.watershed_peaks and dense.split_parts beside skeletonize.  It waits on the voxelizer's device (dense._sync) before the library
call, as every function of dense.py does; tests/test_host_watershed.py holds that wait.

torch is imported first on purpose (see obj2voxel_amd/dense.py)."""
import math
import numbers

import torch  # first

MAX_MIN_DEPTH = 2 ** 32 - 1   # min_depth is one uint32
MAX_SCALE = 2 ** 15           # split_parts: scale * sqrt(2^31 - 1) stays an int32


def _integer(value, name, lo, hi):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or not lo <= value <= hi:
        raise ValueError(f"{name} must be an integer {lo} .. {hi}, not {value!r}")
    return int(value)


def watershed(dv, relief, *, min_depth=0, connectivity=26, out=None):
    """The parts of a relief on the voxelizer's device.  Returns (labels, n): labels int32 [z, y, x], 0 where
    relief <= 0 and 1 .. n elsewhere, and n, the number of parts.

    Every voxel of the set {relief > 0} climbs to its neighbour of greatest key (height, linear index) until it stands on a peak;
    the voxels of a peak are its basin.  A peak whose pass to a higher peak lies less than min_depth below it is merged into that
    one (the elder rule of persistence), so min_depth=0 gives every basin and rising values give coarser partitions that nest.
    Parts are numbered by the linear index of their surviving peak, which is the part's voxel of greatest key.  Everything is an
    integer; one run equals another bit for bit.

        depth2 = dense.inner_distance(dv, solid)
        labels, n = dense.watershed(dv, depth2, min_depth=9)          # squared depths: min_depth in squared units
        peaks, heights = dense.watershed_peaks(labels, depth2, n)

    relief:        an int32 tensor [z, y, x] on dv's device, any strides.  It is only read.
    min_depth:     an integer 0 .. 2^32 - 1, in the relief's units.
    connectivity:  6, 18 or 26.  Ascent is by value, not by slope: a diagonal neighbour counts like a face neighbour.
    out:           an int32 tensor of the relief's shape (any strides, not in relief's storage), written as it is; else a new
                   contiguous tensor.
    On a plateau the flow runs to the voxel of greatest index, and part borders are where ascent paths diverge: they are not
    smoothed."""
    from . import dense   # (at call time: dense imports this module)
    dense._require_shared_runtime()
    device = dense._device(dv)
    dense._check_grid(relief, "relief", torch.int32, device)
    if 0 in relief.shape:
        raise ValueError("relief has an empty dimension")
    dims = (relief.shape[2], relief.shape[1], relief.shape[0])
    dense._limit_voxels(dims)
    min_depth = _integer(min_depth, "min_depth", 0, MAX_MIN_DEPTH)
    if isinstance(connectivity, bool) or connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity must be 6, 18 or 26, not {connectivity!r}")
    if out is None:
        out = torch.empty(tuple(relief.shape), dtype=torch.int32, device=device)
    else:
        dense._check_grid(out, "out", torch.int32, device, tuple(relief.shape))
        if dense._byte_ranges_overlap(out, relief):
            raise ValueError("out must not overlap relief")
    dense._sync(device)   # (the caller's writes to relief and out have landed)
    n = dv.watershed_dense(relief.data_ptr(), dense._strides(relief), dims, connectivity, min_depth, 0, out.data_ptr(), dense._strides(out))
    return out, n


def watershed_peaks(labels, relief, n):
    """(int32 [n, 3] (x, y, z), int32 [n] heights): per label 1 .. n its voxel of greatest key (relief, linear index) - the
    surviving peak of a part of watershed.  Plain torch on the two grids."""
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3 or labels.dtype != torch.int32:
        raise ValueError("labels must be a 3-D torch.int32 tensor [z, y, x]")
    if not isinstance(relief, torch.Tensor) or relief.dtype != torch.int32 or relief.shape != labels.shape or relief.device != labels.device:
        raise ValueError("relief must be a torch.int32 tensor of labels' shape on its device")
    n = _integer(n, "n", 0, 2 ** 31 - 1)
    nz, ny, nx = labels.shape
    index = torch.arange(labels.numel(), dtype=torch.int64, device=labels.device)
    L, H = labels.reshape(-1).to(torch.int64), relief.reshape(-1).to(torch.int64)
    inside = (L > 0) & (L <= n)
    key = torch.full((n + 1,), -1, dtype=torch.int64, device=labels.device)
    key.scatter_reduce_(0, L[inside], (H[inside] << 31) | index[inside], "amax")
    if n and bool((key[1:] < 0).any()):
        raise ValueError(f"labels does not hold every label 1 .. {n}")
    at = key[1:] & 0x7fffffff
    xyz = torch.stack([at % nx, at // nx % ny, at // (nx * ny)], 1).to(torch.int32)
    return xyz, (key[1:] >> 31).to(torch.int32)


def scaled_root(depth2, scale):
    """int32 floor(scale * sqrt(depth2)) of an int32 tensor of values >= 0, exact: a float64 square root of scale^2 * depth2,
    corrected by integer comparison in int64."""
    v = depth2.to(torch.int64) * (scale * scale)
    r = v.to(torch.float64).sqrt().to(torch.int64)
    r = r - (r * r > v).to(torch.int64)
    r = r + ((r + 1) * (r + 1) <= v).to(torch.int64)
    r = r - (r * r > v).to(torch.int64)
    return r.to(torch.int32)


def split_parts(dv, grid, *, min_depth=1.0, scale=4, level=None, background=False, border=True, connectivity=26):
    """The parts of a solid: (labels int32 [z, y, x], n).  The relief is the depth of the set -
    floor(scale * sqrt(inner_distance)), exact - and two tops of it stay two parts if the pass between them lies at least
    min_depth voxels below the lower one.

        solid, origin = dense.voxelize_dense(dv, 512, fill=True)
        labels, n = dense.split_parts(dv, solid, min_depth=2)         # rooms, grains, a handle and its body
        stats = dense.label_stats(dv, labels, n)

    A part is the set of voxels whose steepest way inwards ends on the same deepest place, after the places that a neck of less
    than min_depth separates are taken together: two rooms joined by a corridor are two parts and the corridor is shared between
    them where its ways inwards part, two balls sintered at a neck are two parts.  A part is not a connected component (parts
    touch), not a convex piece, and its border is not smoothed or placed at the narrowest section: it is where the ascent paths of
    the depth map diverge, and on a flat top the flow runs to the voxel of greatest index.

    grid, level, background, border:  as inner_distance takes them.
    min_depth:     a number >= 0, in voxels; ceil(min_depth * scale) is what watershed gets.
    scale:         an integer 1 .. 2^15: the relief's steps per voxel of depth.
    connectivity:  6, 18 or 26."""
    from . import dense
    if isinstance(min_depth, bool) or not isinstance(min_depth, numbers.Real) or not 0.0 <= float(min_depth) < float("inf"):
        raise ValueError(f"min_depth must be a number >= 0 (voxels), not {min_depth!r}")
    scale = _integer(scale, "scale", 1, MAX_SCALE)
    steps = math.ceil(float(min_depth) * scale)
    if steps > MAX_MIN_DEPTH:
        raise ValueError(f"min_depth * scale must be at most {MAX_MIN_DEPTH}")
    if isinstance(connectivity, bool) or connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity must be 6, 18 or 26, not {connectivity!r}")
    depth2 = dense.inner_distance(dv, grid, level=level, background=background, border=border)
    return watershed(dv, scaled_root(depth2, scale), min_depth=steps, connectivity=connectivity)
