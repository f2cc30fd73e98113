"""Seeded watershed - markers grown through a relief - on the voxelizer's device (o2v_hip_grow_dense): the
torch layer, which obj2voxel_amd.dense re-exports as dense.seeded_watershed, dense.grow_labels and dense.markers_from_seeds beside
watershed.  It waits on the voxelizer's device (dense._sync) before the library call, as every function of dense.py does;
tests/test_host_grow.py holds that wait.

torch is imported first on purpose (see obj2voxel_amd/dense.py)."""
import numbers

import torch  # first


def _flag(value, name):
    if not isinstance(value, bool):
        raise TypeError(f"{name} must be a bool, not {value!r}")
    return value


def _grow(dv, device, relief, markers, weights, labels, level, ticks):
    from . import dense
    dims = (relief.shape[2], relief.shape[1], relief.shape[0])
    dense._sync(device)   # (the caller's writes to relief, markers and the outputs have landed)
    return dv.grow_dense(relief.data_ptr(), dense._strides(relief), markers.data_ptr(), dense._strides(markers), dims, weights, 0, labels.data_ptr(),
                         dense._strides(labels), dense._ptr(level), None if level is None else dense._strides(level), dense._ptr(ticks),
                         None if ticks is None else dense._strides(ticks))


def seeded_watershed(dv, relief, markers, *, metric="chamfer", connectivity=26, weights=None, level=False, distance=False, out=None):
    """The catchments of markers in a relief on the voxelizer's device: labels int32 [z, y, x], the marker's
    value where its flood arrives first, 0 where relief <= 0 and where no marker reaches.  With level=True and / or
    distance=True the tuple (labels, level, ticks) with None for what was not asked.

    The relief is watershed's: high is the middle of a part, and the flood runs downhill from the markers - the hierarchical-queue
    flood of Meyer, with the queue's order replaced by a distance and the smallest label on a tie, so the result is a unique fixed
    point: integers, the same bits on every run.  A voxel's level is the highest pass over which a marker reaches it, its ticks the
    length of the way since the flood last descended (or since the marker).

        cores, n = dense.components(dv, dense.erode(dv, solid, 6))          # where the parts are
        depth2 = dense.inner_distance(dv, solid)
        labels = dense.seeded_watershed(dv, depth2, cores, connectivity=6)  # the parts, grown through the depth map
        adj = dense.label_adjacency(dv, labels, n, values=depth2)           # ... and the depth of the necks between them

    relief:        an int32 tensor [z, y, x] on dv's device, any strides; the set is where it is positive.  It is only read.
    markers:       an int32 tensor of relief's shape on its device, any strides: a seed where markers > 0 and relief > 0, of label
                   1 .. 2^31 - 1.  It is only read.
    metric, connectivity, weights:  as geodesic_distance takes them: the steps that exist and what they cost in ticks.
                   Every descent ends at ticks 0, so below the pass between two markers a voxel takes the smallest label among
                   its deeper neighbours: through a depth map connectivity=6 keeps the border where the parts meet, with diagonal
                   steps the smaller label creeps round the other part's outer shell.
    out:           an int32 tensor of relief's shape (any strides, in neither input's storage), written as it is; else a new
                   contiguous tensor."""
    from . import dense
    dense._require_shared_runtime()
    device = dense._device(dv)
    dense._check_grid(relief, "relief", torch.int32, device)
    dense._check_grid(markers, "markers", torch.int32, device, tuple(relief.shape))
    if 0 in relief.shape:
        raise ValueError("relief has an empty dimension")
    dense._limit_voxels((relief.shape[2], relief.shape[1], relief.shape[0]))
    weights = dense._geo_weights(metric, connectivity, weights)
    level, distance = _flag(level, "level"), _flag(distance, "distance")
    if out is None:
        out = torch.empty(tuple(relief.shape), dtype=torch.int32, device=device)
    else:
        dense._check_grid(out, "out", torch.int32, device, tuple(relief.shape))
        if dense._byte_ranges_overlap(out, relief) or dense._byte_ranges_overlap(out, markers):
            raise ValueError("out must not overlap relief or markers")
    q = torch.empty(tuple(relief.shape), dtype=torch.int32, device=device) if level else None
    t = torch.empty(tuple(relief.shape), dtype=torch.int32, device=device) if distance else None
    _grow(dv, device, relief, markers, weights, out, q, t)
    return (out, q, t) if level or distance else out


def grow_labels(dv, grid, markers, *, background=False, level=None, max_distance=None, metric="chamfer", connectivity=26, weights=None):
    """Labels grown from markers through a set, never across a wall: (labels, dist), both int32 [z, y, x].
    labels holds the marker nearest by geodesic_distance's measure - the smallest label on a tie -, dist that distance; 0 and -1
    outside the set and where no marker reaches.  This is seeded_watershed over the relief that is 1 on the set: the geodesic
    Voronoi diagram of the markers, skimage's expand_labels with walls.

    grid:          bool or uint8 (the set is where != 0) or float32 with `level` (where grid < level); packed bits are refused.
    background:    True: the set is the voxels of the box that are not solid.
    markers:       an int32 tensor of grid's shape on its device: a seed where markers > 0 inside the set.
    max_distance:  an integer 0 .. 2^31 - 2: labels = 0 and dist = -1 where dist is above it.  dist is geodesic_distance's, so
                   this is exact bounded growth.  None: no bound."""
    from . import dense
    if isinstance(grid, torch.Tensor) and grid.dtype == torch.int32:
        raise ValueError("grow_labels takes no packed bits: pass a bool, uint8 or float32 grid")
    device, _, level, dims = dense._set_grid(dv, grid, level, dense._limit_voxels, None)
    dense._check_grid(markers, "markers", torch.int32, device, tuple(grid.shape))
    _flag(background, "background")
    weights = dense._geo_weights(metric, connectivity, weights)
    if max_distance is not None and (isinstance(max_distance, bool) or not isinstance(max_distance, numbers.Integral)
                                     or not 0 <= max_distance <= dense.hip.GROW_MAX_TICKS):
        raise ValueError(f"max_distance must be an integer 0 .. {dense.hip.GROW_MAX_TICKS}, not {max_distance!r}")
    solid = grid != 0 if level is None else grid < level
    relief = (~solid if background else solid).to(torch.int32)
    labels = torch.empty(tuple(grid.shape), dtype=torch.int32, device=device)
    dist = torch.empty(tuple(grid.shape), dtype=torch.int32, device=device)
    _grow(dv, device, relief, markers, weights, labels, None, dist)
    if max_distance is not None:
        far = dist > int(max_distance)
        labels[far] = 0
        dist[far] = -1
    return labels, dist


def markers_from_seeds(seeds, shape, *, device):
    """A marker grid from a list of seeds: int32 [z, y, x] of `shape` on `device` with label i + 1 at seeds[i] = (x, y, z) and 0
    elsewhere.  Where two seeds share a voxel the smallest label stays; seeds outside the box are dropped.

    seeds:  an int32 tensor [n, 3] on the device, or a sequence of such triples."""
    device = torch.device(device)
    shape = tuple(shape)
    if len(shape) != 3 or any(isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1 for n in shape):
        raise ValueError(f"shape must be three positive integers (nz, ny, nx), not {shape!r}")
    if shape[0] * shape[1] * shape[2] > 2 ** 31 - 1:
        raise ValueError(f"a grid of shape {shape} has more than 2^31 - 1 voxels")
    if not isinstance(seeds, torch.Tensor):
        seeds = torch.as_tensor(seeds, dtype=torch.int32).reshape(-1, 3).to(device)
    if seeds.dtype != torch.int32:
        raise TypeError(f"seeds must be torch.int32, not {seeds.dtype}")
    if seeds.dim() != 2 or seeds.shape[1] != 3:
        raise ValueError(f"seeds must have shape [n, 3] (x, y, z), not {tuple(seeds.shape)}")
    if seeds.device != device:
        raise ValueError(f"seeds is on {seeds.device}, not on {device}")
    nz, ny, nx = shape
    s = seeds.to(torch.int64)
    inside = (s[:, 0] >= 0) & (s[:, 0] < nx) & (s[:, 1] >= 0) & (s[:, 1] < ny) & (s[:, 2] >= 0) & (s[:, 2] < nz)
    index = ((s[:, 2] * ny + s[:, 1]) * nx + s[:, 0])[inside]
    label = (torch.arange(seeds.shape[0], dtype=torch.int64, device=device) + 1)[inside]
    flat = torch.full((nz * ny * nx,), 2 ** 31, dtype=torch.int64, device=device)
    flat.scatter_reduce_(0, index, label, "amin")
    flat[flat == 2 ** 31] = 0
    return flat.to(torch.int32).reshape(shape)
