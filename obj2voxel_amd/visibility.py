"""Sky visibility and ambient occlusion of dense grids on the voxelizer's device (o2v_hip_openness): the torch
layer, which obj2voxel_amd.dense re-exports as dense.direction_set, dense.openness and dense.shade_colors.  openness waits on the
voxelizer's device (dense._sync) before the library call, as every function of dense.py does; tests/test_host_openness.py holds
that wait.  direction_set needs no device, shade_colors is plain torch.

torch is imported first on purpose (see obj2voxel_amd/dense.py)."""
import math
import numbers

import torch  # first

from . import hip

NOT_A_TARGET = 255                                   # openness: the count of a voxel that is no target
MAX_DIRECTIONS = hip.OPEN_MAX_DIRECTIONS             # ... directions in one call
MAX_COMPONENT = hip.OPEN_MAX_COMPONENT               # ... the magnitude of a direction's component
MAX_MASK_DIRECTIONS = 64                             # ... directions with mask=True: a bit each of an int64
_SET_RADIUS = {6: 1, 26: 1, 98: 2, 290: 3}
_MODES = {"surface": hip.OPEN_SURFACE, "solid": hip.OPEN_SOLID, "empty": hip.OPEN_EMPTY}


def direction_set(n):
    """int32 [n, 3] of (dx, dy, dz): the primitive integer vectors - no common divisor - with components up to 1, 1, 2, 3 in
    magnitude for n = 26, 98, 290, and the six axes alone for n = 6, in ascending order of (dz, dy, dx), which fixes the bit order
    of openness' mask.  A CPU tensor; needs no device."""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n not in _SET_RADIUS:
        raise ValueError(f"a direction set has 6, 26, 98 or 290 directions, not {n!r}")
    r = _SET_RADIUS[n]
    rows = [(dx, dy, dz) for dz in range(-r, r + 1) for dy in range(-r, r + 1) for dx in range(-r, r + 1)
            if math.gcd(math.gcd(abs(dx), abs(dy)), abs(dz)) == 1 and (n != 6 or abs(dx) + abs(dy) + abs(dz) == 1)]
    return torch.tensor(rows, dtype=torch.int32)


def _directions(directions):
    """The rows (dx, dy, dz) of a set size, an int tensor [D, 3] or a list of triples, as Python ints, checked."""
    if isinstance(directions, numbers.Integral) and not isinstance(directions, bool):
        directions = direction_set(int(directions))
    if isinstance(directions, torch.Tensor):
        if directions.dim() != 2 or directions.shape[1] != 3:
            raise ValueError(f"directions must have shape [D, 3], not {tuple(directions.shape)}")
        if directions.dtype.is_floating_point or directions.dtype.is_complex or directions.dtype == torch.bool:
            raise TypeError(f"directions must be integers, not {directions.dtype}")
        directions = directions.tolist()
    if not isinstance(directions, (list, tuple)):
        raise ValueError(f"directions must be 6, 26 or 98, an int tensor [D, 3] or a list of (dx, dy, dz), not {directions!r}")
    rows = []
    for d in directions:
        d = tuple(d) if isinstance(d, (list, tuple)) else (d,)
        if len(d) != 3 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in d):
            raise ValueError(f"a direction must be three integers (dx, dy, dz), not {d!r}")
        d = tuple(int(v) for v in d)
        if d == (0, 0, 0) or max(abs(v) for v in d) > MAX_COMPONENT:
            raise ValueError(f"direction {d} is zero or has a component above {MAX_COMPONENT} in magnitude")
        rows.append(d)
    if not 1 <= len(rows) <= MAX_DIRECTIONS:
        raise ValueError(f"{len(rows)} directions: a call takes 1 ... {MAX_DIRECTIONS}")
    return rows


def openness(dv, grid, *, level=None, directions=26, targets="surface", max_distance=None, mask=False, out=None):
    """In how many directions one sees out from each voxel of a dense grid, on the voxelizer's device: a
    uint8 tensor [z, y, x] with the number of open directions of every target voxel and 255 elsewhere; with mask=True
    (count, mask), mask int64 [z, y, x] with bit i set where direction i is open.  Everything is an integer; one run equals
    another bit for bit.

        solid, _ = dense.voxelize_dense(dv, 512, fill=True)
        count = dense.openness(dv, solid, directions=98, max_distance=16)             # ambient occlusion of the surface voxels
        argb = dense.shade_colors(argb, count, 98)
        shadow = dense.openness(dv, solid, directions=[(1, 2, 3)]) == 0               # a sun shadow

    A ray starts at the voxel's centre and runs along an integer direction; it is open if it leaves the grid, or gets farther
    than max_distance voxels, before it passes through the open interior of a solid voxel (a ray along an edge or through a
    corner of a voxel is not blocked by it).  The start voxel is never tested.

    grid, level:   the set as RayCaster takes it; it is only read.
    directions:    6, 26, 98 or 290 (direction_set), or an int tensor [D, 3] or list of (dx, dy, dz), D <= 254, components up to
                   127 in magnitude.
    targets:       "surface" (solid voxels with an empty one among the six neighbours, outside the grid counting as empty),
                   "solid", "empty", or a bool tensor of the grid's shape on the device.
    max_distance:  r: a ray is open once k_x^2 + k_y^2 + k_z^2 > floor(r * r), k the voxels it has moved per axis; None: unlimited.
    mask:          also the directions as bits, D <= 64.
    out:           a uint8 tensor of the grid's voxel shape (any strides that keep the voxels apart) to write into; it is returned."""
    from . import dense   # (at call time: dense imports this module)
    device, fmt, level, dims = dense._set_grid(dv, grid, level, dense._limit_voxels)
    shape = dims[::-1]
    rows = _directions(directions)
    if not isinstance(mask, bool):
        raise ValueError(f"mask must be True or False, not {mask!r}")
    if mask and len(rows) > MAX_MASK_DIRECTIONS:
        raise ValueError(f"a mask holds {MAX_MASK_DIRECTIONS} directions, not {len(rows)}")
    target_ptr = target_strides = None
    if isinstance(targets, str):
        if targets not in _MODES:
            raise ValueError(f"targets must be 'surface', 'solid', 'empty' or a bool tensor, not {targets!r}")
        mode = _MODES[targets]
    else:
        dense._check_grid(targets, "targets", torch.bool, device, shape)
        mode, target_ptr, target_strides = hip.OPEN_GRID, targets.data_ptr(), dense._strides(targets)
    md2 = 0
    if max_distance is not None:
        if isinstance(max_distance, bool) or not isinstance(max_distance, numbers.Real) or not 1.0 <= float(max_distance) < 65536.0:
            raise ValueError(f"max_distance must be a number in [1, 65536) or None, not {max_distance!r}")
        md2 = int(math.floor(float(max_distance) * float(max_distance)))
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=device)
    else:
        dense._check_grid(out, "out", torch.uint8, device, shape)
    bits = torch.empty(shape, dtype=torch.int64, device=device) if mask else None
    dense._sync(device)   # (the caller's writes to grid and targets have landed, its reads of out are done)
    dv.openness(grid.data_ptr(), fmt, dense._strides(grid), dims, 0.0 if level is None else level, rows, mode, target_ptr, target_strides, md2,
                out.data_ptr(), dense._strides(out), None if bits is None else bits.data_ptr(), None if bits is None else dense._strides(bits))
    return (out, bits) if mask else out


def shade_colors(argb, count, n_directions, *, ambient=64, hemisphere=True, out=None):
    """Ambient occlusion baked into colours: int32 ARGB of `argb` darkened by `count`, what openness gave for n_directions
    directions, where count != 255; other voxels and every alpha are kept.  With D = n_directions and f = min(2 * count, D) if
    hemisphere - a voxel on an open plane sees half of the directions and keeps its colour - else count, each of r, g, b becomes
    (ch * (ambient * D + (256 - ambient) * f) + 128 * D) // (256 * D): ambient / 256 of the colour where nothing is open, all of
    it where f = D.  Plain torch in int64, on CPU or device tensors of one shape; out: an int32 tensor to write into."""
    if not isinstance(argb, torch.Tensor) or argb.dtype != torch.int32:
        raise TypeError("argb must be an int32 tensor")
    if not isinstance(count, torch.Tensor) or count.dtype != torch.uint8:
        raise TypeError("count must be a uint8 tensor, what openness returns")
    if count.shape != argb.shape or count.device != argb.device:
        raise ValueError("argb and count must have one shape and one device")
    if isinstance(n_directions, bool) or not isinstance(n_directions, numbers.Integral) or not 1 <= n_directions <= MAX_DIRECTIONS:
        raise ValueError(f"n_directions must be an integer 1 ... {MAX_DIRECTIONS}, not {n_directions!r}")
    if isinstance(ambient, bool) or not isinstance(ambient, numbers.Integral) or not 0 <= ambient <= 256:
        raise ValueError(f"ambient must be an integer 0 ... 256, not {ambient!r}")
    if not isinstance(hemisphere, bool):
        raise ValueError(f"hemisphere must be True or False, not {hemisphere!r}")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.shape != argb.shape or out.device != argb.device):
        raise ValueError("out must be an int32 tensor of argb's shape on its device")
    D = int(n_directions)
    c = count.to(torch.int64)
    f = torch.clamp(2 * c, max=D) if hemisphere else torch.clamp(c, max=D)
    w = int(ambient) * D + (256 - int(ambient)) * f
    v = argb.to(torch.int64) & 0xffffffff
    shaded = v & 0xff000000
    for shift in (16, 8, 0):
        shaded = shaded | ((((v >> shift) & 0xff) * w + 128 * D) // (256 * D)) << shift
    shaded = torch.where(count != NOT_A_TARGET, shaded, v)
    shaded = torch.where(shaded >= 2 ** 31, shaded - 2 ** 32, shaded).to(torch.int32)
    if out is None:
        return shaded
    out.copy_(shaded)
    return out
