"""Skeletons of dense grids by topological thinning on the voxelizer's device (o2v_hip_thin_dense): the
torch layer, which obj2voxel_amd.dense re-exports as dense.skeletonize and dense.skeleton_nodes beside local_thickness.  It takes
its grid through dense's _set_grid and waits on the voxelizer's device (dense._sync) before the library call, as every function of
dense.py does; tests/test_host_thinning.py holds that wait.

torch is imported first on purpose (see obj2voxel_amd/dense.py)."""
import numbers

import torch  # first

from . import hip

_THIN_MODES = {"ultimate": hip.THIN_ULTIMATE, "curve": hip.THIN_CURVE}
_THIN_FORMATS = {"mask": (hip.THIN_DST_MASK, torch.bool), "degree": (hip.THIN_DST_DEGREE, torch.uint8)}


def skeletonize(dv, grid, *, mode="curve", level=None, background=False, keep=None, max_iterations=None, fmt="mask", out=None):
    """The skeleton of the set by topological thinning: simple voxels - those whose removal changes neither
    the 26-connected components of the set nor the 6-connected ones of the background in their 3^3 block - are removed from the
    border, subfield by subfield, until none is left.  Components, cavities and tunnels stay as they are, and the result is the
    same bits on every run.  Returns the tensor [z, y, x].

        solid, origin = dense.voxelize_dense(dv, 512, fill=True)
        degree = dense.skeletonize(dv, solid, fmt="degree")           # uint8: 0, or 1 + the skeleton voxel's neighbours
        ends, junctions = dense.skeleton_nodes(degree)                # int32 [n, 3] (x, y, z) each

    grid, level, background:  as components takes them: the set is the solid voxels, or with background=True the others (the pore
                     and channel space).  Voxels outside the box are background.
    mode:            "curve": end points (voxels with exactly one neighbour) stay, so arms stay - centrelines; "ultimate": no end
                     points - a ball becomes one voxel, a torus a closed loop, a hollow shell a closed one-voxel surface.  With
                     max_iterations=n "ultimate" is an erosion by n layers that cannot break or merge anything.
    keep:            None, or a bool / uint8 tensor of the voxel shape (any strides): non-zero means never removed - anchors, such
                     as local_thickness's thickest voxels or seeds.
    max_iterations:  None: until an iteration removes nothing; else an integer 1 .. 2^32 - 1.
    fmt:             "mask": bool; "degree": uint8, 0 outside the skeleton and 1 + the number of 26-neighbours in it inside: 1 is
                     isolated, 2 an end, 3 a plain curve voxel, 4 or more a junction.
    out:             any 3-D view of the voxel shape and fmt's dtype (uint8 will do for "mask": 1 / 0), written as it is - the grid
                     itself thins in place (bool or uint8 grids); else a new contiguous tensor.
    The result depends on the parity of the box's origin, and the end-point rule keeps spurs at the corners of blocky shapes."""
    from . import dense   # (at call time: dense imports this module)
    device, gfmt, level, dims = dense._set_grid(dv, grid, level, dense._limit_voxels)
    shape = (dims[2], dims[1], dims[0])
    if mode not in _THIN_MODES:
        raise ValueError(f"mode must be one of {sorted(_THIN_MODES)}, not {mode!r}")
    if fmt not in _THIN_FORMATS:
        raise ValueError(f"fmt must be one of {sorted(_THIN_FORMATS)}, not {fmt!r}")
    dst_format, dtype = _THIN_FORMATS[fmt]
    if max_iterations is None:
        max_iterations = 0
    elif isinstance(max_iterations, bool) or not isinstance(max_iterations, numbers.Integral) or not 1 <= max_iterations <= 2 ** 32 - 1:
        raise ValueError(f"max_iterations must be None or an integer 1 .. {2 ** 32 - 1}, not {max_iterations!r}")
    if keep is not None:
        if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.bool, torch.uint8):
            raise TypeError("keep must be a torch.bool or torch.uint8 tensor")
        dense._check_grid(keep, "keep", keep.dtype, device, shape)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=device)
    else:
        # (a mask may go to a uint8 tensor as 1 / 0: a uint8 grid thins in place)
        dense._check_grid(out, "out", torch.uint8 if isinstance(out, torch.Tensor) and out.dtype == torch.uint8 else dtype, device, shape)
        in_place = gfmt == hip.GRID_U8 and out.data_ptr() == grid.data_ptr() and out.stride() == grid.stride()
        if not in_place and dense._byte_ranges_overlap(out, grid):
            raise ValueError("out must not overlap grid, unless it is the grid itself")
        if keep is not None and dense._byte_ranges_overlap(out, keep):
            raise ValueError("out must not overlap keep")
    dense._sync(device)   # (the caller's writes to grid, keep and out have landed)
    dv.thin_dense(grid.data_ptr(), gfmt, dense._strides(grid), dims, 0.0 if level is None else level, hip.CC_INVERT if background else 0, _THIN_MODES[mode],
                  int(max_iterations), dense._ptr(keep), None if keep is None else dense._strides(keep), out.data_ptr(), dense._strides(out), dst_format)
    return out


def skeleton_nodes(degree):
    """(end points, junctions) of skeletonize's fmt="degree" grid: two int32 tensors [n, 3] of (x, y, z), the voxels of degree 2 and
    of degree 4 or more, in [z, y, x] order.  Plain torch on the degree grid."""
    if not isinstance(degree, torch.Tensor) or degree.dim() != 3 or degree.dtype != torch.uint8:
        raise ValueError("degree must be a 3-D torch.uint8 tensor [z, y, x]")
    return tuple(torch.nonzero(m).flip(1).to(torch.int32) for m in (degree == 2, degree >= 4))
