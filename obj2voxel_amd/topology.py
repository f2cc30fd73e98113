"""Euler numbers, tunnels and cavities of label grids on the voxelizer's device (o2v_hip_euler_stats): the
torch layer, which obj2voxel_amd.dense re-exports as dense.euler_stats, dense.euler_numbers, dense.intrinsic_volumes and
dense.betti_numbers beside label_adjacency.  It waits on the voxelizer's device (dense._sync) before the library call, as every
function of dense.py does; tests/test_host_topology.py holds that wait.

torch is imported first on purpose (see obj2voxel_amd/dense.py)."""
import dataclasses
import numbers

import torch  # first

from . import hip


@dataclasses.dataclass(frozen=True)
class EulerStats:
    """What euler_stats returns: row L of every tensor is for the value L of the grid, row 0 like every other; all int64 [n + 1],
    on the grid's device, exact.  The cells are those of the unit lattice of the box: a cell is closed-in for L if one of the
    voxels it touches holds L, inner if all the positions it touches lie in the box and hold L."""
    voxels: torch.Tensor           # n3
    faces: torch.Tensor            # n2: closed-in faces
    edges: torch.Tensor            # n1: closed-in edges
    vertices: torch.Tensor         # n0: closed-in vertices
    inner_faces: torch.Tensor      # face-adjacent pairs of voxels that both hold L
    inner_edges: torch.Tensor      # 2 x 2 x 1 blocks that hold L throughout
    inner_vertices: torch.Tensor   # 2 x 2 x 2 blocks that hold L throughout
    outside: int                   # the voxels whose value is negative or above n: they are in no row
    n: int                         # the highest value that has a row


def euler_stats(dv, labels, n=None):
    """The cell counts of every value of a label grid, in one read of it on the voxelizer's device: an
    EulerStats.  Everything is an integer and exact; one run equals another bit for bit.

        labels, n = dense.components(dv, solid, connectivity=26)
        st = dense.euler_stats(dv, labels, n)
        dense.euler_numbers(st)[1:]                  # per component: 1 - its tunnels + its cavities
        dense.betti_numbers(dv, solid)               # (components, tunnels, cavities) of the whole set

    labels:  int32, uint8 or bool, any 3-D view [z, y, x], as label_stats takes it; it is only read.
    n:       the highest value that has a row; None: 255 for uint8, 1 for bool, max(labels.max(), 0) for int32 (a device reduction
             and a wait).  A voxel whose value is negative or above n is counted in `outside` and nowhere else."""
    from . import dense   # (at call time: dense imports this module)
    dense._require_shared_runtime()
    device = dense._device(dv)
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3:
        raise ValueError("labels must be a 3-D tensor [z, y, x]")
    if labels.dtype not in (torch.int32, torch.uint8, torch.bool):
        raise TypeError(f"labels must be int32, uint8 or bool, not {labels.dtype}")
    dense._check_grid(labels, "labels", labels.dtype, device)
    if 0 in labels.shape:
        raise ValueError("labels has an empty dimension")
    nz, ny, nx = labels.shape
    dims = (nx, ny, nz)
    dense._limit_voxels(dims)
    top = dense.MAX_STATS_LABELS if labels.dtype == torch.int32 else 1 if labels.dtype == torch.bool else 255
    if n is None:
        n = max(int(labels.max()), 0) if labels.dtype == torch.int32 else top
    elif isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 0 <= n <= top:
        raise ValueError(f"n must be an integer 0 ... {top} for {labels.dtype} labels, not {n!r}")
    n = int(n)
    table = torch.empty((n + 1, hip.EULER_COLUMNS), dtype=torch.int64, device=device)
    dense._sync(device)   # (the caller's writes to labels have landed)
    outside = dv.euler_stats(labels.data_ptr(), hip.LABELS_I32 if labels.dtype == torch.int32 else hip.LABELS_U8, dense._strides(labels), dims, n,
                             table.data_ptr())
    return EulerStats(voxels=table[:, 0], faces=table[:, 1], edges=table[:, 2], vertices=table[:, 3], inner_faces=table[:, 4], inner_edges=table[:, 5],
                      inner_vertices=table[:, 6], outside=outside, n=n)


def _stats(stats):
    if not isinstance(stats, EulerStats):
        raise TypeError("stats must be an EulerStats, what euler_stats returns")
    return stats


def _connectivity(connectivity):
    if isinstance(connectivity, bool) or connectivity not in (6, 26):
        if connectivity == 18 and not isinstance(connectivity, bool):
            raise ValueError("connectivity must be 6 or 26: no cell complex of this kind models 18-connectivity")
        raise ValueError(f"connectivity must be 6 or 26, not {connectivity!r}")
    return connectivity


def euler_numbers(stats, connectivity=26):
    """int64 [n + 1]: the Euler characteristic of every value's voxels.  26: vertices - edges + faces - voxels of the closed-in
    cells - the set as a union of closed cubes; 6: voxels - inner faces + inner edges - inner vertices - the dual complex, voxels
    joined through faces only.  For a set of b0 components, b1 tunnels and b2 cavities it is b0 - b1 + b2.  Plain torch."""
    s = _stats(stats)
    if _connectivity(connectivity) == 26:
        return s.vertices - s.edges + s.faces - s.voxels
    return s.voxels - s.inner_faces + s.inner_edges - s.inner_vertices


def intrinsic_volumes(stats):
    """int64 [n + 1, 4]: (V0, V1, V2, V3) of every value's voxels as a union of closed unit cubes: the Euler characteristic, the
    integral of mean breadth edges - 2 faces + 3 voxels, half the surface area faces - 3 voxels, the volume.  Plain torch."""
    s = _stats(stats)
    return torch.stack([s.vertices - s.edges + s.faces - s.voxels, s.edges - 2 * s.faces + 3 * s.voxels, s.faces - 3 * s.voxels, s.voxels], dim=1)


def betti_numbers(dv, grid, *, level=None, connectivity=26, background=False):
    """(b0, b1, b2) of a set grid, as Python ints: its components, tunnels and cavities at `connectivity`.

        dense.betti_numbers(dv, solid)               # a torus: (1, 1, 0); a hollow sphere: (1, 0, 1)

    grid, level, background:  the set as components takes it.  What lies outside the box is not in the set.
    connectivity:  26, or 6; the complement is then read at the dual connectivity, 6 or 26.

    b0 is the n of components; the Euler characteristic chi is the sum over the components of euler_numbers of their labels
    (components share no cell at their own connectivity, so the rows add); b2 is the number of components of the complement whose
    box touches no side of the grid; b1 = b0 + b2 - chi."""
    from . import dense
    connectivity = _connectivity(connectivity)
    if not isinstance(background, bool):
        raise ValueError(f"background must be True or False, not {background!r}")
    labels, b0 = dense.components(dv, grid, level=level, connectivity=connectivity, background=background)
    chi = int(euler_numbers(euler_stats(dv, labels, b0), connectivity)[1:].sum())
    rest, m = dense.components(dv, grid, level=level, connectivity=32 - connectivity, background=not background)
    box = dense.label_stats(dv, rest, m, sums=False)
    nz, ny, nx = rest.shape
    far = torch.tensor([nx, ny, nz], dtype=torch.int64, device=box.lo.device)
    open_ = ((box.lo[1:] == 0) | (box.hi[1:] == far)).any(dim=1)
    b2 = m - int(open_.sum())
    return b0, b0 + b2 - chi, b2
