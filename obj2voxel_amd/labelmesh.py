"""Smooth meshes of label grids on the voxelizer's device (o2v_hip_label_surface_count / _write / _relax): the
torch layer, which obj2voxel_amd.dense re-exports as dense.label_surfaces, dense.relax_surface, dense.part_mesh and
dense.interface_areas.  It waits on the voxelizer's device (dense._sync) before the library calls, as every function of dense.py
does.

torch is imported first on purpose (see obj2voxel_amd/dense.py)."""
import dataclasses
import numbers

import torch  # first

from . import hip

MAX_ITERATIONS = 1024
MAX_EXTENT = 65536   # origin + shape (+ 1 if closed) per axis: a cell's centre is an exact float32


@dataclasses.dataclass(frozen=True)
class LabelMesh:
    """What label_surfaces returns: the surface nets of a label grid, one mesh for all its parts.  All tensors are new, contiguous
    and on the grid's device; with nothing active they are empty, of these shapes."""
    positions: torch.Tensor   # float32 [V, 3]: the vertices (x, y, z), in voxel space unless a transform was given
    faces: torch.Tensor       # int32 [2 Q, 3]: triangles 2 n and 2 n + 1 are quad n; the normal points from the larger label to the smaller
    pairs: torch.Tensor       # int32 [Q, 2]: the two labels (hi, lo) that quad n lies between
    cells: torch.Tensor       # int32 [V, 3]: the cell (i, j, k) of a vertex, named by its lowest sample; -1 at the lower sides if closed
    links: torch.Tensor       # int32 [V, 6]: the vertices next to it in the net towards -x, +x, -y, +y, -z, +z; -1: none
    origin: tuple = (0, 0, 0)  # the origin the positions were made with


def _iterations(iterations):
    if isinstance(iterations, bool) or not isinstance(iterations, numbers.Integral) or not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"iterations must be an integer 0 ... {MAX_ITERATIONS}, not {iterations!r}")
    return int(iterations)


def _weights(relaxation, reach):
    """relaxation and reach as the float32 values the library gets."""
    for name, v in (("relaxation", relaxation), ("reach", reach)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise ValueError(f"{name} must be a number, not {v!r}")
    relaxation, reach = hip.C.c_float(float(relaxation)).value, hip.C.c_float(float(reach)).value
    if not 0.0 < relaxation <= 1.0:
        raise ValueError(f"relaxation must be above 0 and at most 1, not {relaxation!r}")
    if not 0.0 <= reach <= 0.5:
        raise ValueError(f"reach must be 0 ... 0.5, not {reach!r}")
    return relaxation, reach


def _relax(dv, cells, links, origin, iterations, relaxation, reach, transform, supersampling):
    from . import dense
    n = cells.shape[0]
    positions = torch.empty((n, 3), dtype=torch.float32, device=cells.device)
    if n:
        dv.label_surface_relax(cells.data_ptr(), links.data_ptr(), n, origin, iterations, relaxation, reach, positions.data_ptr())
    return dense._to_model_space(positions, transform, supersampling)


def label_surfaces(dv, labels, *, origin=(0, 0, 0), closed=True, iterations=0, relaxation=0.5, reach=0.5, transform=None, supersampling=1):
    """The interfaces between the parts of a label grid as one indexed mesh, by surface nets on labels: one
    vertex per cell of 2 x 2 x 2 samples that are not all equal, one quad (two triangles) per pair of face-adjacent samples with
    different labels, so the wall between two parts is meshed once and their meshes share its vertices; then `iterations` steps
    that move every vertex towards its neighbours in the net, never out of its cell.  Returns a LabelMesh.

        parts, n = dense.split_parts(dv, solid)
        mesh = dense.label_surfaces(dv, parts, iterations=8)
        for label in range(1, n + 1):
            dense.save_mesh(f"part{label}.ply", *dense.part_mesh(mesh, label))     # watertight, one per part
        pairs, areas = dense.interface_areas(mesh)                                   # the wall between every two parts, in voxel faces

    labels:      int32, uint8 or bool, any 3-D view [z, y, x] on the voxelizer's device, as label_stats takes it; it is only read.
                 Labels are compared as int32: any value is a label, 0 is the background only in that the outside of the box has it.
    origin:      (ox, oy, oz), the one the grid came with: sample (x, y, z) is the voxel centre origin + (x, y, z) + 0.5.
    closed:      True: the box is surrounded by label 0, so every part is capped where it touches a side of the box and every
                 part_mesh is watertight.  False: a surface that leaves the box is open there, as extract_surface's.
    iterations:  0 ... 1024 Jacobi steps; 0: every vertex at its cell's centre, the blocky net (its volume per label is the voxel count).
    relaxation:  (0, 1]: how far a step moves a vertex towards the mean of its linked neighbours.
    reach:       [0, 0.5]: how far a vertex may leave its cell's centre, per axis.  With 0.5 a feature one voxel wide collapses as
                 the iterations go on (the eight vertices of a single voxel meet in its centre); 0.25 keeps it at half its size.
                 The relaxation is Laplacian smoothing: it shrinks noisy labels, and nothing corrects that.
    transform, supersampling:  as extract_surface takes them: positions in model space."""
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
    if not isinstance(closed, bool):
        raise ValueError(f"closed must be True or False, not {closed!r}")
    if supersampling not in (1, 2):
        raise ValueError("supersampling must be 1 or 2")
    iterations = _iterations(iterations)
    relaxation, reach = _weights(relaxation, reach)
    origin = dense._origin(origin)
    transform = dense._mesh_transform(transform)
    nz, ny, nx = labels.shape
    dims = (nx, ny, nz)
    if any(o + n + closed > MAX_EXTENT for o, n in zip(origin, dims)):
        raise ValueError(f"origin {origin} + labels' extent {dims} [x, y, z]{' + 1 (closed)' if closed else ''} is above {MAX_EXTENT}")
    flags = hip.LABEL_SURFACE_CLOSED if closed else 0
    args = (labels.data_ptr(), hip.LABELS_I32 if labels.dtype == torch.int32 else hip.LABELS_U8, dense._strides(labels), dims, flags)
    dense._sync(device)   # (the caller's writes to labels have landed)
    n_vertices, n_quads = dv.label_surface_count(*args)
    cells = torch.empty((n_vertices, 3), dtype=torch.int32, device=device)
    links = torch.empty((n_vertices, 6), dtype=torch.int32, device=device)
    faces = torch.empty((2 * n_quads, 3), dtype=torch.int32, device=device)
    pairs = torch.empty((n_quads, 2), dtype=torch.int32, device=device)
    if n_vertices:
        dv.label_surface_write(*args, cells.data_ptr(), links.data_ptr(), n_vertices, faces.data_ptr() if n_quads else None,
                               pairs.data_ptr() if n_quads else None, n_quads)
    positions = _relax(dv, cells, links, origin, iterations, relaxation, reach, transform, supersampling)
    return LabelMesh(positions=positions, faces=faces, pairs=pairs, cells=cells, links=links, origin=origin)


def _mesh(mesh):
    if not isinstance(mesh, LabelMesh):
        raise TypeError("mesh must be a LabelMesh, what label_surfaces returns")
    return mesh


def relax_surface(dv, mesh, iterations, *, relaxation=0.5, reach=0.5, origin=None, transform=None, supersampling=1):
    """The LabelMesh `mesh` with its positions computed anew: `iterations` steps from the cells' centres, exactly those that
    label_surfaces(iterations=...) makes, without touching the grid - a kept net can be smoothed more, or less, at the cost of
    the relaxation alone.  origin: None: the one the mesh was made with.  Everything but the positions is shared with `mesh`."""
    from . import dense
    dense._require_shared_runtime()
    device = dense._device(dv)
    mesh = _mesh(mesh)
    n = mesh.cells.shape[0]
    dense._check(mesh.cells, "mesh.cells", (torch.int32,), (n, 3), device)
    dense._check(mesh.links, "mesh.links", (torch.int32,), (n, 6), device)
    if supersampling not in (1, 2):
        raise ValueError("supersampling must be 1 or 2")
    iterations = _iterations(iterations)
    relaxation, reach = _weights(relaxation, reach)
    origin = mesh.origin if origin is None else dense._origin(origin)
    transform = dense._mesh_transform(transform)
    dense._sync(device)
    positions = _relax(dv, mesh.cells.contiguous(), mesh.links.contiguous(), origin, iterations, relaxation, reach, transform, supersampling)
    return dataclasses.replace(mesh, positions=positions, origin=origin)


def part_mesh(mesh, label):
    """(positions float32 [v, 3], faces int32 [t, 3]) of one label, in the form set_mesh and save_mesh take: the quads with `label`
    on either side - turned over where it is the smaller of the two, so that every normal points out of the part -, the vertices
    none of them uses dropped and the rest renumbered in their order.  The meshes of two parts hold the wall between them with the
    same positions and opposite normals.  Plain torch on the mesh's device."""
    mesh = _mesh(mesh)
    if isinstance(label, bool) or not isinstance(label, numbers.Integral) or not -2 ** 31 <= label < 2 ** 31:
        raise ValueError(f"label must be an int32 value, not {label!r}")
    hi, lo = mesh.pairs[:, 0] == label, mesh.pairs[:, 1] == label
    keep = (hi | lo).repeat_interleave(2)
    turn = (lo & ~hi).repeat_interleave(2)[keep]
    faces = mesh.faces[keep].to(torch.int64)
    faces = torch.where(turn[:, None], faces[:, [0, 2, 1]], faces)
    used = torch.zeros(mesh.positions.shape[0], dtype=torch.bool, device=faces.device)
    used[faces.reshape(-1)] = True
    number = torch.cumsum(used, dim=0) - 1
    return mesh.positions[used].contiguous(), number[faces].to(torch.int32).contiguous()


def interface_areas(mesh):
    """(pairs int32 [P, 2], areas float64 [P]): the distinct pairs (hi, lo) of the mesh's quads in ascending order, and the area of
    each pair's triangles, in the units of the positions: how much wall two parts share; lo == 0 is a part's outer skin.  With 0
    iterations in voxel space the area is the number of voxel faces, label_adjacency's `faces`.  Plain torch on the mesh's device."""
    mesh = _mesh(mesh)
    device = mesh.pairs.device
    if not mesh.pairs.shape[0]:
        return torch.empty((0, 2), dtype=torch.int32, device=device), torch.empty((0,), dtype=torch.float64, device=device)
    pairs, which = torch.unique(mesh.pairs, dim=0, return_inverse=True)
    p = mesh.positions.to(torch.float64)[mesh.faces.to(torch.int64)]   # [2 Q, 3 corners, 3]
    tri = 0.5 * torch.linalg.norm(torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1), dim=1)
    areas = torch.zeros(pairs.shape[0], dtype=torch.float64, device=device)
    areas.index_add_(0, which.reshape(-1), tri[0::2] + tri[1::2])
    return pairs, areas
