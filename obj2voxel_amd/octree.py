"""Sparse voxel octrees of dense grids on the voxelizer's device (o2v_hip_octree_build / _write / _lookup / _to_dense, DESIGN.md
section 30): the torch layer, which obj2voxel_amd.dense re-exports as dense.Octree, dense.build_octree, dense.octree_lookup,
dense.octree_to_dense, dense.octree_level and dense.octree_depth; the DAG of section 34 (OctreeDag, octree_dag, dag_lookup,
dag_to_dense) and the rays of section 35 (octree_raycast, dag_raycast) are here too.  It waits on the voxelizer's device (dense._sync) before every
library call, as every function of dense.py does; tests/test_host_octree.py holds that wait.

torch is imported first on purpose (see obj2voxel_amd/dense.py)."""
import dataclasses
import numbers

import torch  # first

from . import hip

MAX_OCTREE_DEPTH = hip.OCT_MAX_DEPTH
MAX_OCTREE_EXTENT = 2 ** MAX_OCTREE_DEPTH   # build_octree: origin + extent per axis, the root cube of the deepest tree
MAX_OCTREE_POINTS = 2 ** 31 - 1             # octree_lookup: points per call; octree_to_dense: voxels per call


@dataclasses.dataclass(frozen=True)
class Octree:
    """What build_octree returns (the definition: include/o2v_hip.h).  The root cube is [0, 2^depth)^3 of the global lattice; node
    i is a cell of side 2^(depth - l) for the level l with level_offsets[l] <= i < level_offsets[l + 1]; within a level the nodes
    are in Morton order, and the stored children of a node are contiguous from first_child[i] on."""
    valid: torch.Tensor            # uint8 [N]: bit o = dx + 2 dy + 4 dz is set iff child octant o holds a solid voxel
    full: torch.Tensor             # uint8 [N]: ... iff it is solid throughout
    first_child: torch.Tensor      # int32 [N]: the first stored child (-1: none); at level depth - 1 the index of the node's first voxel
    coords: object                 # int32 [N, 3]: the low corner (x, y, z) of the node's cell, or None
    level_offsets: tuple           # depth + 1 Python ints: level l is [level_offsets[l], level_offsets[l + 1])
    depth: int
    collapsed: bool                # full cells are leaves: nothing below them is stored
    voxels_listed: int             # the solid voxels under the nodes of level depth - 1: the length of a per-voxel attribute array


def _flag(value, name):
    if not isinstance(value, bool):
        raise ValueError(f"{name} must be True or False, not {value!r}")
    return value


def octree_depth(origin, shape):
    """The smallest depth whose root cube [0, 2^depth)^3 holds the box of `shape` (nz, ny, nx) voxels whose voxel (0, 0, 0) is
    `origin` (x, y, z) of the global lattice: at least 1.  Needs no device."""
    from . import dense   # (at call time: dense imports this module)
    origin = dense._origin(origin)
    shape = tuple(int(n) for n in shape)
    if len(shape) != 3 or any(n < 1 for n in shape):
        raise ValueError(f"shape {shape} must be three positive extents (nz, ny, nx)")
    top = max(o + n for o, n in zip(origin, shape[::-1]))
    if top > MAX_OCTREE_EXTENT:
        raise ValueError(f"origin {origin} + the extent {shape[::-1]} [x, y, z] is above {MAX_OCTREE_EXTENT}, the root cube of depth {MAX_OCTREE_DEPTH}")
    return max(1, (top - 1).bit_length())


def build_octree(dv, grid, *, level=None, origin=(0, 0, 0), depth=None, collapse=True, coords=False):
    """The sparse voxel octree of a dense grid, built on the voxelizer's device in one read of the grid: an
    Octree.  Everything is an integer; one run equals another bit for bit.

        tree = dense.build_octree(dv, labels)                        # labels of voxelize_dense(..., fmt="labels", fill=True)
        hit = dense.octree_lookup(dv, tree, points)                  # int32 [n, 4] = (solid, level, node, voxel_index)
        solid = dense.octree_to_dense(dv, tree, labels.shape)        # == (labels != 0)
        rec = dense.to_voxels(dv, labels, palette=palette)
        argb = torch.empty(tree.voxels_listed, dtype=torch.int32, device=rec.device).scatter_(
            0, dense.octree_lookup(dv, tree, rec[:, :3])[:, 3].long(), rec[:, 3])   # (collapse=False: every voxel has a slot)

    grid, level:  the set as to_voxels takes it; it is only read.
    origin:   (x, y, z) of the grid's voxel (0, 0, 0) on the global lattice, on which the root cube [0, 2^depth)^3 sits: trees of
              different boxes of one model line up with each other and with downsample's levels.
    depth:    1 ... 16 with origin + extent <= 2^depth; None: the smallest, octree_depth(origin, grid's voxel shape).
    collapse: full cells are leaves - the tree's size follows the surface of a solid, not its volume - and the voxels inside them
              have no voxel_index; False: every non-empty cell down to level depth - 1 is a node.
    coords:   also the low corners of the nodes' cells, int32 [N, 3]."""
    from . import dense
    device, fmt, level, dims = dense._set_grid(dv, grid, level, dense._limit_voxels)
    origin = dense._origin(origin)
    smallest = octree_depth(origin, dims[::-1])
    if depth is not None:
        if isinstance(depth, bool) or not isinstance(depth, numbers.Integral) or not 1 <= depth <= MAX_OCTREE_DEPTH:
            raise ValueError(f"depth must be an integer 1 ... {MAX_OCTREE_DEPTH} or None, not {depth!r}")
        if depth < smallest:
            raise ValueError(f"origin {origin} + the grid's extent {dims} [x, y, z] is above 2^depth = {2 ** depth}")
    flags = hip.OCT_COLLAPSE if _flag(collapse, "collapse") else 0
    _flag(coords, "coords")
    dense._sync(device)   # (the caller's writes to grid have landed)
    d, counts, nodes, listed = dv.octree_build(grid.data_ptr(), fmt, dense._strides(grid), dims, 0.0 if level is None else level, origin,
                                               0 if depth is None else int(depth), flags)
    valid = torch.empty(nodes, dtype=torch.uint8, device=device)
    full = torch.empty(nodes, dtype=torch.uint8, device=device)
    first_child = torch.empty(nodes, dtype=torch.int32, device=device)
    corners = torch.empty((nodes, 3), dtype=torch.int32, device=device) if coords else None
    dv.octree_write(valid.data_ptr(), full.data_ptr(), first_child.data_ptr(), None if corners is None else corners.data_ptr())
    offsets = [0]
    for c in counts:
        offsets.append(offsets[-1] + int(c))
    return Octree(valid=valid, full=full, first_child=first_child, coords=corners, level_offsets=tuple(offsets), depth=int(d), collapsed=bool(collapse),
                  voxels_listed=int(listed))


def _tree_args(dv, tree):
    """(device, (valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags)) of an Octree, checked."""
    from . import dense
    dense._require_shared_runtime()
    device = dense._device(dv)
    if not isinstance(tree, Octree):
        raise TypeError("tree must be an Octree, what build_octree returns")
    if isinstance(tree.depth, bool) or not isinstance(tree.depth, numbers.Integral) or not 1 <= tree.depth <= MAX_OCTREE_DEPTH:
        raise ValueError(f"tree.depth must be 1 ... {MAX_OCTREE_DEPTH}, not {tree.depth!r}")
    n = None
    for name, dtype in (("valid", torch.uint8), ("full", torch.uint8), ("first_child", torch.int32)):
        t = getattr(tree, name)
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != dtype or not t.is_contiguous():
            raise TypeError(f"tree.{name} must be a contiguous 1-D {dtype} tensor")
        if t.device != device:
            raise ValueError(f"tree.{name} is on {t.device}, the voxelizer on {device}")
        if n is not None and t.shape[0] != n:
            raise ValueError("tree.valid, tree.full and tree.first_child must have one length")
        n = t.shape[0]
    if n == 0:
        raise ValueError("the tree has no nodes: a tree has its root")
    return device, (tree.valid.data_ptr(), tree.full.data_ptr(), tree.first_child.data_ptr(), n, int(tree.depth),
                    hip.OCT_COLLAPSE if _flag(tree.collapsed, "tree.collapsed") else 0)


def octree_lookup(dv, tree, points):
    """The descent through an Octree for every point, on the voxelizer's device: int32 [..., 4] = (solid,
    level, node, voxel_index) for int32 points [..., 3] = (x, y, z) in global coordinates, negative ones allowed.

    solid 1: the point is a solid voxel.  level, node: where the descent ended - at level depth - 1, or higher at an empty octant or
    at a full one of a collapsed tree; outside the root cube (0, -1, -1, -1).  voxel_index: at level depth - 1 the voxel's slot in a
    per-voxel attribute array of tree.voxels_listed entries (Morton order), else -1.  A tree whose first_child points outside its
    arrays gives (0, -2, -1, -1) there and nothing is read outside them."""
    from . import dense
    device, tree_args = _tree_args(dv, tree)
    if not isinstance(points, torch.Tensor) or points.dim() < 1 or points.shape[-1] != 3:
        raise ValueError("points must be a tensor [..., 3] of (x, y, z)")
    if points.dtype != torch.int32:
        raise TypeError(f"points must be int32, not {points.dtype}")
    if points.device != device:
        raise ValueError(f"points is on {points.device}, the voxelizer on {device}")
    n = points.numel() // 3
    if n > MAX_OCTREE_POINTS:
        raise ValueError(f"{n} points are more than {MAX_OCTREE_POINTS} in one call")
    flat = points.reshape(-1, 3).contiguous()
    out = torch.empty((n, 4), dtype=torch.int32, device=device)
    dense._sync(device)   # (the caller's writes to the tree and the points have landed)
    if n:
        dv.octree_lookup(*tree_args, flat.data_ptr(), n, out.data_ptr())
    return out.reshape(points.shape[:-1] + (4,))


def octree_to_dense(dv, tree, shape, *, origin=(0, 0, 0), out=None):
    """An Octree back as a dense grid on the voxelizer's device: a bool tensor of `shape` (nz, ny, nx), True
    where the tree is solid, for the box whose voxel (0, 0, 0) is `origin` (x, y, z) of the global lattice - any box: the part
    outside the root cube is False.

    out:  a bool or uint8 tensor of that shape (any strides that keep the voxels apart) to write 1 / 0 into; it is returned."""
    from . import dense
    device, tree_args = _tree_args(dv, tree)
    origin = dense._origin(origin)
    shape = tuple(int(n) for n in shape)
    if len(shape) != 3 or any(n < 1 for n in shape):
        raise ValueError(f"shape {shape} must be three positive extents (nz, ny, nx)")
    dims = shape[::-1]
    dense._limit_voxels(dims)
    if any(o + n > 2 ** 32 for o, n in zip(origin, dims)):
        raise ValueError(f"origin {origin} + the extent {dims} [x, y, z] is above 2^32")
    if out is None:
        out = torch.empty(shape, dtype=torch.bool, device=device)
    else:
        if isinstance(out, torch.Tensor) and out.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"out must be bool or uint8, not {out.dtype}")
        dense._check_grid(out, "out", out.dtype if isinstance(out, torch.Tensor) else torch.bool, device, shape)
    dense._sync(device)   # (the caller's writes to the tree have landed, its reads of out are done)
    dv.octree_to_dense(*tree_args, origin, dims, out.data_ptr(), dense._strides(out))
    return out


@dataclasses.dataclass(frozen=True)
class OctreeDag:
    """What octree_dag returns (the definition: include/o2v_hip.h): an Octree whose equal subtrees are stored once.  DAG node i is a
    class of tree nodes of the level l with level_offsets[l] <= i < level_offsets[l + 1], the classes of a level in the order of
    their first member; the root is node 0."""
    valid: torch.Tensor            # uint8 [M]
    full: torch.Tensor             # uint8 [M]
    first_child: torch.Tensor      # int32 [M]: the node's first entry in child and skip; -1 at level depth - 1 and without stored children
    child: torch.Tensor            # int32 [P]: the DAG node of each stored child, node by node, within a node in octant order
    skip: object                   # int32 [P]: the listed voxels under the node's stored children before this one, or None
    level_offsets: tuple           # depth + 1 Python ints
    depth: int
    collapsed: bool
    voxels_listed: int             # the tree's: the length of a per-voxel attribute array, which the DAG's voxel_index addresses
    tree_nodes: int                # the nodes of the tree it was made of

    @property
    def nbytes(self):
        """the bytes of its arrays: 6 per node, 4 or 8 per pointer"""
        return sum(t.numel() * t.element_size() for t in (self.valid, self.full, self.first_child, self.child, self.skip) if t is not None)


def octree_dag(dv, tree, skips=True):
    """The sparse voxel DAG of an Octree: its equal subtrees merged on the voxelizer's device, level by level from the bottom
    (DESIGN.md section 34): an OctreeDag.  Two nodes of a level are equal if their valid masks, their full masks and their stored
    children are; a class is numbered by its first member.  Integers only; one run equals another bit for bit.

        tree = dense.build_octree(dv, labels, collapse=False)
        dag = dense.octree_dag(dv, tree)                              # dag.nbytes against 6 * len(tree.valid)
        hit = dense.dag_lookup(dv, dag, points)                       # columns 0, 1, 3 == dense.octree_lookup(dv, tree, points)
        argb[hit[:, 3].long()]                                        # an attribute array made for the tree works unchanged

    skips:  keep per child pointer the listed voxels under the earlier siblings, which is what dag_lookup makes voxel_index of;
            False: 4 bytes per pointer less, and voxel_index is -1."""
    from . import dense
    device, tree_args = _tree_args(dv, tree)
    _flag(skips, "skips")
    offs = tree.level_offsets
    if (not isinstance(offs, tuple) or len(offs) != tree.depth + 1 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in offs)
            or offs[0] != 0 or any(b < a for a, b in zip(offs, offs[1:])) or offs[1] != 1 or offs[-1] != tree_args[3]):
        raise ValueError(f"tree.level_offsets must be {tree.depth + 1} rising integers from 0 through 1 to the tree's {tree_args[3]} nodes, not {offs!r}")
    dense._sync(device)   # (the caller's writes to the tree have landed)
    counts, nodes, pointers = dv.octree_dag_build(*tree_args, [b - a for a, b in zip(offs, offs[1:])])
    valid = torch.empty(nodes, dtype=torch.uint8, device=device)
    full = torch.empty(nodes, dtype=torch.uint8, device=device)
    first_child = torch.empty(nodes, dtype=torch.int32, device=device)
    child = torch.empty(pointers, dtype=torch.int32, device=device)
    skip = torch.empty(pointers, dtype=torch.int32, device=device) if skips else None
    dv.octree_dag_write(valid.data_ptr(), full.data_ptr(), first_child.data_ptr(), child.data_ptr() if pointers else None,
                        skip.data_ptr() if skips and pointers else None)
    offsets = [0]
    for c in counts:
        offsets.append(offsets[-1] + int(c))
    return OctreeDag(valid=valid, full=full, first_child=first_child, child=child, skip=skip, level_offsets=tuple(offsets), depth=int(tree.depth),
                     collapsed=bool(tree.collapsed), voxels_listed=int(tree.voxels_listed), tree_nodes=int(tree_args[3]))


def _dag_args(dv, dag):
    """(device, (valid_ptr, full_ptr, first_child_ptr, child_ptr), skip_ptr, (n_nodes, n_pointers, depth, flags)) of an OctreeDag, checked."""
    from . import dense
    dense._require_shared_runtime()
    device = dense._device(dv)
    if not isinstance(dag, OctreeDag):
        raise TypeError("dag must be an OctreeDag, what octree_dag returns")
    if isinstance(dag.depth, bool) or not isinstance(dag.depth, numbers.Integral) or not 1 <= dag.depth <= MAX_OCTREE_DEPTH:
        raise ValueError(f"dag.depth must be 1 ... {MAX_OCTREE_DEPTH}, not {dag.depth!r}")
    lengths = {}
    for name, dtype, group in (("valid", torch.uint8, "n"), ("full", torch.uint8, "n"), ("first_child", torch.int32, "n"), ("child", torch.int32, "p"),
                               ("skip", torch.int32, "p")):
        t = getattr(dag, name)
        if name == "skip" and t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != dtype or not t.is_contiguous():
            raise TypeError(f"dag.{name} must be a contiguous 1-D {dtype} tensor" + (" or None" if name == "skip" else ""))
        if t.device != device:
            raise ValueError(f"dag.{name} is on {t.device}, the voxelizer on {device}")
        if lengths.setdefault(group, t.shape[0]) != t.shape[0]:
            raise ValueError("dag.valid, dag.full and dag.first_child must have one length, dag.child and dag.skip another")
    if lengths["n"] == 0:
        raise ValueError("the DAG has no nodes: a DAG has its root")
    p = lengths["p"]
    return (device, (dag.valid.data_ptr(), dag.full.data_ptr(), dag.first_child.data_ptr(), dag.child.data_ptr() if p else None),
            dag.skip.data_ptr() if dag.skip is not None and p else None,
            (lengths["n"], p, int(dag.depth), hip.OCT_COLLAPSE if _flag(dag.collapsed, "dag.collapsed") else 0))


def dag_lookup(dv, dag, points):
    """The descent through an OctreeDag for every point, on the voxelizer's device: int32 [..., 4] = (solid,
    level, node, voxel_index) for int32 points [..., 3] = (x, y, z) in global coordinates, negative ones allowed.

    solid, level and voxel_index are those of octree_lookup on the tree the DAG was made of; node is the DAG node, the class of the
    tree node.  voxel_index is -1 throughout for a DAG without skips (but a DAG of a root alone has nothing to skip).  Arrays that point outside themselves give (0, -2, -1, -1)
    there and nothing is read outside them."""
    from . import dense
    device, arrays, skip, rest = _dag_args(dv, dag)
    if not isinstance(points, torch.Tensor) or points.dim() < 1 or points.shape[-1] != 3:
        raise ValueError("points must be a tensor [..., 3] of (x, y, z)")
    if points.dtype != torch.int32:
        raise TypeError(f"points must be int32, not {points.dtype}")
    if points.device != device:
        raise ValueError(f"points is on {points.device}, the voxelizer on {device}")
    n = points.numel() // 3
    if n > MAX_OCTREE_POINTS:
        raise ValueError(f"{n} points are more than {MAX_OCTREE_POINTS} in one call")
    flat = points.reshape(-1, 3).contiguous()
    out = torch.empty((n, 4), dtype=torch.int32, device=device)
    dense._sync(device)   # (the caller's writes to the DAG and the points have landed)
    if n:
        dv.octree_dag_lookup(*arrays, skip, *rest, flat.data_ptr(), n, out.data_ptr())
    return out.reshape(points.shape[:-1] + (4,))


def dag_to_dense(dv, dag, shape, *, origin=(0, 0, 0), out=None):
    """An OctreeDag back as a dense grid on the voxelizer's device: a bool tensor of `shape` (nz, ny, nx),
    True where the DAG is solid, for the box whose voxel (0, 0, 0) is `origin` (x, y, z) of the global lattice - any box: the part
    outside the root cube is False.  It equals octree_to_dense of the tree the DAG was made of.

    out:  a bool or uint8 tensor of that shape (any strides that keep the voxels apart) to write 1 / 0 into; it is returned."""
    from . import dense
    device, arrays, _, rest = _dag_args(dv, dag)
    origin = dense._origin(origin)
    shape = tuple(int(n) for n in shape)
    if len(shape) != 3 or any(n < 1 for n in shape):
        raise ValueError(f"shape {shape} must be three positive extents (nz, ny, nx)")
    dims = shape[::-1]
    dense._limit_voxels(dims)
    if any(o + n > 2 ** 32 for o, n in zip(origin, dims)):
        raise ValueError(f"origin {origin} + the extent {dims} [x, y, z] is above 2^32")
    if out is None:
        out = torch.empty(shape, dtype=torch.bool, device=device)
    else:
        if isinstance(out, torch.Tensor) and out.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"out must be bool or uint8, not {out.dtype}")
        dense._check_grid(out, "out", out.dtype if isinstance(out, torch.Tensor) else torch.bool, device, shape)
    dense._sync(device)   # (the caller's writes to the DAG have landed, its reads of out are done)
    dv.octree_dag_to_dense(*arrays, *rest, origin, dims, out.data_ptr(), dense._strides(out))
    return out


def _ray_args(device, origins, directions, t_max, voxel_index):
    """(shape, origins [n, 3], directions [n, 3], n, t_max) of the rays of a cast, checked as RayCaster.cast checks them."""
    if isinstance(t_max, bool) or not isinstance(t_max, numbers.Real) or not float(t_max) >= 0.0:
        raise ValueError(f"t_max must be a number >= 0 or inf, not {t_max!r}")
    _flag(voxel_index, "voxel_index")
    for name, r in (("origins", origins), ("directions", directions)):
        if not isinstance(r, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor")
        if r.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, not {r.dtype}")
        if r.dim() < 1 or r.shape[-1] != 3:
            raise ValueError(f"{name} must have shape [..., 3], not {tuple(r.shape)}")
        if r.device != device:
            raise ValueError(f"{name} is on {r.device}, the voxelizer on {device}")
    if origins.shape != directions.shape:
        raise ValueError(f"origins {tuple(origins.shape)} and directions {tuple(directions.shape)} must have one shape")
    n = origins.numel() // 3
    if n > MAX_OCTREE_POINTS:
        raise ValueError(f"{n} rays are more than {MAX_OCTREE_POINTS} in one call")
    return tuple(origins.shape[:-1]), origins.reshape(-1, 3).contiguous(), directions.reshape(-1, 3).contiguous(), n, float(t_max)


def _cast(device, call, origins, directions, t_max, voxel_index):
    """The outputs of a cast around call(origins_ptr, directions_ptr, n, t_max, hit_ptr, t_ptr, voxel_index_ptr)."""
    from . import dense
    shape, o, d, n, t_max = _ray_args(device, origins, directions, t_max, voxel_index)
    hit = torch.empty((n, 4), dtype=torch.int32, device=device)
    t = torch.empty((n,), dtype=torch.float32, device=device)
    slot = torch.empty((n,), dtype=torch.int32, device=device) if voxel_index else None
    dense._sync(device)   # (the caller's writes to the arrays and the rays have landed)
    if n:
        call(o.data_ptr(), d.data_ptr(), n, t_max, hit.data_ptr(), t.data_ptr(), None if slot is None else slot.data_ptr())
    out = (hit.reshape(shape + (4,)), t.reshape(shape))
    return out + (slot.reshape(shape),) if voxel_index else out


def octree_raycast(dv, tree, origins, directions, *, t_max=float("inf"), voxel_index=False):
    """The first solid voxel along rays through an Octree, found in the tree itself on the voxelizer's device (DESIGN.md
    section 35): (hit, t), bit for bit what RayCaster(dv, octree_to_dense(dv, tree, ...)).cast(origins, directions, t_max) gives -
    nothing is expanded and nothing is kept.

        hit, depth = dense.octree_raycast(dv, tree, *dense.camera_rays(640, 480, eye, target, up, 40.0, device))

    origins, directions, t_max, hit, t:  as RayCaster.cast takes and gives them; voxel space is the tree's global lattice, the
                  root cube [0, 2^depth)^3, and everything outside it is empty.
    voxel_index:  True: (hit, t, slot) with slot int32 [...], column 3 of octree_lookup at the hit voxel - its place in a per-voxel
                  attribute array - and -1 for a miss, an invalid ray and a hit inside a full cell of a collapsed tree.
    A tree whose first_child points outside its arrays is empty there, as in octree_to_dense; nothing is read outside them."""
    device, tree_args = _tree_args(dv, tree)
    return _cast(device, lambda *rays: dv.octree_raycast(*tree_args, *rays), origins, directions, t_max, voxel_index)


def dag_raycast(dv, dag, origins, directions, *, t_max=float("inf"), voxel_index=False):
    """octree_raycast through an OctreeDag: the same (hit, t) as through the tree it was made of.  The
    skips are added on the way down, so the slot of the hit voxel comes with the hit:

        hit, depth, slot = dense.dag_raycast(dv, dag, origins, directions, voxel_index=True)
        image = argb[slot.clamp(min=0).long()].where(slot >= 0, background)     # argb: made for the tree (build_octree's example)

    slot is -1 throughout for a DAG without skips (but a DAG of a root alone has nothing to skip)."""
    device, arrays, skip, rest = _dag_args(dv, dag)
    return _cast(device, lambda *rays: dv.octree_dag_raycast(*arrays, skip, *rest, *rays), origins, directions, t_max, voxel_index)


def octree_level(tree, l):   # noqa: E741
    """(valid, full, first_child, coords or None) of the nodes of level l of an Octree, 0 <= l < depth: views, in Morton order.
    (valid != 0) scattered to coords >> (depth - l - 1) is the occupancy at 1 / 2^(depth - l - 1).  Plain torch."""
    if not isinstance(tree, Octree):
        raise TypeError("tree must be an Octree, what build_octree returns")
    if isinstance(l, bool) or not isinstance(l, numbers.Integral) or not 0 <= l < tree.depth:
        raise ValueError(f"l must be an integer 0 ... {tree.depth - 1}, not {l!r}")
    a, b = tree.level_offsets[l], tree.level_offsets[l + 1]
    return tree.valid[a:b], tree.full[a:b], tree.first_child[a:b], None if tree.coords is None else tree.coords[a:b]
