"""Dense torch grids from device-resident meshes.

    import torch
    from obj2voxel_amd import dense, hip
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, positions, faces)                   # cuda tensors [V, 3] float32, [F, 3] int32 / int64
    grid, origin = dense.voxelize_dense(dv, 256, fill=True)   # bool (256, 256, 256), indexed [z, y, x]

The mesh goes to the device context without a host copy (o2v_hip_set_triangles_device) and the voxels come back as a dense
tensor written on the device (o2v_hip_write_dense); nothing of either crosses to the host.  Distance grids (fmt "dist2" /
"sdf", and distance_transform on any label tensor) come from o2v_hip_distance_dense; mesh_distance is the
narrow-band distance to the triangles themselves (o2v_hip_mesh_distance_dense); extract_surface turns a
distance grid back into an indexed mesh (o2v_hip_surface_count / _write); RayCaster / raycast find the
first solid voxel along rays through any of these grids (o2v_hip_raycast_build / o2v_hip_raycast);
components / flood and what is built on them (exterior, solidify, remove_small) say what is connected to what in them
(o2v_hip_components_dense / o2v_hip_flood_dense); to_voxels / count_voxels / save_voxels turn any of these
grids back into (x, y, z, argb) records and voxel files (o2v_hip_gather_count / _write / _save);
voxel_faces / count_faces turn them into the blocky mesh of the voxel model (o2v_hip_faces_count / _write)
and save_mesh writes that mesh, or extract_surface's, as STL, PLY or OBJ + MTL; nearest_voxel says which seed voxel of a grid is
closest to every voxel and spread_colors carries the seeds' colours to the voxels that take them - the interior of a solid, a
shell of a given thickness (o2v_hip_nearest_dense); downsample merges blocks of f^3 voxels of any of these
grids into a coarser grid - coverage counts, occupancy by a threshold, labels and mean colours: supersampling at 4x or 8x, LOD
chains (o2v_hip_downsample); crossing_numbers counts the signed crossings of the triangles along the x, y
and z rays through every voxel centre, from both ends, and winding_fill votes on them: a solid fill that keeps the overlap of
parts pushed into each other and outvotes a ray that slips through a hole (o2v_hip_crossings_dense);
label_stats reads a label grid once and gives, per label, the voxel count, the bounding box, the coordinate sums, the second
moments and the exposed faces as exact integers, and component_stats, centroids, covariances, mass_properties, keep_largest and
crop are built on them: the parts of a scan cropped one by one, the largest body kept, a solid's volume, centre of mass and inertia
tensor (o2v_hip_label_stats); geodesic_distance says how far every voxel of a set is from the nearest seed
without leaving the set - hop counts, the chamfer metric or any integer step costs, from listed seeds or the border - and
shortest_paths walks back along those distances (o2v_hip_geodesic_dense / o2v_hip_geodesic_paths);
local_thickness says how thick a solid is at every voxel - the largest inscribed ball that holds it -, thin_regions where it is
thinner than t, and inner_distance, erode, dilate, opening and closing are the ball morphology that falls out of the same passes
(o2v_hip_thickness_dense); skeletonize reduces a set to its skeleton - the one-voxel-wide centrelines of a
solid or of its pore space - by topological thinning, and skeleton_nodes lists the end points and junctions (o2v_hip_thin_dense,
DESIGN.md section 25); watershed splits a relief - usually the depth map - into the basins of its tops, merged by how deep the pass
between them is, split_parts does so for a solid and watershed_peaks lists the parts' tops (o2v_hip_watershed_dense, DESIGN.md
section 26); label_adjacency says which labels of a label grid touch - per pair the face, edge and corner contacts and the passes of
a relief between them -, adjacency_neighbours and coordination turn that list into neighbour lists and counts, and skeleton_graph
makes the nodes, branches and incidences of a skeleton with it (o2v_hip_adjacency_count / o2v_hip_adjacency_write, DESIGN.md
section 27); euler_stats counts per label the cells of the unit lattice that its voxels close in and hold, euler_numbers and
intrinsic_volumes make the Euler characteristic and the Minkowski functionals of them, and betti_numbers the components, tunnels
and cavities of a set (o2v_hip_euler_stats); build_octree turns any of these grids into a sparse voxel octree -
valid and full masks per node, level by level in Morton order, full cells collapsed -, octree_lookup descends it per point,
octree_to_dense expands it into any box and octree_level gives one level of it (o2v_hip_octree_build / _write / _lookup /
_to_dense); openness counts per voxel the directions of a direction_set in which one sees out of the grid -
sky visibility, sun shadows -, and shade_colors bakes it into colours as ambient occlusion (o2v_hip_openness); label_surfaces turns a label
grid into one smooth mesh of all its interfaces - the wall between two parts meshed once -, relax_surface smooths a kept net anew,
part_mesh cuts one part's closed mesh out of it and interface_areas measures the walls (o2v_hip_label_surface_count / _write /
_relax); octree_dag merges the equal subtrees of an Octree into a sparse voxel DAG that keeps every voxel's
slot, dag_lookup descends it per point and dag_to_dense expands it (o2v_hip_octree_dag_build / _write / _lookup / _to_dense,
DESIGN.md section 34); octree_raycast and dag_raycast find the first solid voxel along rays in the tree or the DAG itself, and its
slot, without expanding either (o2v_hip_octree_raycast / o2v_hip_octree_dag_raycast).

torch is imported first on purpose: the library must bind to the HIP runtime torch loaded (a process that loaded the library
before torch holds two separate runtime copies, and this module refuses to work there).
"""
import dataclasses
import math
import numbers
import os

import numpy as np
import torch  # first: see above

from . import hip

FORMATS = {  # name: (o2v_hip_write_dense format, tensor dtype)
    "occupancy": (hip.DENSE_U8, torch.bool),
    "labels": (hip.DENSE_U8, torch.uint8),
    "argb": (hip.DENSE_ARGB32, torch.int32),
    "bits": (hip.DENSE_BITS, torch.int32),
}
DISTANCE_FORMATS = {  # name: (o2v_hip_distance_dense format, tensor dtype)
    "dist2": (hip.DIST_SQ_I32, torch.int32),
    "sdf": (hip.DIST_SDF_F32, torch.float32),
}
STRATEGIES = {"max": hip.STRATEGY_MAX, "blend": hip.STRATEGY_BLEND}
MAX_SAMPLES = 65535  # samples per axis of one pass (x / y tiles above that are not supported here)
MAX_BAND = 32.0      # mesh_distance: the widest band, in voxels
MAX_SURFACE_EXTENT = 65536  # extract_surface: origin + shape per axis
MAX_RAY_EXTENT = 65536      # RayCaster: origin + extent per axis
MAX_CC_DIM = 65536          # components / flood: voxels per axis ...
MAX_CC_VOXELS = 2 ** 31 - 1  # ... and in all: a linear index and a label are one int32
MAX_FACES_EXTENT = 65536    # voxel_faces: origin + extent per axis: a coordinate is an exact float32
_FACES_MERGE = {"none": hip.FACES_MERGE_NONE, "runs": hip.FACES_MERGE_RUNS, "rects": hip.FACES_MERGE_RECTS}
MAX_GATHER_WORDS = 2 ** 31 - 1  # to_voxels / save_voxels: words of 64 voxels along x, ceil(nx / 64) * ny * nz
MAX_NEAREST_D2 = 2 ** 31 - 2    # nearest_voxel / spread_colors: (nx-1)^2 + (ny-1)^2 + (nz-1)^2, the largest squared distance
MIN_DOWN_FACTOR, MAX_DOWN_FACTOR = 2, 8  # downsample: fine voxels per coarse voxel and axis
_DOWN_VALUES = {"min": hip.DOWN_VALUE_MIN, "max": hip.DOWN_VALUE_MAX}
_AXIS_BITS = {"x": hip.AXIS_X, "y": hip.AXIS_Y, "z": hip.AXIS_Z}  # crossing_numbers / winding_fill: the rays of an axis
MAX_STATS_EXTENT = 65536    # label_stats: origin + extent per axis: with fewer than 2^31 voxels no sum reaches 2^63
MAX_STATS_LABELS = 2 ** 31 - 2  # ... and its highest label


def _require_shared_runtime():
    if hip.torch_was_loaded_first() is False:
        raise RuntimeError("obj2voxel_amd.dense: libobj2voxel_amd.so was loaded in this process before torch, so the two use "
                           "separate HIP runtimes and cannot share device memory; import torch before obj2voxel_amd's bindings")


def _device(dv):
    return torch.device("cuda", 0 if dv.device is None else dv.device)


def _sync(device):
    """Everything torch has queued on its current stream of `device` has run (the library reads and writes on its own stream)."""
    torch.cuda.current_stream(device).synchronize()


def _check(t, name, dtypes, shape, device):
    """t as a contiguous tensor, after its dtype, shape (None = any length) and device are checked."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, not {t.dtype}")
    if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
        raise ValueError(f"{name} must have shape {tuple('*' if s is None else s for s in shape)}, not {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, the voxelizer on {device}")
    return t.contiguous()


def _check_grid(t, name, dtype, device, shape=None):
    """A caller's 3-D tensor [z, y, x] of any strides (shape: the one it must have), checked as it is: it is written in place,
    never made contiguous."""
    if not isinstance(t, torch.Tensor) or t.dim() != 3:
        raise ValueError(f"{name} must be a 3-D tensor [z, y, x]")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have the shape {tuple(shape)}, not {tuple(t.shape)}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, not {t.dtype}")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, the voxelizer on {device}")


def _check_sampling(resolution, supersampling, max_layers):
    if resolution < 1 or supersampling not in (1, 2):
        raise ValueError("resolution must be positive and supersampling 1 or 2")
    if max_layers is not None and max_layers < 1:
        raise ValueError("max_layers must be positive")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _strides(t):
    """(x, y, z): the element strides of a 3-D tensor indexed [z, y, x]."""
    return t.stride(2), t.stride(1), t.stride(0)


def set_mesh(dv, positions, faces=None, *, uvs=None, types=None, colors=None, texids=None):
    """The mesh of the next voxelize calls of `dv` (a hip.DeviceVoxelizer), from tensors on its device: positions float32
    [V, 3] and faces int32 / int64 [F, 3], or positions [F, 9] and no faces.  uvs float32 [F, 6], types int32 [F] (hip.TRI_*),
    colors float32 [F, 3] and texids int32 [F] are per triangle and optional.  An out-of-range face index raises
    hip.DeviceError and leaves `dv` without triangles."""
    _require_shared_runtime()
    device = _device(dv)
    if faces is None:
        positions = _check(positions, "positions", (torch.float32,), (None, 9), device)
        count, n_positions, index_bytes = positions.shape[0], 0, 0
    else:
        positions = _check(positions, "positions", (torch.float32,), (None, 3), device)
        faces = _check(faces, "faces", (torch.int32, torch.int64), (None, 3), device)
        count, n_positions, index_bytes = faces.shape[0], positions.shape[0], faces.element_size()
    if uvs is not None:
        uvs = _check(uvs, "uvs", (torch.float32,), (count, 6), device)
    if types is not None:
        types = _check(types, "types", (torch.int32,), (count,), device)
    if colors is not None:
        colors = _check(colors, "colors", (torch.float32,), (count, 3), device)
    if texids is not None:
        texids = _check(texids, "texids", (torch.int32,), (count,), device)
    _sync(device)
    dv.set_triangles_device(_ptr(positions) if count else None, n_positions, _ptr(faces) if count else None, index_bytes, count,
                            _ptr(uvs), _ptr(types), _ptr(colors), _ptr(texids))


def _layout(t, fmt):
    """(write_dense strides x, y, z) of a 3-D tensor indexed [z, y, x]: elements, or 32-bit words for bits."""
    if fmt == "bits" and t.stride(2) != 1:
        raise ValueError("a bits grid needs unit stride along x (its last dimension)")
    return _strides(t)


def voxelize_dense(dv, resolution, *, fmt="occupancy", box="grid", out=None, origin=None, supersampling=1, strategy="max",
                   fill=False, fill_argb=0xFFFFFFFF, unit_transform=None, bounds=None, max_layers=None):
    """Voxelizes the mesh of `dv` (set_mesh) and returns (tensor, origin): voxel (x, y, z) is tensor[z - oz, y - oy, x - ox],
    origin = (ox, oy, oz).

    fmt:  "occupancy" bool, "labels" uint8 (1 surface, 2 interior with fill=True), "argb" int32 (the voxel's 0xAARRGGBB bits;
          not an occupancy: a texel of alpha 0 gives 0), "bits" int32 [nz, ny, ceil(nx / 32)], bit x % 32 of word x / 32.
    box:  "grid" the whole resolution^3 grid at origin 0 (or `origin`), "tight" the voxels' own box.
    out:  a 3-D tensor (any strides, e.g. a slice of a batch) of the format's dtype on the voxelizer's device, written as it
          is and not cleared; its shape is the box's extent.  Otherwise a new zeroed contiguous tensor.
    A grid whose dense stage does not fit the device runs as consecutive z-slabs (o2v_hip_max_slab_layers; max_layers caps
    their height), all written into the one tensor.  A voxel outside the tensor's box raises.

    fmt "dist2" int32 / "sdf" float32: the labels of the box (as fmt="labels", z-slabs included) go to a temporary uint8 tensor,
    then one distance_transform of the whole box goes to the tensor.  "sdf" needs fill=True (its sign is the interior)."""
    _require_shared_runtime()
    if fmt in DISTANCE_FORMATS:
        if fmt == "sdf" and not fill:
            raise ValueError("fmt='sdf' needs fill=True: without the interior every distance would be positive")
        dtype = DISTANCE_FORMATS[fmt][1]
        device = _device(dv)
        if out is not None:
            _check_grid(out, "out", dtype, device)
        labels, origin = voxelize_dense(
            dv, resolution, fmt="labels", box=box, origin=origin, supersampling=supersampling, strategy=strategy, fill=fill,
            fill_argb=fill_argb, unit_transform=unit_transform, bounds=bounds, max_layers=max_layers,
            out=None if out is None else torch.zeros(tuple(out.shape), dtype=torch.uint8, device=device))
        if out is None:
            out = torch.empty(tuple(labels.shape), dtype=dtype, device=device)
        if 0 in labels.shape:
            return out, origin
        return distance_transform(dv, labels, fmt=fmt, out=out), origin
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {sorted(FORMATS)}, not {fmt!r}")
    if box not in ("grid", "tight"):
        raise ValueError(f"box must be 'grid' or 'tight', not {box!r}")
    if strategy not in STRATEGIES:
        raise ValueError(f"strategy must be 'max' or 'blend', not {strategy!r}")
    _check_sampling(resolution, supersampling, max_layers)
    if resolution * supersampling > MAX_SAMPLES:
        raise ValueError(f"resolution x supersampling = {resolution * supersampling} is above {MAX_SAMPLES}: x / y tiles are not "
                         "supported by the dense path")
    if box == "tight" and origin is not None:
        raise ValueError("origin is given by the voxels with box='tight'")
    code, dtype = FORMATS[fmt]
    device = _device(dv)
    if out is not None:
        _check_grid(out, "out", dtype, device)
        _layout(out, fmt)
    kw = dict(supersampling=supersampling, strategy=STRATEGIES[strategy], unit_transform=unit_transform, fill=fill)

    # z-slabs: one pass if the grid fits
    layers = dv.max_slab_layers(resolution, bounds=bounds, **kw)
    if max_layers is not None:
        layers = min(layers, max(4, max_layers // 4 * 4))
    if layers == 0:
        raise hip.DeviceError(f"resolution {resolution}: not even one 4-layer slab of the dense grid fits the device memory")
    if layers >= resolution:
        slabs = [(0, 0)]
    else:
        slabs = [(z, min(resolution, z + layers)) for z in range(0, resolution, layers)]
        if bounds is None:   # (the mesh bounds once for all slabs, as obj2voxel_voxelize() does)
            _, bounds = dv.plan_slabs(resolution, 1, supersampling=supersampling, unit_transform=unit_transform)

    def run(zslab):
        return dv.voxelize(resolution, zslab=zslab, bounds=bounds, read=False, fill_argb=fill_argb, **kw)

    held = None   # the slab whose records the context still holds
    if box == "tight":
        lo, hi = [resolution] * 3, [0] * 3
        for zslab in slabs:
            if run(zslab):
                a, b = dv.voxels_box()
                lo, hi = [min(p, q) for p, q in zip(lo, a)], [max(p, q) for p, q in zip(hi, b)]
            held = zslab
        if hi[0] == 0:
            lo = hi = [0, 0, 0]
        origin, dims = tuple(lo), tuple(h - l for h, l in zip(hi, lo))
    else:
        origin = tuple(int(v) for v in (origin or (0, 0, 0)))
        dims = (resolution,) * 3 if out is None else None
    if out is None:
        nz, ny, nx = dims[2], dims[1], dims[0]
        shape = (nz, ny, (nx + 31) // 32) if fmt == "bits" else (nz, ny, nx)
        out = torch.zeros(shape, dtype=dtype, device=device)
    else:
        nz, ny, nx = out.shape
        if fmt == "bits":
            nx *= 32
        if dims is not None and box == "tight" and (nx < dims[0] or ny < dims[1] or nz < dims[2]):
            raise ValueError(f"out {tuple(out.shape)} is smaller than the voxels' box {dims[::-1]} [z, y, x]")
    if 0 in out.shape:
        if dims is not None and 0 in dims:
            return out, origin
        raise ValueError("out has an empty dimension")
    strides = _layout(out, fmt)
    # the grid as U8 for occupancy: a bool holds 0 / 1, so interior labels (2) are folded back to 1 below
    target = out.view(torch.uint8) if fmt == "occupancy" else out
    _sync(device)   # (torch.zeros / the caller's writes to `out` have landed)
    interior = 0
    for zslab in ([held] if held else []) + [z for z in slabs if z != held]:
        if (dv.count if zslab == held else run(zslab)) == 0:
            continue
        interior += dv.stats()["interior_voxels"]
        outside = dv.write_dense(target.data_ptr(), code, origin, (nx, ny, nz), strides)
        if outside:
            raise ValueError(f"{outside} voxels lie outside the tensor's box (origin {origin}, extent {(nx, ny, nz)} [x, y, z])")
    if fmt == "occupancy" and interior:
        target.clamp_(max=1)
    return out, origin


def distance_transform(dv, labels, fmt="sdf", *, out=None):
    """The exact Euclidean distance transform of `labels`, a uint8 tensor [z, y, x] of any strides on
    the voxelizer's device (0 empty, 1 surface, 2 interior, as fmt="labels" writes), into `out` (any strides, the same shape;
    a new contiguous tensor if None), which is returned.  Seeds are the surface voxels; distances are in voxels, over the box.
    fmt "dist2": int32 squared distances (0x7FFFFFFF everywhere when there is no surface voxel); "sdf": float32
    -sqrt(d2) where labels == 2, +sqrt(d2) elsewhere (+-inf without a surface voxel)."""
    _require_shared_runtime()
    if fmt not in DISTANCE_FORMATS:
        raise ValueError(f"fmt must be one of {sorted(DISTANCE_FORMATS)}, not {fmt!r}")
    code, dtype = DISTANCE_FORMATS[fmt]
    device = _device(dv)
    _check_grid(labels, "labels", torch.uint8, device)
    if 0 in labels.shape:
        raise ValueError("labels has an empty dimension")
    if out is None:
        out = torch.empty(tuple(labels.shape), dtype=dtype, device=device)
    else:
        _check_grid(out, "out", dtype, device, labels.shape)
    nz, ny, nx = labels.shape
    _sync(device)   # (the caller's writes to labels and out have landed)
    dv.distance_dense(labels.data_ptr(), _strides(labels), out.data_ptr(), code, _strides(out), (nx, ny, nz))
    return out


def mesh_distance(dv, resolution, *, band, signed=True, out=None, closest=None, origin=None, supersampling=1, unit_transform=None,
                  bounds=None, max_layers=None):
    """The distance from every voxel centre of a box to the triangles of `dv`'s mesh (set_mesh), exact within `band` voxels
    (0 < band <= 32) and `band` beyond it.  Returns (dist, origin), or (dist, closest, origin) when
    `closest` is given: voxel (x, y, z) is dist[z - oz, y - oy, x - ox].

    signed:   True: negative in the solid fill's parity set (the sign fmt="labels", fill=True gives the interior, surface voxels
              included); False: unsigned, for open meshes and triangle soups.
    out:      a float32 3-D tensor [z, y, x] of any strides on the voxelizer's device; the box is `origin` (default 0) plus its
              shape.  Without it the box is the grid from `origin` on, into a new contiguous tensor.
    closest:  None; True for a new int32 tensor; or an int32 tensor of the box's shape (any strides, not in out's storage):
              the index of the closest triangle (the smallest on a tie), -1 where the distance is the band.
    The transform is voxelize's for the same resolution, supersampling, unit_transform and bounds.  max_layers cuts the box
    into z ranges of at most that many layers, one call each, written into the one tensor (the same bits as one call)."""
    _require_shared_runtime()
    if isinstance(band, bool) or not isinstance(band, numbers.Real) or not (0.0 < float(band) <= MAX_BAND):
        raise ValueError(f"band must be a number with 0 < band <= {MAX_BAND:g} voxels, not {band!r}")
    if not hip.C.c_float(float(band)).value > 0.0:   # (the call takes a float: 1e-46 is 0 there)
        raise ValueError(f"band {band!r} is 0 as a float32")
    _check_sampling(resolution, supersampling, max_layers)
    device = _device(dv)
    origin = tuple(int(v) for v in (origin or (0, 0, 0)))
    if len(origin) != 3 or any(v < 0 or v >= resolution for v in origin):
        raise ValueError(f"origin {origin} must be three voxel coordinates inside the grid")
    if out is None:
        out = torch.empty(tuple(resolution - v for v in origin[::-1]), dtype=torch.float32, device=device)
    else:
        _check_grid(out, "out", torch.float32, device)
        if 0 in out.shape:
            raise ValueError("out has an empty dimension")
        if any(o + n > resolution for o, n in zip(origin, out.shape[::-1])):
            raise ValueError(f"origin {origin} + out's extent {tuple(out.shape[::-1])} [x, y, z] reaches past the grid of {resolution}")
    want_closest = closest is not None
    if closest is True:
        closest = torch.empty(tuple(out.shape), dtype=torch.int32, device=device)
    elif closest is not None:
        _check_grid(closest, "closest", torch.int32, device, out.shape)
        if closest.untyped_storage().data_ptr() == out.untyped_storage().data_ptr():
            raise ValueError("closest must not share out's storage")
    fmt = hip.MESH_DIST_SIGNED_F32 if signed else hip.MESH_DIST_UNSIGNED_F32
    nz, ny, nx = out.shape
    step = nz if max_layers is None else max_layers
    _sync(device)   # (the caller's writes to out and closest have landed)
    for z in range(0, nz, step):
        k = min(step, nz - z)
        o = out[z:z + k]
        c = None if closest is None else closest[z:z + k]
        dv.mesh_distance_dense(resolution, float(band), fmt, (origin[0], origin[1], origin[2] + z), (nx, ny, k), o.data_ptr(),
                               _strides(o), _ptr(c), None if c is None else _strides(c), supersampling=supersampling,
                               unit_transform=unit_transform, bounds=bounds)
    return (out, closest, origin) if want_closest else (out, origin)


def _axes_mask(axes):
    """o2v_hip_crossings_dense's bits of a non-empty subset of "xyz" (any order, no letter twice)."""
    if not isinstance(axes, str):
        raise TypeError(f"axes must be a string of the letters x, y, z, not {type(axes).__name__}")
    if not axes or any(a not in _AXIS_BITS for a in axes) or len(set(axes)) != len(axes):
        raise ValueError(f"axes must be a non-empty subset of 'xyz', not {axes!r}")
    return sum(_AXIS_BITS[a] for a in axes)


def crossing_numbers(dv, resolution, *, axes="xyz", out=None, origin=None, supersampling=1, unit_transform=None, bounds=None,
                     max_layers=None):
    """The signed crossing numbers of `dv`'s mesh (set_mesh) at every voxel centre of a box: along each
    axis of `axes` the triangles that the line through the centre crosses are counted with the sign of their orientation, below
    the centre and above it, and the two counts of every axis are added.  Returns (S, origin), S int32 [z, y, x]: voxel
    (x, y, z) is S[z - oz, y - oy, x - ox].  An outward-wound closed mesh gives 2 len(axes) inside and 0 outside, an
    inward-wound one the negative; parts pushed into each other add up; a ray through a hole is off by one.

    axes:  any non-empty subset of "xyz".
    out:   an int32 3-D tensor [z, y, x] of any strides on the voxelizer's device; the box is `origin` (default 0) plus its
           shape.  Without it the box is the grid from `origin` on, into a new contiguous tensor.
    The transform is voxelize's for the same resolution, supersampling, unit_transform and bounds.  max_layers cuts the box
    into z ranges of at most that many layers, one call each, written into the one tensor (the same bits as one call)."""
    _require_shared_runtime()
    mask = _axes_mask(axes)
    _check_sampling(resolution, supersampling, max_layers)
    device = _device(dv)
    origin = tuple(int(v) for v in (origin or (0, 0, 0)))
    if len(origin) != 3 or any(v < 0 or v >= resolution for v in origin):
        raise ValueError(f"origin {origin} must be three voxel coordinates inside the grid")
    if out is None:
        out = torch.empty(tuple(resolution - v for v in origin[::-1]), dtype=torch.int32, device=device)
    else:
        _check_grid(out, "out", torch.int32, device)
        if 0 in out.shape:
            raise ValueError("out has an empty dimension")
        if any(o + n > resolution for o, n in zip(origin, out.shape[::-1])):
            raise ValueError(f"origin {origin} + out's extent {tuple(out.shape[::-1])} [x, y, z] reaches past the grid of {resolution}")
    nz, ny, nx = out.shape
    step = nz if max_layers is None else max_layers
    _sync(device)   # (the caller's writes to out have landed)
    for z in range(0, nz, step):
        k = min(step, nz - z)
        o = out[z:z + k]
        dv.crossings_dense(resolution, mask, (origin[0], origin[1], origin[2] + z), (nx, ny, k), o.data_ptr(), _strides(o),
                           supersampling=supersampling, unit_transform=unit_transform, bounds=bounds)
    return out, origin


def winding_fill(dv, resolution, *, axes="xyz", rule="nonzero", min_sum=None, box="grid", out=None, origin=None, supersampling=1,
                 strategy="max", unit_transform=None, bounds=None, max_layers=None):
    """A solid fill by a vote of axis rays: uint8 labels in the format of voxelize_dense(fmt="labels",
    fill=True), so distance_transform, RayCaster, to_voxels, voxel_faces, downsample and spread_colors take the result as they
    take fill=True's.  Returns (labels, origin).  Label 1 is the surface voxels of voxelize_dense(fmt="labels") for the same
    arguments and box; label 2 every other voxel of the box whose crossing number S (crossing_numbers, the same axes) says
    inside:

    rule "nonzero":   |S| >= min_sum.  It does not depend on the mesh's winding, and it keeps the overlap of closed parts that
                      are pushed into each other, which the z-parity rule of fill=True hollows out.
    rule "positive":  S >= min_sum.  Inward-wound shells carve: a cavity wound inwards inside an outward-wound body is empty.
    min_sum:          an integer in 1 ... 2 len(axes); the default len(axes) + 1 is more than half of the 2 len(axes) rays, so
                      a ray that slips through a hole of an open mesh is outvoted.
    box, out, origin, supersampling, strategy, unit_transform, bounds, max_layers are voxelize_dense's; every voxel of `out`
    is written: it is cleared once the arguments have been checked, so an error raised after that by a device call (a voxel
    outside the tensor's box, an `out` smaller than the tight box) leaves it cleared.  With box="tight" the box is the surface's
    tight box.  The thresholding is plain torch on the two grids."""
    _require_shared_runtime()
    _axes_mask(axes)
    if rule not in ("nonzero", "positive"):
        raise ValueError(f"rule must be 'nonzero' or 'positive', not {rule!r}")
    if min_sum is None:
        min_sum = len(axes) + 1
    if isinstance(min_sum, bool) or not isinstance(min_sum, numbers.Integral):
        raise TypeError(f"min_sum must be an integer, not {min_sum!r}")
    if not 1 <= min_sum <= 2 * len(axes):
        raise ValueError(f"min_sum must be 1 ... {2 * len(axes)} for axes {axes!r}, not {min_sum}")
    if box not in ("grid", "tight"):
        raise ValueError(f"box must be 'grid' or 'tight', not {box!r}")
    if strategy not in STRATEGIES:
        raise ValueError(f"strategy must be 'max' or 'blend', not {strategy!r}")
    _check_sampling(resolution, supersampling, max_layers)
    if resolution * supersampling > MAX_SAMPLES:
        raise ValueError(f"resolution x supersampling = {resolution * supersampling} is above {MAX_SAMPLES}: x / y tiles are not "
                         "supported by the dense path")
    if box == "tight" and origin is not None:
        raise ValueError("origin is given by the voxels with box='tight'")
    device = _device(dv)
    if out is not None:
        _check_grid(out, "out", torch.uint8, device)
        if 0 in out.shape:
            raise ValueError("out has an empty dimension")
        if box == "grid":
            o = tuple(int(v) for v in (origin or (0, 0, 0)))
            if len(o) != 3 or any(v < 0 for v in o) or any(a + n > resolution for a, n in zip(o, out.shape[::-1])):
                raise ValueError(f"origin {o} + out's extent {tuple(out.shape[::-1])} [x, y, z] reaches past the grid of {resolution}")
        out.zero_()
    labels, origin = voxelize_dense(dv, resolution, fmt="labels", box=box, out=out, origin=origin, supersampling=supersampling,
                                    strategy=strategy, unit_transform=unit_transform, bounds=bounds, max_layers=max_layers)
    if 0 in labels.shape:
        return labels, origin
    # (an `out` larger than the tight box may reach past the grid: the part within it)
    ext = [min(n, resolution - o) for n, o in zip(labels.shape, origin[::-1])]
    part = labels[:ext[0], :ext[1], :ext[2]]
    S, _ = crossing_numbers(dv, resolution, axes=axes, origin=origin, supersampling=supersampling, unit_transform=unit_transform,
                            bounds=bounds, max_layers=max_layers, out=torch.empty(tuple(part.shape), dtype=torch.int32, device=device))
    inside = (S.abs() >= min_sum) if rule == "nonzero" else (S >= min_sum)
    part.masked_fill_(inside & (part == 0), 2)
    return labels, origin


def extract_surface(dv, field, level=0.0, *, origin=(0, 0, 0), transform=None, supersampling=1):
    """The level set `level` of `field` as an indexed triangle mesh, by surface nets: one vertex per
    cell of 2 x 2 x 2 samples the surface passes through, one quad (two triangles) per grid edge it crosses.  Returns
    (positions float32 [V, 3], faces int32 [T, 3]), new contiguous tensors in the shape set_mesh takes; (0, 3) both when there is
    no surface.  Inside is field < level; the normals point from inside to outside.

    field:      a float32 3-D tensor [z, y, x] of any strides on the voxelizer's device (what mesh_distance and fmt="sdf"
                return); it is only read.  A surface that leaves the box is open there.
    origin:     (ox, oy, oz), the one the field came with: sample (x, y, z) is the voxel centre origin + (x, y, z) + 0.5.
    transform:  None: positions in voxel space.  dv.transform() (the 12 floats, model to sample space): positions in model
                space, A^-1 (supersampling * p), computed in float64 and rounded once."""
    _require_shared_runtime()
    if isinstance(level, bool) or not isinstance(level, numbers.Real) or not float("-inf") < float(level) < float("inf"):
        raise ValueError(f"level must be a finite number, not {level!r}")
    level = hip.C.c_float(float(level)).value
    if not float("-inf") < level < float("inf"):
        raise ValueError("level is not finite as a float32")
    if supersampling not in (1, 2):
        raise ValueError("supersampling must be 1 or 2")
    device = _device(dv)
    _check_grid(field, "field", torch.float32, device)
    if 0 in field.shape:
        raise ValueError("field has an empty dimension")
    origin = _origin(origin)
    if any(o + n > MAX_SURFACE_EXTENT for o, n in zip(origin, field.shape[::-1])):
        raise ValueError(f"origin {origin} + field's extent {tuple(field.shape[::-1])} [x, y, z] is above {MAX_SURFACE_EXTENT}")
    transform = _mesh_transform(transform)
    nz, ny, nx = field.shape
    args = (field.data_ptr(), _strides(field), (nx, ny, nz), level)
    _sync(device)   # (the caller's writes to field have landed)
    n_vertices, n_triangles = dv.surface_count(*args)
    positions = torch.empty((n_vertices, 3), dtype=torch.float32, device=device)
    faces = torch.empty((n_triangles, 3), dtype=torch.int32, device=device)
    if n_vertices:
        dv.surface_write(*args, origin, positions.data_ptr(), n_vertices, _ptr(faces) if n_triangles else None, n_triangles)
    return _to_model_space(positions, transform, supersampling), faces


def _mesh_transform(transform):
    """The transform argument of extract_surface and label_surfaces: None, or its 12 numbers as a float64 tensor on the host."""
    if transform is None:
        return None
    transform = torch.as_tensor(transform, dtype=torch.float64).reshape(-1)
    if transform.numel() != 12:
        raise ValueError("transform must hold 12 numbers: a row-major 3 x 3 matrix, then the translation")
    return transform


def _to_model_space(positions, transform, supersampling):
    """Voxel-space positions float32 [V, 3] in model space: A^-1 (supersampling * p - t) for transform = (A, t) as _mesh_transform
    returns it, computed in float64 and rounded once; the positions themselves if transform is None or there are none."""
    if transform is None or not positions.shape[0]:
        return positions
    device = positions.device
    inverse = torch.linalg.inv(transform[:9].reshape(3, 3)).to(device)   # (3 x 3, on the host)
    p = positions.to(torch.float64) * supersampling - transform[9:].to(device)
    return (p[:, None, :] * inverse[None, :, :]).sum(dim=2).to(torch.float32).contiguous()


def _origin(origin):
    """The origin of a box as three ints, none negative."""
    origin = tuple(int(v) for v in origin)
    if len(origin) != 3 or any(v < 0 for v in origin):
        raise ValueError(f"origin {origin} must be three voxel coordinates, none negative")
    return origin


def _grid_format(grid, level):
    """(format, level as a float32 or None) of a grid tensor by its dtype - bool / uint8: GRID_U8, int32: GRID_BITS, float32
    with a finite level: GRID_F32_BELOW -, as RayCaster, components and flood take it."""
    if grid.dtype in (torch.bool, torch.uint8):
        fmt = hip.GRID_U8
    elif grid.dtype == torch.int32:
        fmt = hip.GRID_BITS
    elif grid.dtype == torch.float32:
        fmt = hip.GRID_F32_BELOW
    else:
        raise TypeError(f"grid must be bool, uint8, int32 (bits) or float32, not {grid.dtype}")
    if fmt == hip.GRID_F32_BELOW:
        if level is None:
            raise ValueError("a float32 grid needs level: a voxel is solid where grid < level")
        if isinstance(level, bool) or not isinstance(level, numbers.Real) or not float("-inf") < float(level) < float("inf"):
            raise ValueError(f"level must be a finite number, not {level!r}")
        level = hip.C.c_float(float(level)).value
        if not float("-inf") < level < float("inf"):
            raise ValueError("level is not finite as a float32")
    elif level is not None:
        raise ValueError(f"level is for float32 grids, not {grid.dtype}")
    return fmt, level


class RayCaster:
    """First hits of rays in a dense grid on the voxelizer's device.

        caster = dense.RayCaster(dv, grid)                  # one pass over the grid; the snapshot stays in dv
        hit, t = caster.cast(origins, directions)           # int32 [..., 4] = (x, y, z, face), float32 [...]

    grid:    a 3-D tensor [z, y, x] of any strides: bool or uint8 (solid where != 0: occupancy, labels), int32 (the words of
             fmt="bits": the last dimension counts 32-voxel words, unit stride along it) or float32 with `level` (solid where
             grid < level: an SDF or TSDF with level=0).  `level` with any other dtype raises.
    origin:  (ox, oy, oz), the one the grid came with: voxel (x, y, z) is the unit cube at origin + (x, y, z).
    The snapshot is taken at once: the grid may change or be freed afterwards.  A voxelizer holds one snapshot; a later
    RayCaster on the same `dv` replaces it, and casting with the earlier one raises RuntimeError."""

    def __init__(self, dv, grid, *, level=None, origin=(0, 0, 0)):
        def limit(dims):
            if any(o + n > MAX_RAY_EXTENT for o, n in zip(origin, dims)):
                raise ValueError(f"origin {origin} + the grid's extent {dims} [x, y, z] is above {MAX_RAY_EXTENT}")
        origin = _origin(origin)
        device, fmt, level, dims = _set_grid(dv, grid, level, limit)
        self.dv, self.device, self.origin, self.dims = dv, device, origin, dims
        _sync(device)   # (the caller's writes to grid have landed)
        self._generation = dv.raycast_build(grid.data_ptr(), fmt, _strides(grid), dims, 0.0 if level is None else level, origin)

    def cast(self, origins, directions, t_max=float("inf")):
        """(hit, t) of the rays origins + t * directions, float32 tensors [..., 3] of one shape on the device, in voxel space;
        directions need not be normalised (t is in units of their length).  hit int32 [..., 4] = (x, y, z, face): the first
        solid voxel and the face the ray entered it through (0 / 1: low / high x, 2 / 3: y, 4 / 5: z; -1: the ray started
        inside it, t = 0); t float32 [...].  A miss, also one past t_max (a number >= 0), is (-1, -1, -1, -1) and +inf; a ray with
        a non-finite component or an origin beyond 2^22 is (-1, -1, -1, -2) and NaN.  New contiguous tensors."""
        if self.dv.raycast_generation() != self._generation:
            raise RuntimeError("this RayCaster's snapshot has been replaced by a later build on the same voxelizer")
        if isinstance(t_max, bool) or not isinstance(t_max, numbers.Real) or not float(t_max) >= 0.0:
            raise ValueError(f"t_max must be a number >= 0 or inf, not {t_max!r}")
        for name, r in (("origins", origins), ("directions", directions)):
            if not isinstance(r, torch.Tensor):
                raise TypeError(f"{name} must be a torch tensor")
            if r.dtype != torch.float32:
                raise TypeError(f"{name} must be torch.float32, not {r.dtype}")
            if r.dim() < 1 or r.shape[-1] != 3:
                raise ValueError(f"{name} must have shape [..., 3], not {tuple(r.shape)}")
            if r.device != self.device:
                raise ValueError(f"{name} is on {r.device}, the voxelizer on {self.device}")
        if origins.shape != directions.shape:
            raise ValueError(f"origins {tuple(origins.shape)} and directions {tuple(directions.shape)} must have one shape")
        shape = tuple(origins.shape[:-1])
        o, d = origins.reshape(-1, 3).contiguous(), directions.reshape(-1, 3).contiguous()
        n = o.shape[0]
        hit = torch.empty((n, 4), dtype=torch.int32, device=self.device)
        t = torch.empty((n,), dtype=torch.float32, device=self.device)
        if n:
            _sync(self.device)   # (the caller's writes to the rays have landed)
            self.dv.raycast(o.data_ptr(), d.data_ptr(), n, float(t_max), hit.data_ptr(), t.data_ptr())
        return hit.reshape(shape + (4,)), t.reshape(shape)


def raycast(dv, grid, origins, directions, *, t_max=float("inf"), level=None, origin=(0, 0, 0)):
    """RayCaster(dv, grid, level=level, origin=origin).cast(origins, directions, t_max) in one call."""
    return RayCaster(dv, grid, level=level, origin=origin).cast(origins, directions, t_max)


def camera_rays(width, height, eye, target, up, fov_y_degrees, device):
    """(origins, directions), float32 [height, width, 3] each: the rays of a pinhole camera at `eye` looking at `target`
    through the centres of width x height pixels, row 0 at the top; fov_y_degrees is the vertical field of view.  The
    directions have unit length, so RayCaster.cast gives distances in voxels.  Plain torch."""
    if width < 1 or height < 1 or not 0.0 < float(fov_y_degrees) < 180.0:
        raise ValueError("width and height must be positive and 0 < fov_y_degrees < 180")
    eye, target, up = (torch.as_tensor(v, dtype=torch.float64).reshape(3) for v in (eye, target, up))
    forward = target - eye
    if float(forward.norm()) == 0.0:
        raise ValueError("eye and target coincide")
    forward = forward / forward.norm()
    right = torch.linalg.cross(forward, up)
    if not float(right.norm()) > 1e-9 * float(up.norm()):
        raise ValueError("up is parallel to the viewing direction")
    right = right / right.norm()
    true_up = torch.linalg.cross(right, forward)
    half = float(torch.tan(torch.deg2rad(torch.tensor(float(fov_y_degrees), dtype=torch.float64)) / 2))
    v = (1.0 - (torch.arange(height, dtype=torch.float64) + 0.5) * (2.0 / height)) * half
    u = ((torch.arange(width, dtype=torch.float64) + 0.5) * (2.0 / width) - 1.0) * (half * width / height)
    directions = forward[None, None, :] + u[None, :, None] * right[None, None, :] + v[:, None, None] * true_up[None, None, :]
    directions = directions / directions.norm(dim=2, keepdim=True)
    origins = eye.expand(height, width, 3)
    return origins.to(torch.float32).contiguous().to(device), directions.to(torch.float32).contiguous().to(device)


# ---- connected components and flood fill --------------------------------------------------------------

def _limit_voxels(dims):
    """The size limit of components / flood / nearest_voxel: a linear index and a label are one int32."""
    if max(dims) > MAX_CC_DIM or dims[0] * dims[1] * dims[2] > MAX_CC_VOXELS:
        raise ValueError(f"the grid's extent {dims} [x, y, z] is above {MAX_CC_DIM} along an axis or {MAX_CC_VOXELS} voxels in all")


def _limit_words(dims):
    """The size limit of to_voxels / count_voxels / save_voxels and voxel_faces: no linear index, words of 64 voxels."""
    if max(dims) > MAX_CC_DIM or -(-dims[0] // 64) * dims[1] * dims[2] > MAX_GATHER_WORDS:
        raise ValueError(f"the grid's extent {dims} [x, y, z] is above {MAX_CC_DIM} along an axis or {MAX_GATHER_WORDS} "
                         "words of 64 voxels along x in all")


def _set_grid(dv, grid, level, limit, connectivity=None):
    """(device, format, level, (nx, ny, nz)) of a set grid - the grid of RayCaster, components, flood, to_voxels, voxel_faces and
    nearest_voxel -, checked.  limit((nx, ny, nz)) raises where the extent is above the caller's size limit."""
    _require_shared_runtime()
    device = _device(dv)
    if not isinstance(grid, torch.Tensor) or grid.dim() != 3:
        raise ValueError("grid must be a 3-D tensor [z, y, x]")
    fmt, level = _grid_format(grid, level)
    if connectivity is not None and (isinstance(connectivity, bool) or connectivity not in (6, 18, 26)):
        raise ValueError(f"connectivity must be 6, 18 or 26, not {connectivity!r}")
    if grid.device != device:
        raise ValueError(f"grid is on {grid.device}, the voxelizer on {device}")
    if 0 in grid.shape:
        raise ValueError("grid has an empty dimension")
    if fmt == hip.GRID_BITS and grid.stride(2) != 1:
        raise ValueError("a bits grid needs unit stride along x (its last dimension)")
    nz, ny, nx = grid.shape
    if fmt == hip.GRID_BITS:
        nx *= 32
    limit((nx, ny, nz))
    return device, fmt, level, (nx, ny, nz)


def components(dv, grid, *, level=None, connectivity=6, background=False, out=None):
    """The connected components of a dense grid on the voxelizer's device.  Returns (labels, n): labels
    int32 [z, y, x], 0 outside the set and 1 .. n inside it, the components numbered by their first voxel in [z, y, x] order -
    the numbering of scipy.ndimage.label -, and n, their number.

    grid:          as RayCaster takes it: bool or uint8 (solid where != 0), int32 (the words of fmt="bits"; labels then has 32
                   voxels per word along x) or float32 with `level` (solid where grid < level).  It is only read.
    connectivity:  6, 18 or 26: neighbours share a face; a face or an edge; a face, an edge or a corner.
    background:    False: the components of the solid voxels; True: of the voxels of the box that are not solid.
    out:           an int32 tensor of the labels' shape (any strides, not in grid's storage), written as it is; else a new
                   contiguous tensor.  Contiguous labels need no per-voxel scratch in the context."""
    device, fmt, level, dims = _set_grid(dv, grid, level, _limit_voxels, connectivity)
    shape = (dims[2], dims[1], dims[0])
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=device)
    else:
        _check_grid(out, "out", torch.int32, device, shape)
    _sync(device)   # (the caller's writes to grid and out have landed)
    n = dv.components_dense(grid.data_ptr(), fmt, _strides(grid), dims, 0.0 if level is None else level, connectivity,
                            hip.CC_INVERT if background else 0, out.data_ptr(), _strides(out))
    return out, n


def _seeds(seeds, device):
    """seeds as a contiguous int32 tensor [n, 3] on the device (None: no seeds)."""
    if seeds is None:
        return None
    if not isinstance(seeds, torch.Tensor):
        seeds = torch.as_tensor(seeds, dtype=torch.int64).reshape(-1, 3).to(device)
    if seeds.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"seeds must be torch.int32 or torch.int64, not {seeds.dtype}")
    if seeds.dim() != 2 or seeds.shape[1] != 3:
        raise ValueError(f"seeds must have shape [n, 3] (x, y, z), not {tuple(seeds.shape)}")
    if seeds.device != device:
        raise ValueError(f"seeds is on {seeds.device}, the voxelizer on {device}")
    if seeds.dtype == torch.int64:   # (a seed that does not fit an int32 is outside every box: it is ignored, as the call ignores it)
        seeds = seeds.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    return seeds.contiguous()


def flood(dv, grid, *, seeds=None, border=False, level=None, connectivity=6, background=False, values=(1, 0, 0), out=None):
    """Flood fill from seeds: a uint8 tensor [z, y, x] that holds values[0] in the components of the
    set that hold a seed, values[1] in its other components and values[2] outside the set.  grid, level, connectivity and
    background as components takes them.

    seeds:   an int32 / int64 tensor [n, 3] of (x, y, z) on the device, or a sequence of such triples; a seed outside the box
             or not in the set is ignored.
    border:  True: every voxel of the set on the six faces of the box is a seed as well.
    values:  three integers 0 .. 255.
    out:     a uint8 tensor of the grid's shape (any strides, not in grid's storage), or a bool tensor when the values are 0 / 1."""
    device, fmt, level, dims = _set_grid(dv, grid, level, _limit_voxels, connectivity)
    shape = (dims[2], dims[1], dims[0])
    values = tuple(values)
    if len(values) != 3 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v <= 255 for v in values):
        raise ValueError(f"values must be three integers 0 .. 255, not {values!r}")
    seeds = _seeds(seeds, device)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=device)
    elif isinstance(out, torch.Tensor) and out.dtype == torch.bool:
        if any(v > 1 for v in values):
            raise ValueError(f"a bool out needs values of 0 / 1, not {values!r}")
        _check_grid(out, "out", torch.bool, device, shape)
    else:
        _check_grid(out, "out", torch.uint8, device, shape)
    n = 0 if seeds is None else seeds.shape[0]
    flags = (hip.CC_INVERT if background else 0) | (hip.CC_SEED_BORDER if border else 0)
    _sync(device)   # (the caller's writes to grid, seeds and out have landed)
    dv.flood_dense(grid.data_ptr(), fmt, _strides(grid), dims, 0.0 if level is None else level, connectivity, flags,
                   seeds.data_ptr() if n else None, n, values, out.data_ptr(), _strides(out))
    return out


def exterior(dv, grid, *, level=None, connectivity=6):
    """bool [z, y, x]: the empty voxels that reach the border of the box through empty voxels - flood with background=True,
    border=True and values (1, 0, 0)."""
    device, _, _, dims = _set_grid(dv, grid, level, _limit_voxels, connectivity)
    out = torch.empty((dims[2], dims[1], dims[0]), dtype=torch.bool, device=device)
    return flood(dv, grid, border=True, level=level, connectivity=connectivity, background=True, values=(1, 0, 0), out=out)


def solidify(dv, grid, *, level=None, connectivity=6, out=None):
    """uint8 labels [z, y, x]: 1 = solid, 2 = empty but enclosed (no path of empty voxels to the border of the box), 0 =
    exterior - one flood of the empty voxels from the border with values (0, 2, 1).  This is the format of fmt="labels",
    fill=True, so distance_transform(..., "sdf"), RayCaster and extract_surface take it as it is, and on a single closed body it
    is the same grid; where closed parts overlap it holds the union, which the parity rule of fill=True hollows out.

    What it is not: a repair of the mesh.  A surface with a hole one voxel wide leaks - the flood gets in and the body has no
    interior.  A pocket of outside air that surface voxels seal off - a dent closed by the voxels' thickness - counts as
    interior.  `connectivity` is that of the empty space: 6 leaks least."""
    return flood(dv, grid, border=True, level=level, connectivity=connectivity, background=True, values=(0, 2, 1), out=out)


def component_sizes(labels, n):
    """int64 [n + 1]: the voxels per label of components' (labels, n); index 0 is the background.  Plain torch."""
    return torch.bincount(labels.reshape(-1), minlength=n + 1)


def remove_small(dv, grid, min_voxels, *, level=None, connectivity=26):
    """bool [z, y, x]: the solid voxels whose component has at least min_voxels voxels.  Plain torch over components."""
    if isinstance(min_voxels, bool) or not isinstance(min_voxels, numbers.Integral) or min_voxels < 0:
        raise ValueError(f"min_voxels must be an integer >= 0, not {min_voxels!r}")
    labels, n = components(dv, grid, level=level, connectivity=connectivity)
    keep = component_sizes(labels, n) >= min_voxels
    keep[0] = False
    return keep[labels.to(torch.int64)]


# ---- geodesic distances and shortest paths ---------------------------------------------------------------

CHAMFER_UNIT = 3   # the chamfer metric's face step: dist.float() / CHAMFER_UNIT reads in voxels
_GEO_WEIGHTS = {("steps", 6): (1, 0, 0), ("steps", 18): (1, 1, 0), ("steps", 26): (1, 1, 1),
                ("chamfer", 6): (3, 0, 0), ("chamfer", 18): (3, 4, 0), ("chamfer", 26): (3, 4, 5)}


def _geo_weights(metric, connectivity, weights):
    """The (face, edge, corner) step costs of geodesic_distance / shortest_paths: `weights` if given, else the metric's, cut to
    the connectivity."""
    if weights is not None:
        if isinstance(weights, (str, bytes)) or not hasattr(weights, "__iter__"):
            raise ValueError(f"weights must be three integers 0 .. {hip.GEO_MAX_WEIGHT}, not {weights!r}")
        weights = tuple(weights)
        if len(weights) != 3 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v <= hip.GEO_MAX_WEIGHT for v in weights) \
                or not any(weights):
            raise ValueError(f"weights must be three integers 0 .. {hip.GEO_MAX_WEIGHT}, not all 0, not {weights!r}")
        return tuple(int(v) for v in weights)
    if isinstance(connectivity, bool) or connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity must be 6, 18 or 26, not {connectivity!r}")
    if metric not in ("steps", "chamfer"):
        raise ValueError(f"metric must be 'steps' or 'chamfer', not {metric!r}")
    return _GEO_WEIGHTS[metric, connectivity]


def geodesic_distance(dv, grid, seeds=None, *, border=False, metric="chamfer", connectivity=26, weights=None, background=False,
                      max_distance=None, level=None, out=None):
    """How far every voxel of the set is from the nearest seed without leaving the set: an int32 tensor
    [z, y, x] of the smallest sum of step costs over all paths inside the set, 0 at a seed, -1 where the voxel is not in the
    set, not reached, or further than max_distance.  grid, level and background as components takes them.

    seeds:         an int32 / int64 tensor [n, 3] of (x, y, z) on the device, or a sequence of such triples; a seed outside the
                   box or not in the set is ignored.
    border:        True: every voxel of the set on the six faces of the box is a seed as well.
    metric:        "chamfer": a face, edge, corner step costs 3, 4, 5 - dist.float() / CHAMFER_UNIT approximates the Euclidean
                   length in voxels; "steps": every step costs 1 (hop counts).
    connectivity:  6, 18 or 26: the steps that exist - faces; faces and edges; faces, edges and corners.  A diagonal step
                   needs only its two end voxels in the set.
    weights:       (face, edge, corner) costs, integers 0 .. 65 535, 0 = no such step, not all 0; overrides metric and connectivity.
    max_distance:  an integer 0 .. 2^31 - 2: nothing further than that is reached, and nothing is propagated through such a
                   voxel (bounded region growing); None: no cap.
    out:           an int32 tensor of the grid's shape (any strides, not in grid's storage), written as it is; else a new
                   contiguous tensor.  A contiguous out needs no per-voxel scratch in the context."""
    device, fmt, level, dims = _set_grid(dv, grid, level, _limit_voxels, connectivity)
    shape = (dims[2], dims[1], dims[0])
    weights = _geo_weights(metric, connectivity, weights)
    if max_distance is None:
        max_distance = hip.GEO_MAX_DISTANCE
    elif isinstance(max_distance, bool) or not isinstance(max_distance, numbers.Integral) or not 0 <= max_distance <= hip.GEO_MAX_DISTANCE:
        raise ValueError(f"max_distance must be an integer 0 .. {hip.GEO_MAX_DISTANCE}, not {max_distance!r}")
    seeds = _seeds(seeds, device)
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=device)
    else:
        _check_grid(out, "out", torch.int32, device, shape)
    n = 0 if seeds is None else seeds.shape[0]
    flags = (hip.CC_INVERT if background else 0) | (hip.CC_SEED_BORDER if border else 0)
    _sync(device)   # (the caller's writes to grid, seeds and out have landed)
    dv.geodesic_dense(grid.data_ptr(), fmt, _strides(grid), dims, 0.0 if level is None else level, weights, flags,
                      seeds.data_ptr() if n else None, n, int(max_distance), out.data_ptr(), _strides(out))
    return out


def shortest_paths(dv, dist, targets, *, metric="chamfer", connectivity=26, weights=None, max_len=None):
    """The shortest paths from targets back to the seeds of a geodesic_distance grid.  Returns (paths,
    lengths): paths int32 [n, L, 3], row i the voxels (x, y, z) of target i's path from the target to a seed, padded with -1;
    lengths int32 [n], the voxels of the whole path with both ends, -1 for a target outside the box or not reached, -2 where the
    grid was not made with these weights.  Of a path longer than L its first L voxels are there; lengths holds the true length.
    Among equally short ways the walk takes the first neighbour in ascending (dz, dy, dx) order.

    dist:      what geodesic_distance returned (int32 [z, y, x], any strides); metric, connectivity and weights as given there.
    targets:   an int32 / int64 tensor [n, 3] of (x, y, z) on the device, or a sequence of such triples.
    max_len:   L; None: max(dist at the targets) // (the smallest weight above 0) + 1, which holds every path - one small read."""
    _require_shared_runtime()
    device = _device(dv)
    _check_grid(dist, "dist", torch.int32, device)
    if 0 in dist.shape:
        raise ValueError("dist has an empty dimension")
    dims = (dist.shape[2], dist.shape[1], dist.shape[0])
    _limit_voxels(dims)
    weights = _geo_weights(metric, connectivity, weights)
    if targets is None:
        raise ValueError("targets must be a tensor [n, 3] or a sequence of (x, y, z)")
    targets = _seeds(targets, device)
    n = targets.shape[0]
    if max_len is not None and (isinstance(max_len, bool) or not isinstance(max_len, numbers.Integral) or not 0 <= max_len <= 2 ** 31 - 1):
        raise ValueError(f"max_len must be an integer 0 .. {2 ** 31 - 1}, not {max_len!r}")
    _sync(device)   # (the caller's writes to dist and targets have landed)
    if max_len is None:
        max_len = 1
        if n:
            t = targets.to(torch.int64)
            inside = ((t >= 0) & (t < torch.tensor(dims, dtype=torch.int64, device=device))).all(dim=1)
            t = t[inside]
            if t.shape[0]:
                max_len = max(int(dist[t[:, 2], t[:, 1], t[:, 0]].max()), 0) // min(w for w in weights if w) + 1
    paths = torch.full((n, max_len, 3), -1, dtype=torch.int32, device=device)
    lengths = torch.full((n,), -1, dtype=torch.int32, device=device)
    _sync(device)   # (the fills have landed)
    if n:
        dv.geodesic_paths(dist.data_ptr(), _strides(dist), dims, weights, targets.data_ptr(), n, int(max_len), paths.data_ptr() if max_len else None,
                          lengths.data_ptr())
    return paths, lengths


# ---- local thickness and ball morphology -----------------------------------------------------------------

MAX_THICK_RADIUS2 = hip.THICK_MAX_RADIUS2   # local_thickness and the morphology: floor(radius^2) + 1 is at most this (radius < 128)
_THICK_FORMATS = {"r2": (0, torch.int32), "thickness": (hip.THICK_F32, torch.float32)}


def _limit_thickness(dims):
    """The size limits of local_thickness and the morphology: a centre is one int32 index, a squared distance one int32."""
    _limit_voxels(dims)
    if sum((n - 1) ** 2 for n in dims) > MAX_NEAREST_D2:
        raise ValueError(f"the grid's extent {dims} [x, y, z] has (nx-1)^2 + (ny-1)^2 + (nz-1)^2 above {MAX_NEAREST_D2}")


def _radius_cap(radius, name="radius"):
    """cap = floor(radius^2) + 1 of a radius in voxels: the ball {|q|^2 < cap} is {|q| <= radius}."""
    if isinstance(radius, bool) or not isinstance(radius, numbers.Real) or not float(radius) >= 0.0:
        raise ValueError(f"{name} must be a number >= 0, not {radius!r}")
    r2 = float(radius) * float(radius)
    if not r2 < MAX_THICK_RADIUS2:
        raise ValueError(f"{name} {radius!r}: floor({name}^2) + 1 is above {MAX_THICK_RADIUS2} (at most {math.sqrt(MAX_THICK_RADIUS2 - 1):.2f} voxels)")
    return math.floor(r2) + 1


def _byte_ranges_overlap(a, b):
    """Whether the address ranges two tensors reach overlap - what o2v_hip_thickness_dense refuses of its two outputs (two
    slices of one batch tensor share a storage and do not overlap)."""
    def span(t):
        reach = sum((n - 1) * abs(st) for n, st in zip(t.shape, t.stride())) + 1
        return t.data_ptr(), t.data_ptr() + reach * t.element_size()
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def _thickness(dv, grid, cap, level, background, border, flags, dst_dtype, out, depth2, out_name="out", depth2_name="depth2"):
    """One o2v_hip_thickness_dense call: (dst, depth2 or None), new contiguous tensors where out / depth2 is None / True."""
    device, fmt, level, dims = _set_grid(dv, grid, level, _limit_thickness)
    shape = (dims[2], dims[1], dims[0])
    if out is None:
        out = torch.empty(shape, dtype=dst_dtype, device=device)
    else:
        _check_grid(out, out_name, dst_dtype, device, shape)
        _outside_storage(out, out_name, grid)
    if depth2 is True:
        depth2 = torch.empty(shape, dtype=torch.int32, device=device)
    elif depth2 is not None and depth2 is not False:
        _check_grid(depth2, depth2_name, torch.int32, device, shape)
        _outside_storage(depth2, depth2_name, grid)
        if _byte_ranges_overlap(depth2, out):
            raise ValueError(f"{depth2_name} must not overlap {out_name}")
    else:
        depth2 = None
    flags |= (hip.THICK_BACKGROUND if background else 0) | (hip.THICK_BORDER if border else 0)
    _sync(device)   # (the caller's writes to grid, out and depth2 have landed)
    dv.thickness_dense(grid.data_ptr(), fmt, _strides(grid), dims, 0.0 if level is None else level, flags, cap, out.data_ptr(), _strides(out),
                       _ptr(depth2), None if depth2 is None else _strides(depth2))
    return out, depth2


def local_thickness(dv, grid, max_radius, *, level=None, background=False, border=True, fmt="r2", depth2=None, out=None):
    """How thick the set is at every voxel: the largest ball that lies inside the set and holds the voxel,
    as the squared radius T = max { min(depth2(c), cap) : |p - c|^2 < min(depth2(c), cap) } - exact integers, the same bits on
    every run.  Returns the tensor [z, y, x], 0 outside the set, or (thickness, depth2) when depth2 is given.

        solid, origin = dense.voxelize_dense(dv, 512, fill=True)
        t = dense.local_thickness(dv, solid, 8, fmt="thickness")      # float32, in voxels; 15.1 (the cap) means "a ball of radius 8 fits"
        thin = dense.thin_regions(dv, solid, 5)                       # bool: thinner than 5 voxels

    grid, level, background:  as components takes them: the set is the solid voxels, or with background=True the others.
    max_radius:  a number >= 0 and below 128, in voxels: the largest ball looked for is {|q| <= max_radius}, cap =
                 floor(max_radius^2) + 1.  Values at the cap (T == cap) mean "at least": the voxel lies in the opening by that
                 ball.  The ball stage costs about half the local thickness squared in writes per voxel of the regions thinner
                 than the cap, so the cap is mandatory: set it to the largest thickness that matters.
    border:      True: the world outside the box is not in the set, so the box's faces are skin; False: the box is a window
                 into a larger body and the balls are clipped to it.
    fmt:         "r2": int32 T; "thickness": float32 2 sqrt(T) - 1, the diameter of that ball in voxels.  A wall w voxels wide
                 reads w for odd w and w - 1 for even w: a digital ball is centred on a voxel, so its diameter is odd.
    depth2:      None; True for a new int32 tensor; or an int32 tensor of the voxel shape (any strides): the squared distance
                 to the nearest voxel that is not in the set (border=True: the outside of the box included), 0 outside the set,
                 0x7FFFFFFF where there is no such voxel.  Passing it saves the context 4 bytes of scratch per voxel.
    out:         a tensor of the voxel shape and fmt's dtype (any strides, not in grid's storage), written as it is; else a new
                 contiguous tensor."""
    if fmt not in _THICK_FORMATS:
        raise ValueError(f"fmt must be one of {sorted(_THICK_FORMATS)}, not {fmt!r}")
    flag, dtype = _THICK_FORMATS[fmt]
    cap = _radius_cap(max_radius, "max_radius")
    want_depth2 = depth2 is not None and depth2 is not False
    out, depth2 = _thickness(dv, grid, cap, level, background, border, flag, dtype, out, depth2)
    return (out, depth2) if want_depth2 else out


def inner_distance(dv, grid, *, level=None, background=False, border=True, out=None):
    """int32 [z, y, x]: for every voxel of the set the squared distance to the nearest voxel that is not in it - depth2 of
    local_thickness alone; 0 outside the set, 0x7FFFFFFF where there is no such voxel.  With border=True
    the world outside the box is not in the set.  distance_transform measures from the surface voxels outwards and inwards; this
    is the depth of the solid itself.  out: an int32 tensor of the voxel shape (any strides, not in grid's storage)."""
    _, depth2 = _thickness(dv, grid, 1, level, background, border, hip.THICK_OPEN_ONLY, torch.int32, None, True if out is None else out, depth2_name="out")
    return depth2


def erode(dv, grid, radius, *, level=None, background=False, border=True):
    """bool [z, y, x]: the erosion of the set by the ball {|q| <= radius}: the voxels whose whole ball lies
    in the set, depth2 > radius^2.  border=True: the world outside the box is empty, so the set is eroded from the box's faces too."""
    r2 = _radius_cap(radius) - 1
    return inner_distance(dv, grid, level=level, background=background, border=border) > r2


def opening(dv, grid, radius, *, level=None, background=False, border=True):
    """bool [z, y, x]: the opening of the set by the ball {|q| <= radius}: the union of the balls of that
    radius that lie inside the set - what is left when everything thinner is shaved off.  Two distance transforms, no ball stage."""
    cap = _radius_cap(radius)
    dst, _ = _thickness(dv, grid, cap, level, background, border, hip.THICK_OPEN_ONLY, torch.int32, None, None)
    return dst == cap


def dilate(dv, grid, radius, *, level=None):
    """bool [z, y, x]: the dilation of the set by the ball {|q| <= radius}: the complement of the background's erosion.  It works
    on the background with border=False - the world outside the box is empty space like any other, nothing there pushes back -,
    and a body cannot grow past the box: pad the grid first if it should."""
    return ~erode(dv, grid, radius, level=level, background=True, border=False)


def closing(dv, grid, radius, *, level=None):
    """bool [z, y, x]: the closing of the set by the ball {|q| <= radius}: the complement of the background's opening - gaps and
    holes that no ball of that radius fits into are filled.  Like dilate it works on the background with border=False: a gap
    between the body and the box's face counts as open to the outside only if a ball clipped to the box fits into it."""
    return ~opening(dv, grid, radius, level=level, background=True, border=False)


def thin_regions(dv, grid, min_thickness, *, level=None, background=False, border=True):
    """bool [z, y, x]: the voxels of the set where it is thinner than min_thickness voxels: the set less its
    opening by the ball of radius (min_thickness - 1) / 2, the largest ball whose diameter 2 r + 1 stays within min_thickness.  Two
    distance transforms and no ball stage, whatever the thickness: the check to run before printing or milling a model."""
    if isinstance(min_thickness, bool) or not isinstance(min_thickness, numbers.Real) or not float(min_thickness) >= 1.0:
        raise ValueError(f"min_thickness must be a number >= 1 (voxels), not {min_thickness!r}")
    cap = _radius_cap((float(min_thickness) - 1.0) / 2.0, "(min_thickness - 1) / 2")
    dst, _ = _thickness(dv, grid, cap, level, background, border, hip.THICK_OPEN_ONLY, torch.int32, None, None)
    return (dst > 0) & (dst < cap)


# ---- skeletons: topological thinning ---------------------------------------------------------------------

from .skeleton import skeleton_nodes, skeletonize  # noqa: E402,F401  (the torch layer of o2v_hip_thin_dense, a module of its own)

# ---- parts: watershed basins of a relief, merged by persistence ---------------------------------------------

from .watershed import split_parts, watershed, watershed_peaks  # noqa: E402,F401  (the torch layer of o2v_hip_watershed_dense)
from .grow import grow_labels, markers_from_seeds, seeded_watershed  # noqa: E402,F401  (the torch layer of o2v_hip_grow_dense)
from .labelmesh import LabelMesh, interface_areas, label_surfaces, part_mesh, relax_surface  # noqa: E402,F401  (the torch layer of o2v_hip_label_surface_*)

# ---- which labels touch: the region adjacency of a label grid ------------------------------------------------

from .adjacency import (LabelAdjacency, SkeletonGraph, adjacency_neighbours, coordination, label_adjacency,  # noqa: E402,F401
                        skeleton_graph)   # (the torch layer of o2v_hip_adjacency_count / _write)

# ---- Euler numbers, tunnels and cavities: the cell counts of a label grid ------------------------------------

from .topology import EulerStats, betti_numbers, euler_numbers, euler_stats, intrinsic_volumes  # noqa: E402,F401  (the torch layer of o2v_hip_euler_stats)

# ---- sparse voxel octrees: build, look up, expand --------------------------------------------------------------

from .octree import (Octree, build_octree, octree_depth, octree_level, octree_lookup,  # noqa: E402,F401
                     octree_to_dense)   # (the torch layer of o2v_hip_octree_build / _write / _lookup / _to_dense)
# ---- sparse voxel DAGs: equal subtrees of an octree merged ----------------------------------------------------
from .octree import OctreeDag, dag_lookup, dag_to_dense, octree_dag  # noqa: E402,F401   (o2v_hip_octree_dag_build / _write / _lookup / _to_dense)
# ---- rays through octrees and DAGs ---------------------------------------------------------------------------
from .octree import dag_raycast, octree_raycast  # noqa: E402,F401   (o2v_hip_octree_raycast / o2v_hip_octree_dag_raycast)

# ---- sky visibility and ambient occlusion -------------------------------------------------------------------

from .visibility import direction_set, openness, shade_colors  # noqa: E402,F401  (the torch layer of o2v_hip_openness)


# ---- dense grids as voxel lists and voxel files --------------------------------------------------------

def _gather_args(dv, grid, level, origin, argb, colors, palette):
    """(device, (grid_ptr, format, strides, dims, level), (origin, colour mode, argb, colors_ptr, color_strides, palette)): the
    arguments of dv.gather_count and, with the colour part, of dv.gather_write / gather_save, checked."""
    device, fmt, level, dims = _set_grid(dv, grid, level, _limit_words)
    origin = _origin(origin)
    if any(o + n > 2 ** 32 for o, n in zip(origin, dims)):
        raise ValueError(f"origin {origin} + the grid's extent {dims} [x, y, z] is above 2^32")
    if isinstance(argb, bool) or not isinstance(argb, numbers.Integral) or not -2 ** 31 <= argb < 2 ** 32:
        raise ValueError(f"argb must be an integer of 32 bits, not {argb!r}")
    if colors is not None and palette is not None:
        raise ValueError("colors and palette exclude each other")
    mode, colors_ptr, color_strides = hip.GATHER_COLOR_CONSTANT, None, None
    if colors is not None:
        _check_grid(colors, "colors", torch.int32, device, (dims[2], dims[1], dims[0]))
        mode, colors_ptr, color_strides = hip.GATHER_COLOR_GRID, colors.data_ptr(), _strides(colors)
    if palette is not None:
        if fmt != hip.GRID_U8:
            raise ValueError(f"palette needs a bool or uint8 grid, not {grid.dtype}")
        palette = [int(v) for v in (palette.reshape(-1).tolist() if isinstance(palette, torch.Tensor) else palette)]
        if len(palette) != 256 or any(not -2 ** 31 <= v < 2 ** 32 for v in palette):
            raise ValueError("palette must be 256 integers of 32 bits")
        mode = hip.GATHER_COLOR_PALETTE
    return (device, (grid.data_ptr(), fmt, _strides(grid), dims, 0.0 if level is None else level),
            (origin, mode, argb, colors_ptr, color_strides, palette))


def count_voxels(dv, grid, *, level=None):
    """The number of solid voxels of a dense grid, counted on the voxelizer's device.  grid and level as
    to_voxels takes them."""
    device, grid_args, _ = _gather_args(dv, grid, level, (0, 0, 0), 0, None, None)
    _sync(device)   # (the caller's writes to grid have landed)
    return dv.gather_count(*grid_args)


def to_voxels(dv, grid, *, level=None, origin=(0, 0, 0), argb=0xFFFFFFFF, colors=None, palette=None, first=0, count=None):
    """The solid voxels of a dense grid as records on the voxelizer's device: an int32 tensor [n, 4] of
    (origin + (x, y, z), argb bits) in ascending (z, y, x) - the order of grid.nonzero(), the layout of dv.read_voxels().

    grid:     as RayCaster and components take it: bool or uint8 (solid where != 0), int32 (the words of fmt="bits": 32 voxels
              per word along x) or float32 with `level` (solid where grid < level).  It is only read.
    argb:     the colour of every record, unless
    colors:   an int32 tensor of the grid's voxel shape [z, y, x] (any strides: fmt="argb" grids), the colour per voxel, or
    palette:  a sequence or tensor of 256 integers, the colour per value of a bool / uint8 grid (labels 1 / 2 -> a surface and a
              fill colour).  colors and palette exclude each other.
    first, count:  records [first, first + count) of the numbering only (count None: to the end), so that a list too large for
              the device can be taken in parts; each call counts again."""
    device, grid_args, color_args = _gather_args(dv, grid, level, origin, argb, colors, palette)
    for name, v in (("first", first), ("count", count)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0):
            raise ValueError(f"{name} must be an integer >= 0, not {v!r}")
    _sync(device)   # (the caller's writes to grid and colors have landed)
    total = dv.gather_count(*grid_args)
    if first > total or (count is not None and count > total - first):
        raise ValueError(f"records [{first}, {first} + {count}) reach past the grid's {total} solid voxels")
    n = total - first if count is None else count
    records = torch.empty((n, 4), dtype=torch.int32, device=device)
    if n:
        dv.gather_write(*grid_args, *color_args, first, n, records.data_ptr())
    return records


def save_voxels(dv, grid, path, *, fmt=None, resolution=None, level=None, origin=(0, 0, 0), argb=0xFFFFFFFF, colors=None, palette=None):
    """The solid voxels of a dense grid written to the voxel file `path`, in the order and with the
    colours of to_voxels, through the writers of obj2voxel_voxelize(); the records cross to the host in batches of 2^20.
    Returns the number of voxels.

    fmt:         "vl32", "ply", "xyzrgb", "qef" or "vox"; None: the path's extension.
    resolution:  the grid resolution the paletted formats record; None: max(origin + extent).
    A path that cannot be opened, a type that is no output format and a writer that fails raise hip.DeviceError with the
    library's message."""
    device, grid_args, color_args = _gather_args(dv, grid, level, origin, argb, colors, palette)
    reach = max(o + n for o, n in zip(color_args[0], grid_args[3]))
    if resolution is None:
        resolution = reach
    if isinstance(resolution, bool) or not isinstance(resolution, numbers.Integral) or not reach <= resolution < 2 ** 32:
        raise ValueError(f"resolution must be an integer from origin + extent = {reach} to 2^32 - 1, not {resolution!r}")
    if fmt is not None and not isinstance(fmt, str):
        raise TypeError(f"fmt must be a string or None, not {fmt!r}")
    _sync(device)   # (the caller's writes to grid and colors have landed)
    return dv.gather_save(*grid_args, *color_args, path, fmt, int(resolution))


def from_voxels(records, shape, *, origin=(0, 0, 0), fmt="occupancy"):
    """The inverse of to_voxels, in plain torch: a [z, y, x] tensor of `shape` on the records' device with the records' voxels
    set - fmt "occupancy": bool, "labels": uint8 1, "argb": int32 argb (0 elsewhere).  records: an integer tensor [n, 4] of
    (x, y, z, argb); a record outside origin + shape raises ValueError.  from_voxels(to_voxels(dv, g), g.shape) == (g != 0)."""
    if fmt not in ("occupancy", "labels", "argb"):
        raise ValueError(f"fmt must be 'occupancy', 'labels' or 'argb', not {fmt!r}")
    if not isinstance(records, torch.Tensor) or records.dim() != 2 or records.shape[1] != 4 or records.dtype not in (torch.int32, torch.int64):
        raise ValueError("records must be an int32 or int64 tensor [n, 4] of (x, y, z, argb)")
    shape, origin = tuple(int(v) for v in shape), tuple(int(v) for v in origin)
    if len(shape) != 3 or any(v < 1 for v in shape) or len(origin) != 3 or any(v < 0 for v in origin):
        raise ValueError("shape must be three positive extents [z, y, x] and origin three voxel coordinates, none negative")
    xyz = records[:, :3].to(torch.int64)
    if records.dtype == torch.int32:
        xyz = xyz & 0xFFFFFFFF   # (the coordinates are uint32 bits)
    xyz = xyz - torch.tensor(origin, dtype=torch.int64, device=records.device)
    extent = torch.tensor((shape[2], shape[1], shape[0]), dtype=torch.int64, device=records.device)
    if bool(((xyz < 0) | (xyz >= extent)).any()):
        raise ValueError(f"records lie outside the box of shape {shape} [z, y, x] at origin {origin}")
    dtype = FORMATS[fmt][1]
    grid = torch.zeros(shape, dtype=dtype, device=records.device)
    values = records[:, 3].to(torch.int32) if fmt == "argb" else torch.ones((), dtype=dtype, device=records.device).expand(xyz.shape[0])
    grid[xyz[:, 2], xyz[:, 1], xyz[:, 0]] = values
    return grid


# ---- dense grids as blocky meshes -----------------------------------------------------------------------

def _faces_args(dv, grid, level, origin, merge, argb, colors, palette):
    """(device, the arguments of dv.faces_count, origin): the grid and colour arguments as to_voxels checks them, the merge
    mode, and the origin within the box whose coordinates are exact float32."""
    if merge not in _FACES_MERGE:
        raise ValueError(f"merge must be 'none', 'runs' or 'rects', not {merge!r}")
    device, grid_args, (origin, mode, argb, colors_ptr, color_strides, palette) = _gather_args(dv, grid, level, origin, argb, colors, palette)
    if any(o + n > MAX_FACES_EXTENT for o, n in zip(origin, grid_args[3])):
        raise ValueError(f"origin {origin} + the grid's extent {grid_args[3]} [x, y, z] is above {MAX_FACES_EXTENT}")
    return device, grid_args + (_FACES_MERGE[merge], mode, argb, colors_ptr, color_strides, palette), origin


def count_faces(dv, grid, *, level=None, merge="none", argb=0xFFFFFFFF, colors=None, palette=None):
    """The number of quads voxel_faces would return, counted on the voxelizer's device.  With
    merge="none" and one colour it is the model's surface area in voxel faces.  Arguments as voxel_faces takes them."""
    device, args, _ = _faces_args(dv, grid, level, (0, 0, 0), merge, argb, colors, palette)
    _sync(device)   # (the caller's writes to grid and colors have landed)
    return dv.faces_count(*args)


def voxel_faces(dv, grid, *, level=None, origin=(0, 0, 0), merge="runs", argb=0xFFFFFFFF, colors=None, palette=None, transform=None):
    """The voxel model of a dense grid as a mesh on the voxelizer's device: one quad per exposed voxel
    face, coloured by its voxel.  Returns (positions float32 [4Q, 3], faces int32 [2Q, 3], quad_argb int32 [Q]), new contiguous
    tensors in the shape set_mesh takes: quad q owns vertices 4q .. 4q + 3 and triangles 2q and 2q + 1, whose normals point out
    of the solid voxel.  Quads come row by row, direction by direction (-x, +x, -y, +y, -z, +z) within a row, then by x.

    grid, level, argb, colors, palette:  as to_voxels takes them.
    origin:     (ox, oy, oz): voxel (x, y, z) is the cube from origin + (x, y, z) to origin + (x, y, z) + 1; origin + extent is
                at most 65 536 per axis, so that every coordinate is an exact float32.
    merge:      "runs": exposed faces of one direction that are neighbours along x (along y for the -x and +x faces) and whose
                voxels have the same colour become one quad; "rects": and runs of neighbouring rows (along y for the -z and
                +z faces, along z for the others) that begin together, are equally long and of one colour become one
                rectangle, so that a flat wall is one quad; "none": a quad per face.
    transform:  None: positions in voxel space.  dv.transform() (the 12 floats, model to voxel space): positions in model
                space, A^-1 p, computed in float64 and rounded once, as extract_surface does."""
    device, args, origin = _faces_args(dv, grid, level, origin, merge, argb, colors, palette)
    if transform is not None:
        transform = torch.as_tensor(transform, dtype=torch.float64).reshape(-1)
        if transform.numel() != 12:
            raise ValueError("transform must hold 12 numbers: a row-major 3 x 3 matrix, then the translation")
    _sync(device)   # (the caller's writes to grid and colors have landed)
    n_quads = dv.faces_count(*args)
    if 4 * n_quads > 2 ** 31 - 1:
        raise ValueError(f"the grid has {n_quads} quads: 4 vertices each are more than 2^31 - 1 int32 indices")
    positions = torch.empty((4 * n_quads, 3), dtype=torch.float32, device=device)
    faces = torch.empty((2 * n_quads, 3), dtype=torch.int32, device=device)
    quad_argb = torch.empty((n_quads,), dtype=torch.int32, device=device)
    if n_quads:
        dv.faces_write(*args, origin, positions.data_ptr(), faces.data_ptr(), quad_argb.data_ptr(), n_quads)
    if transform is not None and n_quads:
        inverse = torch.linalg.inv(transform[:9].reshape(3, 3)).to(device)   # (3 x 3, on the host)
        p = positions.to(torch.float64) - transform[9:].to(device)
        positions = (p[:, None, :] * inverse[None, :, :]).sum(dim=2).to(torch.float32).contiguous()
    return positions, faces, quad_argb


# ---- the nearest seed voxel and its colour ---------------------------------------------------------------

def _nearest_args(dv, seeds, level, surface_only):
    """(device, (seeds_ptr, format, strides, dims, level, flags), voxel shape) of the seed grid of nearest_voxel / spread_colors,
    checked as components checks its grid, and against the distance limit."""
    device, fmt, level, dims = _set_grid(dv, seeds, level, _limit_voxels)
    if sum((n - 1) ** 2 for n in dims) > MAX_NEAREST_D2:
        raise ValueError(f"the grid's extent {dims} [x, y, z] has (nx-1)^2 + (ny-1)^2 + (nz-1)^2 above {MAX_NEAREST_D2}")
    if surface_only and fmt != hip.GRID_U8:
        raise ValueError(f"surface_only needs a bool or uint8 grid (a seed is a voxel of value 1), not {seeds.dtype}")
    flags = hip.NEAREST_SEED_ONE if surface_only else 0
    return device, (seeds.data_ptr(), fmt, _strides(seeds), dims, 0.0 if level is None else level, flags), (dims[2], dims[1], dims[0])


def _outside_storage(t, name, seeds):
    if t.untyped_storage().data_ptr() == seeds.untyped_storage().data_ptr():
        raise ValueError(f"{name} must not share the seeds' storage")


def nearest_voxel(dv, seeds, *, level=None, surface_only=False, dist2=None, out=None):
    """For every voxel of a dense grid the seed voxel closest to it: an int32 tensor [z, y, x] of the
    seed's linear index (sz * ny + sy) * nx + sx - among several seeds at the same distance the smallest index, the seed itself
    on a seed, -1 everywhere when there is no seed.  nearest_coords turns it into coordinates; colors.view(-1)[nearest] is not
    needed for colours: spread_colors does that on the device.  Returns nearest, or (nearest, dist2) when dist2 is given.

    seeds:         as components takes its grid: bool or uint8 (a seed where != 0), int32 (the words of fmt="bits": 32 voxels
                   per word along x) or float32 with `level` (a seed where seeds < level).  It is only read.
    surface_only:  True: a seed is a voxel of value 1 of a bool / uint8 grid - the surface of fmt="labels", whose interior is 2.
    dist2:         None; True for a new int32 tensor; or an int32 tensor of the voxel shape (any strides): the squared distance
                   to that seed, 0x7FFFFFFF without seeds - what distance_transform(..., "dist2") gives for the same seeds.
    out:           an int32 tensor of the voxel shape (any strides, not in the seeds' storage), written as it is; else a new
                   contiguous tensor."""
    device, args, shape = _nearest_args(dv, seeds, level, surface_only)
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=device)
    else:
        _check_grid(out, "out", torch.int32, device, shape)
        _outside_storage(out, "out", seeds)
    want_dist2 = dist2 is not None and dist2 is not False
    if dist2 is True:
        dist2 = torch.empty(shape, dtype=torch.int32, device=device)
    elif want_dist2:
        _check_grid(dist2, "dist2", torch.int32, device, shape)
        _outside_storage(dist2, "dist2", seeds)
        if dist2.untyped_storage().data_ptr() == out.untyped_storage().data_ptr():
            raise ValueError("dist2 must not share out's storage")
    else:
        dist2 = None
    _sync(device)   # (the caller's writes to seeds, out and dist2 have landed)
    dv.nearest_dense(*args, out.data_ptr(), _strides(out), _ptr(dist2), None if dist2 is None else _strides(dist2))
    return (out, dist2) if want_dist2 else out


def spread_colors(dv, seeds, colors, *, level=None, surface_only=False, inside_only=False, max_distance=None, out=None):
    """The seeds' colours carried to the voxels they are nearest to: every voxel that is not a seed takes
    colors at its nearest seed (nearest_voxel's: the smallest index on a tie); seeds keep theirs, and without seeds nothing
    changes.  Returns the painted tensor.

        labels, origin = dense.voxelize_dense(dv, 256, fmt="labels", fill=True)
        argb, _ = dense.voxelize_dense(dv, 256, fmt="argb", fill=True)
        dense.spread_colors(dv, labels, argb, surface_only=True, inside_only=True, out=argb)   # the interior takes the surface's colours

    seeds, level, surface_only:  as nearest_voxel takes them.
    colors:        an int32 tensor of the voxel shape [z, y, x] (any strides: an fmt="argb" grid); any 32 bits per voxel.
    inside_only:   True (with surface_only=True): only the voxels whose seeds element is non-zero are painted - the interior (2)
                   of a label grid; the exterior keeps its bits.
    max_distance:  a number >= 0, in voxels: only voxels at most that far from their seed are painted (d2 <= floor(r * r), exact:
                   d2 is an integer) - a coloured shell of that thickness.  None: no limit.
    out:           None: a painted contiguous copy, colors untouched; colors itself: painted in place; another int32 tensor of
                   that shape (any strides, not in the seeds' storage): filled with colors, then painted."""
    device, args, shape = _nearest_args(dv, seeds, level, surface_only)
    if inside_only and not surface_only:
        raise ValueError("inside_only needs surface_only=True: the seeds are the voxels of value 1, the inside the other non-zero ones")
    max_dist2 = hip.NEAREST_NO_LIMIT
    if max_distance is not None:
        if isinstance(max_distance, bool) or not isinstance(max_distance, numbers.Real) or not float(max_distance) >= 0.0:
            raise ValueError(f"max_distance must be a number >= 0 or None, not {max_distance!r}")
        if float(max_distance) * float(max_distance) < hip.NEAREST_NO_LIMIT:
            max_dist2 = math.floor(max_distance * max_distance)
    _check_grid(colors, "colors", torch.int32, device, shape)
    same = out is colors or (isinstance(out, torch.Tensor) and out.dtype == colors.dtype and out.data_ptr() == colors.data_ptr()
                             and out.shape == colors.shape and out.stride() == colors.stride())
    if out is None:
        target = colors.clone(memory_format=torch.contiguous_format)
    elif same:
        target = colors
    else:
        _check_grid(out, "out", torch.int32, device, shape)
        target = out
    _outside_storage(target, "colors" if same else "out", seeds)
    if out is not None and not same:
        target.copy_(colors)
    nearest = torch.empty(shape, dtype=torch.int32, device=device)
    flags = args[5] | (hip.NEAREST_VALUES_INSIDE if inside_only else 0)
    _sync(device)   # (the caller's writes to seeds and colors and the copy above have landed)
    dv.nearest_dense(*args[:5], flags, nearest.data_ptr(), _strides(nearest), None, None, target.data_ptr(), _strides(target), max_dist2)
    return target


def nearest_coords(nearest):
    """int32 [z, y, x, 3]: the (x, y, z) of nearest_voxel's linear indices, (-1, -1, -1) where nearest < 0.  Plain torch."""
    if not isinstance(nearest, torch.Tensor) or nearest.dim() != 3:
        raise ValueError("nearest must be a 3-D tensor [z, y, x]")
    if nearest.dtype != torch.int32:
        raise TypeError(f"nearest must be torch.int32, not {nearest.dtype}")
    _, ny, nx = nearest.shape
    i = nearest.clamp(min=0)
    row = torch.div(i, nx, rounding_mode="floor")
    xyz = torch.stack((i - row * nx, row % ny, torch.div(row, ny, rounding_mode="floor")), dim=-1).to(torch.int32)
    xyz[nearest < 0] = -1
    return xyz


# ---- downsampling: coverage, LODs, mean colours ---------------------------------------------------------

def _limit_dim(dims):
    """The size limit of downsample: no linear index, only the extent per axis."""
    if max(dims) > MAX_CC_DIM:
        raise ValueError(f"the grid's extent {dims} [x, y, z] is above {MAX_CC_DIM} along an axis")


def _down_factor(factor):
    if isinstance(factor, bool) or not isinstance(factor, numbers.Integral) or not MIN_DOWN_FACTOR <= factor <= MAX_DOWN_FACTOR:
        raise ValueError(f"factor must be an integer {MIN_DOWN_FACTOR} ... {MAX_DOWN_FACTOR}, not {factor!r}")
    return int(factor)


def downsample_box(origin, shape, factor):
    """(coarse origin (x, y, z), coarse shape (nz, ny, nx)) of the box of `shape` (nz, ny, nx) fine voxels whose voxel (0, 0, 0)
    is `origin` (x, y, z) of the fine lattice, merged in blocks of factor^3 aligned to that lattice: per axis
    floor(origin / factor) and ceil((origin + n) / factor) - floor(origin / factor).  Needs no device."""
    factor = _down_factor(factor)
    origin = _origin(origin)
    shape = tuple(int(n) for n in shape)
    if len(shape) != 3 or any(n < 1 for n in shape):
        raise ValueError(f"shape {shape} must be three positive extents (nz, ny, nx)")
    dims = shape[::-1]
    if any(o + n > 2 ** 32 for o, n in zip(origin, dims)):
        raise ValueError(f"origin {origin} + the extent {dims} [x, y, z] is above 2^32")
    corigin = tuple(o // factor for o in origin)
    cdims = tuple(-(-(o + n) // factor) - c for o, n, c in zip(origin, dims, corigin))
    return corigin, cdims[::-1]


def downsample(dv, grid, factor, *, level=None, origin=(0, 0, 0), reduce="any", count=False, values=None, colors=None, out=None,
               out_count=None, out_values=None, out_colors=None):
    """A dense grid merged into a coarser one on the voxelizer's device: blocks of factor^3 fine voxels,
    aligned to the global lattice (the block of coarse voxel X covers the fine coordinates [X factor, (X + 1) factor) per axis;
    what lies outside the grid's box is empty), become one coarse voxel each.  Returns (solid[, count][, values][, argb],
    coarse_origin) in that order: solid bool, count int16, values uint8, argb int32, all indexed [z, y, x] over the box of
    downsample_box(origin, grid's voxel shape, factor), and that box's origin (x, y, z).

        fine, o = dense.voxelize_dense(dv, 2 * R)
        half, o2 = dense.downsample(dv, fine, 2, origin=o)            # what voxelize_dense(dv, R, supersampling=2) gives
        solid, n, o4 = dense.downsample(dv, fine, 4, origin=o, count=True)
        coverage = n.float() / 4 ** 3                                  # the soft occupancy: count.float() / factor ** 3

    grid:     as components takes it: bool or uint8 (solid where != 0), int32 (the words of fmt="bits": 32 voxels per word along
              x) or float32 with `level` (solid where grid < level).  Any 3-D view; it is only read.
    factor:   2 ... 8.
    origin:   the fine-lattice coordinates (x, y, z) of grid[0, 0, 0]: voxelize_dense's origin.
    reduce:   "any": a coarse voxel is solid if a fine voxel of its block is; "all": if all factor^3 are; "majority": if at
              least ceil(factor^3 / 2) are; or that threshold itself, an integer 1 ... factor^3.
    count:    True: also the number of solid fine voxels per block.
    values:   "min" / "max" (bool / uint8 grids): also, where solid, the smallest / largest non-zero byte of the block, else 0.
              With the labels of fill=True (1 surface, 2 interior) "min" gives "surface if any sub-voxel is surface".
    colors:   an int32 tensor of the grid's voxel shape (any strides: an fmt="argb" grid): also, where solid, the mean per 8-bit
              channel over the block's solid fine voxels, rounded half up, else 0.  Colours of voxels that are not solid are not used.
    out, out_count, out_values, out_colors:  tensors of the coarse shape to write (bool or uint8, int16, uint8, int32; any
              strides, as they are); else new contiguous ones.  out_count, out_values and out_colors ask for their output too.

    Halving repeatedly - downsample(downsample(g, 2), 2) - gives "any of any" occupancy, which for reduce="any" is the occupancy
    of one step by 4; with another threshold it is not, and its colours are a mean of means, not the mean: each level weighs its
    solid children equally, however many fine voxels they stood for.  Take every level of a chain from the finest grid instead."""
    factor = _down_factor(factor)
    device, fmt, level, dims = _set_grid(dv, grid, level, _limit_dim)
    cube = factor ** 3
    if isinstance(reduce, str):
        if reduce not in ("any", "majority", "all"):
            raise ValueError(f"reduce must be 'any', 'majority', 'all' or an integer 1 ... {cube}, not {reduce!r}")
        min_count = {"any": 1, "majority": (cube + 1) // 2, "all": cube}[reduce]
    elif isinstance(reduce, bool) or not isinstance(reduce, numbers.Integral) or not 1 <= reduce <= cube:
        raise ValueError(f"reduce must be 'any', 'majority', 'all' or an integer 1 ... {cube}, not {reduce!r}")
    else:
        min_count = int(reduce)
    corigin, cshape = downsample_box(origin, (dims[2], dims[1], dims[0]), factor)
    origin = _origin(origin)
    if values is None and out_values is not None:
        raise ValueError("out_values needs values='min' or 'max'")
    if values is not None:
        if values not in _DOWN_VALUES:
            raise ValueError(f"values must be None, 'min' or 'max', not {values!r}")
        if fmt != hip.GRID_U8:
            raise ValueError(f"values needs a bool or uint8 grid, not {grid.dtype}")
    if colors is None and out_colors is not None:
        raise ValueError("out_colors needs colors")
    if colors is not None:
        _check_grid(colors, "colors", torch.int32, device, (dims[2], dims[1], dims[0]))
    if not isinstance(count, bool):
        raise ValueError(f"count must be True or False, not {count!r}")

    def output(t, name, *dtypes):
        """The caller's tensor for an output, checked (its dtype one of dtypes), or a new contiguous one of the first dtype."""
        if t is None:
            return torch.empty(cshape, dtype=dtypes[0], device=device)
        _check_grid(t, name, t.dtype if isinstance(t, torch.Tensor) and t.dtype in dtypes else dtypes[0], device, cshape)
        return t

    solid = output(out, "out", torch.bool, torch.uint8)
    n = output(out_count, "out_count", torch.int16) if count or out_count is not None else None
    val = output(out_values, "out_values", torch.uint8) if values is not None else None
    argb = output(out_colors, "out_colors", torch.int32) if colors is not None else None
    _sync(device)   # (the caller's writes to grid, colors and the outputs have landed)
    dv.downsample(grid.data_ptr(), fmt, _strides(grid), dims, 0.0 if level is None else level, origin, factor, min_count,
                  _DOWN_VALUES.get(values, hip.DOWN_VALUE_MIN), _ptr(colors), None if colors is None else _strides(colors),
                  _ptr(n), None if n is None else _strides(n), solid.data_ptr(), _strides(solid),
                  _ptr(val), None if val is None else _strides(val), _ptr(argb), None if argb is None else _strides(argb))
    return tuple(t for t in (solid, n, val, argb) if t is not None) + (corigin,)


# ---- per-label statistics -------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class LabelStats:
    """What label_stats returns: row L of every tensor is for the value L of the grid, row 0 like every other; all int64, on the
    grid's device, exact.  A field that was not asked for is None."""
    count: torch.Tensor      # [n + 1]: the voxels that hold L
    lo: torch.Tensor         # [n + 1, 3]: the smallest (x, y, z), global coordinates; 0 for a row without voxels
    hi: torch.Tensor         # [n + 1, 3]: the largest (x, y, z) + 1 - exclusive -; 0 for a row without voxels
    sum: torch.Tensor        # [n + 1, 3]: the sums of x, y, z (integer voxel coordinates, without the centre's + 0.5)
    moment: torch.Tensor     # [n + 1, 6]: the sums of xx, yy, zz, xy, xz, yz
    faces: torch.Tensor      # [n + 1]: the voxel faces of L whose neighbour holds another value or lies outside the box
    outside: int             # the voxels whose value is negative or above n: they are in no row
    origin: tuple            # (x, y, z) of grid[0, 0, 0]

    @property
    def n(self):
        return self.count.shape[0] - 1


def label_stats(dv, labels, n=None, *, origin=(0, 0, 0), box=True, sums=True, moments=False, faces=False):
    """Per value of a label grid, in one read of it on the voxelizer's device: a LabelStats with the
    count, the bounding box (box), the coordinate sums (sums), the sums of the coordinates' products (moments) and the exposed
    faces (faces) of every value 0 ... n.  Everything is an integer and exact; one run equals another bit for bit.

        labels, n = dense.components(dv, grid)
        st = dense.label_stats(dv, labels, n, moments=True)
        dense.centroids(st)[1:]                      # float64 [n, 3], voxel centres
        part, o = dense.crop(grid, st, 3)            # the view of grid that holds component 3, and its origin

    labels:  int32 (what components returns), uint8 (the labels of fill=True, of solidify, of flood) or bool (occupancy: row 1
             is the solid, row 0 the empty space); any 3-D view [z, y, x]; it is only read.
    n:       the highest value that is counted; None: 255 for uint8, 1 for bool, max(labels.max(), 0) for int32 (a device
             reduction and a wait).  A voxel whose value is negative or above n is counted in `outside` and nowhere else.
    origin:  (x, y, z) of labels[0, 0, 0]; the box and the sums are in these global coordinates.  origin + extent may not be
             above 65 536 on any axis, nor the grid hold more than 2^31 - 1 voxels: then no sum can reach 2^63."""
    _require_shared_runtime()
    device = _device(dv)
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3:
        raise ValueError("labels must be a 3-D tensor [z, y, x]")
    if labels.dtype not in (torch.int32, torch.uint8, torch.bool):
        raise TypeError(f"labels must be int32, uint8 or bool, not {labels.dtype}")
    _check_grid(labels, "labels", labels.dtype, device)
    if 0 in labels.shape:
        raise ValueError("labels has an empty dimension")
    for name, flag in (("box", box), ("sums", sums), ("moments", moments), ("faces", faces)):
        if not isinstance(flag, bool):
            raise ValueError(f"{name} must be True or False, not {flag!r}")
    origin = _origin(origin)
    nz, ny, nx = labels.shape
    dims = (nx, ny, nz)
    _limit_voxels(dims)
    if any(o + d > MAX_STATS_EXTENT for o, d in zip(origin, dims)):
        raise ValueError(f"origin {origin} + the grid's extent {dims} [x, y, z] is above {MAX_STATS_EXTENT}")
    top = MAX_STATS_LABELS if labels.dtype == torch.int32 else 1 if labels.dtype == torch.bool else 255
    if n is None:
        n = max(int(labels.max()), 0) if labels.dtype == torch.int32 else top
    elif isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 0 <= n <= top:
        raise ValueError(f"n must be an integer 0 ... {top} for {labels.dtype} labels, not {n!r}")
    n = int(n)
    which = (hip.STATS_BOX if box else 0) | (hip.STATS_SUMS if sums else 0) | (hip.STATS_MOMENTS if moments else 0) | (hip.STATS_FACES if faces else 0)
    table = torch.empty((n + 1, hip.STATS_COLUMNS), dtype=torch.int64, device=device)
    _sync(device)   # (the caller's writes to labels have landed)
    outside = dv.label_stats(labels.data_ptr(), hip.LABELS_I32 if labels.dtype == torch.int32 else hip.LABELS_U8, _strides(labels), dims, origin,
                             n, which, table.data_ptr())
    count = table[:, 0]
    lo = hi = None
    if box:
        some = (count > 0)[:, None]
        lo, hi = torch.where(some, table[:, 1:4], 0), torch.where(some, table[:, 4:7] + 1, 0)
    return LabelStats(count=count, lo=lo, hi=hi, sum=table[:, 7:10] if sums else None, moment=table[:, 10:16] if moments else None,
                      faces=table[:, 16] if faces else None, outside=outside, origin=origin)


def component_stats(dv, grid, *, level=None, connectivity=6, background=False, **which):
    """(labels, n, stats): components(dv, grid, ...) and label_stats of its labels; `which` are label_stats' origin, box, sums,
    moments and faces.  Row 0 of stats is what is not in the set."""
    labels, n = components(dv, grid, level=level, connectivity=connectivity, background=background)
    return labels, n, label_stats(dv, labels, n, **which)


def _need(stats, *fields):
    if not isinstance(stats, LabelStats):
        raise TypeError("stats must be a LabelStats, what label_stats returns")
    for f in fields:
        if getattr(stats, f) is None:
            raise ValueError(f"the statistics were made without {f}: ask label_stats for " + {"lo": "box", "hi": "box", "sum": "sums", "moment": "moments"}[f])


def centroids(stats):
    """float64 [n + 1, 3]: the mean voxel centre (x, y, z) of every row, sum / count + 0.5; NaN for a row without voxels."""
    _need(stats, "sum")
    count = stats.count.to(torch.float64)[:, None]
    return torch.where(count > 0, stats.sum.to(torch.float64) / count + 0.5, float("nan"))


def _second_moments(moment):
    """[..., 6] sums of xx, yy, zz, xy, xz, yz as symmetric matrices [..., 3, 3]."""
    m = moment
    return torch.stack([m[..., 0], m[..., 3], m[..., 4], m[..., 3], m[..., 1], m[..., 5], m[..., 4], m[..., 5], m[..., 2]], dim=-1).reshape(m.shape[:-1] + (3, 3))


def covariances(stats):
    """float64 [n + 1, 3, 3]: the covariance of the positions of every row's solid about its centroid, the row taken as a union of
    unit cubes: E[p p^T] - E[p] E[p]^T over the voxel coordinates, plus the cube's own 1/12 on the diagonal.  NaN for a row
    without voxels."""
    _need(stats, "sum", "moment")
    count = stats.count.to(torch.float64)
    mean = stats.sum.to(torch.float64) / count[:, None]
    cov = _second_moments(stats.moment.to(torch.float64)) / count[:, None, None] - mean[:, :, None] * mean[:, None, :]
    cov = cov + torch.eye(3, dtype=torch.float64, device=cov.device) / 12.0
    return torch.where((count > 0)[:, None, None], cov, float("nan"))


def mass_properties(stats, rows, *, transform=None, supersampling=1):
    """(volume, centre of mass float64 [3], inertia tensor float64 [3, 3] about that centre) of the union of the rows `rows` at
    unit density - rows=(1, 2) for the labels of a filled model, surface and interior.  The body is the union of the rows' unit
    cubes, so each voxel brings its own 1/12 per axis.

    transform:  None: voxel units.  dv.transform() (12 floats, model to sample space) with the run's supersampling: model space,
                p -> A^-1 (supersampling * p - t) as extract_surface maps its vertices, in float64; the volume scales by the
                |det| of that map and the inertia tensor with it."""
    _need(stats, "sum", "moment")
    rows = [int(r) for r in rows]
    if not rows or any(not 0 <= r <= stats.n for r in rows) or len(set(rows)) != len(rows):
        raise ValueError(f"rows {rows} must be distinct rows 0 ... {stats.n}, at least one")
    if supersampling not in (1, 2):
        raise ValueError("supersampling must be 1 or 2")
    idx = torch.tensor(rows, dtype=torch.int64, device=stats.count.device)
    count = int(stats.count[idx].sum())
    s1 = stats.sum[idx].sum(dim=0).cpu().to(torch.float64)            # (exact integers up to here)
    s2 = _second_moments(stats.moment[idx].sum(dim=0)).cpu().to(torch.float64)
    if count == 0:
        nan = float("nan")
        return 0.0, torch.full((3,), nan, dtype=torch.float64), torch.full((3, 3), nan, dtype=torch.float64)
    v = float(count)
    centre = s1 / v + 0.5
    # the second moments of the cubes about the origin: sum (c c^T) over the centres c = p + 0.5, and V / 12 on the diagonal
    half = 0.5 * (s1[:, None] + s1[None, :]) + 0.25 * v
    about_origin = s2 + half + torch.eye(3, dtype=torch.float64) * (v / 12.0)
    central = about_origin - v * centre[:, None] * centre[None, :]
    volume = v
    if transform is not None:
        transform = torch.as_tensor(transform, dtype=torch.float64).reshape(-1)
        if transform.numel() != 12:
            raise ValueError("transform must hold 12 numbers: a row-major 3 x 3 matrix, then the translation")
        inverse = torch.linalg.inv(transform[:9].reshape(3, 3))
        b = inverse * float(supersampling)                              # the linear part of voxel -> model
        det = abs(float(torch.linalg.det(b)))
        centre = inverse @ (centre * supersampling - transform[9:])
        central = det * (b @ central @ b.T)
        volume = v * det
    inertia = torch.eye(3, dtype=torch.float64) * torch.trace(central) - central
    return volume, centre, inertia


def keep_largest(dv, grid, k=1, *, level=None, connectivity=26):
    """bool [z, y, x]: the solid voxels of the k largest components of the grid; of components of one size the one with the
    smaller label - the first in [z, y, x] order - comes first.  The empty space (row 0) is never a candidate; with fewer than k
    components all are kept."""
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 1:
        raise ValueError(f"k must be an integer >= 1, not {k!r}")
    labels, n = components(dv, grid, level=level, connectivity=connectivity)
    stats = label_stats(dv, labels, n, box=False, sums=False)
    order = torch.sort(stats.count[1:], descending=True, stable=True).indices[:k] + 1   # (stable: ties stay in label order)
    keep = torch.zeros(n + 1, dtype=torch.bool, device=labels.device)
    keep[order] = True
    return keep[labels.to(torch.int64)]


def crop(grid, stats, label):
    """(view, origin): the part of `grid` - any tensor [z, y, x] of the shape the statistics were made of - inside the bounding
    box of `label`, as a view, and the global (x, y, z) of its voxel (0, 0, 0).  An empty view at the grid's origin for a row
    without voxels."""
    _need(stats, "lo", "hi")
    if isinstance(label, bool) or not isinstance(label, numbers.Integral) or not 0 <= label <= stats.n:
        raise ValueError(f"label must be a row 0 ... {stats.n}, not {label!r}")
    if not isinstance(grid, torch.Tensor) or grid.dim() != 3:
        raise ValueError("grid must be a 3-D tensor [z, y, x]")
    lo, hi = stats.lo[label].tolist(), stats.hi[label].tolist()
    if lo == hi:
        return grid[:0, :0, :0], stats.origin
    ox, oy, oz = stats.origin
    if hi[0] - ox > grid.shape[2] or hi[1] - oy > grid.shape[1] or hi[2] - oz > grid.shape[0]:
        raise ValueError(f"grid's shape {tuple(grid.shape)} does not hold the box of label {label}")
    return grid[lo[2] - oz:hi[2] - oz, lo[1] - oy:hi[1] - oy, lo[0] - ox:hi[0] - ox], tuple(lo)


# ---- mesh files ------------------------------------------------------------------------------------------------------------------

_MESH_BATCH = 1 << 20   # triangles (vertices) per write


def _host_array(t, name, kinds, width):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if a.ndim != 2 or a.shape[1] != width or a.dtype.kind not in kinds:
        raise ValueError(f"{name} must be [n, {width}] of kind {kinds!r}, not {a.dtype} {a.shape}")
    return a


def _triangle_argb(argb, n_vertices, n_triangles):
    """(per-triangle uint32 or None, per-vertex uint32 or None) of save_mesh's argb: one per triangle, per quad (two triangles
    each, in order) or per vertex, looked for in that order."""
    if argb is None:
        return None, None
    a = argb.detach().cpu().numpy() if isinstance(argb, torch.Tensor) else np.asarray(argb)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError("argb must be a 1-D integer array")
    a = (a.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    if len(a) == n_triangles:
        return a, None
    if 2 * len(a) == n_triangles:
        return np.repeat(a, 2), None
    if len(a) == n_vertices:
        return None, a
    raise ValueError(f"argb has {len(a)} entries: neither one per triangle ({n_triangles}), per quad nor per vertex ({n_vertices})")


def _save_stl(path, p, f):
    rec = np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")])
    with open(path, "wb") as out:
        out.write(b"obj2voxel_amd dense.save_mesh".ljust(80, b" ") + np.uint32(len(f)).astype("<u4").tobytes())
        for i in range(0, len(f), _MESH_BATCH):
            v = p[f[i:i + _MESH_BATCH]]                                   # [n, 3, 3] float32
            n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).astype(np.float32)
            length = np.sqrt((n * n).sum(axis=1, dtype=np.float32), dtype=np.float32)
            n = np.where(length[:, None] > 0, n / np.where(length > 0, length, 1)[:, None], 0).astype(np.float32)
            block = np.zeros(len(v), rec)
            block["n"], block["v"] = n, v
            out.write(block.tobytes())


def _rgba(argb):
    return np.stack([argb >> 16 & 255, argb >> 8 & 255, argb & 255, argb >> 24], axis=1).astype(np.uint8)


def _save_ply(path, p, f, tri_argb, vert_argb):
    if tri_argb is not None:
        # a colour per vertex: the colour of its triangles, or - where triangles of two colours share a vertex - corners of their own
        vert_argb = np.zeros(len(p), np.uint32)
        vert_argb[f.reshape(-1)] = np.repeat(tri_argb, 3)
        if not np.array_equal(vert_argb[f], np.repeat(tri_argb, 3).reshape(-1, 3)):
            p, vert_argb = p[f.reshape(-1)], np.repeat(tri_argb, 3)
            f = np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)
    colored = vert_argb is not None
    vt = np.dtype([("p", "<f4", 3)] + ([("c", "u1", 4)] if colored else []))
    ft = np.dtype([("n", "u1"), ("i", "<i4", 3)])
    header = ["ply", "format binary_little_endian 1.0", "comment obj2voxel_amd dense.save_mesh", f"element vertex {len(p)}",
              "property float x", "property float y", "property float z"]
    if colored:
        header += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode())
        for i in range(0, len(p), _MESH_BATCH):
            block = np.zeros(len(p[i:i + _MESH_BATCH]), vt)
            block["p"] = p[i:i + _MESH_BATCH]
            if colored:
                block["c"] = _rgba(vert_argb[i:i + _MESH_BATCH])
            out.write(block.tobytes())
        for i in range(0, len(f), _MESH_BATCH):
            block = np.zeros(len(f[i:i + _MESH_BATCH]), ft)
            block["n"], block["i"] = 3, f[i:i + _MESH_BATCH]
            out.write(block.tobytes())


def _save_obj(path, p, f, tri_argb):
    mtl = os.path.splitext(path)[0] + ".mtl"
    with open(path, "w") as out:
        out.write("# obj2voxel_amd dense.save_mesh\n")
        if tri_argb is not None:
            out.write(f"mtllib {os.path.basename(mtl)}\n")
        for i in range(0, len(p), _MESH_BATCH):
            out.write("".join("v %.9g %.9g %.9g\n" % tuple(v) for v in p[i:i + _MESH_BATCH].tolist()))
        if tri_argb is None:
            order, groups = np.arange(len(f)), [(None, 0, len(f))]
        else:
            # the colours in order of first appearance; the triangles of a colour together, in their own order
            colors, first, inverse = np.unique(tri_argb, return_index=True, return_inverse=True)
            rank = np.empty(len(colors), np.int64)
            rank[np.argsort(first, kind="stable")] = np.arange(len(colors))
            order = np.argsort(rank[inverse], kind="stable")
            bounds = np.concatenate([[0], np.cumsum(np.bincount(rank[inverse], minlength=len(colors)))])
            by_rank = colors[np.argsort(first, kind="stable")]
            groups = [(int(c), int(bounds[k]), int(bounds[k + 1])) for k, c in enumerate(by_rank)]
        one_based = f[order] + 1
        for c, lo, hi in groups:
            if c is not None:
                out.write("usemtl c_%08X\n" % c)
            for i in range(lo, hi, _MESH_BATCH):
                out.write("".join("f %d %d %d\n" % tuple(t) for t in one_based[i:min(hi, i + _MESH_BATCH)].tolist()))
    if tri_argb is not None:
        with open(mtl, "w") as out:
            out.write("# obj2voxel_amd dense.save_mesh\n")
            for c, _, _ in groups:
                out.write("newmtl c_%08X\nKd %.9g %.9g %.9g\nd %.9g\n" % (c, (c >> 16 & 255) / 255, (c >> 8 & 255) / 255, (c & 255) / 255, (c >> 24) / 255))


def save_mesh(path, positions, faces, *, argb=None, fmt=None):
    """An indexed triangle mesh - what voxel_faces and extract_surface return - written to a mesh file,
    on the host, in batches.

    positions:  float32 [V, 3]; faces: integer [T, 3], indices into positions (tensors on any device, or arrays).
    argb:       None, or an integer array of one colour (argb bits) per triangle, per quad (two triangles each: voxel_faces'
                quad_argb) or per vertex - told apart by its length, in that order.
    fmt:        "stl", "ply" or "obj"; None: the path's extension.  Anything else raises ValueError.
      .stl  binary; the normal of a triangle is its normalised float32 cross product (v1 - v0) x (v2 - v0), zero where that
            is zero; colours are not stored.
      .ply  binary_little_endian 1.0: vertices float x y z, plus uchar red green blue alpha when colours are given (triangles of
            two colours that share a vertex get corners of their own); faces list uchar int vertex_indices.
      .obj  with a .mtl of the same name beside it when colours are given: one newmtl c_AARRGGBB with Kd (and d, the alpha) per
            distinct colour, the triangles grouped by usemtl in order of the colours' first appearance - the form the library's
            own OBJ reader takes.  Colours per triangle or quad only."""
    path = os.fspath(path)
    if fmt is not None and not isinstance(fmt, str):
        raise TypeError(f"fmt must be a string or None, not {fmt!r}")
    kind = (os.path.splitext(path)[1][1:] if fmt is None else fmt).lower()
    if kind not in ("stl", "ply", "obj"):
        raise ValueError(f"{kind!r} is not a mesh file type: stl, ply or obj")
    p = np.ascontiguousarray(_host_array(positions, "positions", "f", 3), dtype=np.float32)
    f = _host_array(faces, "faces", "iu", 3).astype(np.int64)
    if len(f) and (f.min() < 0 or f.max() >= len(p)):
        raise ValueError(f"faces index outside the {len(p)} positions")
    tri_argb, vert_argb = _triangle_argb(argb, len(p), len(f))
    if kind == "stl":
        _save_stl(path, p, f)
    elif kind == "ply":
        _save_ply(path, p, f, tri_argb, vert_argb)
    else:
        if vert_argb is not None:
            raise ValueError("an .obj file takes colours per triangle or quad (materials); per-vertex colours need .ply")
        _save_obj(path, p, f, tri_argb)
