"""ctypes binding of the device C-ABI (include/o2v_hip.h): one DeviceVoxelizer per GPU / z-slab."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import lib

TRI_MATERIALLESS, TRI_UNTEXTURED, TRI_TEXTURED = 1, 2, 3
STRATEGY_MAX, STRATEGY_BLEND = 0, 1


class _Params(C.Structure):
    _fields_ = [("resolution", C.c_uint32), ("supersampling", C.c_uint32), ("strategy", C.c_uint32),
                ("unit_transform", C.c_int32 * 9), ("bounds_known", C.c_uint32), ("bounds", C.c_float * 6),
                ("z_begin", C.c_uint32), ("z_end", C.c_uint32), ("flags", C.c_uint32),
                ("x_begin", C.c_uint32), ("x_end", C.c_uint32), ("y_begin", C.c_uint32), ("y_end", C.c_uint32),
                ("fill_argb", C.c_uint32)]


FLAG_KERNEL_TIMES = 2  # ... every launch bracketed by events: DeviceVoxelizer.kernel_times()
FLAG_STAGE_TIMES = 4   # ... an event between the stages of a pass: the stage times and total_ms of DeviceVoxelizer.timings()
FLAG_EXACT_CLIP = 1  # o2v_hip_params::flags: the clip kernel without its work-removal shortcuts (include/o2v_hip.h)
FLAG_FILL_INTERIOR = 8  # ... solid voxelization: the interior voxels (colour fill_argb) behind the surface records
DENSE_U8, DENSE_ARGB32, DENSE_BITS = 0, 1, 2  # o2v_hip_write_dense formats
DIST_SQ_I32, DIST_SDF_F32 = 0, 1  # o2v_hip_distance_dense formats
RAY_GRID_U8, RAY_GRID_BITS, RAY_GRID_F32_BELOW = 0, 1, 2  # o2v_hip_raycast_build formats
GRID_U8, GRID_BITS, GRID_F32_BELOW = 0, 1, 2  # the same formats, as o2v_hip_components_dense / o2v_hip_flood_dense name them
CC_INVERT, CC_SEED_BORDER = 16, 32  # ... their flags (with FLAG_STAGE_TIMES: the counters)
CC_SCRATCH_LABELS, CC_SCRATCH_LABELS_STRIDED, CC_SCRATCH_FLOOD = 0, 1, 2  # o2v_hip_components_scratch_bytes
MESH_DIST_UNSIGNED_F32, MESH_DIST_SIGNED_F32 = 0, 1  # o2v_hip_mesh_distance_dense formats
GATHER_COLOR_CONSTANT, GATHER_COLOR_GRID, GATHER_COLOR_PALETTE = 0, 1, 2  # o2v_hip_gather_write / _save colour modes
FACES_MERGE_NONE, FACES_MERGE_RUNS, FACES_MERGE_RECTS = 0, 1, 3  # o2v_hip_faces_count / _write merge modes
NEAREST_SEED_ONE, NEAREST_VALUES_INSIDE = 1, 2  # o2v_hip_nearest_dense flags
NEAREST_NO_LIMIT = 0x7FFFFFFF  # ... its max_dist2 without a limit
DOWN_VALUE_MIN, DOWN_VALUE_MAX = 0, 1  # o2v_hip_downsample value modes
AXIS_X, AXIS_Y, AXIS_Z = 1, 2, 4  # o2v_hip_crossings_dense: the bits of `axes`
LABELS_I32, LABELS_U8 = 0, 1  # o2v_hip_label_stats formats
GEO_MAX_WEIGHT, GEO_MAX_DISTANCE = 65535, 2 ** 31 - 2  # o2v_hip_geodesic_dense: the largest weight, the largest (and default) max_distance
GEO_SCRATCH_CONTIGUOUS, GEO_SCRATCH_STRIDED = 0, 1  # o2v_hip_geodesic_scratch_bytes
GROW_MAX_TICKS = 2 ** 31 - 2  # o2v_hip_grow_dense: where the ticks saturate
GROW_SCRATCH_LABELS, GROW_SCRATCH_LEVEL, GROW_SCRATCH_TICKS = 1, 2, 4  # o2v_hip_grow_scratch_bytes: which of the three live in scratch
THICK_BACKGROUND, THICK_BORDER, THICK_F32, THICK_OPEN_ONLY = 16, 32, 64, 128  # o2v_hip_thickness_dense flags (with FLAG_STAGE_TIMES: the ball voxels counted)
THICK_MAX_RADIUS2 = 1 << 14  # ... its largest max_radius2
THIN_ULTIMATE, THIN_CURVE = 0, 1  # o2v_hip_thin_dense modes: no end points; end points stay
THIN_DST_MASK, THIN_DST_DEGREE = 0, 1  # ... its dst formats: 1 / 0; 1 + the 26-neighbours in the skeleton
STATS_BOX, STATS_SUMS, STATS_MOMENTS, STATS_FACES = 1, 2, 4, 8  # ... the bits of `which`
STATS_COLUMNS = 17  # ... the int64 columns of a row of its table
ADJ_ZERO = 16  # o2v_hip_adjacency_count flag: the value 0 is a label like any other (with FLAG_STAGE_TIMES: the counters)
ADJ_COLUMNS = 5  # ... the int64 columns of a row of its table: faces, edges, corners, pass_high, pass_low
OCT_COLLAPSE = 64  # o2v_hip_octree_build / _lookup / _to_dense: full cells are leaves
OCT_MAX_DEPTH = 16  # ... the deepest tree: a root cube of 65 536 voxels along an axis
OPEN_SURFACE, OPEN_SOLID, OPEN_EMPTY, OPEN_GRID = 0, 1, 2, 3  # o2v_hip_openness: the target modes
OPEN_MAX_DIRECTIONS = 254  # ... the most directions of a call (a count is one byte, 255 marks the voxels that are no targets)
OPEN_MAX_COMPONENT = 127  # ... the largest magnitude of a direction's component
LABEL_SURFACE_CLOSED = 1  # o2v_hip_label_surface_count / _write: the box is surrounded by label 0, every part is capped at its sides
EULER_COLUMNS = 7  # o2v_hip_euler_stats: the int64 columns of a row of its table: voxels, closed-in faces, edges, vertices, inner faces, edges, vertices
ERR_BAD_ARGUMENT = 3
ERR_LIMIT = 5
ERR_IO = 6  # o2v_hip_gather_save: the file cannot be opened, is of no output type, or stopped taking voxels


class _Texture(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32),
                ("channels", C.c_uint32), ("wrap", C.c_uint32)]


class Timings(C.Structure):
    _fields_ = [("bounds_ms", C.c_float), ("expand_ms", C.c_float), ("voxelize_ms", C.c_float),
                ("scan_ms", C.c_float), ("resolve_ms", C.c_float), ("total_ms", C.c_float), ("passes", C.c_uint32),
                ("plan_ms", C.c_float), ("collective_ms", C.c_float), ("collective_parts_ms", C.c_float * 5), ("fill_ms", C.c_float)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["collective_parts_ms"] = [float(x) for x in self.collective_parts_ms]   # status + bounds (one reduce), -, histograms + block extents (one gather), -, counts
        return d


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("triangles", "leaves", "tiles", "candidates", "hits", "voxels",
                                          "grid_cells", "grid_bytes", "bricks", "dirty_bricks", "pool_slots", "direct_hits", "jobs",
                                          "certain_hits", "skipped_jobs", "bypassed_leaves", "interior_voxels")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("ms", C.c_float), ("launches", C.c_uint32)]


class DeviceError(RuntimeError):
    pass


def _bind():
    L = lib()
    L.o2v_hip_device_count.restype = C.c_int
    L.o2v_hip_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.o2v_hip_destroy.argtypes = [C.c_void_p]
    L.o2v_hip_last_error.argtypes = [C.c_void_p]
    L.o2v_hip_last_error.restype = C.c_char_p
    L.o2v_hip_set_triangles.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_uint64]
    L.o2v_hip_set_textures.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.o2v_hip_voxelize.argtypes = [C.c_void_p, C.POINTER(_Params), C.POINTER(C.c_uint64)]
    L.o2v_hip_read_voxels.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]
    L.o2v_hip_get_timings.argtypes = [C.c_void_p, C.POINTER(Timings)]
    L.o2v_hip_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.o2v_hip_get_transform.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_debug_counters.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_debug_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.o2v_hip_debug_check_third.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_debug_check_div.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    L.o2v_hip_comm_unique_id.argtypes = [C.c_void_p]
    L.o2v_hip_comm_create_rccl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.o2v_hip_comm_create_callbacks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.o2v_hip_comm_destroy.argtypes = [C.c_void_p]
    L.o2v_hip_comm_kind.argtypes = [C.c_void_p]
    L.o2v_hip_comm_kind.restype = C.c_char_p
    L.o2v_hip_comm_last_error.argtypes = [C.c_void_p]
    L.o2v_hip_comm_last_error.restype = C.c_char_p
    L.o2v_hip_voxelize_sharded.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_Params), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
    L.o2v_hip_group_create.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.o2v_hip_group_destroy.argtypes = [C.c_void_p]
    L.o2v_hip_group_size.argtypes = [C.c_void_p]
    L.o2v_hip_group_size.restype = C.c_uint32
    L.o2v_hip_group_ctx.argtypes = [C.c_void_p, C.c_uint32]
    L.o2v_hip_group_ctx.restype = C.c_void_p
    L.o2v_hip_group_comm_kind.argtypes = [C.c_void_p]
    L.o2v_hip_group_comm_kind.restype = C.c_char_p
    L.o2v_hip_group_last_error.argtypes = [C.c_void_p]
    L.o2v_hip_group_last_error.restype = C.c_char_p
    L.o2v_hip_group_set_triangles.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_uint64, C.c_int]
    L.o2v_hip_group_set_textures.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.o2v_hip_group_voxelize.argtypes = [C.c_void_p, C.POINTER(_Params), C.c_void_p, C.c_void_p]
    L.o2v_hip_plan_slabs.argtypes = [C.c_void_p, C.POINTER(_Params), C.c_uint32, C.c_void_p, C.c_void_p]
    L.o2v_hip_get_kernel_times.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.o2v_hip_build_id.restype = C.c_char_p
    L.o2v_mesh_load_file.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
    L.o2v_mesh_arrays.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 5 + [C.POINTER(C.c_uint32)]
    L.o2v_mesh_arrays.restype = C.c_uint64
    L.o2v_mesh_texture.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_Texture)]
    L.o2v_mesh_free.argtypes = [C.c_void_p]
    L.o2v_hip_set_triangles_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint64]
    L.o2v_hip_write_dense.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.o2v_hip_voxels_box.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.o2v_hip_distance_dense.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.o2v_hip_distance_scratch_bytes.argtypes = [C.c_void_p, C.c_uint32]
    L.o2v_hip_distance_scratch_bytes.restype = C.c_uint64
    L.o2v_hip_distance_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_mesh_distance_dense.argtypes = [C.c_void_p, C.POINTER(_Params), C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    L.o2v_hip_mesh_distance_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_surface_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.o2v_hip_surface_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_uint64,
                                        C.c_void_p, C.c_uint64]
    L.o2v_hip_surface_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_raycast_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    L.o2v_hip_raycast.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_float, C.c_void_p, C.c_void_p]
    L.o2v_hip_raycast_scratch_bytes.argtypes = [C.c_void_p]
    L.o2v_hip_raycast_scratch_bytes.restype = C.c_uint64
    L.o2v_hip_raycast_generation.argtypes = [C.c_void_p]
    L.o2v_hip_raycast_generation.restype = C.c_uint64
    L.o2v_hip_raycast_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_components_dense.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32,
                                           C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.o2v_hip_flood_dense.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.o2v_hip_components_scratch_bytes.argtypes = [C.c_void_p, C.c_uint32]
    L.o2v_hip_components_scratch_bytes.restype = C.c_uint64
    L.o2v_hip_components_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_components_counters.argtypes = [C.c_void_p, C.c_void_p]
    _gather = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float]   # ctx, grid, format, strides, dims, level
    _gather_color = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]   # origin, mode, argb, colors, strides, palette
    L.o2v_hip_gather_count.argtypes = _gather + [C.POINTER(C.c_uint64)]
    L.o2v_hip_gather_write.argtypes = _gather + _gather_color + [C.c_uint64, C.c_uint64, C.c_void_p]
    L.o2v_hip_gather_save.argtypes = _gather + _gather_color + [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.o2v_hip_gather_scratch_bytes.argtypes = [C.c_void_p]
    L.o2v_hip_gather_scratch_bytes.restype = C.c_uint64
    L.o2v_hip_gather_times.argtypes = [C.c_void_p, C.c_void_p]
    _faces = _gather + [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]   # ..., merge, mode, argb, colors, strides, palette
    L.o2v_hip_faces_count.argtypes = _faces + [C.POINTER(C.c_uint64)]
    L.o2v_hip_faces_write.argtypes = _faces + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.o2v_hip_faces_scratch_bytes.argtypes = [C.c_void_p, C.c_uint32]
    L.o2v_hip_faces_scratch_bytes.restype = C.c_uint64
    L.o2v_hip_faces_scratch_bytes_merge.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    L.o2v_hip_faces_scratch_bytes_merge.restype = C.c_uint64
    L.o2v_hip_faces_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_nearest_dense.argtypes = _gather + [C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint32]   # ..., flags, 3 x (grid, strides), max_dist2
    L.o2v_hip_nearest_scratch_bytes.argtypes = [C.c_void_p]
    L.o2v_hip_nearest_scratch_bytes.restype = C.c_uint64
    L.o2v_hip_nearest_times.argtypes = [C.c_void_p, C.c_void_p]
    # ..., origin, factor, min_count, value_mode, 5 x (grid, strides): colors, count, solid, values, argb
    L.o2v_hip_downsample.argtypes = _gather + [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 10
    L.o2v_hip_downsample_box.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.o2v_hip_downsample_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_crossings_dense.argtypes = [C.c_void_p, C.POINTER(_Params), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.o2v_hip_crossings_times.argtypes = [C.c_void_p, C.c_void_p]
    # ctx, labels, format, strides, dims, origin, n_labels, which, table, out_outside
    L.o2v_hip_label_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                      C.POINTER(C.c_uint64)]
    L.o2v_hip_label_stats_times.argtypes = [C.c_void_p, C.c_void_p]
    # ctx, grid, format, strides, dims, level, weights, flags, seeds, n_seeds, max_distance, dist, dist_strides, out_reached
    L.o2v_hip_geodesic_dense.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_uint32, C.c_void_p,
                                         C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    # ctx, dist, dist_strides, dims, weights, targets, n_targets, max_len, paths, lengths
    L.o2v_hip_geodesic_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                         C.c_void_p]
    L.o2v_hip_geodesic_scratch_bytes.argtypes = [C.c_void_p, C.c_uint32]
    L.o2v_hip_geodesic_scratch_bytes.restype = C.c_uint64
    L.o2v_hip_geodesic_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_geodesic_counters.argtypes = [C.c_void_p, C.c_void_p]
    # ..., flags, max_radius2, dst, dst_strides, depth2, depth2_strides
    L.o2v_hip_thickness_dense.argtypes = _gather + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
    L.o2v_hip_thickness_scratch_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    L.o2v_hip_thickness_scratch_bytes.restype = C.c_uint64
    L.o2v_hip_thickness_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_thickness_counters.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_thickness_cover_table.argtypes = [C.c_uint32, C.c_void_p]
    # ..., flags, mode, max_iterations, keep, keep_strides, dst, dst_strides, dst_format
    L.o2v_hip_thin_dense.argtypes = _gather + [C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32]
    L.o2v_hip_thin_scratch_bytes.argtypes = [C.c_void_p, C.c_int]
    L.o2v_hip_thin_scratch_bytes.restype = C.c_uint64
    L.o2v_hip_thin_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_thin_counters.argtypes = [C.c_void_p, C.c_void_p]
    # ctx, relief, strides, dims, connectivity, min_depth, flags, labels, labels_strides, count
    L.o2v_hip_watershed_dense.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 3 + [C.c_void_p] * 3
    L.o2v_hip_watershed_scratch_bytes.argtypes = [C.c_void_p]
    L.o2v_hip_watershed_scratch_bytes.restype = C.c_uint64
    L.o2v_hip_watershed_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_watershed_counters.argtypes = [C.c_void_p, C.c_void_p]
    # ctx, relief, relief_strides, markers, marker_strides, dims, weights, flags, labels, strides, level, strides, ticks, strides, reached
    L.o2v_hip_grow_dense.argtypes = [C.c_void_p] * 7 + [C.c_uint32] + [C.c_void_p] * 7
    L.o2v_hip_grow_scratch_bytes.argtypes = [C.c_void_p, C.c_uint32]
    L.o2v_hip_grow_scratch_bytes.restype = C.c_uint64
    L.o2v_hip_grow_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_grow_counters.argtypes = [C.c_void_p, C.c_void_p]
    # ctx, labels, format, strides, dims, n_labels, connectivity, flags, values, value_strides, out_pairs, out_outside
    L.o2v_hip_adjacency_count.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.o2v_hip_adjacency_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.o2v_hip_adjacency_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_adjacency_counters.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_adjacency_scratch_bytes.argtypes = [C.c_uint64]
    L.o2v_hip_adjacency_scratch_bytes.restype = C.c_uint64
    # ctx, labels, format, strides, dims, n_labels, table, out_outside
    L.o2v_hip_euler_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]
    L.o2v_hip_euler_stats_times.argtypes = [C.c_void_p, C.c_void_p]
    # ctx, grid, format, strides, dims, level, origin, depth, flags, out_depth, level_counts, out_nodes, out_voxels_listed
    L.o2v_hip_octree_build.argtypes = _gather + [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint64),
                                                 C.POINTER(C.c_uint64)]
    L.o2v_hip_octree_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _tree = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]   # ctx, valid, full, first_child, n_nodes, depth, flags
    L.o2v_hip_octree_lookup.argtypes = _tree + [C.c_void_p, C.c_uint64, C.c_void_p]
    L.o2v_hip_octree_to_dense.argtypes = _tree + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.o2v_hip_octree_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_octree_scratch_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.o2v_hip_octree_scratch_bytes.restype = C.c_uint64
    L.o2v_hip_octree_depth.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_octree_depth.restype = C.c_uint32
    # ctx, valid, full, first_child, n_nodes, depth, flags, level_counts, out_level_counts, out_nodes, out_pointers
    L.o2v_hip_octree_dag_build.argtypes = _tree + [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.o2v_hip_octree_dag_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # ctx, valid, full, first_child, child, (skip,) n_nodes, n_pointers, depth, flags
    L.o2v_hip_octree_dag_lookup.argtypes = [C.c_void_p] * 6 + [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.o2v_hip_octree_dag_to_dense.argtypes = [C.c_void_p] * 5 + [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.o2v_hip_octree_dag_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_octree_dag_scratch_bytes.argtypes = [C.c_void_p, C.c_uint32]
    L.o2v_hip_octree_dag_scratch_bytes.restype = C.c_uint64
    # ... origins, directions, n, t_max, hit, t, voxel_index
    _rays = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.o2v_hip_octree_raycast.argtypes = _tree + _rays
    L.o2v_hip_octree_dag_raycast.argtypes = [C.c_void_p] * 6 + [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32] + _rays
    L.o2v_hip_octree_raycast_times.argtypes = [C.c_void_p, C.c_void_p]
    # ctx, grid, format, strides, dims, level, directions, n_directions, target_mode, target_grid, target_strides, max_distance2, flags,
    # dst, dst_strides, mask, mask_strides, out_targets
    L.o2v_hip_openness.argtypes = _gather + [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.o2v_hip_openness_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_openness_scratch_bytes.argtypes = [C.c_void_p]
    L.o2v_hip_openness_scratch_bytes.restype = C.c_uint64
    # ctx, labels, format, strides, dims, flags, out_vertices, out_quads
    L.o2v_hip_label_surface_count.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint64)]
    # ctx, labels, format, strides, dims, flags, cells, links, vertex_capacity, faces, pairs, quad_capacity
    L.o2v_hip_label_surface_write.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                              C.c_void_p, C.c_void_p, C.c_uint64]
    # ctx, cells, links, n_vertices, origin, iterations, relaxation, reach, positions
    L.o2v_hip_label_surface_relax.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_void_p]
    L.o2v_hip_label_surface_times.argtypes = [C.c_void_p, C.c_void_p]
    L.o2v_hip_max_slab_layers.argtypes = [C.c_void_p, C.POINTER(_Params), C.POINTER(C.c_uint32)]
    return L


def torch_was_loaded_first():
    """True if torch was imported before this process loaded the library (the two then share one HIP runtime), False if not,
    None if the library is not loaded yet."""
    return _lib.torch_was_loaded_first


def build_id():
    """Hash of the device sources the loaded library was built from (o2v_hip_build_id)."""
    return _bind().o2v_hip_build_id().decode()


def load_mesh_file(path):
    """o2v_mesh_load_file: (verts [T, 9], materials dict for set_triangles, textures list for set_textures) of an OBJ / STL
    file, read by the library's own readers."""
    L = _bind()
    h = C.c_void_p()
    if L.o2v_mesh_load_file(str(path).encode(), None, C.byref(h)) != 0:
        raise DeviceError(f"o2v_mesh_load_file({path}) failed: unknown type or unreadable file")
    try:
        ptrs = [C.c_void_p() for _ in range(5)]
        ntex = C.c_uint32(0)
        T = int(L.o2v_mesh_arrays(h, *[C.byref(q) for q in ptrs], C.byref(ntex)))

        def arr(q, ctype, width, dtype):
            if not q.value or not T:
                return None
            return np.ctypeslib.as_array(C.cast(q, C.POINTER(ctype)), shape=(T * width,)).astype(dtype).reshape(T, width).copy()
        verts = arr(ptrs[0], C.c_float, 9, np.float32)
        mat = {}
        for key, q, ctype, width, dtype in (("uvs", ptrs[1], C.c_float, 6, np.float32), ("types", ptrs[2], C.c_uint32, 1, np.uint32),
                                            ("colors", ptrs[3], C.c_float, 3, np.float32), ("texids", ptrs[4], C.c_int32, 1, np.int32)):
            a = arr(q, ctype, width, dtype)
            if a is not None:
                mat[key] = a.reshape(T) if width == 1 else a
        textures = []
        for i in range(ntex.value):
            t = _Texture()
            L.o2v_mesh_texture(h, i, C.byref(t))
            pix = np.ctypeslib.as_array(C.cast(t.pixels, C.POINTER(C.c_uint8)), shape=(t.height, t.width, t.channels)).copy()
            textures.append((pix, int(t.wrap)))
        return (np.zeros((0, 9), np.float32) if verts is None else verts), mat, textures
    finally:
        L.o2v_mesh_free(h)


def raycast_scratch_bytes(dims):
    """o2v_hip_raycast_scratch_bytes: the context scratch the snapshot of a raycast_build over dims (x, y, z) takes."""
    return int(_bind().o2v_hip_raycast_scratch_bytes(_u32x3(dims)))


def components_scratch_bytes(dims, which=CC_SCRATCH_LABELS):
    """o2v_hip_components_scratch_bytes: the context scratch a components_dense (CC_SCRATCH_LABELS: contiguous labels,
    CC_SCRATCH_LABELS_STRIDED: any other) or flood_dense (CC_SCRATCH_FLOOD) call over dims (x, y, z) takes."""
    return int(_bind().o2v_hip_components_scratch_bytes(_u32x3(dims), which))


def geodesic_scratch_bytes(dims, which=GEO_SCRATCH_CONTIGUOUS):
    """o2v_hip_geodesic_scratch_bytes: the context scratch a geodesic_dense call over dims (x, y, z) takes with a contiguous dist
    (GEO_SCRATCH_CONTIGUOUS) or any other (GEO_SCRATCH_STRIDED)."""
    return int(_bind().o2v_hip_geodesic_scratch_bytes(_u32x3(dims), which))


def thickness_scratch_bytes(dims, max_radius2, have_depth2=False):
    """o2v_hip_thickness_scratch_bytes: the context scratch a thickness_dense call over dims (x, y, z) with that cap takes, with
    (have_depth2) or without a depth2 grid of the caller's; on top of it 4 bytes per kept ball centre."""
    return int(_bind().o2v_hip_thickness_scratch_bytes(_u32x3(dims), int(max_radius2), 1 if have_depth2 else 0))


def adjacency_scratch_bytes(pairs):
    """o2v_hip_adjacency_scratch_bytes: the context scratch that the sorted list of `pairs` pairs of an adjacency_count takes (the
    pair table grows with the data: adjacency_counters)."""
    return int(_bind().o2v_hip_adjacency_scratch_bytes(int(pairs)))


def grow_scratch_bytes(dims, which=0):
    """o2v_hip_grow_scratch_bytes: the context scratch a grow_dense call over dims (x, y, z) takes; `which`: the OR of
    GROW_SCRATCH_LABELS / _LEVEL / _TICKS for those of the three that are absent or not contiguous."""
    return int(_bind().o2v_hip_grow_scratch_bytes(_u32x3(dims), which))


def watershed_scratch_bytes(dims):
    """o2v_hip_watershed_scratch_bytes: the context scratch of a watershed_dense call over dims (x, y, z) that the box fixes (the
    peaks, the pair table and the pair list grow with the data: watershed_counters)."""
    return int(_bind().o2v_hip_watershed_scratch_bytes(_u32x3(dims)))


def thin_scratch_bytes(dims, have_keep=False):
    """o2v_hip_thin_scratch_bytes: the context scratch a thin_dense call over dims (x, y, z) takes, with or without a keep grid."""
    return int(_bind().o2v_hip_thin_scratch_bytes(_u32x3(dims), 1 if have_keep else 0))


def thickness_cover_table(max_radius2):
    """o2v_hip_thickness_cover_table: uint32 [3, max_radius2 + 1], row k - 1 the smallest radius^2 L_k[R] at which the discrete
    ball {|q|^2 < L} of a neighbour at (1, 0, 0), (1, 1, 0), (1, 1, 1) (k = 1, 2, 3) contains the ball of radius^2 R; column 0 is
    0.  Needs no device."""
    if isinstance(max_radius2, bool) or not isinstance(max_radius2, int) or not 1 <= max_radius2 <= THICK_MAX_RADIUS2:
        raise ValueError(f"max_radius2 must be an int 1 ... {THICK_MAX_RADIUS2}, not {max_radius2!r}")
    out = np.zeros((3, max_radius2 + 1), np.uint32)
    rc = _bind().o2v_hip_thickness_cover_table(max_radius2, _ptr(out))
    if rc != 0:
        raise DeviceError("o2v_hip_thickness_cover_table failed (code %d)" % rc)
    return out


def gather_scratch_bytes(dims):
    """o2v_hip_gather_scratch_bytes: the context scratch a gather_count over dims (x, y, z) takes."""
    return int(_bind().o2v_hip_gather_scratch_bytes(_u32x3(dims)))


def faces_scratch_bytes(dims, color_mode=GATHER_COLOR_CONSTANT, merge=None):
    """o2v_hip_faces_scratch_bytes: the context scratch a faces_count over dims (x, y, z) takes at most; with a merge mode
    o2v_hip_faces_scratch_bytes_merge: FACES_MERGE_RECTS takes more than the other two."""
    if merge is None:
        return int(_bind().o2v_hip_faces_scratch_bytes(_u32x3(dims), color_mode))
    return int(_bind().o2v_hip_faces_scratch_bytes_merge(_u32x3(dims), color_mode, merge))


def octree_scratch_bytes(dims, origin=(0, 0, 0), depth=0):
    """o2v_hip_octree_scratch_bytes: the most context scratch an octree_build of the box origin + [0, dims) (x, y, z) takes."""
    return int(_bind().o2v_hip_octree_scratch_bytes(_u32x3(dims), _u32x3(origin), int(depth)))


def _level_counts(level_counts):
    counts = [int(c) for c in level_counts]
    if len(counts) > OCT_MAX_DEPTH or any(not 0 <= c < 2 ** 64 for c in counts):
        raise ValueError(f"level_counts must be at most {OCT_MAX_DEPTH} counts, not {level_counts!r}")
    return (C.c_uint64 * OCT_MAX_DEPTH)(*(counts + [0] * (OCT_MAX_DEPTH - len(counts))))


def octree_dag_scratch_bytes(level_counts, depth):
    """o2v_hip_octree_dag_scratch_bytes: the most context scratch an octree_dag_build of a tree of these nodes per level takes; 0
    for level counts a build refuses."""
    return int(_bind().o2v_hip_octree_dag_scratch_bytes(_level_counts(level_counts), int(depth)))


def openness_scratch_bytes(dims):
    """o2v_hip_openness_scratch_bytes: the most context scratch an openness call over dims (x, y, z) takes."""
    return int(_bind().o2v_hip_openness_scratch_bytes(_u32x3(dims)))


def octree_depth(origin, dims):
    """o2v_hip_octree_depth: the smallest depth whose root cube [0, 2^depth)^3 holds origin + [0, dims) (x, y, z); 0 if a dim is 0 or
    origin + dims is above 65 536.  Needs no device."""
    if any(not 0 <= int(v) < 2 ** 32 for v in tuple(origin) + tuple(dims)):
        return 0
    return int(_bind().o2v_hip_octree_depth(_u32x3(origin), _u32x3(dims)))


def device_count():
    return _bind().o2v_hip_device_count()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u32x3(v):
    return (C.c_uint32 * 3)(*[int(x) for x in v])


def _u64x3(v):
    return None if v is None else (C.c_uint64 * 3)(*[int(x) for x in v])


def downsample_box(origin, dims, factor):
    """o2v_hip_downsample_box: (coarse origin, coarse dims), each (x, y, z), of the box origin + [0, dims) of the fine lattice
    merged in blocks of factor^3 aligned to the global lattice.  Needs no device."""
    co, cd = (C.c_uint32 * 3)(), (C.c_uint32 * 3)()
    if any(not 0 <= int(v) < 2 ** 32 for v in tuple(origin) + tuple(dims)) or not 0 <= int(factor) < 2 ** 32:
        raise DeviceError("o2v_hip_downsample_box failed (code %d): an argument does not fit 32 bits" % ERR_BAD_ARGUMENT)
    rc = _bind().o2v_hip_downsample_box(_u32x3(origin), _u32x3(dims), int(factor), co, cd)
    if rc != 0:
        raise DeviceError("o2v_hip_downsample_box failed (code %d): the factor must be 2 ... 8, the dims positive and origin + dims at "
                          "most 2^32" % rc)
    return tuple(int(v) for v in co), tuple(int(v) for v in cd)


class DeviceVoxelizer:
    """Owns one GPU's dense grid slab and work buffers; reusable across voxelize() calls."""

    def __init__(self, device=0, _borrowed_ctx=None):
        self._L = _bind()
        self._owned = _borrowed_ctx is None
        self.device = None if _borrowed_ctx is not None else device
        self._n_out = C.c_uint64(0)
        if _borrowed_ctx is not None:       # a rank of a DeviceGroup: the group owns the context
            self._ctx = C.c_void_p(_borrowed_ctx)
            return
        self._ctx = C.c_void_p()
        rc = self._L.o2v_hip_create(device, C.byref(self._ctx))
        if rc != 0:
            raise DeviceError(f"o2v_hip_create(device={device}) failed with code {rc}: no usable MI355X / HIP runtime")
        self._keep = []

    def close(self):
        if self._ctx and self._owned:
            self._L.o2v_hip_destroy(self._ctx)
        self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise DeviceError(f"{what} failed with code {rc}: {self._L.o2v_hip_last_error(self._ctx).decode()}")

    def set_triangles(self, verts, uvs=None, types=None, colors=None, texids=None):
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
        T = verts.shape[0]
        uvs = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(T, 6)
        types = None if types is None else np.ascontiguousarray(types, dtype=np.uint32).reshape(T)
        colors = None if colors is None else np.ascontiguousarray(colors, dtype=np.float32).reshape(T, 3)
        texids = None if texids is None else np.ascontiguousarray(texids, dtype=np.int32).reshape(T)
        self._check(self._L.o2v_hip_set_triangles(self._ctx, _ptr(verts), _ptr(uvs), _ptr(types), _ptr(colors),
                                                  _ptr(texids), T), "o2v_hip_set_triangles")
        self.n_tris = T

    def set_triangles_device(self, positions_ptr, n_positions, faces_ptr, index_bytes, count, uvs_ptr=None, types_ptr=None,
                             colors_ptr=None, texids_ptr=None):
        """o2v_hip_set_triangles_device: the arrays of set_triangles as device addresses (integers) on this context's device.
        faces_ptr None: positions_ptr is [count, 9] float32.  Else positions [n_positions, 3] float32 and faces [count, 3] of
        index_bytes (4 or 8).  The caller must have finished writing the arrays."""
        rc = self._L.o2v_hip_set_triangles_device(self._ctx, positions_ptr, n_positions, faces_ptr, index_bytes, uvs_ptr, types_ptr,
                                                  colors_ptr, texids_ptr, count)
        if rc == 0:
            self.n_tris = count
        elif "face index" in self._L.o2v_hip_last_error(self._ctx).decode():
            self.n_tris = 0   # (the context was left with no triangles)
        self._check(rc, "o2v_hip_set_triangles_device")

    def write_dense(self, ptr, fmt, origin, dims, strides):
        """o2v_hip_write_dense: the last voxelize call's records into the dense grid at device address `ptr` (DENSE_U8 /
        DENSE_ARGB32 / DENSE_BITS; origin, dims, strides per axis x, y, z).  Returns the number of records outside the box."""
        o, d, s, outside = _u32x3(origin), _u32x3(dims), _u64x3(strides), C.c_uint64(0)
        self._check(self._L.o2v_hip_write_dense(self._ctx, ptr, fmt, o, d, s, C.byref(outside)), "o2v_hip_write_dense")
        return outside.value

    def voxels_box(self):
        """o2v_hip_voxels_box: ((lo x, y, z), (hi x, y, z)), the last call's records' box [lo, hi); zeros if there are none."""
        lo, hi = (C.c_uint32 * 3)(), (C.c_uint32 * 3)()
        self._check(self._L.o2v_hip_voxels_box(self._ctx, lo, hi), "o2v_hip_voxels_box")
        return tuple(lo), tuple(hi)

    def distance_dense(self, labels_ptr, label_strides, dst_ptr, fmt, dst_strides, dims):
        """o2v_hip_distance_dense: the squared distance (DIST_SQ_I32) or SDF (DIST_SDF_F32) of the uint8 label grid at device
        address labels_ptr into dst_ptr; strides in elements and dims per axis x, y, z."""
        ls, ds, d = _u64x3(label_strides), _u64x3(dst_strides), _u32x3(dims)
        self._check(self._L.o2v_hip_distance_dense(self._ctx, labels_ptr, ls, dst_ptr, fmt, ds, d), "o2v_hip_distance_dense")

    def distance_scratch_bytes(self, dims, fmt):
        """o2v_hip_distance_scratch_bytes: the context scratch a distance_dense call over dims (x, y, z) needs."""
        return int(self._L.o2v_hip_distance_scratch_bytes(_u32x3(dims), fmt))

    def _stage_times(self, name, n=3):   # (o2v_hip_distance_times, o2v_hip_mesh_distance_times, o2v_hip_surface_times)
        ms = (C.c_float * n)()
        self._check(getattr(self._L, name)(self._ctx, ms), name)
        return tuple(float(v) for v in ms)

    def distance_times(self):
        """o2v_hip_distance_times: the device times (ms) of the last distance_dense call's x, y and z passes."""
        return self._stage_times("o2v_hip_distance_times")

    def mesh_distance_dense(self, resolution, band, fmt, origin, dims, dst_ptr, dst_strides, closest_ptr=None, closest_strides=None, *,
                            supersampling=1, unit_transform=None, bounds=None):
        """o2v_hip_mesh_distance_dense: the narrow-band distance (voxels, truncated at `band`) from the centres of the box
        origin + [0, dims) to the context's triangles, MESH_DIST_UNSIGNED_F32 or MESH_DIST_SIGNED_F32, into float32 at device
        address dst_ptr and, if closest_ptr is given, the closest triangle's index (int32, -1 outside the band); strides in
        elements, origin, dims and strides per axis x, y, z."""
        p = self._params(resolution, supersampling, 0, unit_transform, bounds, (0, 0))
        self._check(self._L.o2v_hip_mesh_distance_dense(self._ctx, C.byref(p), float(band), fmt, _u32x3(origin), _u32x3(dims), dst_ptr,
                                                        _u64x3(dst_strides), closest_ptr, _u64x3(closest_strides)), "o2v_hip_mesh_distance_dense")

    def mesh_distance_times(self):
        """o2v_hip_mesh_distance_times: the device times (ms) of the last mesh_distance_dense call's binning, parity and
        distance stages (parity 0 when unsigned)."""
        return self._stage_times("o2v_hip_mesh_distance_times")

    def surface_count(self, field_ptr, strides, dims, level):
        """o2v_hip_surface_count: (vertices, triangles) of the level set `level` of the float32 grid at device address
        field_ptr (strides in elements and dims per axis x, y, z), by surface nets; what surface_write needs stays in the
        context."""
        v, t = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.o2v_hip_surface_count(self._ctx, field_ptr, _u64x3(strides), _u32x3(dims), float(level), C.byref(v), C.byref(t)),
                    "o2v_hip_surface_count")
        return v.value, t.value

    def surface_write(self, field_ptr, strides, dims, level, origin, positions_ptr, vertex_capacity, faces_ptr, triangle_capacity):
        """o2v_hip_surface_write: the mesh surface_count counted for the same field, strides, dims and level, into float32
        positions [vertices, 3] (voxel space, sample (x, y, z) at origin + (x, y, z) + 0.5) and int32 faces [triangles, 3] at
        device addresses, contiguous."""
        self._check(self._L.o2v_hip_surface_write(self._ctx, field_ptr, _u64x3(strides), _u32x3(dims), float(level), _u32x3(origin), positions_ptr,
                                                  vertex_capacity, faces_ptr, triangle_capacity), "o2v_hip_surface_write")

    def surface_times(self):
        """o2v_hip_surface_times: the device times (ms) of the last surface_count call's classify and count + scan stages and
        of the last surface_write call's vertex and face stages."""
        return self._stage_times("o2v_hip_surface_times", 4)

    def raycast_build(self, grid_ptr, fmt, strides, dims, level=0.0, origin=(0, 0, 0)):
        """o2v_hip_raycast_build: the snapshot of the grid at device address grid_ptr (RAY_GRID_U8: element != 0; RAY_GRID_BITS:
        the words write_dense DENSE_BITS writes; RAY_GRID_F32_BELOW: float32 < level; strides and dims per axis x, y, z) that
        raycast walks, kept in the context.  Returns its generation (raycast_generation): every build, refused or not, replaces
        the last one."""
        try:
            self._check(self._L.o2v_hip_raycast_build(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level), _u32x3(origin)),
                        "o2v_hip_raycast_build")
        finally:
            generation = self.raycast_generation()
        return generation

    def raycast_generation(self):
        """o2v_hip_raycast_generation: the number of raycast_build calls made on this context, refused ones included."""
        return int(self._L.o2v_hip_raycast_generation(self._ctx))

    def raycast(self, origins_ptr, directions_ptr, n, t_max, hit_ptr, t_ptr):
        """o2v_hip_raycast: n rays (float32 [n, 3] origins and directions at device addresses) through the last raycast_build,
        into int32 hit [n, 4] = (x, y, z, face) and float32 t [n]; a miss is (-1, -1, -1, -1), +inf."""
        self._check(self._L.o2v_hip_raycast(self._ctx, origins_ptr, directions_ptr, n, float(t_max), hit_ptr, t_ptr), "o2v_hip_raycast")

    def raycast_scratch_bytes(self, dims):
        """o2v_hip_raycast_scratch_bytes: the context scratch the snapshot of a raycast_build over dims (x, y, z) takes."""
        return raycast_scratch_bytes(dims)

    def raycast_times(self):
        """o2v_hip_raycast_times: the device times (ms) of the last raycast_build and the last raycast."""
        return self._stage_times("o2v_hip_raycast_times", 2)

    def components_dense(self, grid_ptr, fmt, strides, dims, level, connectivity, flags, labels_ptr, label_strides):
        """o2v_hip_components_dense: the connected components (connectivity 6, 18 or 26) of the set of the grid at device address
        grid_ptr (GRID_U8: element != 0; GRID_BITS; GRID_F32_BELOW: float32 < level; CC_INVERT in flags: the complement inside the
        box) into int32 labels at labels_ptr, 1 + the rank of a voxel's component by its smallest linear index, 0 outside the
        set; strides in elements and dims per axis x, y, z.  Returns the number of components."""
        n = C.c_uint64(0)
        self._check(self._L.o2v_hip_components_dense(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level), connectivity, flags,
                                                     labels_ptr, _u64x3(label_strides), C.byref(n)), "o2v_hip_components_dense")
        return n.value

    def flood_dense(self, grid_ptr, fmt, strides, dims, level, connectivity, flags, seeds_ptr, n_seeds, values, out_ptr, out_strides):
        """o2v_hip_flood_dense: uint8 out = values[0] in the components of the set that hold a seed (int32 [n_seeds, 3] local
        (x, y, z) at device address seeds_ptr; CC_SEED_BORDER in flags: and the set's voxels on the box's faces), values[1] in
        the others, values[2] outside the set.  Returns the number of voxels that got values[0]."""
        n = C.c_uint64(0)
        v = (C.c_uint8 * 3)(*[int(x) for x in values])
        self._check(self._L.o2v_hip_flood_dense(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level), connectivity, flags,
                                                seeds_ptr, n_seeds, v, out_ptr, _u64x3(out_strides), C.byref(n)), "o2v_hip_flood_dense")
        return n.value

    def components_scratch_bytes(self, dims, which=CC_SCRATCH_LABELS):
        """o2v_hip_components_scratch_bytes: the context scratch a components_dense / flood_dense call over dims (x, y, z) takes."""
        return components_scratch_bytes(dims, which)

    def components_times(self):
        """o2v_hip_components_times: the device times (ms) of the last components_dense / flood_dense call's classify, tile,
        seam, flatten (+ root count) and write (+ seeds) stages."""
        return self._stage_times("o2v_hip_components_times", 5)

    def components_counters(self):
        """o2v_hip_components_counters: (pairs united across tile seams, atomic mins that went round again) of the last call
        made with FLAG_STAGE_TIMES in its flags."""
        out = (C.c_uint64 * 2)()
        self._check(self._L.o2v_hip_components_counters(self._ctx, out), "o2v_hip_components_counters")
        return int(out[0]), int(out[1])

    def gather_count(self, grid_ptr, fmt, strides, dims, level):
        """o2v_hip_gather_count: the number of solid voxels of the grid at device address grid_ptr (GRID_U8 / GRID_BITS /
        GRID_F32_BELOW with level; strides in elements and dims per axis x, y, z).  The one pass over the grid: the set's bits
        and the records' offsets stay in the context for gather_write."""
        n = C.c_uint64(0)
        self._check(self._L.o2v_hip_gather_count(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level), C.byref(n)),
                    "o2v_hip_gather_count")
        return int(n.value)

    @staticmethod
    def _gather_color(origin, color_mode, argb, colors_ptr, color_strides, palette):
        pal = None if palette is None else (C.c_uint32 * 256)(*[int(v) & 0xFFFFFFFF for v in palette])
        return _u32x3(origin), color_mode, int(argb) & 0xFFFFFFFF, colors_ptr, _u64x3(color_strides), pal

    def gather_write(self, grid_ptr, fmt, strides, dims, level, origin, color_mode, argb, colors_ptr, color_strides, palette, first, n,
                     records_ptr):
        """o2v_hip_gather_write: records [first, first + n) of the grid's solid voxels in ascending (z, y, x) - uint32 (origin +
        (x, y, z), argb) - to the device address records_ptr.  The grid arguments are those of the gather_count before it.
        color_mode: GATHER_COLOR_CONSTANT (argb), _GRID (colors_ptr: a uint32 grid, color_strides in elements) or _PALETTE
        (palette: 256 integers, indexed by the voxel's byte)."""
        self._check(self._L.o2v_hip_gather_write(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level),
                                                 *self._gather_color(origin, color_mode, argb, colors_ptr, color_strides, palette),
                                                 first, n, records_ptr), "o2v_hip_gather_write")

    def gather_save(self, grid_ptr, fmt, strides, dims, level, origin, color_mode, argb, colors_ptr, color_strides, palette, path, file_type,
                    resolution):
        """o2v_hip_gather_save: the same records, all of them, into the voxel file `path` (file_type: an extension without dot, or
        None for the path's) through the file sinks of obj2voxel_voxelize(), in batches.  Returns the number of voxels."""
        n = C.c_uint64(0)
        self._check(self._L.o2v_hip_gather_save(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level),
                                                *self._gather_color(origin, color_mode, argb, colors_ptr, color_strides, palette),
                                                None if path is None else os.fsencode(path), None if file_type is None else str(file_type).encode(), resolution,
                                                C.byref(n)), "o2v_hip_gather_save")
        return int(n.value)

    def gather_scratch_bytes(self, dims):
        """o2v_hip_gather_scratch_bytes: the context scratch a gather_count over dims (x, y, z) takes."""
        return gather_scratch_bytes(dims)

    def gather_times(self):
        """o2v_hip_gather_times: the device times (ms) of the last gather_count's classify and count + scan stages and of the
        last gather_write."""
        return self._stage_times("o2v_hip_gather_times", 3)

    def _faces_args(self, grid_ptr, fmt, strides, dims, level, merge, color_mode, argb, colors_ptr, color_strides, palette):
        pal = None if palette is None else (C.c_uint32 * 256)(*[int(v) & 0xFFFFFFFF for v in palette])
        return (self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level), merge, color_mode, int(argb) & 0xFFFFFFFF, colors_ptr,
                _u64x3(color_strides), pal)

    def faces_count(self, grid_ptr, fmt, strides, dims, level, merge, color_mode, argb, colors_ptr, color_strides, palette):
        """o2v_hip_faces_count: the number of quads of the grid's exposed voxel faces (grid arguments as gather_count takes them;
        merge: FACES_MERGE_NONE - one per face -, FACES_MERGE_RUNS - one per run of faces of one colour - or FACES_MERGE_RECTS - one
        per chain of equal runs in neighbouring rows; the colour arguments
        as gather_write takes them).  The one pass over the grid: the set's bits stay in the context for faces_write."""
        n = C.c_uint64(0)
        self._check(self._L.o2v_hip_faces_count(*self._faces_args(grid_ptr, fmt, strides, dims, level, merge, color_mode, argb, colors_ptr,
                                                                  color_strides, palette), C.byref(n)), "o2v_hip_faces_count")
        return int(n.value)

    def faces_write(self, grid_ptr, fmt, strides, dims, level, merge, color_mode, argb, colors_ptr, color_strides, palette, origin,
                    positions_ptr, faces_ptr, quad_argb_ptr, quad_capacity):
        """o2v_hip_faces_write: all quads of the faces_count before it (the same arguments) to the device addresses positions_ptr
        (float32 [4Q, 3]), faces_ptr (int32 [2Q, 3], or None) and quad_argb_ptr (uint32 [Q], or None), each with room for
        quad_capacity quads."""
        self._check(self._L.o2v_hip_faces_write(*self._faces_args(grid_ptr, fmt, strides, dims, level, merge, color_mode, argb, colors_ptr,
                                                                  color_strides, palette), _u32x3(origin), positions_ptr, faces_ptr,
                                                quad_argb_ptr, quad_capacity), "o2v_hip_faces_write")

    def faces_scratch_bytes(self, dims, color_mode=GATHER_COLOR_CONSTANT, merge=None):
        """o2v_hip_faces_scratch_bytes (merge None) / _merge: the context scratch a faces_count over dims (x, y, z) takes at most."""
        return faces_scratch_bytes(dims, color_mode, merge)

    def faces_times(self):
        """o2v_hip_faces_times: the device times (ms) of the last faces_count's classify and count + scan stages and of the last
        faces_write."""
        return self._stage_times("o2v_hip_faces_times", 3)

    def nearest_dense(self, grid_ptr, fmt, strides, dims, level, flags, nearest_ptr, nearest_strides, dist2_ptr=None, dist2_strides=None,
                      values_ptr=None, value_strides=None, max_dist2=NEAREST_NO_LIMIT):
        """o2v_hip_nearest_dense: for every voxel the linear index (z * ny + y) * nx + x of the nearest seed of the grid at device
        address grid_ptr (grid arguments as gather_count takes them; NEAREST_SEED_ONE in flags: a uint8 element that is 1), the
        smallest index on a tie and -1 without seeds, into int32 at nearest_ptr; if dist2_ptr is given the squared distance
        (int32); if values_ptr is given, int32 values updated in place: a voxel that is no seed and has d2 <= max_dist2 takes its
        nearest seed's value (NEAREST_VALUES_INSIDE: only where the uint8 grid is non-zero).  Strides in elements per axis x, y, z."""
        self._check(self._L.o2v_hip_nearest_dense(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level), flags, nearest_ptr,
                                                  _u64x3(nearest_strides), dist2_ptr, _u64x3(dist2_strides), values_ptr,
                                                  _u64x3(value_strides), max_dist2), "o2v_hip_nearest_dense")

    def downsample(self, grid_ptr, fmt, strides, dims, level, origin, factor, min_count, value_mode=DOWN_VALUE_MIN, colors_ptr=None,
                   color_strides=None, count_ptr=None, count_strides=None, solid_ptr=None, solid_strides=None, values_ptr=None,
                   value_strides=None, argb_ptr=None, argb_strides=None):
        """o2v_hip_downsample: the grid at device address grid_ptr (GRID_U8 / GRID_BITS / GRID_F32_BELOW with `level`), whose voxel
        (0, 0, 0) is `origin` of the fine lattice, merged in blocks of factor^3 aligned to that lattice, over the coarse box of
        downsample_box: the solid fine voxels per block (int16 at count_ptr), 1 where they are at least min_count (uint8 at
        solid_ptr), the smallest / largest non-zero byte of such a block (DOWN_VALUE_MIN / _MAX, uint8 at values_ptr, U8 grids)
        and the mean colour of its solid voxels (uint32 at argb_ptr, from the uint32 grid at colors_ptr).  At least one output;
        strides in elements per axis x, y, z."""
        self._check(self._L.o2v_hip_downsample(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level), _u32x3(origin), factor,
                                               min_count, value_mode, colors_ptr, _u64x3(color_strides), count_ptr, _u64x3(count_strides),
                                               solid_ptr, _u64x3(solid_strides), values_ptr, _u64x3(value_strides), argb_ptr,
                                               _u64x3(argb_strides)), "o2v_hip_downsample")

    def downsample_times(self):
        """o2v_hip_downsample_times: the device time (ms) of the last downsample call's launch, as a 1-tuple."""
        return self._stage_times("o2v_hip_downsample_times", 1)

    def crossings_dense(self, resolution, axes, origin, dims, dst_ptr, dst_strides, *, supersampling=1, unit_transform=None, bounds=None):
        """o2v_hip_crossings_dense: the signed crossing numbers of the context's triangles along the rays of `axes` (AXIS_X |
        AXIS_Y | AXIS_Z), from both ends of every line, at the voxel centres of the box origin + [0, dims), into int32 at device
        address dst_ptr; strides in elements, origin, dims and strides per axis x, y, z."""
        p = self._params(resolution, supersampling, 0, unit_transform, bounds, (0, 0))
        self._check(self._L.o2v_hip_crossings_dense(self._ctx, C.byref(p), int(axes), _u32x3(origin), _u32x3(dims), dst_ptr, _u64x3(dst_strides)),
                    "o2v_hip_crossings_dense")

    def crossings_times(self):
        """o2v_hip_crossings_times: the device times (ms) of the last crossings_dense call's x, y and z rays (0 for an axis not
        asked for)."""
        return self._stage_times("o2v_hip_crossings_times")

    def label_stats(self, labels_ptr, fmt, strides, dims, origin, n_labels, which, table_ptr):
        """o2v_hip_label_stats: per value 0 ... n_labels of the label grid at device address labels_ptr (LABELS_I32 / LABELS_U8;
        strides in elements, strides, dims and origin per axis x, y, z) a row of STATS_COLUMNS int64 at device address table_ptr
        ([n_labels + 1, 17], contiguous): the count, and of `which` (STATS_BOX | STATS_SUMS | STATS_MOMENTS | STATS_FACES) the
        inclusive box in global coordinates, the sums of x, y, z, of xx, yy, zz, xy, xz, yz and the exposed faces; columns not asked
        for hold 0.  Returns the number of voxels whose value is negative or above n_labels (they add to no row)."""
        outside = C.c_uint64(0)
        self._check(self._L.o2v_hip_label_stats(self._ctx, labels_ptr, fmt, _u64x3(strides), _u32x3(dims), _u32x3(origin), n_labels, which,
                                                table_ptr, C.byref(outside)), "o2v_hip_label_stats")
        return int(outside.value)

    def label_stats_times(self):
        """o2v_hip_label_stats_times: the device times (ms) of the last label_stats call's table initialisation and pass."""
        return self._stage_times("o2v_hip_label_stats_times", 2)

    def geodesic_dense(self, grid_ptr, fmt, strides, dims, level, weights, flags, seeds_ptr, n_seeds, max_distance, dist_ptr, dist_strides):
        """o2v_hip_geodesic_dense: int32 dist = the smallest sum of weights (face, edge, corner step; 0: no such step) over the
        paths inside the set from a seed (int32 [n_seeds, 3] local (x, y, z) at device address seeds_ptr; with CC_SEED_BORDER every
        voxel of the set on the box's faces too), -1 where the voxel is not in the set, not reached or further than max_distance.
        flags: CC_INVERT | CC_SEED_BORDER | FLAG_STAGE_TIMES.  Returns the number of voxels reached."""
        n = C.c_uint64(0)
        w = (C.c_uint32 * 3)(*[int(v) for v in weights])
        self._check(self._L.o2v_hip_geodesic_dense(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level), w, flags, seeds_ptr, n_seeds,
                                                   max_distance, dist_ptr, _u64x3(dist_strides), C.byref(n)), "o2v_hip_geodesic_dense")
        return int(n.value)

    def geodesic_paths(self, dist_ptr, dist_strides, dims, weights, targets_ptr, n_targets, max_len, paths_ptr, lengths_ptr):
        """o2v_hip_geodesic_paths: the walk back through a dist grid of geodesic_dense from each of the int32 [n_targets, 3]
        targets to a seed: lengths int32 [n_targets] (the voxels of the path; -1: not reached or outside the box; -2: the grid
        was not made with these weights), paths int32 [n_targets, max_len, 3], of which the first min(length, max_len) voxels of
        a row are written."""
        w = (C.c_uint32 * 3)(*[int(v) for v in weights])
        self._check(self._L.o2v_hip_geodesic_paths(self._ctx, dist_ptr, _u64x3(dist_strides), _u32x3(dims), w, targets_ptr, n_targets, max_len,
                                                   paths_ptr, lengths_ptr), "o2v_hip_geodesic_paths")

    def geodesic_scratch_bytes(self, dims, which=GEO_SCRATCH_CONTIGUOUS):
        """o2v_hip_geodesic_scratch_bytes: the context scratch a geodesic_dense call over dims (x, y, z) takes."""
        return geodesic_scratch_bytes(dims, which)

    def geodesic_times(self):
        """o2v_hip_geodesic_times: the device times (ms) of the last geodesic_dense call's classify, initialisation + seeds,
        propagation and write stages."""
        return self._stage_times("o2v_hip_geodesic_times", 4)

    def geodesic_counters(self):
        """o2v_hip_geodesic_counters: (rounds, tile visits, in-tile sweeps, host reads during the propagation) of the last
        geodesic_dense call made with FLAG_STAGE_TIMES (else zeros)."""
        out = (C.c_uint64 * 4)()
        self._check(self._L.o2v_hip_geodesic_counters(self._ctx, out), "o2v_hip_geodesic_counters")
        return tuple(int(v) for v in out)

    def thickness_dense(self, grid_ptr, fmt, strides, dims, level, flags, max_radius2, dst_ptr, dst_strides, depth2_ptr=None, depth2_strides=None):
        """o2v_hip_thickness_dense: the local thickness of the set of the grid at device pointer grid_ptr (dims, strides, fmt and
        level as components_dense takes them; THICK_BACKGROUND: its complement) as squared radii: int32 T = the largest
        min(depth2, max_radius2) over the inscribed balls that hold the voxel, 0 outside the set, into dst_ptr (THICK_F32: float32
        2 sqrt(T) - 1; THICK_OPEN_ONLY: max_radius2 inside the opening, min(depth2, max_radius2) elsewhere); if depth2_ptr is given
        the squared distance to the nearest voxel that is not in the set (THICK_BORDER: the outside of the box included) into
        int32 there.  Strides in elements per axis x, y, z."""
        self._check(self._L.o2v_hip_thickness_dense(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level), flags, max_radius2, dst_ptr,
                                                    _u64x3(dst_strides), depth2_ptr, _u64x3(depth2_strides)), "o2v_hip_thickness_dense")

    def thickness_scratch_bytes(self, dims, max_radius2, have_depth2=False):
        """o2v_hip_thickness_scratch_bytes: the context scratch a thickness_dense call over dims (x, y, z) takes."""
        return thickness_scratch_bytes(dims, max_radius2, have_depth2)

    def thickness_times(self):
        """o2v_hip_thickness_times: the device times (ms) of the last thickness_dense call's depth, opening, list, ball and
        conversion stages."""
        return self._stage_times("o2v_hip_thickness_times", 5)

    def thickness_counters(self):
        """o2v_hip_thickness_counters: (candidate centres, centres kept, ball voxels visited) of the last thickness_dense call;
        the last only with FLAG_STAGE_TIMES (else 0)."""
        out = (C.c_uint64 * 3)()
        self._check(self._L.o2v_hip_thickness_counters(self._ctx, out), "o2v_hip_thickness_counters")
        return tuple(int(v) for v in out)

    def thin_dense(self, grid_ptr, fmt, strides, dims, level, flags, mode, max_iterations, keep_ptr, keep_strides, dst_ptr, dst_strides, dst_format):
        """o2v_hip_thin_dense: the skeleton of the set of the grid at device pointer grid_ptr (dims, strides, fmt and level as
        components_dense takes them; CC_INVERT: its complement) by topological thinning - simple border voxels removed subfield by
        subfield until an iteration removes nothing, or max_iterations (if not 0) have run; THIN_CURVE keeps end points,
        THIN_ULTIMATE does not; a voxel where the uint8 grid at keep_ptr (None: no such grid) is non-zero is never removed.  Into
        the uint8 grid at dst_ptr: THIN_DST_MASK 1 / 0, THIN_DST_DEGREE 1 + the 26-neighbours in the skeleton.  dst may be the
        grid itself (uint8, the same strides).  Strides in elements per axis x, y, z."""
        self._check(self._L.o2v_hip_thin_dense(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level), flags, mode, max_iterations, keep_ptr,
                                               _u64x3(keep_strides), dst_ptr, _u64x3(dst_strides), dst_format), "o2v_hip_thin_dense")

    def thin_scratch_bytes(self, dims, have_keep=False):
        """o2v_hip_thin_scratch_bytes: the context scratch a thin_dense call over dims (x, y, z) takes."""
        return thin_scratch_bytes(dims, have_keep)

    def thin_times(self):
        """o2v_hip_thin_times: the device times (ms) of the last thin_dense call's classify, iterate and write stages."""
        return self._stage_times("o2v_hip_thin_times", 3)

    def thin_counters(self):
        """o2v_hip_thin_counters: (iterations, launches, tile turns, voxels removed) of the last thin_dense call made with
        FLAG_STAGE_TIMES (else zeros)."""
        out = (C.c_uint64 * 4)()
        self._check(self._L.o2v_hip_thin_counters(self._ctx, out), "o2v_hip_thin_counters")
        return tuple(int(v) for v in out)

    def watershed_dense(self, relief_ptr, strides, dims, connectivity, min_depth, flags, labels_ptr, labels_strides):
        """o2v_hip_watershed_dense: the parts of the int32 relief at device pointer relief_ptr - the set is where it is positive;
        every voxel climbs to its neighbour (connectivity 6, 18 or 26) of greatest key (height, linear index) until a peak, and
        peaks whose pass to a higher one is less than min_depth below them are merged into it (elder rule).  Into the int32 grid
        at labels_ptr: 0 outside the set, else 1 + the rank of the part's surviving peak in ascending index.  Strides in elements
        and dims per axis x, y, z.  Returns the number of parts."""
        n = C.c_uint32(0)
        self._check(self._L.o2v_hip_watershed_dense(self._ctx, relief_ptr, _u64x3(strides), _u32x3(dims), connectivity, min_depth, flags, labels_ptr,
                                                    _u64x3(labels_strides), C.byref(n)), "o2v_hip_watershed_dense")
        return int(n.value)

    def watershed_scratch_bytes(self, dims):
        """o2v_hip_watershed_scratch_bytes: the context scratch of a watershed_dense call over dims (x, y, z) that the box fixes."""
        return watershed_scratch_bytes(dims)

    def watershed_times(self):
        """o2v_hip_watershed_times: the times (ms) of the last watershed_dense call's ascent, flatten, pairs, merge (on the host)
        and labels stages."""
        return self._stage_times("o2v_hip_watershed_times", 5)

    def watershed_counters(self):
        """o2v_hip_watershed_counters: (peaks, boundary pairs seen, distinct adjacent basin pairs, table growths, table bytes,
        survivors) of the last watershed_dense call made with FLAG_STAGE_TIMES (else zeros)."""
        out = (C.c_uint64 * 6)()
        self._check(self._L.o2v_hip_watershed_counters(self._ctx, out), "o2v_hip_watershed_counters")
        return tuple(int(v) for v in out)

    def grow_dense(self, relief_ptr, relief_strides, markers_ptr, marker_strides, dims, weights, flags, labels_ptr, labels_strides, level_ptr=None,
                   level_strides=None, ticks_ptr=None, ticks_strides=None):
        """o2v_hip_grow_dense: the seeded watershed of the int32 relief at device pointer relief_ptr - the set is where it is
        positive - from the int32 markers at markers_ptr (a seed where both are positive), with the step weights (face, edge,
        corner; 0: no such step).  Into the int32 grids at labels_ptr, level_ptr and ticks_ptr (the last two may be None): the
        label, the level and the ticks of every voxel, 0 / 0 / -1 outside the set and where no marker reaches.  Strides in
        elements and dims per axis x, y, z.  Returns the number of voxels reached."""
        w = (C.c_uint32 * 3)(*[int(v) for v in weights])
        n = C.c_uint64(0)
        self._check(self._L.o2v_hip_grow_dense(self._ctx, relief_ptr, _u64x3(relief_strides), markers_ptr, _u64x3(marker_strides), _u32x3(dims), w, flags,
                                               labels_ptr, _u64x3(labels_strides), level_ptr, None if level_ptr is None else _u64x3(level_strides), ticks_ptr,
                                               None if ticks_ptr is None else _u64x3(ticks_strides), C.byref(n)), "o2v_hip_grow_dense")
        return int(n.value)

    def grow_scratch_bytes(self, dims, which=0):
        """o2v_hip_grow_scratch_bytes: the context scratch a grow_dense call over dims (x, y, z) takes."""
        return grow_scratch_bytes(dims, which)

    def grow_times(self):
        """o2v_hip_grow_times: the device times (ms) of the last grow_dense call's init, level rounds, sources, tick rounds,
        tight, label rounds and write stages."""
        return self._stage_times("o2v_hip_grow_times", 7)

    def grow_counters(self):
        """o2v_hip_grow_counters: (rounds, tile visits, in-tile sweeps) of the level, the ticks and the labels - nine numbers - of
        the last grow_dense call made with FLAG_STAGE_TIMES (else zeros)."""
        out = (C.c_uint64 * 9)()
        self._check(self._L.o2v_hip_grow_counters(self._ctx, out), "o2v_hip_grow_counters")
        return tuple(int(v) for v in out)

    def adjacency_count(self, labels_ptr, fmt, strides, dims, n_labels, connectivity, flags, values_ptr=None, value_strides=None):
        """o2v_hip_adjacency_count: which of the labels 1 ... n_labels (0 ... n_labels with ADJ_ZERO in flags) of the label grid at
        device address labels_ptr (LABELS_I32 / LABELS_U8; strides in elements, strides and dims per axis x, y, z) touch, at
        connectivity 6, 18 or 26; values_ptr: None or an int32 grid of the same dims at value_strides.  The sorted list stays in
        the context for adjacency_write.  Returns (pairs, outside): the number of pairs, and of voxels that are negative or above
        n_labels."""
        pairs, outside = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.o2v_hip_adjacency_count(self._ctx, labels_ptr, fmt, _u64x3(strides), _u32x3(dims), n_labels, connectivity, flags, values_ptr,
                                                    None if value_strides is None else _u64x3(value_strides), C.byref(pairs), C.byref(outside)),
                    "o2v_hip_adjacency_count")
        return int(pairs.value), int(outside.value)

    def adjacency_write(self, pairs_ptr, table_ptr, capacity):
        """o2v_hip_adjacency_write: the list of the last adjacency_count into the device arrays pairs_ptr (int32 [m, 2], sorted by
        (a, b)) and table_ptr (int64 [m, ADJ_COLUMNS]) of room for `capacity` pairs."""
        self._check(self._L.o2v_hip_adjacency_write(self._ctx, pairs_ptr, table_ptr, capacity), "o2v_hip_adjacency_write")

    def adjacency_times(self):
        """o2v_hip_adjacency_times: the times (ms) of the last adjacency_count call's table initialisation, pass, list and sort
        (on the host)."""
        return self._stage_times("o2v_hip_adjacency_times", 4)

    def adjacency_counters(self):
        """o2v_hip_adjacency_counters: (flushes into LDS, flushes to global memory, table growths, table bytes) of the last
        adjacency_count call made with FLAG_STAGE_TIMES (else zeros)."""
        out = (C.c_uint64 * 4)()
        self._check(self._L.o2v_hip_adjacency_counters(self._ctx, out), "o2v_hip_adjacency_counters")
        return tuple(int(v) for v in out)

    def adjacency_scratch_bytes(self, pairs):
        """o2v_hip_adjacency_scratch_bytes: the context scratch of the sorted list of `pairs` pairs."""
        return adjacency_scratch_bytes(pairs)

    def euler_stats(self, labels_ptr, fmt, strides, dims, n_labels, table_ptr):
        """o2v_hip_euler_stats: per value 0 ... n_labels of the label grid at device address labels_ptr (LABELS_I32 / LABELS_U8;
        strides in elements, strides and dims per axis x, y, z) a row of EULER_COLUMNS int64 at device address table_ptr
        ([n_labels + 1, 7], contiguous): its voxels, the closed-in faces, edges and vertices of the unit lattice and the inner
        ones.  Returns the number of voxels whose value is negative or above n_labels: they are in no row."""
        outside = C.c_uint64(0)
        self._check(self._L.o2v_hip_euler_stats(self._ctx, labels_ptr, fmt, _u64x3(strides), _u32x3(dims), n_labels, table_ptr, C.byref(outside)),
                    "o2v_hip_euler_stats")
        return int(outside.value)

    def euler_stats_times(self):
        """o2v_hip_euler_stats_times: the device times (ms) of the last euler_stats call's table initialisation and pass."""
        return self._stage_times("o2v_hip_euler_stats_times", 2)

    def label_surface_count(self, labels_ptr, fmt, strides, dims, flags=LABEL_SURFACE_CLOSED):
        """o2v_hip_label_surface_count: (vertices, quads) of the surface nets of the label grid at device address labels_ptr
        (LABELS_I32 / LABELS_U8; strides in elements, strides and dims per axis x, y, z); LABEL_SURFACE_CLOSED in flags: the box
        is surrounded by label 0.  What label_surface_write needs stays in the context."""
        v, q = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.o2v_hip_label_surface_count(self._ctx, labels_ptr, fmt, _u64x3(strides), _u32x3(dims), flags, C.byref(v), C.byref(q)),
                    "o2v_hip_label_surface_count")
        return v.value, q.value

    def label_surface_write(self, labels_ptr, fmt, strides, dims, flags, cells_ptr, links_ptr, vertex_capacity, faces_ptr, pairs_ptr, quad_capacity):
        """o2v_hip_label_surface_write: the net label_surface_count counted for the same grid and flags, into int32 cells
        [vertices, 3], links [vertices, 6], faces [2 quads, 3] and pairs [quads, 2] at device addresses, contiguous."""
        self._check(self._L.o2v_hip_label_surface_write(self._ctx, labels_ptr, fmt, _u64x3(strides), _u32x3(dims), flags, cells_ptr, links_ptr,
                                                        vertex_capacity, faces_ptr, pairs_ptr, quad_capacity), "o2v_hip_label_surface_write")

    def label_surface_relax(self, cells_ptr, links_ptr, n_vertices, origin, iterations, relaxation, reach, positions_ptr):
        """o2v_hip_label_surface_relax: `iterations` Jacobi steps of the net's relaxation from the cells' centres, into float32
        positions [n_vertices, 3] at a device address (voxel space; iterations 0: the centres)."""
        self._check(self._L.o2v_hip_label_surface_relax(self._ctx, cells_ptr, links_ptr, n_vertices, _u32x3(origin), iterations, float(relaxation),
                                                        float(reach), positions_ptr), "o2v_hip_label_surface_relax")

    def label_surface_times(self):
        """o2v_hip_label_surface_times: the device times (ms) of the last label_surface_count call's classify and count + scan
        stages, of the last label_surface_write call's vertex and face stages and of the last label_surface_relax call."""
        return self._stage_times("o2v_hip_label_surface_times", 5)

    def octree_build(self, grid_ptr, fmt, strides, dims, level, origin, depth=0, flags=OCT_COLLAPSE):
        """o2v_hip_octree_build: the sparse voxel octree of the set grid at device address grid_ptr (grid arguments as gather_count
        takes them) whose voxel (0, 0, 0) is `origin` of the global lattice, into the context's scratch.  depth 0: the smallest
        depth whose root cube [0, 2^depth)^3 holds the box; OCT_COLLAPSE in flags: full cells are leaves.  Returns (depth, level
        counts [depth], nodes, voxels listed); octree_write copies the arrays out."""
        d, counts, n, v = C.c_uint32(0), (C.c_uint64 * 16)(), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.o2v_hip_octree_build(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level), _u32x3(origin), depth, flags,
                                                 C.byref(d), counts, C.byref(n), C.byref(v)), "o2v_hip_octree_build")
        return d.value, tuple(int(c) for c in counts[:d.value]), n.value, v.value

    def octree_write(self, valid_ptr, full_ptr, first_child_ptr, coords_ptr=None):
        """o2v_hip_octree_write: the last octree_build's nodes into the contiguous device arrays valid, full (uint8 [nodes]),
        first_child (int32 [nodes]) and, unless None, coords (int32 [nodes, 3])."""
        self._check(self._L.o2v_hip_octree_write(self._ctx, valid_ptr, full_ptr, first_child_ptr, coords_ptr), "o2v_hip_octree_write")

    def octree_lookup(self, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags, points_ptr, n, out_ptr):
        """o2v_hip_octree_lookup: the descent through the tree in the caller's device arrays for n int32 points (x, y, z) in global
        coordinates; out int32 [n, 4] = (solid, level, node, voxel_index)."""
        self._check(self._L.o2v_hip_octree_lookup(self._ctx, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags, points_ptr, n, out_ptr),
                    "o2v_hip_octree_lookup")

    def octree_to_dense(self, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags, origin, dims, out_ptr, out_strides):
        """o2v_hip_octree_to_dense: 1 where the tree is solid and 0 elsewhere into the uint8 grid at out_ptr, the box origin + [0,
        dims) of the global lattice, which may stick out of the root cube."""
        self._check(self._L.o2v_hip_octree_to_dense(self._ctx, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags, _u32x3(origin), _u32x3(dims),
                                                    out_ptr, _u64x3(out_strides)), "o2v_hip_octree_to_dense")

    def octree_times(self):
        """o2v_hip_octree_times: the device times (ms) of the last octree_build's classify, pyramid and order stages and of the last
        octree_write."""
        return self._stage_times("o2v_hip_octree_times", 4)

    def octree_dag_build(self, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags, level_counts):
        """o2v_hip_octree_dag_build: the equal subtrees of the tree in the caller's device arrays merged, level by level, into the
        context's scratch.  level_counts: the tree's nodes per level.  Returns (classes per level [depth], nodes, pointers);
        octree_dag_write copies the arrays out."""
        counts, n, p = (C.c_uint64 * OCT_MAX_DEPTH)(), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.o2v_hip_octree_dag_build(self._ctx, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags, _level_counts(level_counts), counts,
                                                     C.byref(n), C.byref(p)), "o2v_hip_octree_dag_build")
        return tuple(int(c) for c in counts[:depth]), n.value, p.value

    def octree_dag_write(self, valid_ptr, full_ptr, first_child_ptr, child_ptr, skip_ptr=None):
        """o2v_hip_octree_dag_write: the last octree_dag_build's DAG into the contiguous device arrays valid, full (uint8 [nodes]),
        first_child (int32 [nodes]), child and, unless None, skip (int32 [pointers])."""
        self._check(self._L.o2v_hip_octree_dag_write(self._ctx, valid_ptr, full_ptr, first_child_ptr, child_ptr, skip_ptr), "o2v_hip_octree_dag_write")

    def octree_dag_lookup(self, valid_ptr, full_ptr, first_child_ptr, child_ptr, skip_ptr, n_nodes, n_pointers, depth, flags, points_ptr, n, out_ptr):
        """o2v_hip_octree_dag_lookup: the descent through the DAG in the caller's device arrays for n int32 points (x, y, z); out int32
        [n, 4] = (solid, level, node, voxel_index), voxel_index -1 where skip_ptr is None."""
        self._check(self._L.o2v_hip_octree_dag_lookup(self._ctx, valid_ptr, full_ptr, first_child_ptr, child_ptr, skip_ptr, n_nodes, n_pointers, depth, flags,
                                                      points_ptr, n, out_ptr), "o2v_hip_octree_dag_lookup")

    def octree_dag_to_dense(self, valid_ptr, full_ptr, first_child_ptr, child_ptr, n_nodes, n_pointers, depth, flags, origin, dims, out_ptr, out_strides):
        """o2v_hip_octree_dag_to_dense: 1 where the DAG is solid and 0 elsewhere into the uint8 grid at out_ptr, the box origin + [0,
        dims) of the global lattice, which may stick out of the root cube."""
        self._check(self._L.o2v_hip_octree_dag_to_dense(self._ctx, valid_ptr, full_ptr, first_child_ptr, child_ptr, n_nodes, n_pointers, depth, flags,
                                                        _u32x3(origin), _u32x3(dims), out_ptr, _u64x3(out_strides)), "o2v_hip_octree_dag_to_dense")

    def octree_dag_times(self):
        """o2v_hip_octree_dag_times: the device times (ms) of the last octree_dag_build's merge of the last level, merge of the levels
        above and output, and of the last octree_dag_write."""
        return self._stage_times("o2v_hip_octree_dag_times", 4)

    def octree_raycast(self, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags, origins_ptr, directions_ptr, n, t_max, hit_ptr, t_ptr,
                       voxel_index_ptr=None):
        """o2v_hip_octree_raycast: n rays (float32 [n, 3] origins and directions at device addresses) through the tree in the
        caller's device arrays, into int32 hit [n, 4] = (x, y, z, face), float32 t [n] and, unless None, int32 voxel_index [n]; a
        miss is (-1, -1, -1, -1), +inf, -1."""
        self._check(self._L.o2v_hip_octree_raycast(self._ctx, valid_ptr, full_ptr, first_child_ptr, n_nodes, depth, flags, origins_ptr, directions_ptr, n,
                                                   float(t_max), hit_ptr, t_ptr, voxel_index_ptr), "o2v_hip_octree_raycast")

    def octree_dag_raycast(self, valid_ptr, full_ptr, first_child_ptr, child_ptr, skip_ptr, n_nodes, n_pointers, depth, flags, origins_ptr, directions_ptr, n,
                           t_max, hit_ptr, t_ptr, voxel_index_ptr=None):
        """o2v_hip_octree_dag_raycast: the same through the DAG in the caller's device arrays; voxel_index is -1 where skip_ptr is
        None."""
        self._check(self._L.o2v_hip_octree_dag_raycast(self._ctx, valid_ptr, full_ptr, first_child_ptr, child_ptr, skip_ptr, n_nodes, n_pointers, depth, flags,
                                                       origins_ptr, directions_ptr, n, float(t_max), hit_ptr, t_ptr, voxel_index_ptr),
                    "o2v_hip_octree_dag_raycast")

    def octree_raycast_times(self):
        """o2v_hip_octree_raycast_times: the device time (ms) of the last octree_raycast or octree_dag_raycast."""
        return self._stage_times("o2v_hip_octree_raycast_times", 1)

    def openness(self, grid_ptr, fmt, strides, dims, level, directions, target_mode, target_ptr, target_strides, max_distance2, dst_ptr, dst_strides,
                 mask_ptr=None, mask_strides=None, flags=0):
        """o2v_hip_openness: per target voxel of the set grid at device address grid_ptr (grid arguments as gather_count takes them)
        the number of the directions - rows (dx, dy, dz) of ints - along which a ray from its centre leaves the box or passes
        max_distance2 (0: unlimited) before it enters a solid voxel, into the uint8 grid at dst_ptr (255: no target), and the
        directions as bits into the int64 grid at mask_ptr unless None.  target_mode: OPEN_SURFACE, OPEN_SOLID, OPEN_EMPTY, or
        OPEN_GRID with the uint8 grid at target_ptr.  Returns the number of targets."""
        rows = [tuple(int(v) for v in d) for d in directions]
        flat = (C.c_int32 * (3 * len(rows)))(*[v for d in rows for v in d])
        n = C.c_uint64(0)
        self._check(self._L.o2v_hip_openness(self._ctx, grid_ptr, fmt, _u64x3(strides), _u32x3(dims), float(level), flat, len(rows), target_mode, target_ptr,
                                             None if target_strides is None else _u64x3(target_strides), max_distance2, flags, dst_ptr, _u64x3(dst_strides),
                                             mask_ptr, None if mask_strides is None else _u64x3(mask_strides), C.byref(n)), "o2v_hip_openness")
        return n.value

    def openness_times(self):
        """o2v_hip_openness_times: the device times (ms) of the last openness call's build, targets and walk stages."""
        return self._stage_times("o2v_hip_openness_times", 3)

    def nearest_scratch_bytes(self, dims):
        """o2v_hip_nearest_scratch_bytes: the context scratch a nearest_dense call over dims (x, y, z) needs."""
        return int(self._L.o2v_hip_nearest_scratch_bytes(_u32x3(dims)))

    def nearest_times(self):
        """o2v_hip_nearest_times: the device times (ms) of the last nearest_dense call's x, y and z passes."""
        return self._stage_times("o2v_hip_nearest_times")

    def set_textures(self, textures):
        """textures: sequence of (uint8 [h, w, c] pixels, wrap) with c in (3, 4)."""
        arr = (_Texture * max(1, len(textures)))()
        keep = []
        for i, (pix, wrap) in enumerate(textures):
            pix = np.ascontiguousarray(pix, dtype=np.uint8)
            keep.append(pix)
            h, w, c = pix.shape
            arr[i] = _Texture(pix.ctypes.data, w, h, c, int(wrap))
        self._check(self._L.o2v_hip_set_textures(self._ctx, C.cast(arr, C.c_void_p), len(textures)),
                    "o2v_hip_set_textures")

    @staticmethod
    def _params(resolution, supersampling, strategy, unit_transform, bounds, zslab, flags=0, xtile=(0, 0), ytile=(0, 0),
                fill_argb=0):
        p = _Params()
        p.fill_argb = fill_argb
        p.x_begin, p.x_end = xtile
        p.y_begin, p.y_end = ytile
        p.flags = flags
        p.resolution, p.supersampling, p.strategy = resolution, supersampling, strategy
        ut = (1, 0, 0, 0, 1, 0, 0, 0, 1) if unit_transform is None else tuple(int(x) for x in np.ravel(unit_transform))
        p.unit_transform = (C.c_int32 * 9)(*ut)
        if bounds is not None:
            p.bounds_known = 1
            p.bounds = (C.c_float * 6)(*[float(x) for x in np.ravel(bounds)])
        p.z_begin, p.z_end = zslab
        return p

    def plan_slabs(self, resolution, n_slabs, *, supersampling=1, unit_transform=None, bounds=None):
        """o2v_hip_plan_slabs: (cuts, bounds) -- n_slabs+1 ascending z cuts that equalise the predicted work per slab,
        and the mesh bounds (float32 [6]) to hand back to voxelize(bounds=...)."""
        p = self._params(resolution, supersampling, 0, unit_transform, bounds, (0, 0))
        cuts = np.zeros(n_slabs + 1, dtype=np.uint32)
        bnd = np.zeros(6, dtype=np.float32)
        self._check(self._L.o2v_hip_plan_slabs(self._ctx, C.byref(p), n_slabs, _ptr(cuts), _ptr(bnd)), "o2v_hip_plan_slabs")
        return [int(z) for z in cuts], bnd

    def max_slab_layers(self, resolution, *, supersampling=1, strategy=STRATEGY_MAX, unit_transform=None, bounds=None, fill=False):
        """o2v_hip_max_slab_layers: the thickest z-slab (output layers) a voxelize call of these settings fits the device with."""
        p = self._params(resolution, supersampling, strategy, unit_transform, bounds, (0, 0), FLAG_FILL_INTERIOR if fill else 0)
        layers = C.c_uint32(0)
        self._check(self._L.o2v_hip_max_slab_layers(self._ctx, C.byref(p), C.byref(layers)), "o2v_hip_max_slab_layers")
        return layers.value

    def voxelize(self, resolution, *, supersampling=1, strategy=STRATEGY_MAX, unit_transform=None, bounds=None,
                 zslab=(0, 0), read=True, exact_clip=False, kernel_times=False, stage_times=False, xtile=(0, 0), ytile=(0, 0),
                 fill=False, fill_argb=0xFFFFFFFF):
        """xtile / ytile: an x / y range of the output grid (o2v_hip_params::x_begin ..; begin a multiple of 4), like zslab.
        fill: solid voxelization (O2V_HIP_FLAG_FILL_INTERIOR): the surface records, then the interior voxels in colour fill_argb."""
        flags = (FLAG_EXACT_CLIP if exact_clip else 0) | (FLAG_KERNEL_TIMES if kernel_times else 0) | (FLAG_STAGE_TIMES if stage_times else 0)
        if fill:
            p = self._params(resolution, supersampling, strategy, unit_transform, bounds, zslab, flags | FLAG_FILL_INTERIOR,
                             tuple(xtile), tuple(ytile), fill_argb)
        elif tuple(xtile) != (0, 0) or tuple(ytile) != (0, 0):
            p = self._params(resolution, supersampling, strategy, unit_transform, bounds, zslab, flags, tuple(xtile), tuple(ytile))
        elif unit_transform is None and bounds is None:
            # (a loop of identical calls - bench.py's timed steps - does not build the parameter block again every time)
            key = (resolution, supersampling, strategy, zslab, flags)
            if getattr(self, "_plain_key", None) != key:
                self._plain_key, self._plain_params = key, self._params(resolution, supersampling, strategy, None, None, zslab, flags)
            p = self._plain_params
        else:
            p = self._params(resolution, supersampling, strategy, unit_transform, bounds, zslab, flags)
        n = self._n_out
        self._check(self._L.o2v_hip_voxelize(self._ctx, C.byref(p), C.byref(n)), "o2v_hip_voxelize")
        self.count = n.value
        if not read:
            return self.count
        return self.read_voxels()

    def voxelize_sharded(self, comm, resolution, *, supersampling=1, strategy=STRATEGY_MAX, unit_transform=None, bounds=None,
                         read=True, stage_times=False, fill=False, fill_argb=0xFFFFFFFF):
        """o2v_hip_voxelize_sharded: collective over `comm` (a Comm); this rank voxelizes its planned z-slab (fill: and fills it).
        Returns (voxels or count of this rank, counts of all ranks, z cuts)."""
        flags = (FLAG_STAGE_TIMES if stage_times else 0) | (FLAG_FILL_INTERIOR if fill else 0)
        fill_argb = fill_argb if fill else 0
        # (a loop of identical calls - bench.py's timed steps - reuses the parameter block and the two small result arrays)
        key = (resolution, supersampling, strategy, flags, fill_argb, comm.world) if unit_transform is None and bounds is None else None
        if key is None or getattr(self, "_sharded_key", None) != key:
            self._sharded_key = key
            self._sharded_params = self._params(resolution, supersampling, strategy, unit_transform, bounds, (0, 0), flags,
                                                fill_argb=fill_argb)
            self._sharded_counts = np.zeros(comm.world, dtype=np.uint64)
            self._sharded_cuts = np.zeros(comm.world + 1, dtype=np.uint32)
            self._sharded_ptrs = (_ptr(self._sharded_counts), _ptr(self._sharded_cuts))
        p, n, counts, cuts = self._sharded_params, self._n_out, self._sharded_counts, self._sharded_cuts
        self._check(self._L.o2v_hip_voxelize_sharded(self._ctx, comm.handle, C.byref(p), C.byref(n), *self._sharded_ptrs),
                    "o2v_hip_voxelize_sharded")
        self.count = n.value
        return (self.read_voxels() if read else self.count), counts.tolist(), cuts.tolist()

    def read_voxels(self):
        out = np.empty((self.count, 4), dtype=np.uint32)
        if self.count:
            self._check(self._L.o2v_hip_read_voxels(self._ctx, _ptr(out), 0, self.count), "o2v_hip_read_voxels")
        return out

    def timings(self):
        t = Timings()
        self._L.o2v_hip_get_timings(self._ctx, C.byref(t))
        return t.as_dict()

    def kernel_times(self):
        """{kernel name: (ms, launches)} of the last voxelize(kernel_times=True) call."""
        buf = (KernelTime * 64)()
        n = C.c_uint32(0)
        self._L.o2v_hip_get_kernel_times(self._ctx, buf, 64, C.byref(n))
        return {buf[i].name.decode(): (float(buf[i].ms), int(buf[i].launches)) for i in range(min(n.value, 64))}

    def stats(self):
        s = Stats()
        self._L.o2v_hip_get_stats(self._ctx, C.byref(s))
        return s.as_dict()

    def debug_counters(self):
        out = np.zeros(16, dtype=np.uint64)
        self._L.o2v_hip_debug_counters(self._ctx, _ptr(out))
        return out

    def hits(self):
        """Every hit record of the last run (general route): uint32 array [n, 8] = cell x, y, z, keyhi, keylo, bits of w, u, v."""
        n = C.c_uint64(0)
        self._check(self._L.o2v_hip_debug_hits(self._ctx, None, 0, C.byref(n)), "o2v_hip_debug_hits")
        out = np.zeros((n.value, 8), dtype=np.uint32)
        if n.value:
            self._check(self._L.o2v_hip_debug_hits(self._ctx, _ptr(out), n.value, C.byref(n)), "o2v_hip_debug_hits")
        return out

    def check_third(self):
        """(differing inputs, first of them or None) of x / 3 against the clip loop's short form, all 2^32 float32 patterns."""
        out = np.zeros(2, dtype=np.uint64)
        self._check(self._L.o2v_hip_debug_check_third(self._ctx, _ptr(out)), "o2v_hip_debug_check_third")
        return int(out[0]), (int(out[1]) - 1 if out[0] else None)

    def check_div(self, samples=1024, seed=1):
        """256 x 256 table [numerator's biased exponent, divisor's]: pairs out of `samples` whose lean quotient differs from n / d."""
        out = np.zeros(65536, dtype=np.uint32)
        self._check(self._L.o2v_hip_debug_check_div(self._ctx, samples, seed, _ptr(out)), "o2v_hip_debug_check_div")
        return out.reshape(256, 256)

    def transform(self):
        out = np.zeros(12, dtype=np.float32)
        self._L.o2v_hip_get_transform(self._ctx, _ptr(out))
        return out


class _Callbacks(C.Structure):
    _fields_ = [("user", C.c_void_p),
                ("allreduce_min_u32", C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t)),
                ("allreduce_max_u32", C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t)),
                ("allreduce_sum_u64", C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t)),
                ("allgather", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)),
                ("broadcast", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int))]


class Comm:
    """The collectives of the sharded voxelization (include/o2v_hip.h, multi-GPU section) for one rank."""

    def __init__(self, handle, rank, world, keep=None):
        self._L = _bind()
        self.handle, self.rank, self.world, self._keep = handle, rank, world, keep

    @property
    def kind(self):
        return self._L.o2v_hip_comm_kind(self.handle).decode()

    def close(self):
        if self.handle:
            self._L.o2v_hip_comm_destroy(self.handle)
            self.handle = None

    @staticmethod
    def unique_id():
        """ncclGetUniqueId through the library: 128 bytes that rank 0 ships to every rank."""
        buf = (C.c_uint8 * 128)()
        if _bind().o2v_hip_comm_unique_id(buf) != 0:
            raise DeviceError("o2v_hip_comm_unique_id failed: librccl is not available")
        return bytes(buf)

    @classmethod
    def rccl(cls, unique_id, rank, world, device):
        """RCCL over xGMI: every rank calls this with rank 0's unique id (blocks until all have joined)."""
        h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        rc = _bind().o2v_hip_comm_create_rccl(buf, rank, world, device, C.byref(h))
        if rc != 0:
            raise DeviceError(f"o2v_hip_comm_create_rccl failed with code {rc}")
        return cls(h, rank, world)

    @classmethod
    def torch_distributed(cls, dist):
        """Host-memory collectives over an initialised torch.distributed group (gloo): for the CPU-side tests of the
        N > 1 path and for ranks that share one GPU, where RCCL cannot be used.  With the nccl backend the host
        buffers travel through device tensors (bench.py's fallback if the library's own communicator cannot be made)."""
        import torch
        rank, world = dist.get_rank(), dist.get_world_size()
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"

        def array(ptr, n, ctype):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,))

        def guarded(fn):
            # ctypes prints and swallows an exception raised inside a callback and the C side would see 0 = success: the
            # library would then plan its slabs from un-reduced data.  Any failure is reported as a failed collective.
            def wrapper(*args):
                try:
                    fn(*args)
                    return 0
                except BaseException as e:  # noqa: BLE001 - must not propagate into the C caller
                    import sys
                    print(f"obj2voxel_amd: collective callback failed: {type(e).__name__}: {e}", file=sys.stderr)
                    return 1
            return wrapper

        def allreduce(op, ctype):
            def fn(user, buf, n):
                a = array(buf, n, ctype)
                t = torch.from_numpy(a.astype(np.int64)).to(dev)  # gloo has no unsigned reductions; the values fit int64
                dist.all_reduce(t, op=op)
                a[:] = t.cpu().numpy().astype(a.dtype)
            return guarded(fn)

        @guarded
        def allgather(user, buf, bytes_per_rank):
            a = array(buf, bytes_per_rank * world, C.c_uint8)
            parts = [torch.empty(bytes_per_rank, dtype=torch.uint8, device=dev) for _ in range(world)]
            dist.all_gather(parts, torch.from_numpy(a[rank * bytes_per_rank:(rank + 1) * bytes_per_rank].copy()).to(dev))
            a[:] = torch.cat(parts).cpu().numpy()

        @guarded
        def broadcast(user, buf, n, root):
            a = array(buf, n, C.c_uint8)
            t = torch.from_numpy(a.copy()).to(dev)
            dist.broadcast(t, src=root)
            a[:] = t.cpu().numpy()

        F = dict(_Callbacks._fields_)
        cb = _Callbacks(None,
                        F["allreduce_min_u32"](allreduce(dist.ReduceOp.MIN, C.c_uint32)),
                        F["allreduce_max_u32"](allreduce(dist.ReduceOp.MAX, C.c_uint32)),
                        F["allreduce_sum_u64"](allreduce(dist.ReduceOp.SUM, C.c_uint64)),
                        F["allgather"](allgather), F["broadcast"](broadcast))
        h = C.c_void_p()
        rc = _bind().o2v_hip_comm_create_callbacks(C.byref(cb), rank, world, C.byref(h))
        if rc != 0:
            raise DeviceError(f"o2v_hip_comm_create_callbacks failed with code {rc}")
        return cls(h, rank, world, keep=cb)


class DeviceGroup:
    """o2v_hip_group: one process, one context and host thread per listed GPU, grid sharded by z-slab."""

    UPLOAD_H2D, UPLOAD_BROADCAST, UPLOAD_PEER = 0, 1, 2

    def __init__(self, devices):
        self._L = _bind()
        self._g = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        rc = self._L.o2v_hip_group_create(arr, len(devices), C.byref(self._g))
        if rc != 0:
            raise DeviceError(f"o2v_hip_group_create({list(devices)}) failed with code {rc}")
        self.size = len(devices)
        self.ranks = [DeviceVoxelizer(_borrowed_ctx=self._L.o2v_hip_group_ctx(self._g, r)) for r in range(self.size)]

    @property
    def comm_kind(self):
        return self._L.o2v_hip_group_comm_kind(self._g).decode()

    def close(self):
        if self._g:
            self._L.o2v_hip_group_destroy(self._g)
            self._g = C.c_void_p()

    def _check(self, rc, what):
        if rc != 0:
            raise DeviceError(f"{what} failed with code {rc}: {self._L.o2v_hip_group_last_error(self._g).decode()}")

    def set_triangles(self, verts, uvs=None, types=None, colors=None, texids=None, upload=0):
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
        T = verts.shape[0]
        uvs = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(T, 6)
        types = None if types is None else np.ascontiguousarray(types, dtype=np.uint32).reshape(T)
        colors = None if colors is None else np.ascontiguousarray(colors, dtype=np.float32).reshape(T, 3)
        texids = None if texids is None else np.ascontiguousarray(texids, dtype=np.int32).reshape(T)
        self._check(self._L.o2v_hip_group_set_triangles(self._g, _ptr(verts), _ptr(uvs), _ptr(types), _ptr(colors),
                                                        _ptr(texids), T, upload), "o2v_hip_group_set_triangles")

    def set_textures(self, textures):
        arr = (_Texture * max(1, len(textures)))()
        keep = []
        for i, (pix, wrap) in enumerate(textures):
            pix = np.ascontiguousarray(pix, dtype=np.uint8)
            keep.append(pix)
            h, w, c = pix.shape
            arr[i] = _Texture(pix.ctypes.data, w, h, c, int(wrap))
        self._check(self._L.o2v_hip_group_set_textures(self._g, C.cast(arr, C.c_void_p), len(textures)), "o2v_hip_group_set_textures")

    def voxelize(self, resolution, *, supersampling=1, strategy=STRATEGY_MAX, unit_transform=None, bounds=None, read=True,
                 stage_times=False, fill=False, fill_argb=0xFFFFFFFF):
        """Returns (list of per-rank voxel arrays, or the per-rank counts if read=False; z cuts).  fill: solid voxelization, every
        rank filling its own slab (DeviceVoxelizer.voxelize)."""
        flags = (FLAG_STAGE_TIMES if stage_times else 0) | (FLAG_FILL_INTERIOR if fill else 0)
        p = DeviceVoxelizer._params(resolution, supersampling, strategy, unit_transform, bounds, (0, 0), flags,
                                    fill_argb=fill_argb if fill else 0)
        counts = np.zeros(self.size, dtype=np.uint64)
        cuts = np.zeros(self.size + 1, dtype=np.uint32)
        self._check(self._L.o2v_hip_group_voxelize(self._g, C.byref(p), _ptr(counts), _ptr(cuts)), "o2v_hip_group_voxelize")
        for r, d in enumerate(self.ranks):
            d.count = int(counts[r])
        cuts = [int(z) for z in cuts]
        if not read:
            return [int(c) for c in counts], cuts
        return [d.read_voxels() for d in self.ranks], cuts
