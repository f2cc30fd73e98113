"""Skeletons by topological thinning (o2v_hip_thin_dense and obj2voxel_amd.dense.skeletonize, skeleton_nodes) on the GPU, against
the numpy reference of tests/thinning_ref.py: np.array_equal on the skeleton's bits and on the degree grid, the iterations and
the removed voxels included.

Every case runs in a child process of its own (tests/thinning_cases.py, through tests/gpu_child.py).  The timeouts are ten times
the wall time measured for the case on the MI355X, rounded up to the next 5 s, with a floor of 30 s (8.4, 2.6,
3.9, 3.8, 3.1, 7.3 and 3.9 s for the first seven in the order below, 4.8, 4.7, 5.7, 3.0 and 4.3 s for the five that follow; a child's
start, the import of torch and the device's, is 2 s of each); most of a case's time is the reference's.

The last five are the kernels at their limits: several tiles per workgroup as the host picks them for boxes of 12 000 and 131 000
tiles, the chunk loop's second turn above 2^20 chunks (2 147 395 600 voxels; 34.6 GB of scratch and two grids of 2.1 GB, and no
skip where that memory is missing), 514 iterations, 65 536 voxels along each axis, and one context through calls of different
sizes.  Their large sets are isolated objects with a reference per object (tests/thinning_sets.py; the rule is proved on the host,
tests/test_host_thinning.py)."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "thinning_cases")


def test_formats_and_layouts():
    out = _run("formats_and_layouts", timeout=85)
    print(out)
    assert "compared with the reference" in out


def test_known_shapes():
    out = _run("known_shapes", timeout=30)
    print(out)
    assert "the pinned results" in out


def test_tile_borders():
    out = _run("tile_borders", timeout=40)
    print(out)   # (per set: the voxels, the iterations, the tile turns with and without the tile rule)
    assert "with and without the tile pass" in out and "staircase (ultimate):" in out and out.count("tile turns") >= 9


def test_keep_and_caps():
    out = _run("keep_and_caps", timeout=40)
    print(out)
    assert "max_iterations 1, 2, 3" in out


def test_degree():
    out = _run("degree", timeout=35)
    print(out)
    assert "24 end points" in out


def test_pipeline():
    out = _run("pipeline", timeout=75)
    print(out)
    assert out.count("pipeline:") == 2


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=40, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    assert "ok refusals" in out and "2147483648 voxels" in out


def test_tile_chunks():
    out = _run("tile_chunks", timeout=50)
    print(out)   # (per grid and call: tiles, chunk, chunks, objects, counters)
    assert "chunk 3 and 32, ragged, both modes" in out and out.count("chunk 3,") == 8 and out.count("chunk 32,") == 2 and "with keep on" in out


def test_grid_turns():
    out = _run("grid_turns", timeout=50)
    print(out)
    assert out.count("139 second-turn chunks") == 2 and out.count("1048715 chunks on 1048576 workgroups") == 2


def test_long_runs():
    out = _run("long_runs", timeout=60)
    print(out)
    assert "[[1025, 1, 1]] (x, y, z) in 514 iterations, 2049 removed" in out and out.count("514 iterations") == 3 and "[[36, 36, 36]] (x, y, z) in 19 iterations" in out


def test_long_axes():
    out = _run("long_axes", timeout=30)
    print(out)
    assert out.count("ultimate leaves [20, 32767, 65472, 65516] in 11 iterations, 134 removed") == 3


def test_call_sequence():
    out = _run("call_sequence", timeout=45)
    print(out)
    assert "six calls on one context" in out and out.count("call_sequence ") == 6
