"""Skeletons by topological thinning (o2v_hip_thin_dense and obj2voxel_amd.dense.skeletonize, skeleton_nodes) on the GPU, against
the numpy reference of tests/thinning_ref.py: np.array_equal on the skeleton's bits and on the degree grid, the iterations and
the removed voxels included.

Every case runs in a child process of its own (tests/thinning_cases.py, through tests/gpu_child.py).  The timeouts are ten times
the wall time measured for the case on the MI355X, rounded up to the next 5 s, with a floor of 30 s (8.4, 2.6,
3.9, 3.8, 3.1, 7.3 and 3.9 s in the order below; a child's start, the import of torch and the device's, is 2 s of each); most of a
case's time is the reference's."""
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
