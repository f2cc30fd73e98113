"""Surface extraction (o2v_hip_surface_count / _write and obj2voxel_amd.dense.extract_surface) on the GPU, bit for bit against
the numpy reference of tests/surface_ref.py.

Every case runs in a child process of its own (tests/surface_cases.py, through tests/gpu_child.py)."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "surface_cases")


def test_shapes():
    out = _run("shapes")
    print(out)   # (what the case covered)
    assert "compared" in out


def test_strides():
    assert "compared" in _run("strides")


def test_rounding():
    assert "compared" in _run("rounding")


def test_pipeline_mesh_tsdf_mesh_voxels():
    out = _run("pipeline")
    print(out)
    assert out.count("pipeline level") == 3


def test_dense_field_and_empty():
    out = _run("dense_field", timeout=300)
    assert "dense_field vertices" in out and "ok empty" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    _run("refusals", timeout=300, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})


def test_bench_mesh_sampled():
    out = _run("bench_mesh", timeout=900)
    print(out)
    assert out.count("bench_mesh level") == 2


def test_strided_grid_in_turns():
    """More than 2^20 blocks of words: k_surf_count, k_surf_vertices and k_surf_faces take their blocks in two turns."""
    # (timeouts of the three cases below: three times their measured wall of 13.5 s, 2.1 s and 3.1 s, rounded up; a child's start,
    # the import of torch and the device's, is 2 s of each)
    out = _run("in_turns", timeout=60)
    print(out)
    assert "in_turns x stride 2:" in out and "in_turns: dims" in out and "all compared" in out


def test_vertex_limit_and_totals_above_32_bits():
    out = _run("vertex_limit", timeout=30)
    print(out)
    assert "vertex_limit: dims" in out


def test_full_blocks_and_longest_axes():
    out = _run("full_blocks", timeout=30)
    print(out)
    assert "full_blocks: dims" in out and out.count("longest axes:") == 8
