"""The narrow-band distance to the triangles (o2v_hip_mesh_distance_dense and obj2voxel_amd.dense.mesh_distance) on the GPU,
bit for bit against the numpy reference of tests/mesh_distance_ref.py.

Every case runs in a child process of its own (tests/mesh_distance_cases.py, through tests/gpu_child.py)."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "mesh_distance_cases")


def test_shapes():
    assert "compared" in _run("shapes")


def test_boxes_strides_and_z_ranges():
    _run("boxes")


def test_sign_agrees_with_the_fill():
    _run("fill_agree")


def test_transform_of_voxelize():
    _run("transform")


def test_crowded_tile():
    _run("crowded", timeout=300)


def test_empty_mesh():
    _run("empty", timeout=120)


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    _run("refusals", timeout=300, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})


def test_bench_mesh_sampled():
    _run("bench_mesh", timeout=900)


# ---- at the limits the call documents ------------------------------------------------------------------------------------

def test_widest_and_odd_bands():
    out = _run("bands")
    print(out)   # (what the case covered)
    assert "compared" in out


def test_band_threshold_to_one_float32_step():
    out = _run("band_threshold")
    print(out)   # (what the case covered)
    assert "band_threshold v*" in out


def test_meshes_that_leave_the_grid():
    out = _run("cropped")
    print(out)   # (what the case covered)
    assert "compared" in out


def test_longest_box():
    out = _run("longest_box")
    print(out)   # (what the case covered)
    assert "longest_box axis 2 res 70000" in out
