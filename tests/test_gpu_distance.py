"""The distance transform (o2v_hip_distance_dense and obj2voxel_amd.dense's distance_transform / voxelize_dense fmt="dist2"
and "sdf") on the GPU, bit for bit against the numpy references of tests/distance_ref.py.

Every case runs in a child process of its own (tests/distance_cases.py, through tests/gpu_child.py)."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "distance_cases")


def test_random_label_grids():
    assert "compared" in _run("random")


def test_strided_labels_and_out():
    _run("strided")


def test_corner_seed_plane():
    _run("corner")


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    _run("refusals", timeout=300, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})


def test_voxelize_dense_sdf_of_closed_meshes():
    _run("mesh")


def test_bench_mesh_sampled_brute_force():
    _run("bench_mesh")


# ---- at the limits the call documents: more lines than lanes, the longest lines, the largest value, the deepest stacks ----

def test_more_lines_than_lanes():
    out = _run("lane_cap")
    print(out)   # (what the case covered)
    assert "lane_cap permuted" in out


def test_longest_lines():
    out = _run("long_lines")
    print(out)   # (what the case covered)
    assert "entries from the scratch" in out


def test_value_limit():
    out = _run("value_limit")
    print(out)   # (what the case covered)
    assert "value_limit" in out


def test_deep_stacks_and_long_pop_runs():
    out = _run("deep_stacks")
    print(out)   # (what the case covered)
    assert "deep_stacks" in out
