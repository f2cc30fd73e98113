"""The nearest-voxel transform (o2v_hip_nearest_dense and obj2voxel_amd.dense's nearest_voxel / spread_colors) on the GPU, bit
for bit against the numpy references of tests/nearest_ref.py.

Every case runs in a child process of its own (tests/nearest_cases.py, through tests/gpu_child.py)."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "nearest_cases")


def test_random_seed_grids():
    assert "compared" in _run("random")


def test_ties_take_the_smallest_index():
    out = _run("ties")
    print(out)   # (the share of voxels with more than one nearest seed, per grid)
    assert "lattice share" in out


def test_seed_formats_agree():
    assert "formats" in _run("formats")


def test_strided_seeds_and_outputs():
    _run("strided")


def test_values_in_place_inside_only_and_max_distance():
    out = _run("values")
    print(out)   # (the voxels at each distance limit and one past it)
    assert "max_distance 4.5 max_dist2 20" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=300, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    assert "refused" in out


def test_interior_of_a_mesh_takes_the_nearest_surface_colour():
    assert "mesh: torus" in _run("mesh")


# ---- at the limits the call documents: more lines than lanes, the longest lines, the deepest stacks, the largest box -------------------------

def test_more_lines_than_lanes():
    out = _run("lane_cap")
    print(out)   # (what the case covered)
    assert "y lines without a payload" in out


def test_longest_lines():
    out = _run("long_lines")
    print(out)   # (what the case covered)
    assert "taken past 2^15 along axis x" in out and "axis y" in out and "axis z" in out


def test_deep_stacks_and_long_pop_runs():
    out = _run("deep_stacks")
    print(out)   # (what the case covered)
    assert "deep_stacks" in out


def test_largest_box_next_to_2_31_voxels():
    out = _run("largest_box")
    print(out)   # (what the case covered)
    assert "largest index 2146688999" in out
