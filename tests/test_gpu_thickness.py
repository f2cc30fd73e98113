"""Local thickness and ball morphology (o2v_hip_thickness_dense and obj2voxel_amd.dense.local_thickness, inner_distance, erode,
dilate, opening, closing, thin_regions) on the GPU, against the numpy reference of tests/thickness_ref.py: np.array_equal on the
int32 squared radii and depths, on the bits of the float32 thickness and on the bool grids, and the counters against the
reference's candidate and kept centres.

Every case runs in a child process of its own (tests/thickness_cases.py, through tests/gpu_child.py).  The timeouts follow the
rule of tests/test_gpu_geodesic.py: ten times the wall time measured for the case on the MI355X, rounded up to the next 5 s, with a
floor of 30 s (DESIGN.md section 24 has the measured times, in the order below; a child's start, the import of torch and the
device's, is 2 s of each); most of a case's time is the reference's."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "thickness_cases")


def test_formats_and_layouts():
    out = _run("formats_and_layouts", timeout=35)
    print(out)
    assert "compared" in out


def test_large_radii():
    out = _run("large_radii", timeout=70)
    print(out)   # (the disc's and the ball's centres and times)
    assert "disc of radius 100 at cap 2^14" in out and "ball of radius 17 at cap 400" in out


def test_many_centres():
    out = _run("many_centres", timeout=35)
    print(out)
    assert "twice the same bits" in out and "no centre listed" in out


def test_clipping():
    out = _run("clipping", timeout=30)
    print(out)
    assert "through faces, edges and corners" in out


def test_morphology():
    out = _run("morphology", timeout=40)
    print(out)
    assert "sphere at 48:" in out and "two cubes at 48:" in out


def test_pipeline():
    out = _run("pipeline", timeout=30)
    print(out)   # (the shell's thinnest and thickest value)
    assert "pipeline: a shell at 64:" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=30, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    assert "ok refusals" in out and "voxels do not fit an int32 index" in out


# ---- at the limits the call documents: block turns past 2^28 voxels, the largest box, the longest axes, a core made by the border ----
# (Each case prints what it covered.  Measured on the MI355X, DESIGN.md section 24: the four children take 2.4, 3.7, 2.8 and 3.4 s, most
# of it the child's start and the reference, so the rule above gives the floor of 30 s.  The largest box's two calls take 356 and
# 343 ms and its child 3.7 s: three times that is below the floor, which holds.)

def test_block_turns_past_2_28_voxels():
    out = _run("block_turns", timeout=30)
    print(out)   # (the voxels and block turns, the counters, the call times)
    assert "blocks 1051648 = 2^20 + 3072 in a second turn" in out and "twice the same bits" in out


def test_largest_box_next_to_2_31_voxels():
    out = _run("largest_box", timeout=30)
    print(out)   # (the counters, the largest centre index, the call times)
    assert "voxels 2146689000" in out and "largest centre index 2145023608" in out


def test_longest_axes():
    out = _run("long_axes", timeout=30)
    print(out)   # (what the case covered, per axis)
    assert all(f"taken past 2^15 along axis {a}" in out for a in "xyz")


def test_a_core_made_by_the_border_alone():
    out = _run("border_core", timeout=30)
    print(out)
    assert "the core starts at x = 64 of the row y = 64, z = 64" in out
