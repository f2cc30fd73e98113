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
