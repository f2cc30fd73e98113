"""Ray casting (o2v_hip_raycast_build / o2v_hip_raycast and obj2voxel_amd.dense.RayCaster) on the GPU, bit for bit against the
numpy reference of tests/raycast_ref.py: every hit as int32, every t as the bits of its float32.

Every case runs in a child process of its own (tests/raycast_cases.py, through tests/gpu_child.py).  The timeouts are three
times the wall time measured for the case on the MI355X, rounded up to the next 30 s (36, 55, 15, 3, 6
and 4 s in the order below; a child's start, the import of torch and the device's, is 2 s of each); most of a case's time is
the reference's, which walks every cell."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "raycast_cases")


def test_formats_and_shapes():
    out = _run("formats_and_shapes", timeout=120)
    print(out)   # (what the case covered: per grid the rays, the shares that hit and miss, the reference's fine steps)
    assert "compared" in out and out.count(" rays, hit ") == 13


def test_no_skip_ab():
    out = _run("no_skip_ab", timeout=180)
    print(out)
    assert "compared" in out and out.count("walking every cell") == 13


def test_extremes():
    out = _run("extremes", timeout=60)
    print(out)
    assert "single voxel:" in out and "checkerboard:" in out and "empty:" in out and "full:" in out


def test_snapshot():
    out = _run("snapshot", timeout=30)
    print(out)
    assert "compared" in out


def test_pipeline():
    out = _run("pipeline", timeout=30)
    print(out)
    assert "pipeline:" in out and "depth image:" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=30, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    assert "ok refusals" in out and "no o2v_hip_raycast_build" in out
