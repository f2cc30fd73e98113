"""Connected components and flood fill (o2v_hip_components_dense / o2v_hip_flood_dense and obj2voxel_amd.dense.components, flood,
exterior, solidify, remove_small) on the GPU, against the numpy reference of tests/components_ref.py: np.array_equal on int32
labels and uint8 floods, the counts included.

Every case runs in a child process of its own (tests/components_cases.py, through tests/gpu_child.py).  The timeouts are three
times the wall time measured for the case on the MI355X, rounded up to the next 30 s (4, 11, 12, 6, 6, 18 and 3 s in the
order below; a child's start, the import of torch and the device's, is 2 s of each); most of a case's time is the reference's."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "components_cases")


def test_formats_and_layouts():
    out = _run("formats_and_layouts", timeout=30)
    print(out)
    assert "compared" in out


def test_connectivity_and_polarity():
    out = _run("connectivity_and_polarity", timeout=60)
    print(out)   # (per set: the components, the reference's time, the stage times)
    assert "compared" in out and out.count(" components, reference ") == 24


def test_no_tiles_ab():
    out = _run("no_tiles_ab", timeout=60, env={"O2V_CC_NO_TILES": "1"})
    print(out)
    assert "with and without the tile pass" in out and out.count("no tiles ") == 24


def test_extremes():
    out = _run("extremes", timeout=30)
    print(out)
    assert "single voxel:" in out and "checkerboard:" in out and "serpentine (no tiles):" in out and "comb:" in out


def test_flood():
    out = _run("flood", timeout=30)
    print(out)
    assert "compared" in out


def test_pipeline():
    out = _run("pipeline", timeout=60)
    print(out)
    assert "pipeline:" in out and "sphere at 256:" in out and "scan_like at 512:" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=30, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    assert "ok refusals" in out and "2147483648 voxels" in out
