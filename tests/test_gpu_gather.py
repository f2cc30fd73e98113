"""Dense grids as voxel lists and voxel files (o2v_hip_gather_count / _write / _save and obj2voxel_amd.dense.to_voxels,
count_voxels, save_voxels, from_voxels) on the GPU, against the numpy reference of tests/gather_ref.py and closed forms:
np.array_equal on uint32 records, the counts included.

Every case runs in a child process of its own (tests/gather_cases.py, through tests/gpu_child.py).  The timeouts are three
times the wall time measured for the case on the MI355X, rounded up to the next 30 s (3, 3, 2, 2, 2, 8 and 2 s in
the order below; a child's start, the import of torch and the device's, is 2 s of each)."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "gather_cases")


def test_formats_and_layouts():
    out = _run("formats_and_layouts", timeout=30)
    print(out)
    assert "compared" in out


def test_ranges():
    out = _run("ranges", timeout=30)
    print(out)
    assert "compared" in out and out.count(" ranges, ") == 3


def test_snapshot():
    out = _run("snapshot", timeout=30)
    print(out)
    assert "guard bands" in out


def test_above_2_32():
    out = _run("above_2_32", timeout=30)
    print(out)
    assert "count 4299161600" in out and "compared 2000 records" in out


def test_pipeline():
    out = _run("pipeline", timeout=30)
    print(out)
    assert "sphere at 96:" in out and "pipeline:" in out and "33636 enclosed" in out


def test_files():
    out = _run("files", timeout=30)
    print(out)
    assert "three batches" in out and "compared 5 formats twice" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=30, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    assert "ok refusals" in out
