"""Blocky meshes (o2v_hip_faces_count / _write and obj2voxel_amd.dense.voxel_faces, count_faces, save_mesh) on the GPU, against the
numpy reference of tests/faces_ref.py and closed forms: np.array_equal on uint32 views of positions, faces and colours, the counts
included.

Every case runs in a child process of its own (tests/faces_cases.py, through tests/gpu_child.py).  The timeouts are three times
the wall time measured for the case on the MI355X, rounded up to the next 30 s (4.2, 2.7, 2.4, 2.2, 2.6 and
2.5 s for the six cases that were there first, in the order below; a child's start, the import of torch and the device's, is 2 s of
each).  `interleaved` has not been timed on the MI355X: five calls on two grids of 780 voxels after the child's start, so its
30 s are the neighbours' rule applied to the neighbours' 2 - 3 s."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "faces_cases")


def test_formats_and_layouts():
    out = _run("formats_and_layouts", timeout=30)
    print(out)
    assert "compared" in out


def test_long_runs():
    out = _run("long_runs", timeout=30)
    print(out)
    assert "compared 7 meshes" in out


def test_snapshot():
    out = _run("snapshot", timeout=30)
    print(out)
    assert "guard bands" in out


def test_count_above_2_32():
    out = _run("count_above_2_32", timeout=30)
    print(out)
    assert out.count("count 6442450944") == 2 and "refused:" in out and "6442450944 quads" in out


def test_pipeline():
    out = _run("pipeline", timeout=30)
    print(out)
    assert "pipeline: surface area" in out and "sphere at 96:" in out


def test_interleaved():
    out = _run("interleaved", timeout=30)
    print(out)
    assert "interleaved:" in out and "records of B compared" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=30, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    assert "ok refusals" in out
