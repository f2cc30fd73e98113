"""Rectangles of blocky meshes (O2V_HIP_FACES_MERGE_RECTS of o2v_hip_faces_count / _write, merge="rects" of
obj2voxel_amd.dense.voxel_faces and count_faces) on the GPU, against the numpy reference of tests/rects_ref.py and closed forms:
np.array_equal on uint32 views of positions, faces and colours, the counts included.

Every case runs in a child process of its own (tests/rects_cases.py, through tests/gpu_child.py).  The timeouts follow the rule of
tests/test_gpu_faces.py: three times the wall time measured for the case on the MI355X, rounded up to the next 30 s.  None of
the six has been timed on the MI355X yet, so each takes its neighbours' 30 s: the cases of tests/test_gpu_faces.py, of the same
shapes, take 2.2 - 4.2 s there, a child's start included."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "rects_cases")


def test_formats_and_layouts():
    out = _run("formats_and_layouts", timeout=30)
    print(out)
    assert "compared" in out and "runs stacked" in out


def test_boundaries():
    out = _run("boundaries", timeout=30)
    print(out)
    assert "compared 6 boundary grids" in out


def test_long_rects():
    out = _run("long_rects", timeout=30)
    print(out)
    assert "compared 7 meshes" in out and out.count("times") == 7


def test_snapshot():
    out = _run("snapshot", timeout=30)
    print(out)
    assert "guard bands" in out


def test_pipeline():
    out = _run("pipeline", timeout=30)
    print(out)
    assert "rectangles" in out and "sphere at 96:" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=30, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    assert "ok refusals" in out and "805306368 quads" in out
