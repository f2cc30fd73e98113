"""Watershed parts (o2v_hip_watershed_dense and obj2voxel_amd.dense.watershed, watershed_peaks, split_parts) on the GPU, against the
numpy reference of tests/watershed_ref.py: np.array_equal / torch.equal on the labels, equality of the count and of the counters.

Every case runs in a child process of its own (tests/watershed_cases.py, through tests/gpu_child.py).  The timeouts are ten times
the wall time measured for the case on the MI355X, rounded up to the next 5 s, with a floor of 30 s (3.1, 2.5,
2.1, 2.5, 3.3, 2.5, 3.8, 2.8 and 2.3 s in the order below; a child's start, the import of torch and the device's, is 2 s of each);
most of a case's time is the reference's."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "watershed_cases")


def test_formats_and_layouts():
    out = _run("formats_and_layouts", timeout=35)
    print(out)
    assert "72 calls compared with the reference" in out


def test_known_shapes():
    out = _run("known_shapes", timeout=30)
    print(out)
    assert "the pinned results" in out


def test_tile_borders():
    out = _run("tile_borders", timeout=30)
    print(out)
    assert "with and without the tile pass" in out and "staircase up:" in out and "staircase down:" in out


def test_long_chains():
    out = _run("long_chains", timeout=30)
    print(out)
    assert "ramps of 2050 voxels" in out and "ramps of 65536 voxels" in out


def test_many_peaks():
    out = _run("many_peaks", timeout=35)
    print(out)
    assert "49923 peaks in 66049 words" in out


def test_table_growth():
    out = _run("table_growth", timeout=30)
    print(out)
    assert out.count("13042 distinct pairs") == 3


def test_pipeline():
    out = _run("pipeline", timeout=40)
    print(out)
    assert out.count("pipeline:") == 2


def test_call_sequence():
    out = _run("call_sequence", timeout=30)
    print(out)
    assert "seven calls on one context" in out and out.count("call_sequence ") == 7


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=30, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    assert "ok refusals" in out and "2147483648 voxels" in out
