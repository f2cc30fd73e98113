"""Geodesic distances and shortest paths (o2v_hip_geodesic_dense / o2v_hip_geodesic_paths and obj2voxel_amd.dense.geodesic_distance,
shortest_paths) on the GPU, against the numpy reference of tests/geodesic_ref.py: np.array_equal on int32 distances, paths and
lengths, `reached` included.

Every case runs in a child process of its own (tests/geodesic_cases.py, through tests/gpu_child.py).  The timeouts are ten times
the wall time measured for the case on the MI355X, rounded up to the next 5 s, with a floor of 30 s (4.7, 3.7,
7.5, 3.6, 3.2, 2.6 and 3.1 s in the order below; a child's start, the import of torch and the device's, is 2 s of each); most of a
case's time is the reference's."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "geodesic_cases")


def test_formats_and_layouts():
    out = _run("formats_and_layouts", timeout=50)
    print(out)
    assert "compared" in out


def test_tiles():
    out = _run("tiles", timeout=40)
    print(out)   # (the corridor's rounds, visits and sweeps; the serpentine's times)
    assert "u corridor:" in out and "serpentine (1, 0, 0):" in out and "compared" in out


def test_no_tiles_ab():
    out = _run("no_tiles_ab", timeout=75, env={"O2V_GEO_NO_TILES": "1"})
    print(out)
    assert "with and without the tile pass" in out and out.count("no tiles ") >= 3 and "u corridor (no tiles):" in out


def test_max_distance():
    out = _run("max_distance", timeout=40)
    print(out)
    assert "a cap of 2^31 - 1 is refused" in out


def test_paths():
    out = _run("paths", timeout=35)
    print(out)
    assert "sets of paths" in out and "serpentine:" in out


def test_pipeline():
    out = _run("pipeline", timeout=30)
    print(out)
    assert "pipeline:" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=35, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    assert "ok refusals" in out and "2147483648 voxels" in out
