"""Seeded watershed (o2v_hip_grow_dense and obj2voxel_amd.dense.seeded_watershed, grow_labels, markers_from_seeds) on the GPU,
against the numpy reference of tests/grow_ref.py: np.array_equal on int32 labels, levels and ticks, `reached` included.

Every case runs in a child process of its own (tests/grow_cases.py, through tests/gpu_child.py).  The timeouts are ten times the
wall time measured for the case on the MI355X, rounded up to the next 5 s, with a floor of 30 s (3.5, 4.5, 10.8, 4.4,
3.0 and 3.1 s in the order below; a child's start, the import of torch and the device's, is 2 s of each); most of a case's time is
the reference's."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "grow_cases")


def test_layouts():
    out = _run("layouts", timeout=40)
    print(out)
    assert "compared" in out


def test_tiles():
    out = _run("tiles", timeout=45)
    print(out)   # (the serpentines' rounds, visits and sweeps per phase, and their times)
    assert "serpentine:" in out and "saturation serpentine:" in out and "compared" in out


def test_no_tiles_ab():
    out = _run("no_tiles_ab", timeout=110, env={"O2V_GROW_NO_TILES": "1"})
    print(out)
    assert "with and without the tile pass" in out and out.count("no tiles ") >= 2 and "serpentine (no tiles):" in out


def test_flat_is_geodesic():
    out = _run("flat_is_geodesic", timeout=45)
    print(out)
    assert "pairs of grow_labels and geodesic_distance" in out


def test_pipeline():
    out = _run("pipeline", timeout=30)
    print(out)
    assert "pipeline:" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=35, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    assert "ok refusals" in out and "2147483648 voxels" in out
