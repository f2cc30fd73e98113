"""Per-label statistics (o2v_hip_label_stats and obj2voxel_amd.dense.label_stats with what is built on it) on the GPU, bit for bit
against the numpy reference of tests/label_stats_ref.py and against closed forms in Python ints.

Every case runs in a child process of its own (tests/label_stats_cases.py, through tests/gpu_child.py).  The rule for the
timeouts: ten times the wall time measured for the case on the MI355X (a child's start included), with the neighbours' 30 s as
a floor.  Measured on the MI355X, inside the child (its start, 2 - 4 s for the neighbours, not included): shapes_and_layouts
0.8 s, many_labels 0.4 s (either way), out_of_range 0.5 s, magnitudes 0.3 s (the call on 2 146 435 072 voxels: 2.2 ms on the
device), faces 0.4 s, pipeline 1.9 s, refusals 0.3 s.  Ten times any of these is below the floor, so each case takes the
neighbours' 30 s.
Each case prints its own wall time ("case ... took ... s")."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "label_stats_cases")

# seconds inside the child on the MI355X
MEASURED = {"shapes_and_layouts": 0.8, "many_labels": 0.4, "out_of_range": 0.5, "magnitudes": 0.3, "faces": 0.4, "pipeline": 1.9, "refusals": 0.3}


def _timeout(case):
    return max(30, int(10 * (MEASURED[case] + 4)))


def test_shapes_and_layouts():
    out = _run("shapes_and_layouts", timeout=_timeout("shapes_and_layouts"))
    print(out)
    assert "shapes_and_layouts: compared 918 calls on 54 grids in 7 layouts" in out


def test_many_labels():
    out = _run("many_labels", timeout=_timeout("many_labels"), env={"O2V_LS_NO_TABLE": "0"})
    print(out)
    assert "many_labels: 6 grids with the table in LDS" in out


def test_many_labels_without_the_table():
    out = _run("many_labels", timeout=_timeout("many_labels"), env={"O2V_LS_NO_TABLE": "1"})
    print(out)
    assert "many_labels: 6 grids with every run to global memory" in out


def test_out_of_range():
    out = _run("out_of_range", timeout=_timeout("out_of_range"))
    print(out)
    assert "out_of_range: compared 16 calls" in out


def test_magnitudes():
    out = _run("magnitudes", timeout=_timeout("magnitudes"))
    print(out)
    assert "magnitudes: 2 146 435 072 voxels" in out


def test_faces():
    out = _run("faces", timeout=_timeout("faces"))
    print(out)
    assert "faces: compared 14 0 / 1 grids with count_faces" in out and "faces: connectivity 26" in out


def test_pipeline():
    out = _run("pipeline", timeout=_timeout("pipeline"))
    print(out)
    assert "33636 interior voxels" in out and "pipeline: scan_like at 256" in out and "pipeline: random grid" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=_timeout("refusals"), env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    print(out)
    assert "refused 26" in out
