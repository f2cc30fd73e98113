"""Euler numbers (o2v_hip_euler_stats and obj2voxel_amd.dense.euler_stats with what is built on it) on the GPU, bit for bit against
the numpy reference of tests/topology_ref.py and against closed forms in Python ints.

Every case runs in a child process of its own (tests/topology_cases.py, through tests/gpu_child.py).  The rule for the timeouts:
ten times the wall time measured for the case on the MI355X (a child's start included), with the neighbours' 30 s as a floor.
MEASURED holds the seconds inside the child on the MI355X (its start, 2 - 4 s for the neighbours, not included); the call of
magnitudes on 2 146 435 072 voxels takes 2.5 ms on the device (one row, expanded: every read is a cache hit).  Ten times any of
these is below the floor, so each case takes the neighbours' 30 s.
Each case prints its own wall time ("case ... took ... s")."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "topology_cases")

# seconds inside the child on the MI355X
MEASURED = {"shapes_and_layouts": 0.7, "row_ends": 0.2, "many_labels": 0.4, "hot_rows": 0.3, "magnitudes": 0.3, "pipeline": 2.9, "refusals": 0.3}


def _timeout(case):
    return max(30, int(10 * (MEASURED[case] + 4)))


def test_shapes_and_layouts():
    out = _run("shapes_and_layouts", timeout=_timeout("shapes_and_layouts"))
    print(out)
    assert "shapes_and_layouts: compared 255 calls on 51 grids in 5 layouts" in out


def test_row_ends():
    out = _run("row_ends", timeout=_timeout("row_ends"))
    print(out)
    assert "row_ends: compared 20 calls with the single-voxel row" in out


def test_many_labels():
    out = _run("many_labels", timeout=_timeout("many_labels"), env={"O2V_EU_NO_TABLE": "0"})
    print(out)
    assert "many_labels: 8 grids with the table in LDS" in out


def test_many_labels_without_the_table():
    out = _run("many_labels", timeout=_timeout("many_labels"), env={"O2V_EU_NO_TABLE": "1"})
    print(out)
    assert "many_labels: 8 grids with every row to global memory" in out


def test_hot_rows():
    out = _run("hot_rows", timeout=_timeout("hot_rows"))
    print(out)
    assert "hot_rows: 2 calls on 64^3" in out


def test_magnitudes():
    out = _run("magnitudes", timeout=_timeout("magnitudes"))
    print(out)
    assert "magnitudes: 2 146 435 072 voxels, 6449790975 closed-in edges" in out


def test_pipeline():
    out = _run("pipeline", timeout=_timeout("pipeline"))
    print(out)
    assert "pipeline: two linked tori at 64^3: betti (2, 2, 0)" in out and "= 6 voxels - 2 inner faces" in out and "pipeline: a ring with a spur" in out
    assert "pipeline: scan_like at 128, filled: betti" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=_timeout("refusals"), env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    print(out)
    assert "refused 22 calls" in out
