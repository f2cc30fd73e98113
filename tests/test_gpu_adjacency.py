"""Region adjacency (o2v_hip_adjacency_count / _write and obj2voxel_amd.dense.label_adjacency with what is built on it) on the GPU,
bit for bit against the numpy reference of tests/adjacency_ref.py and against closed forms in Python ints.

Every case runs in a child process of its own (tests/adjacency_cases.py, through tests/gpu_child.py).  The rule for the timeouts:
ten times the wall time measured for the case on the MI355X (a child's start included), with the neighbours' 30 s as a floor.
MEASURED holds the seconds inside the child on the MI355X (its start, 2 - 4 s for the neighbours, not included); the call of
magnitudes on 2 145 386 496 voxels takes 42 ms on the device.  Ten times any of these is below the floor, so each case takes the
neighbours' 30 s.
Each case prints its own wall time ("case ... took ... s")."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "adjacency_cases")

# seconds inside the child on the MI355X
MEASURED = {"shapes_and_layouts": 0.9, "row_ends": 0.2, "many_pairs": 1.6, "hot_pair": 0.4, "magnitudes": 0.3, "pipeline": 2.6, "refusals": 0.3}


def _timeout(case):
    return max(30, int(10 * (MEASURED[case] + 4)))


def test_shapes_and_layouts():
    out = _run("shapes_and_layouts", timeout=_timeout("shapes_and_layouts"))
    print(out)
    assert "shapes_and_layouts: compared 624 calls on 78 grids in 5 layouts" in out


def test_row_ends():
    out = _run("row_ends", timeout=_timeout("row_ends"))
    print(out)
    assert "row_ends: compared 24 calls with the closed forms" in out


def test_many_pairs():
    out = _run("many_pairs", timeout=_timeout("many_pairs"), env={"O2V_ADJ_NO_TABLE": "0", "O2V_ADJ_TABLE_LOG2": "10"})
    print(out)
    assert "many_pairs: 394396 pairs, with the table in LDS" in out


def test_many_pairs_without_the_table():
    out = _run("many_pairs", timeout=_timeout("many_pairs"), env={"O2V_ADJ_NO_TABLE": "1", "O2V_ADJ_TABLE_LOG2": "10"})
    print(out)
    assert "many_pairs: 394396 pairs, every flush to global memory" in out


def test_hot_pair():
    out = _run("hot_pair", timeout=_timeout("hot_pair"))
    print(out)
    assert "hot_pair: 12 calls on 64^3" in out


def test_magnitudes():
    out = _run("magnitudes", timeout=_timeout("magnitudes"))
    print(out)
    assert "magnitudes: 2 145 386 496 voxels, one pair, 19273917430 contacts" in out


def test_pipeline():
    out = _run("pipeline", timeout=_timeout("pipeline"))
    print(out)
    assert "pipeline: two balls" in out and "= contacts + box sides" in out and "pipeline: a ring with a spur" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=_timeout("refusals"), env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    print(out)
    assert "refused 25 counts and 13 writes" in out
