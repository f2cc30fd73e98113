"""Sparse voxel DAGs (o2v_hip_octree_dag_build / _write / _lookup / _to_dense and obj2voxel_amd.dense.octree_dag with what is built
on it) on the GPU, bit for bit against the numpy reference of tests/dag_ref.py and against closed forms.

Every case runs in a child process of its own (tests/dag_cases.py, through tests/gpu_child.py).  The rule for the timeouts is
tests/test_gpu_octree.py's: ten times the wall time measured for the case on the MI355X (a child's start included), with 30 s as
the floor.  MEASURED holds the seconds inside the child on the MI355X (its start, 2 - 4 s, not included); most of a case's time is
the numpy reference's.  Each case prints its own wall time ("case ... took ... s")."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "dag_cases")

# seconds inside the child on the MI355X
MEASURED = {"shapes_and_layouts": 1.6, "table": 0.9, "queries": 0.5, "determinism": 0.4, "pipeline": 2.0, "refusals": 0.4}


def _timeout(case):
    return max(30, int(10 * (MEASURED[case] + 4)))


def test_shapes_and_layouts():
    out = _run("shapes_and_layouts", timeout=_timeout("shapes_and_layouts"))
    print(out)
    assert "shapes_and_layouts: compared 588 DAGs of 273 grids" in out


def test_table():
    out = _run("table", timeout=_timeout("table"))
    print(out)
    assert "table: random 128^3: 299593 tree nodes, DAG level counts [1, 8, 64, 512, 4096, 32768, 25" in out
    assert "box 128^3, not collapsed: 299593 tree nodes -> level counts [1, 1, 1, 1, 1, 1, 1]" in out
    assert "two balls side by side: level counts [1, 1, 8, 32, 105, 305, 95] pointers 2290" in out


def test_queries():
    out = _run("queries", timeout=_timeout("queries"))
    print(out)
    assert "queries: 16018 points looked up against the scalar descent and the tree's, 22 boxes expanded, 4 trees that are none refused" in out


def test_determinism():
    out = _run("determinism", timeout=_timeout("determinism"))
    print(out)
    assert "determinism: 6 builds on two contexts gave equal bytes" in out


def test_pipeline():
    out = _run("pipeline", timeout=_timeout("pipeline"))
    print(out)
    assert "pipeline: scan_like at 128, filled:" in out and "colours read back through the DAG" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=_timeout("refusals"), env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    print(out)
    assert "refused 92 calls" in out
