"""Smooth meshes of label grids (o2v_hip_label_surface_count / _write / _relax and obj2voxel_amd.dense.label_surfaces with what is
built on it) on the GPU, bit for bit against the numpy reference of tests/labelmesh_ref.py - positions included -, against K10, K14
and K24 where they count the same things, and against closed forms.

Every case runs in a child process of its own (tests/labelmesh_cases.py, through tests/gpu_child.py).  The rule for the timeouts:
ten times the wall time measured for the case on the MI355X (a child's start included), with the neighbours' 30 s as a floor.
MEASURED holds the seconds inside the child on the MI355X (its start, 2 - 4 s for the neighbours, not included).  Each case prints
its own wall time ("case ... took ... s").

The limits at 2^31 - 1 vertices and triangles cannot be reached by a grid that runs in seconds; they are checked by reading the host
code (tests/labelmesh_cases.py says where)."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "labelmesh_cases")

# seconds inside the child on the MI355X
MEASURED = {"shapes_and_layouts": 0.5, "block_ends": 0.4, "against_k10": 0.4, "against_adjacency": 0.3, "invariants": 0.6, "relax": 0.4, "pipeline": 2.4,
            "refusals": 0.5}


def _timeout(case):
    return max(30, int(10 * (MEASURED[case] + 4)))


def test_shapes_and_layouts():
    out = _run("shapes_and_layouts", timeout=_timeout("shapes_and_layouts"), env={"O2V_LSF_NO_TILE": "0"})
    print(out)
    assert "shapes_and_layouts: compared 480 calls on 60 grids in 4 layouts with the tile in LDS" in out


def test_shapes_and_layouts_without_the_tile():
    out = _run("shapes_and_layouts", timeout=_timeout("shapes_and_layouts"), env={"O2V_LSF_NO_TILE": "1"})
    print(out)
    assert "shapes_and_layouts: compared 480 calls on 60 grids in 4 layouts with every row re-read through L2" in out


def test_block_ends():
    out = _run("block_ends", timeout=_timeout("block_ends"), env={"O2V_LSF_NO_TILE": "0"})
    print(out)
    assert "block_ends: compared 8 nets on 130 x 9 x 15 with the tile in LDS" in out


def test_block_ends_without_the_tile():
    out = _run("block_ends", timeout=_timeout("block_ends"), env={"O2V_LSF_NO_TILE": "1"})
    print(out)
    assert "block_ends: compared 8 nets on 130 x 9 x 15 with every row re-read through L2" in out


def test_against_k10():
    out = _run("against_k10", timeout=_timeout("against_k10"))
    print(out)
    assert "against_k10: 6 bool grids" in out


def test_against_adjacency():
    out = _run("against_adjacency", timeout=_timeout("against_adjacency"))
    print(out)
    assert "against_adjacency: 4 grids" in out


def test_invariants():
    out = _run("invariants", timeout=_timeout("invariants"))
    print(out)
    assert "invariants: 8 part meshes closed, their volumes the voxel counts" in out


def test_relax():
    out = _run("relax", timeout=_timeout("relax"))
    print(out)
    assert "relax: compared 18 settings and 2 calls with links from anywhere" in out


def test_pipeline():
    out = _run("pipeline", timeout=_timeout("pipeline"))
    print(out)
    assert "pipeline: scan_like at 64:" in out and "voxelized again" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=_timeout("refusals"), env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    print(out)
    assert "refused 65 calls" in out
