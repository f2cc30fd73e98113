"""Signed crossing numbers (o2v_hip_crossings_dense, obj2voxel_amd.dense.crossing_numbers and winding_fill) on the GPU, equal
with np.array_equal to the numpy reference of tests/crossings_ref.py.

Every case runs in a child process of its own (tests/crossings_cases.py, through tests/gpu_child.py).  The rule for the
timeouts: ten times the wall time measured for the case on the MI355X (a child's start included), with the neighbours' 30 s as
a floor.  Measured on the MI355X, inside the child (its start, 2 - 4 s for the neighbours, not included): axes 0.3 s, boxes
0.2 s, strided 0.2 s, exact 2.2 s, many 0.3 s, refusals 0.3 s, fill 0.7 s.  Ten times any of these is below the floor, so each
case takes the neighbours' 30 s.
Each case prints its own wall time ("case ... took ... s")."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "crossings_cases")


def test_axes():
    out = _run("axes", timeout=30)
    print(out)
    assert "axes: compared 154 grids" in out


def test_boxes():
    out = _run("boxes", timeout=30)
    print(out)
    assert "boxes: compared" in out


def test_strided():
    out = _run("strided", timeout=30)
    print(out)
    assert "strided: compared 16 outputs" in out


def test_exact():
    out = _run("exact", timeout=30)
    print(out)
    assert "exact: compared 72 grids" in out


def test_many():
    out = _run("many", timeout=30)
    print(out)
    assert "many: 66000 triangles and one large one" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=30, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    print(out)
    assert "refused 21" in out


def test_fill():
    out = _run("fill", timeout=30)
    print(out)
    assert "fill: two cubes, 33636 interior voxels, the parity rule 29540" in out and "fill: positive rule" in out
