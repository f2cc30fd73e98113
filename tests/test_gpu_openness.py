"""Sky visibility (o2v_hip_openness and obj2voxel_amd.dense.openness, direction_set, shade_colors) on the GPU, bit for bit against
the numpy reference of tests/openness_ref.py and against closed forms, on every voxel of dst and mask.

Every case runs in a child process of its own (tests/openness_cases.py, through tests/gpu_child.py).  The rule for the timeouts is
the one of tests/test_gpu_octree.py: ten times the wall time measured for the case on the MI355X (a child's start included), with the
neighbours' 30 s as a floor.  MEASURED holds the seconds inside the child on the MI355X (its start, 2 - 4 s for the neighbours, not
included); most of a case's time is the numpy reference.  Each case prints its own wall time ("case ... took ... s")."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "openness_cases")

# seconds inside the child on the MI355X
MEASURED = {"shapes_and_formats": 2.4, "skip_equals_fine": 1.0, "closed_forms": 0.4, "determinism": 1.0, "pipeline": 3.0, "magnitudes": 0.7, "refusals": 0.4}


def _timeout(case):
    return max(30, int(10 * (MEASURED[case] + 4)))


def test_shapes_and_formats():
    out = _run("shapes_and_formats", timeout=_timeout("shapes_and_formats"))
    print(out)
    assert "shapes_and_formats: compared 144 calls on 18 grids in 8 formats and layouts, 4 direction sets, 4 target modes and 4 cut-offs" in out


def test_skip_equals_fine():
    out = _run("skip_equals_fine", timeout=_timeout("skip_equals_fine"))
    print(out)
    assert "skip_equals_fine: 4 calls with and without O2V_OPEN_NO_SKIP=1 gave equal bytes on 130x70x70 with 8 voxels; 10 of 12 64^3 blocks" in out


def test_closed_forms():
    out = _run("closed_forms", timeout=_timeout("closed_forms"))
    print(out)
    assert "closed_forms: the box's face, edge and corner (65, 121, 169 of 290)" in out


def test_determinism():
    out = _run("determinism", timeout=_timeout("determinism"))
    print(out)
    assert "determinism: 4 repeated calls on two contexts gave equal bytes; the RayCaster built before casts the same" in out


def test_pipeline():
    out = _run("pipeline", timeout=_timeout("pipeline"))
    print(out)
    assert "pipeline: scan_like at 128, filled:" in out and "gathered back with their colours" in out


def test_magnitudes():
    out = _run("magnitudes", timeout=_timeout("magnitudes"))
    print(out)
    assert "magnitudes: 20 calls at 65 536 x 2 x 2 with m = 127" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=_timeout("refusals"), env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    print(out)
    assert "refused 40 calls" in out
