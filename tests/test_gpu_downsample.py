"""Downsampling (o2v_hip_downsample and obj2voxel_amd.dense.downsample) on the GPU, bit for bit against the numpy reference of
tests/downsample_ref.py.

Every case runs in a child process of its own (tests/downsample_cases.py, through tests/gpu_child.py).  The rule for the
timeouts: ten times the wall time measured for the case on the MI355X (a child's start included), with the neighbours' 30 s as
a floor.  Measured on the MI355X, inside the child (its start, 2 - 4 s for the neighbours, not included): factors
0.8 s, formats 0.3 s, strided 0.5 s, thresholds_values_colours 0.2 s, refusals 0.3 s, mesh 0.4 s.  Ten times any of these is below
the floor, so each case takes the neighbours' 30 s.
Each case prints its own wall time ("case ... took ... s")."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "downsample_cases")


def test_factors():
    out = _run("factors", timeout=30)
    print(out)
    assert "224 grids with all four outputs, 224 single outputs, 1295 origin residues" in out


def test_formats():
    out = _run("formats", timeout=30)
    print(out)
    assert "compared 112 grids as uint8, bool, bits and float32" in out


def test_strided():
    out = _run("strided", timeout=30)
    print(out)
    assert "strided: compared" in out


def test_thresholds_values_colours():
    out = _run("thresholds_values_colours", timeout=30)
    print(out)
    assert "thresholds_values_colours: compared" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=30, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    print(out)
    assert "refused 46" in out


def test_mesh():
    out = _run("mesh", timeout=30)
    print(out)
    assert "sphere at 16 supersampling 2: 1160 voxels" in out and "sphere at 21 supersampling 2: 1994 voxels" in out and "mean colours" in out
