"""Sparse voxel octrees (o2v_hip_octree_build / _write / _lookup / _to_dense and obj2voxel_amd.dense.build_octree with what is built
on it) on the GPU, bit for bit against the numpy reference of tests/octree_ref.py and against closed forms in Python ints.

Every case runs in a child process of its own (tests/octree_cases.py, through tests/gpu_child.py).  The rule for the timeouts: ten
times the wall time measured for the case on the MI355X (a child's start included), with the neighbours' 30 s as a floor.  MEASURED
holds the seconds inside the child on the MI355X (its start, 2 - 4 s for the neighbours, not included); the build of magnitudes on
2 146 435 072 voxels takes 2.7 ms on the device (one byte, expanded: every read is a cache hit).  Ten times any of these is below
the floor, so each case takes the neighbours' 30 s.
Each case prints its own wall time ("case ... took ... s")."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "octree_cases")

# seconds inside the child on the MI355X
MEASURED = {"shapes_and_layouts": 1.6, "block_edges": 1.1, "queries": 0.5, "determinism": 0.4, "magnitudes": 0.4, "pipeline": 2.9, "refusals": 0.3}


def _timeout(case):
    return max(30, int(10 * (MEASURED[case] + 4)))


def test_shapes_and_layouts():
    out = _run("shapes_and_layouts", timeout=_timeout("shapes_and_layouts"))
    print(out)
    assert "shapes_and_layouts: compared 1176 builds of 273 grids in 10 formats and layouts" in out


def test_block_edges():
    out = _run("block_edges", timeout=_timeout("block_edges"))
    print(out)
    assert "block_edges: random 128^3: 262144 nodes at level 6" in out and "level counts [1, 8, 32, 136, 696, 4680]" in out


def test_queries():
    out = _run("queries", timeout=_timeout("queries"))
    print(out)
    assert "queries: 16018 points looked up against the scalar descent, 30 round trips" in out


def test_determinism():
    out = _run("determinism", timeout=_timeout("determinism"))
    print(out)
    assert "determinism: 6 builds on two contexts gave equal bytes" in out


def test_magnitudes():
    out = _run("magnitudes", timeout=_timeout("magnitudes"))
    print(out)
    assert "magnitudes: 2 146 435 072 voxels, 699051 nodes, 2097152 voxels listed" in out


def test_pipeline():
    out = _run("pipeline", timeout=_timeout("pipeline"))
    print(out)
    assert "pipeline: scan_like at 128, filled:" in out and "= downsample(4, any); colours attached" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=_timeout("refusals"), env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    print(out)
    assert "refused 80 calls" in out
