"""Rays through sparse voxel octrees and DAGs (o2v_hip_octree_raycast / o2v_hip_octree_dag_raycast and obj2voxel_amd.dense's
octree_raycast and dag_raycast) on the GPU, bit for bit against the numpy reference of tests/treeray_ref.py and against RayCaster.

Every case runs in a child process of its own (tests/treeray_cases.py, through tests/gpu_child.py).  The reference's walk over a grid
of the cases `shapes` and `stack_ab` is made once, here, and handed to the children through a directory (treeray_ref.scene); it is
the one tests/test_host_treeray.py uses, so a run of both modules makes it once.  The rule for the timeouts is
tests/test_gpu_dag.py's: ten times the wall time measured for the case on the MI355X (a child's start included), with 30 s as the
floor.  MEASURED holds the seconds inside the child on the MI355X (its start, 2 - 4 s, not included), for the cases of one grid the
longest of them.  Each case prints its own wall time ("case ... took ... s")."""
import functools

import pytest

from tests import gpu_child
from tests import treeray_ref as TR

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "treeray_cases")

# seconds inside the child on the MI355X
MEASURED = {"shapes": 0.4, "stack_ab": 0.5, "extremes": 0.4, "against_raycaster": 0.6, "not_a_tree": 1.5, "pipeline": 2.2, "determinism": 0.3, "refusals": 0.3}

GRIDS = range(len(TR.grids()))


def _timeout(case):
    return max(30, int(10 * (MEASURED[case] + 4)))


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """the directory the children find the reference's walks in; scene(k) puts grid k's there"""
    return {TR.SCENES_ENV: str(tmp_path_factory.mktemp("treeray_scenes"))}


def _scene(monkeypatch, scenes, k):
    monkeypatch.setenv(TR.SCENES_ENV, scenes[TR.SCENES_ENV])
    return TR.scene(k)[0]   # (made, or taken from an earlier module of this run, and put into the directory)


@pytest.mark.parametrize("k", GRIDS)
def test_shapes(monkeypatch, scenes, k):
    name = _scene(monkeypatch, scenes, k)
    out = _run("shapes:%d" % k, timeout=_timeout("shapes"), env=scenes)
    print(out)
    assert "shapes[%d]: %s, depth" % (k, name) in out and "casts of 4518 rays as tree and DAG, collapsed and not" in out


@pytest.mark.parametrize("k", GRIDS)
def test_stack_ab(monkeypatch, scenes, k):
    name = _scene(monkeypatch, scenes, k)
    out = _run("stack_ab:%d" % k, timeout=_timeout("stack_ab"), env=scenes)
    print(out)
    assert "stack_ab[%d]: %s: 16 casts with and without O2V_TREERAY_NO_STACK=1 gave the reference's bits" % (k, name) in out


def test_extremes():
    out = _run("extremes", timeout=_timeout("extremes"))
    print(out)
    assert "extremes: 12 casts of 4000 rays" in out


def test_against_raycaster():
    out = _run("against_raycaster", timeout=_timeout("against_raycaster"))
    print(out)
    assert "against_raycaster: 24 casts of" in out and "gave RayCaster's bits on 6 grids" in out


def test_not_a_tree():
    out = _run("not_a_tree", timeout=_timeout("not_a_tree"))
    print(out)
    assert "not_a_tree: 88 casts through 44 sets of arrays that are no tree gave the reference's bits" in out


def test_pipeline():
    out = _run("pipeline", timeout=_timeout("pipeline"))
    print(out)
    assert "pipeline: scan_like at 128, filled: a 128 x 128 image," in out and "every pixel's colour through the slot" in out


def test_determinism():
    out = _run("determinism", timeout=_timeout("determinism"))
    print(out)
    assert "determinism: 6 casts on two contexts gave equal bytes" in out


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    out = _run("refusals", timeout=_timeout("refusals"), env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})
    print(out)
    assert "refused 91 calls, a correct cast behind each" in out
