"""The narrow-band distance to the triangles (o2v_hip_mesh_distance_dense and obj2voxel_amd.dense.mesh_distance) on the GPU,
bit for bit against the numpy reference of tests/mesh_distance_ref.py.

Every case runs in a child process of its own (tests/mesh_distance_cases.py) under `timeout -k 10`, one at a time; a child that
dies of a signal or runs out of time fails its test, and no further child is started."""
import os
import shutil
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_stopped = []


def _run(case, timeout=600, env=None):
    if _stopped:
        pytest.fail(f"not started: an earlier child ended abnormally ({_stopped[0]})")
    cmd = [sys.executable, "-m", "tests.mesh_distance_cases", case]
    if shutil.which("timeout"):
        cmd = ["timeout", "-k", "10", str(timeout)] + cmd
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout + 30)
    except subprocess.TimeoutExpired:
        _stopped.append(f"{case}: timed out")
        pytest.fail(f"case {case} timed out after {timeout} s")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _stopped.append(f"{case}: exit {r.returncode}")
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), f"case {case}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout


def test_shapes():
    assert "compared" in _run("shapes")


def test_boxes_strides_and_z_ranges():
    _run("boxes")


def test_sign_agrees_with_the_fill():
    _run("fill_agree")


def test_transform_of_voxelize():
    _run("transform")


def test_crowded_tile():
    _run("crowded", timeout=300)


def test_empty_mesh():
    _run("empty", timeout=120)


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    _run("refusals", timeout=300, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})


def test_bench_mesh_sampled():
    _run("bench_mesh", timeout=900)
