"""The distance transform (o2v_hip_distance_dense and obj2voxel_amd.dense's distance_transform / voxelize_dense fmt="dist2"
and "sdf") on the GPU, bit for bit against the numpy references of tests/distance_ref.py.

Every case runs in a child process of its own (tests/distance_cases.py) under `timeout -k 10`, one at a time; a child that
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
    cmd = [sys.executable, "-m", "tests.distance_cases", case]
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


def test_random_label_grids():
    assert "compared" in _run("random")


def test_strided_labels_and_out():
    _run("strided")


def test_corner_seed_plane():
    _run("corner")


def test_refusals():
    # (torch's caching allocator off: each tensor is an allocation of its own, so a short one is short)
    _run("refusals", timeout=300, env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})


def test_voxelize_dense_sdf_of_closed_meshes():
    _run("mesh")


def test_bench_mesh_sampled_brute_force():
    _run("bench_mesh")
