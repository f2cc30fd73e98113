"""Device-resident input and dense output (o2v_hip_set_triangles_device, o2v_hip_write_dense, o2v_hip_voxels_box, and the
torch layer obj2voxel_amd.dense) on the GPU.

Every case runs in a child process of its own (tests/dense_cases.py), which imports torch before it loads the library: the
device buffers come from torch, and an earlier test module of this pytest process may have loaded the library already.  One
child at a time; a child that dies of a signal or runs out of time fails its test, and no further child is started."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_stopped = []


def _run(case, timeout=600, env=None):
    if _stopped:
        pytest.fail(f"not started: an earlier child ended abnormally ({_stopped[0]})")
    full_env = dict(os.environ, **(env or {}))
    try:
        r = subprocess.run([sys.executable, "-m", "tests.dense_cases", case], cwd=ROOT, env=full_env, capture_output=True,
                           text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _stopped.append(f"{case}: timed out")
        pytest.fail(f"case {case} timed out after {timeout} s")
    if r.returncode < 0:
        _stopped.append(f"{case}: signal {-r.returncode}")
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), f"case {case}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout


def test_device_upload_equals_host_upload():
    out = _run("upload")
    assert "compared 60" in out, out


def test_face_index_out_of_range_is_refused():
    _run("bad_index")


def test_pointer_checks():
    _run("pointers", env={"PYTORCH_NO_HIP_MEMORY_CACHING": "1", "PYTORCH_NO_CUDA_MEMORY_CACHING": "1"})


def test_write_dense_equals_numpy_scatter():
    _run("write_dense")


def test_voxels_box():
    _run("voxels_box")


def test_torch_layer():
    _run("torch")


def test_torch_layer_refuses_library_loaded_first():
    _run("lib_first", timeout=300)
