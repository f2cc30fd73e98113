"""Device-resident input and dense output (o2v_hip_set_triangles_device, o2v_hip_write_dense, o2v_hip_voxels_box, and the
torch layer obj2voxel_amd.dense) on the GPU.

Every case runs in a child process of its own (tests/dense_cases.py, through tests/gpu_child.py), which imports torch before
it loads the library: the device buffers come from torch."""
import functools

import pytest

from tests import gpu_child

pytestmark = pytest.mark.gpu

_run = functools.partial(gpu_child.run, "dense_cases")


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
