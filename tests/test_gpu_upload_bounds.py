"""Occupancy-only route: the bounds of a pass are the upload's (ctx->mesh_bounds_hint, valid for the triangles of that upload)
and its transform is computed on the host and handed to the kernels as an argument - neither k_bounds nor k_setup is launched
(o2v_device.hip: host_transform, host_k0).  The results must be what they were: the oracle's records, its transform bit for
bit, and the records and transform of a process that runs both launches (O2V_ALL_LAUNCHES=1)."""
import os

import numpy as np
import pytest

from obj2voxel_amd import meshes
from tests import gpu_child, upload_bounds_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shortcut():
    """the compared calls in this process: with the shortcut"""
    assert os.environ.get("O2V_ALL_LAUNCHES") != "1"
    return cases.ab_calls()


@pytest.fixture(scope="module")
def all_launches(tmp_path_factory):
    """the same calls in a child process with O2V_ALL_LAUNCHES=1"""
    out = str(tmp_path_factory.mktemp("upload_bounds") / "ab.npz")
    gpu_child.run("upload_bounds_cases", "ab", timeout=300, env={"O2V_ALL_LAUNCHES": "1", "O2V_TEST_UPLOAD_BOUNDS_OUT": out})
    with np.load(out) as f:
        return cases.unpack(f)


@pytest.mark.parametrize("res", [128, 256])
@pytest.mark.parametrize("unit", [None, cases.PERMUTE], ids=["identity", "permuted"])
def test_shortcut_taken(oracle, shortcut, res, unit):
    v = cases.sphere()
    xf, vox, kernels, rc = shortcut[f"sphere_{res}" + ("" if unit is None else "_permuted")]
    assert rc == 0
    assert "k_bounds" not in kernels and "k_setup" not in kernels and "k_voxelize_occ" in kernels, kernels
    want = meshes.sorted_voxels(oracle.voxelize(v, res, unit_transform=unit))
    assert vox.shape == want.shape and np.array_equal(vox, want)
    want_xf = oracle.mesh_transform(cases.bounds_of(v), res, unit)
    assert np.array_equal(xf.view(np.uint32), want_xf.view(np.uint32)), (xf, want_xf)


def test_same_as_with_both_launches(shortcut, all_launches):
    """host transform against device transform, bit for bit, and the records behind them: the sphere's calls and the awkward
    boxes (far from the origin, flat, a longest axis that is no power of two at resolution 300)"""
    assert sorted(shortcut) == sorted(all_launches)
    for name in sorted(shortcut):
        if name == "nan":
            continue
        xf_a, vox_a, kernels_a, rc_a = shortcut[name]
        xf_b, vox_b, kernels_b, rc_b = all_launches[name]
        assert rc_a == 0 and rc_b == 0, name
        assert "k_bounds" in kernels_b and "k_setup" in kernels_b, (name, kernels_b)
        assert "k_bounds" not in kernels_a and "k_setup" not in kernels_a, (name, kernels_a)
        differ = np.flatnonzero(xf_a.view(np.uint32) != xf_b.view(np.uint32))
        assert differ.size == 0, (name, differ, xf_a, xf_b)
        assert len(vox_a) > 0 and vox_a.shape == vox_b.shape and np.array_equal(vox_a, vox_b), name


def test_bounds_follow_the_upload(oracle):
    from obj2voxel_amd import hip
    d = hip.DeviceVoxelizer(0)
    try:
        for i, m in enumerate(cases.follow_meshes()):
            d.set_triangles(m)
            got = meshes.sorted_voxels(d.voxelize(128, kernel_times=True))
            assert "k_bounds" not in d.kernel_times() and "k_voxelize_occ" in d.kernel_times(), d.kernel_times()
            xf = d.transform()
            assert np.array_equal(xf, oracle.mesh_transform(cases.bounds_of(m), 128)), i
            assert np.array_equal(got, meshes.sorted_voxels(oracle.voxelize(m, 128))), i
    finally:
        d.close()


def test_bounds_follow_a_device_resident_upload():
    pytest.importorskip("torch")
    gpu_child.run("upload_bounds_cases", "device_upload", timeout=300)


def test_callers_bounds_win(oracle):
    from obj2voxel_amd import hip
    v = meshes.uv_sphere(60, radius=0.9)
    bounds = [-1, -1, -1, 1, 1, 1]
    d = hip.DeviceVoxelizer(0)
    try:
        d.set_triangles(v)
        got = meshes.sorted_voxels(d.voxelize(256, bounds=bounds, kernel_times=True))
        kernels = d.kernel_times()
        xf = d.transform()
    finally:
        d.close()
    assert "k_bounds" not in kernels and "k_voxelize_occ" in kernels, kernels
    assert np.array_equal(xf, oracle.mesh_transform(bounds, 256))
    assert np.array_equal(got, meshes.sorted_voxels(oracle.voxelize(v, 256, bounds=bounds)))


def test_coloured_mesh_keeps_its_launches():
    from obj2voxel_amd import hip
    v = meshes.uv_sphere(30)
    d = hip.DeviceVoxelizer(0)
    try:
        d.set_triangles(v, types=np.full(len(v), hip.TRI_UNTEXTURED, np.uint32), colors=meshes.triangle_colors(len(v)))
        d.voxelize(128, read=False, kernel_times=True)
        kernels = d.kernel_times()
    finally:
        d.close()
    assert "k_bounds" in kernels and "k_setup" in kernels, kernels


def test_nan_vertex_same_as_with_both_launches(shortcut, all_launches):
    xf_a, vox_a, _, rc_a = shortcut["nan"]
    xf_b, vox_b, _, rc_b = all_launches["nan"]
    assert rc_a == rc_b
    assert vox_a.shape == vox_b.shape and np.array_equal(vox_a, vox_b)
    assert np.array_equal(xf_a.view(np.uint32), xf_b.view(np.uint32))


def test_zslab_call(oracle):
    from obj2voxel_amd import hip
    v = cases.sphere()
    d = hip.DeviceVoxelizer(0)
    try:
        d.set_triangles(v)
        got = meshes.sorted_voxels(d.voxelize(256, zslab=(64, 128), kernel_times=True))
        kernels = d.kernel_times()
    finally:
        d.close()
    assert "k_bounds" not in kernels and "k_setup" not in kernels, kernels
    want = meshes.sorted_voxels(oracle.voxelize(v, 256))
    want = want[(want[:, 2] >= 64) & (want[:, 2] < 128)]
    assert len(want) > 0 and got.shape == want.shape and np.array_equal(got, want)
