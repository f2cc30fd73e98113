"""The streaming stages of the occupancy-only route (material-less meshes): k_bounds, the occupancy pass' k_scan_flags and
k_emit_occ.  Each test pins one part of their contract that a faster kernel could break unnoticed elsewhere:
  - the emission leaves every dirty brick of the one-byte grid zeroed and the scan leaves the flag map clear: a second call
    in the same context, on triangles whose bricks were all dirty in the first call, equals the oracle;
  - k_bounds folds the workgroups' partials and reads the tail of n_floats % 12 floats: extreme vertices there, in the last
    workgroup's range, give the oracle's transform and voxels;
  - the emission's n_out keeps counting past cap_vox: with every buffer starting tiny, the host grows the record buffer and
    re-runs, and the result equals the oracle.
"""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from obj2voxel_amd import meshes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _equal(got, want):
    got, want = meshes.sorted_voxels(got), meshes.sorted_voxels(want)
    assert got.shape == want.shape, f"voxel count {got.shape[0]} != oracle {want.shape[0]}"
    assert np.array_equal(got, want), "records differ from the oracle"


@pytest.fixture()
def dv():
    from obj2voxel_amd import hip
    d = hip.DeviceVoxelizer(0)
    yield d
    d.close()


def test_second_occupancy_call_in_dirty_bricks_equals_oracle(dv, oracle):
    """Half of a sphere's triangles after the whole sphere, in one box: every brick the second call marks was dirty in the
    first, and held voxels of the other half there.  A cell or flag left set by the first call would be an extra record."""
    v = meshes.uv_sphere(60, radius=0.9)
    bounds = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    dv.set_triangles(v)
    first = dv.voxelize(300, bounds=bounds)
    _equal(first, oracle.voxelize(v, 300, bounds=bounds))
    half = np.ascontiguousarray(v[::2])
    dv.set_triangles(half)
    second = dv.voxelize(300, bounds=bounds)
    want = oracle.voxelize(half, 300, bounds=bounds)
    assert len(want) < len(first)
    _equal(second, want)
    # and the whole sphere again: the same records as the first time
    dv.set_triangles(v)
    _equal(dv.voxelize(300, bounds=bounds), first)


@pytest.mark.parametrize("where", ["tail", "last_group"])
def test_bounds_from_the_last_floats(dv, oracle, where):
    """k_bounds: the extremes of the mesh in the last n_floats % 12 floats (the last triangle of a mesh with T % 4 == 1 -
    nine floats that no float4 triple covers), or in the last whole triple.  Enough triangles for every one of the kernel's
    workgroups to have work, so the last workgroup's range is the end of the array."""
    body = meshes.uv_sphere(300, radius=0.4)
    corner = np.array([[-0.7, -0.55, -0.6], [0.65, 0.8, 0.45], [0.65, -0.55, 0.45]], np.float32).reshape(1, 9)
    pad = (1 - len(body) - 1) % 4  # triangles that make T % 4 == 1
    v = np.concatenate([body, np.repeat(body[:1], pad, axis=0), corner]).astype(np.float32)
    assert len(v) % 4 == 1 and (len(v) * 9) % 12 == 9
    if where == "last_group":
        v = np.concatenate([v[:-2], v[-1:], v[-2:-1]])   # the extremes one triangle earlier: in the last float4 triple
    bounds = np.concatenate([v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)]).astype(np.float32)
    assert np.array_equal(bounds, np.array([-0.7, -0.55, -0.6, 0.65, 0.8, 0.45], np.float32))
    dv.set_triangles(v)
    got = dv.voxelize(256)
    assert np.array_equal(dv.transform(), oracle.mesh_transform(bounds, 256))
    _equal(got, oracle.voxelize(v, 256))


def test_tiny_record_buffer_grows_and_reruns(oracle, tmp_path):
    """Every buffer starts tiny (test hook O2V_TEST_TINY_BUFFERS), the record buffer among them: k_emit_occ writes what fits
    and counts the rest, the host grows the buffer and runs the pass again.  In a process of its own, so that the hook holds
    from the context's creation on."""
    script = textwrap.dedent("""
        import json, sys
        import numpy as np
        from obj2voxel_amd import hip, meshes
        v = meshes.uv_sphere(50)
        d = hip.DeviceVoxelizer(0)
        d.set_triangles(v)
        got = meshes.sorted_voxels(d.voxelize(256))
        passes = d.timings()["passes"]
        again = meshes.sorted_voxels(d.voxelize(256))
        d.close()
        np.save(sys.argv[1], got)
        print(json.dumps({"passes": int(passes), "again_equal": bool(np.array_equal(got, again))}))
    """)
    out = str(tmp_path / "records.npy")
    env = dict(os.environ, O2V_TEST_TINY_BUFFERS="1")
    r = subprocess.run([sys.executable, "-c", script, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["passes"] > 1 and res["again_equal"]
    v = meshes.uv_sphere(50)
    _equal(np.load(out), oracle.voxelize(v, 256))
