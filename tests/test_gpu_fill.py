"""Solid fill (O2V_HIP_FLAG_FILL_INTERIOR) on the device, record for record: the surface part against the same call without
the flag (and once against the oracle), the interior against the numpy restatement of the parity set (tests/fill_ref.py), through
slabs, tiles, several devices, the C API and the command line."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from obj2voxel_amd import meshes
from tests import fill_ref
from tests.fill_cases import ARGB, check_fill as _check_fill, materials as _materials, power_of_two_bounds as _power_of_two_bounds

pytestmark = pytest.mark.gpu


def _torus(n_major=48, n_minor=20, R=0.7, r=0.25):
    """A closed non-convex mesh: every vertex computed once and shared by index."""
    u = 2 * np.pi * np.arange(n_major) / n_major
    v = 2 * np.pi * np.arange(n_minor) / n_minor
    P = np.empty((n_major, n_minor, 3), np.float32)
    P[..., 0] = ((R + r * np.cos(v))[None, :] * np.cos(u)[:, None])
    P[..., 1] = ((R + r * np.cos(v))[None, :] * np.sin(u)[:, None])
    P[..., 2] = (r * np.sin(v))[None, :] * np.ones(n_major)[:, None]
    tris = []
    for i in range(n_major):
        for j in range(n_minor):
            a, b = P[i, j], P[(i + 1) % n_major, j]
            c, d = P[(i + 1) % n_major, (j + 1) % n_minor], P[i, (j + 1) % n_minor]
            tris += [np.concatenate([a, b, c]), np.concatenate([a, c, d])]
    return np.array(tris, np.float32)


def _nested():
    return np.concatenate([fill_ref.weld(meshes.uv_sphere(24)), fill_ref.weld(meshes.uv_sphere(16, radius=0.45, center=(0.1, 0.05, 0.0)))])


CASES = [  # mesh, resolution, supersampling, strategy, materials
    ("cube", 16, 1, 0, "none"),
    ("sphere", 40, 2, 1, "coloured"),
    ("nested", 64, 1, 1, "textured"),
    ("torus", 96, 2, 0, "coloured"),
    ("torus", 128, 1, 0, "none"),
    ("nested", 200, 1, 0, "textured"),
    ("sphere", 1024, 1, 0, "none"),   # (user bounds 8 x the mesh: a sphere 128 voxels across)
    ("torus", 1024, 2, 1, "coloured"),
]


@pytest.mark.parametrize("mesh,res,ss,strategy,mat", CASES)
def test_fill_equals_restatement(mesh, res, ss, strategy, mat):
    from obj2voxel_amd import hip
    v = {"cube": meshes.unit_cube, "sphere": lambda: fill_ref.weld(meshes.uv_sphere(30)), "nested": _nested, "torus": _torus}[mesh]()
    kwm, tex = _materials(mat, v)
    bounds = [-8, -8, -8, 8, 8, 8] if res >= 1024 else None
    dv = hip.DeviceVoxelizer(0)
    try:
        dv.set_textures(tex)
        dv.set_triangles(v, **kwm)
        surf, filled = _check_fill(dv, v, res, ss, bounds=bounds, strategy=strategy)
        assert fill_ref.odd_edges(fill_ref.sample_vertices(v, dv.transform())) == []
        assert len(filled) > len(surf) or res <= 16
    finally:
        dv.close()


def test_surface_part_equals_oracle(oracle):
    from obj2voxel_amd import hip
    v = _nested()
    kwm, _ = _materials("coloured", v)
    dv = hip.DeviceVoxelizer(0)
    try:
        dv.set_triangles(v, **kwm)
        surf, filled = _check_fill(dv, v, 72, 2, strategy=1)
        want = oracle.voxelize(v, 72, supersampling=2, strategy=1, **kwm)
        assert np.array_equal(meshes.sorted_voxels(filled[:len(surf)]), meshes.sorted_voxels(want))
    finally:
        dv.close()


@pytest.mark.parametrize("ss", [1, 2])
def test_exact_coincidences(ss):
    """Vertices on column centres: edges and shared vertices through columns, vertical faces, horizontal faces exactly at
    layer centres."""
    from obj2voxel_amd import hip
    G, h = 48, 0.5 * ss
    dv = hip.DeviceVoxelizer(0)
    try:
        dv.set_triangles(meshes.unit_cube())
        bounds, m = _power_of_two_bounds(dv, G, ss)
        cen = lambda k: k * ss + h  # noqa: E731
        # a box with faces through centres, and an octahedron with its vertices on centres (edges along lattice diagonals)
        box = meshes.unit_cube().reshape(-1, 3).astype(np.float64)
        lo, hi = np.array([cen(5), cen(6), cen(4)]), np.array([cen(20), cen(17), cen(15)])
        box = (lo + box * (hi - lo)).reshape(-1)
        c, r = np.array([cen(33), cen(32), cen(30)]), 8 * ss
        P = [c + d for d in (np.array([r, 0, 0]), np.array([0, r, 0]), np.array([-r, 0, 0]), np.array([0, -r, 0]))]
        top, bot = c + np.array([0, 0, r]), c - np.array([0, 0, r])
        octa = []
        for k in range(4):
            a, b = P[k], P[(k + 1) % 4]
            octa += [np.concatenate([a, b, top]), np.concatenate([b, a, bot])]
        want_s = np.concatenate([box, np.concatenate(octa)]).astype(np.float64)
        v = ((want_s - 0.25) / m).astype(np.float32).reshape(-1, 9)   # (exact: a half-integer less 1/4, over a power of two)
        dv.set_triangles(v)
        _, filled = _check_fill(dv, v, G, ss, bounds=bounds)
        sv = fill_ref.sample_vertices(v, dv.transform())
        assert np.array_equal(sv.reshape(-1), want_s.astype(np.float32))
        assert fill_ref.odd_edges(sv) == []
        # no interior voxel above the top of either solid (the columns of a closed mesh close)
        for (x0, x1, y0, y1, ztop) in ((5, 20, 6, 17, 15), (33 - 8, 33 + 8, 32 - 8, 32 + 8, 30 + 8)):
            f = filled[(filled[:, 0] >= x0) & (filled[:, 0] <= x1) & (filled[:, 1] >= y0) & (filled[:, 1] <= y1)]
            assert f[:, 2].max() <= ztop
    finally:
        dv.close()


def _sorted_keys(parts, G):
    return np.sort(np.concatenate([fill_ref.keys(p, G) for p in parts]))


def test_slabs_and_tiles_equal_one_pass():
    from obj2voxel_amd import hip
    v = fill_ref.weld(meshes.uv_sphere(40))
    G = 128
    dv = hip.DeviceVoxelizer(0)
    try:
        dv.set_triangles(v)
        whole = dv.voxelize(G, fill=True, fill_argb=ARGB)
        want = fill_ref.keys(whole, G)
        cuts = [0, 30, 56, 72, 100, 128]   # [56, 72) lies inside the sphere in its middle
        slabs = [dv.voxelize(G, zslab=(a, b), fill=True, fill_argb=ARGB) for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(_sorted_keys(slabs, G), want)
        xs, ys = [0, 40, 56, 72, 128], [0, 56, 72, 128]
        tiles = [dv.voxelize(G, xtile=(x0, x1), ytile=(y0, y1), fill=True, fill_argb=ARGB)
                 for x0, x1 in zip(xs, xs[1:]) for y0, y1 in zip(ys, ys[1:])]
        assert np.array_equal(_sorted_keys(tiles, G), want)
        # a block of the interior with no surface triangle in it: filled all the same
        inner = dv.voxelize(G, xtile=(56, 72), ytile=(56, 72), zslab=(56, 72), fill=True, fill_argb=ARGB)
        assert dv.stats()["interior_voxels"] == len(inner) == 16 ** 3
        assert np.all(inner[:, 3] == ARGB)
    finally:
        dv.close()


def _capi_collect(a, capi, v, res, fill, argb=ARGB, ss=1):
    inp, out = capi.TriangleInput(v), capi.CollectingOutput()
    inst = a.obj2voxel_alloc()
    a.obj2voxel_set_input_callback(inst, inp.callback, None)
    a.obj2voxel_set_output_callback(inst, out.callback, None)
    a.obj2voxel_set_resolution(inst, res)
    a.obj2voxel_set_supersampling(inst, ss)
    if fill:
        a.o2v_set_fill(inst, 1, argb)
    assert a.obj2voxel_voxelize(inst) == 0
    a.obj2voxel_free(inst)
    return out.voxels()


def test_capi_slabs_and_long_bar_in_tiles(monkeypatch):
    from obj2voxel_amd import capi, hip
    a = capi.api()
    a.obj2voxel_set_log_level(capi.LOG_SILENT)
    C.CDLL(__import__("obj2voxel_amd").LIB_PATH).o2v_release_cached_device_memory()
    v = _torus()
    dv = hip.DeviceVoxelizer(0)
    try:
        dv.set_triangles(v)
        want = meshes.sorted_voxels(dv.voxelize(100, fill=True, fill_argb=ARGB))
        assert np.array_equal(meshes.sorted_voxels(_capi_collect(a, capi, v, 100, True)), want)
        monkeypatch.setenv("O2V_TEST_SLAB_LAYERS", "8")
        assert np.array_equal(meshes.sorted_voxels(_capi_collect(a, capi, v, 100, True)), want)
        monkeypatch.delenv("O2V_TEST_SLAB_LAYERS")
        # a thin closed bar 100 000 voxels long: x tiles of the device call, and obj2voxel_voxelize()'s own tiles
        G = 100_000
        bar = meshes.unit_cube().reshape(-1, 3) * np.array([1.0, 6e-5, 5e-5], np.float32)
        bar = bar.astype(np.float32).reshape(-1, 9)
        dv.set_triangles(bar)
        parts = [dv.voxelize(G, xtile=(0, 65532), fill=True, fill_argb=ARGB), dv.voxelize(G, xtile=(65532, G), fill=True, fill_argb=ARGB)]
        got = _sorted_keys(parts, G)
        sv = fill_ref.sample_vertices(bar, dv.transform())
        surf = _sorted_keys([p[p[:, 3] != ARGB] for p in parts], G)
        interior = np.setdiff1d(fill_ref.parity_keys(sv, G, 1), surf)
        assert len(interior) > 90_000
        assert np.array_equal(got, np.union1d(surf, interior))
        via_api = _capi_collect(a, capi, bar, G, True)
        assert np.array_equal(fill_ref.keys(via_api, G), got)
    finally:
        dv.close()
        C.CDLL(__import__("obj2voxel_amd").LIB_PATH).o2v_release_cached_device_memory()
        a.obj2voxel_set_log_level(capi.LOG_INFO)


def test_cli_fill_color_writes_vl32(tmp_path):
    import obj2voxel_amd
    from obj2voxel_amd import hip
    cli = os.path.join(os.path.dirname(obj2voxel_amd.LIB_PATH), "obj2voxel-amd")
    v = _torus(32, 12)
    stl = tmp_path / "torus.stl"
    with open(stl, "wb") as f:
        f.write(b"binary stl".ljust(80, b" ") + struct.pack("<I", len(v)))
        for t in v:
            f.write(struct.pack("<12fH", 0, 0, 0, *t.tolist(), 0))
    out = tmp_path / "out.vl32"
    r = subprocess.run([cli, str(stl), str(out), "-r", "64", "--fill-color", "%08X" % ARGB], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.frombuffer(out.read_bytes(), dtype=">u4").astype(np.uint32).reshape(-1, 4)
    dv = hip.DeviceVoxelizer(0)
    try:
        dv.set_triangles(v)
        want = dv.voxelize(64, fill=True, fill_argb=ARGB)
    finally:
        dv.close()
    assert np.array_equal(meshes.sorted_voxels(got), meshes.sorted_voxels(want))
    assert np.any(got[:, 3] == ARGB)


@pytest.mark.parametrize("n_ranks", [2, 3])
def test_group_fill_union_equals_single_device(n_ranks):
    from obj2voxel_amd import hip
    have = hip.device_count()
    devices = list(range(n_ranks)) if have >= n_ranks else [r % have for r in range(n_ranks)]
    v = _nested()
    single = hip.DeviceVoxelizer(0)
    g = hip.DeviceGroup(devices)
    try:
        single.set_triangles(v)
        want = meshes.sorted_voxels(single.voxelize(144, supersampling=2, fill=True, fill_argb=ARGB))
        g.set_triangles(v)
        parts, cuts = g.voxelize(144, supersampling=2, fill=True, fill_argb=ARGB)
        for r, p in enumerate(parts):
            assert np.all((p[:, 2] >= cuts[r]) & (p[:, 2] < cuts[r + 1]))
        assert np.array_equal(meshes.sorted_voxels(np.concatenate(parts)), want)
    finally:
        g.close()
        single.close()


def test_no_leftover_state():
    from obj2voxel_amd import hip
    v = _torus()
    dv = hip.DeviceVoxelizer(0)
    try:
        dv.set_triangles(v)
        first = meshes.sorted_voxels(dv.voxelize(90, strategy=1, fill=True, fill_argb=ARGB))
        plain = dv.voxelize(90, strategy=1)
        assert dv.stats()["interior_voxels"] == 0 and not np.any(plain[:, 3] == ARGB)
        again = meshes.sorted_voxels(dv.voxelize(90, strategy=1, fill=True, fill_argb=ARGB))
        assert np.array_equal(first, again)
        n_plain = len(plain)
        assert np.array_equal(meshes.sorted_voxels(dv.voxelize(90, strategy=1)), meshes.sorted_voxels(plain)) and len(first) > n_plain
    finally:
        dv.close()


def test_sphere_volume_at_512():
    from obj2voxel_amd import hip
    v = meshes.uv_sphere(100)
    dv = hip.DeviceVoxelizer(0)
    try:
        dv.set_triangles(v)
        n = dv.voxelize(512, fill=True, read=False)
        r = (512 - 0.5) / 2   # the mesh transform maps [-1, 1] onto [0.25, S - 0.25]
        vol = 4.0 / 3.0 * np.pi * r ** 3
        assert abs(n - vol) / vol < 0.01, (n, vol)
        assert dv.stats()["interior_voxels"] > 0.9 * vol
    finally:
        dv.close()
