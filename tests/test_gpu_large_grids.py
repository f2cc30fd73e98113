"""Grids whose pass boxes reach the limit of the 16-bit coordinate fields, through the drop-in C API, the device C-ABI and
groups of devices.

The reference takes any uint32 resolution (u32 coordinates, 64-bit Morton keys: src/util.hpp:185-196).  Here voxel
coordinates and leaf extents travel in 16-bit fields relative to the box of one pass (Params::so, Leaf::bmin_xy / bmin_z_dx
/ dy_dz, the job records of k_voxelize), so a pass' box may be at most 65 535 samples wide along each axis, and
obj2voxel_voxelize() cuts a finer grid into x / y tiles and z-slabs.  These tests fill those fields to their limit (a pass
box of exactly 65 535 samples, a single leaf spanning a whole pass box, a last tile of 1 - 4 voxels), check that a box one
sample wider is refused rather than wrapped, and voxelize meshes that are long in z (a pole at a sample resolution above
65 535) on one device and on several.  Every comparison with the oracle is record for record."""
import ctypes as C
import time

import numpy as np
import pytest

from obj2voxel_amd import meshes

pytestmark = pytest.mark.gpu

PIX = meshes.checker_texture(64, 8)


def _devices(n):
    from obj2voxel_amd import hip
    have = hip.device_count()
    return list(range(n)) if have >= n else [r % have for r in range(n)]


def _release():
    # (grids of tens of GB: give them back before the next test)
    C.CDLL(__import__("obj2voxel_amd").LIB_PATH).o2v_release_cached_device_memory()


def _uvs(v):
    """Texture coordinates that change along every axis of the mesh (the long one included), several texture periods."""
    p = v.reshape(-1, 3, 3).astype(np.float64)
    u = (p[..., 0] + p[..., 1] + p[..., 2]) * 37.0
    w = (p[..., 0] - p[..., 1] + 2.0 * p[..., 2]) * 23.0
    return np.ascontiguousarray(np.stack([u, w], axis=-1).reshape(-1, 6), dtype=np.float32)


# routes through the C API: "plain" (materialless, MAX: the occupancy route), "coloured" (obj2voxel_set_triangle_colored,
# which the reference renders white: the occupancy route as well), "textured_max" / "textured_blend" (the weighted route)
def _capi_voxelize(v, res, ss=1, route="plain", bounds=None):
    """obj2voxel_voxelize() of `v` through the triangle and voxel callbacks: (error code, records)."""
    from obj2voxel_amd import capi
    a = capi.api()
    a.obj2voxel_set_log_level(capi.LOG_ERROR)
    T = len(v)
    tex = None
    try:
        inst = a.obj2voxel_alloc()
        if route.startswith("textured"):
            tex = a.obj2voxel_texture_alloc()
            assert a.obj2voxel_texture_load_pixels(tex, PIX.ctypes.data, 64, 64, 3)
            inp = capi.TriangleInput(v, uvs=_uvs(v), texture=tex)
        elif route == "coloured":
            inp = capi.TriangleInput(v, colors=meshes.triangle_colors(T))
        else:
            inp = capi.TriangleInput(v)
        out = capi.CollectingOutput()
        a.obj2voxel_set_input_callback(inst, inp.callback, None)
        a.obj2voxel_set_output_callback(inst, out.callback, None)
        a.obj2voxel_set_resolution(inst, res)
        a.obj2voxel_set_supersampling(inst, ss)
        a.obj2voxel_set_color_strategy(inst, capi.BLEND_STRATEGY if route == "textured_blend" else capi.MAX_STRATEGY)
        if bounds is not None:
            a.obj2voxel_set_mesh_boundaries(inst, (C.c_float * 6)(*bounds))
        rc = a.obj2voxel_voxelize(inst)
        a.obj2voxel_free(inst)
    finally:
        if tex:
            a.obj2voxel_texture_free(tex)
        a.obj2voxel_set_log_level(capi.LOG_INFO)
        _release()
    return rc, out.voxels()


def _want(oracle, v, res, ss=1, route="plain", bounds=None):
    T = len(v)
    kw = {}
    if route.startswith("textured"):
        kw = dict(uvs=_uvs(v), types=np.full(T, 3, np.uint32), texids=np.zeros(T, np.int32), textures=[(PIX, 1)])
    return oracle.voxelize(v, res, supersampling=ss, strategy=1 if route == "textured_blend" else 0, bounds=bounds, **kw)


def _check_capi(oracle, v, res, ss=1, route="plain", bounds=None):
    """obj2voxel_voxelize() succeeds and every record equals the oracle's; returns the records."""
    from obj2voxel_amd import capi
    rc, got = _capi_voxelize(v, res, ss, route, bounds)
    assert rc == capi.ERR_OK, f"obj2voxel_voxelize() returned {rc}"
    want = _want(oracle, v, res, ss, route, bounds)
    assert len(got) == len(want)
    assert np.array_equal(meshes.sorted_voxels(got), meshes.sorted_voxels(want))
    if route.startswith("textured"):
        assert len(np.unique(got[:, 3])) > 2
    return got


# ---- 1. a mesh taller than a pass box ------------------------------------------------------------------------------

@pytest.mark.parametrize("res,ss,route", [(100_000, 1, "plain"), (70_000, 1, "coloured"), (70_000, 1, "textured_max"),
                                          (40_000, 2, "textured_blend")])
def test_pole_taller_than_a_pass_box(oracle, res, ss, route):
    """A thin pole along z (a few voxels across, as tall as the grid) at a sample resolution above 65 535: every layer fits the
    memory, but one whole-height pass would be wider than 65 535 samples in z, so obj2voxel_voxelize() must cut it into
    z-slabs as it cuts x / y into tiles.  The reference voxelizes it; so must the drop-in call."""
    v = meshes.z_pole()
    got = _check_capi(oracle, v, res, ss, route)
    assert int(got[:, 2].max()) > 0.99 * res
    assert res < len(got) < 10 * res        # (at least one voxel per layer, a few across)


@pytest.mark.parametrize("route", ["plain", "textured_blend"])
def test_pole_across_the_tile_and_slab_borders(oracle, route):
    """With the unit cube as the mesh boundaries the grid is not fitted to the pole: at a resolution of 100 000 a pole leaning
    from (0.6550, 0.6550, 0) to (0.6560, 0.6560, 1) crosses the x tile border, the y tile border and the z-slab border, all at
    65 532.  Records on both sides of every border, all equal to the oracle's."""
    v = meshes.z_pole(base=(0.6550, 0.6550), tilt=(0.001, 0.001))
    got = _check_capi(oracle, v, 100_000, 1, route, bounds=(0.0, 0.0, 0.0, 1.0, 1.0, 1.0))
    for k in range(3):
        assert (got[:, k] < 65_532).any() and (got[:, k] >= 65_532).any(), "xyz"[k]


# ---- 2. slivers that fill a pass box --------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["plain", "textured_blend"])
@pytest.mark.parametrize("res,ss", [(65_535, 1), (65_532, 1), (32_767, 2), (100_000, 1)])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_sliver_spanning_the_pass_box(oracle, axis, res, ss, route):
    """Two long thin triangles whose boxes span the whole grid along one axis: one leaf / root whose clamped extent along that
    axis is as wide as the pass box - 65 535 samples in a last tile of 3 voxels at 65 535, exactly one tile at 65 532, 65 534
    samples at 2 x 32 767, cut at the tile / slab border at 100 000 - so the extent fields are filled to the top.  The
    occupancy route and the weighted route (which pack leaves separately)."""
    v = meshes.sliver(axis)
    got = _check_capi(oracle, v, res, ss, route)
    assert int(got[:, axis].max()) == res - 1 and int(got[:, axis].min()) == 0
    assert res < len(got) < 20 * res


# ---- 3. resolutions at the tile edge --------------------------------------------------------------------------------

@pytest.mark.parametrize("mesh", ["diagonal_strip", "z_pole"])
@pytest.mark.parametrize("res,ss", [(65_531, 1), (65_532, 1), (65_533, 1), (65_535, 1), (65_536, 1),
                                    (32_763, 2), (32_764, 2), (32_765, 2), (32_767, 2), (32_768, 2)])
def test_resolution_at_the_tile_edge(oracle, mesh, res, ss):
    """Resolutions around the switch from one pass to x / y tiles (a tile is (65 535 / ss) & ~3 voxels: 65 532 or 32 764),
    with a last tile of 1 to 4 voxels: a ribbon across the whole x / y plane and a pole along the whole z axis."""
    v = meshes.diagonal_strip(400, width=6e-5) if mesh == "diagonal_strip" else meshes.z_pole()
    got = _check_capi(oracle, v, res, ss)
    for k in ((0, 1) if mesh == "diagonal_strip" else (2,)):
        assert int(got[:, k].max()) == res - 1


# ---- 4. the pass-box limit of the device C-ABI is exact -------------------------------------------------------------

def _limit_refused(d, res, ss, **box):
    from obj2voxel_amd import hip
    with pytest.raises(hip.DeviceError, match="65535 samples"):
        d.voxelize(res, supersampling=ss, **box)


@pytest.mark.parametrize("res,ss", [(70_000, 1), (40_000, 2)])
def test_pass_box_limit_is_exact_in_z(oracle, res, ss):
    """o2v_hip_voxelize on a pole: a z-slab of exactly 65 535 samples (65 535 layers, or 32 767 at 2x supersampling) is
    voxelized like the oracle's records below it; one layer more is refused with a message naming the limit, not wrapped;
    the refused call leaves the context as it was (the same slab again, then the rest of the grid)."""
    from obj2voxel_amd import hip
    top = 65_535 // ss
    v = meshes.z_pole()
    want = _want(oracle, v, res, ss)
    want_lo = meshes.sorted_voxels(want[want[:, 2] < top])
    d = hip.DeviceVoxelizer(0)
    try:
        d.set_triangles(v)
        first = meshes.sorted_voxels(d.voxelize(res, supersampling=ss, zslab=(0, top)))
        assert len(first) > top and int(first[:, 2].max()) == top - 1
        assert np.array_equal(first, want_lo)
        _limit_refused(d, res, ss, zslab=(0, top + 1))
        again = meshes.sorted_voxels(d.voxelize(res, supersampling=ss, zslab=(0, top)))
        assert np.array_equal(again, want_lo)
        rest = d.voxelize(res, supersampling=ss, zslab=(top, res))
        assert np.array_equal(meshes.sorted_voxels(np.concatenate([first, rest])), meshes.sorted_voxels(want))
    finally:
        d.close()
        _release()


def test_pass_box_limit_is_exact_in_x(oracle):
    """The same along x, with x tiles of the device C-ABI on a sliver along x at a resolution of 70 000: a tile of exactly
    65 535 samples (the sliver's leaf extent at the top of its 16-bit field) equals the oracle's records with x < 65 535, a
    tile of 65 536 is refused, the context stays usable; the tile from 65 532 to the end equals the rest."""
    from obj2voxel_amd import hip
    res = 70_000
    v = meshes.sliver(0)
    want = _want(oracle, v, res)
    want_lo = meshes.sorted_voxels(want[want[:, 0] < 65_535])
    d = hip.DeviceVoxelizer(0)
    try:
        d.set_triangles(v)
        first = meshes.sorted_voxels(d.voxelize(res, xtile=(0, 65_535)))
        assert int(first[:, 0].max()) == 65_534
        assert np.array_equal(first, want_lo)
        _limit_refused(d, res, 1, xtile=(0, 65_536))
        again = meshes.sorted_voxels(d.voxelize(res, xtile=(0, 65_535)))
        assert np.array_equal(again, want_lo)
        rest = meshes.sorted_voxels(d.voxelize(res, xtile=(65_532, res)))
        assert np.array_equal(rest, meshes.sorted_voxels(want[want[:, 0] >= 65_532]))
    finally:
        d.close()
        _release()


# ---- 5. several devices ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mesh", ["z_pole", "diagonal_strip"])
def test_capi_over_several_devices_above_the_pass_box(oracle, monkeypatch, mesh):
    """obj2voxel_voxelize() with O2V_DEVICES naming several devices, at a sample resolution of 100 000: the sharded
    voxelization plans z-slabs of one pass box each, so such a grid is voxelized on one device of the group, tiles and
    slabs as with one device; the records equal the oracle's."""
    monkeypatch.setenv("O2V_DEVICES", ",".join(str(d) for d in _devices(3)))
    v = meshes.z_pole() if mesh == "z_pole" else meshes.diagonal_strip(400, width=6e-5)
    got = _check_capi(oracle, v, 100_000)
    assert int(got[:, 2 if mesh == "z_pole" else 0].max()) > 0.99 * 100_000


@pytest.mark.parametrize("n_ranks", [1, 3])
def test_group_refuses_a_grid_above_the_pass_box_cleanly(oracle, n_ranks):
    """o2v_hip_group_voxelize (o2v_hip_voxelize_sharded) takes no grid wider than 65 535 samples: every rank returns the error
    - reported through the status word, so that no rank waits for the others in a collective - within seconds, and the group
    then voxelizes a grid within the limit correctly."""
    from obj2voxel_amd import hip
    g = hip.DeviceGroup(_devices(n_ranks))
    try:
        v = meshes.z_pole()
        g.set_triangles(v)
        for res, ss in ((100_000, 1), (40_000, 2)):
            t0 = time.monotonic()
            with pytest.raises(hip.DeviceError) as e:
                g.voxelize(res, supersampling=ss)
            assert time.monotonic() - t0 < 30.0
            msg = str(e.value)
            for r in range(n_ranks):
                assert f"rank {r} (device" in msg, msg
            assert msg.count("65536 samples" if n_ranks > 1 else "65535 samples") == n_ranks, msg
        parts, cuts = g.voxelize(3000)
        assert cuts[0] == 0 and cuts[-1] == 3000
        assert np.array_equal(meshes.sorted_voxels(np.concatenate(parts)), meshes.sorted_voxels(oracle.voxelize(v, 3000)))
    finally:
        g.close()
        _release()
