"""The nearest-voxel transform without a GPU: the separable numpy reference against a lexicographic brute force, what the tie
grids of the device test prove, and the argument checks and call sequence of obj2voxel_amd.dense's nearest_voxel, spread_colors
and nearest_coords with the device calls stubbed."""
import numpy as np
import pytest

from tests import distance_ref as R
from tests import nearest_ref as N

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_dense import StubVoxelizer, on_cpu  # noqa: E402,F401


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 4), (1, 1, 70), (70, 1, 1), (5, 9, 13), (12, 11, 10)])
@pytest.mark.parametrize("density", [0.0, 0.02, 0.2, 1.0])
def test_separable_reference_equals_brute_force(shape, density):
    seed = np.random.default_rng(hash((shape, density)) & 0xFFFF).random(shape) < density
    near, d2 = N.separable_nearest(seed)
    want, want_d2 = N.brute_nearest(seed)
    assert near.dtype == np.int32 and np.array_equal(near, want) and np.array_equal(d2, want_d2)
    # the distance to the seed it names is the distance transform's
    assert np.array_equal(N.d2_of(near), R.brute_d2(seed.astype(np.uint8)))
    assert np.array_equal(d2, R.separable_d2(seed.astype(np.uint8)))
    if density == 0.0:
        assert (near == -1).all() and (d2 == R.INF).all()
    if density == 1.0:
        assert np.array_equal(near.ravel(), np.arange(seed.size))


@pytest.mark.parametrize("name", sorted(N.tie_grids()))
def test_tie_grids_tell_the_tie_rules_apart(name):
    """With the larger coordinate winning the reference must differ from the brute force, or the grid proves nothing."""
    seed = N.tie_grids()[name]
    want, want_d2 = N.brute_nearest(seed)
    low, high = N.separable_nearest(seed), N.separable_nearest(seed, ties="high")
    assert np.array_equal(low[0], want) and np.array_equal(low[1], want_d2)
    assert np.array_equal(high[1], want_d2) and np.array_equal(N.d2_of(high[0]), want_d2)   # (another nearest seed, as near)
    if name in N.NO_TIES:
        assert N.tie_share(seed) == 0.0 and np.array_equal(high[0], want)
    else:
        assert not np.array_equal(high[0], want)
        assert int((high[0] != want).sum()) <= round(N.tie_share(seed) * seed.size)


def test_the_lattice_has_ties_on_a_quarter_of_its_voxels():
    assert N.tie_share(N.tie_grids()["lattice"]) >= 0.25
    small = np.zeros((9, 9, 9), bool)
    small[::4, ::4, ::4] = True
    assert round(N.tie_share(small) * small.size) == 386


@pytest.mark.parametrize("along_z", [False, True])
def test_deep_stack_closed_form_is_the_reference(along_z):
    """What tests/nearest_cases.py compares the device against on distance_ref's deep-stack grids."""
    y, x = np.indices((1024, 2100))
    closed = np.where((2099 - x) ** 2 <= (1023 - y) ** 2, y * 2100 + 2099, 1023 * 2100 + x).astype(np.int32)
    lab = R.deep_stack_labels(along_z, 41)
    near, d2 = N.separable_nearest(lab == 1)
    assert np.array_equal(near, closed.reshape(lab.shape))
    assert np.array_equal(d2, np.minimum((2099 - x) ** 2, (1023 - y) ** 2).astype(np.int32).reshape(lab.shape))


# ---- obj2voxel_amd.dense with the device calls stubbed -------------------------------------------------------------------------

class NearStub(StubVoxelizer):
    def nearest_dense(self, grid_ptr, fmt, strides, dims, level, flags, nearest_ptr, nearest_strides, dist2_ptr=None, dist2_strides=None,
                      values_ptr=None, value_strides=None, max_dist2=hip.NEAREST_NO_LIMIT):
        self.calls.append(dict(grid=grid_ptr, fmt=fmt, strides=tuple(strides), dims=tuple(dims), level=level, flags=flags, nearest=nearest_ptr,
                               nearest_strides=tuple(nearest_strides), dist2=dist2_ptr,
                               dist2_strides=None if dist2_strides is None else tuple(dist2_strides), values=values_ptr,
                               value_strides=None if value_strides is None else tuple(value_strides), max_dist2=max_dist2))


def test_nearest_voxel_formats_strides_and_outputs():
    dv = NearStub()
    lab = torch.zeros((2, 5, 6, 7), dtype=torch.uint8)
    out = dense.nearest_voxel(dv, lab[1])
    c = dv.calls[-1]
    assert out.dtype == torch.int32 and tuple(out.shape) == (5, 6, 7) and out.is_contiguous()
    assert (c["grid"], c["fmt"], c["strides"], c["dims"], c["flags"]) == (lab[1].data_ptr(), hip.GRID_U8, (1, 7, 42), (7, 6, 5), 0)
    assert c["nearest"] == out.data_ptr() and c["nearest_strides"] == (1, 7, 42)
    assert c["dist2"] is None and c["values"] is None and c["max_dist2"] == 0x7FFFFFFF
    out, d2 = dense.nearest_voxel(dv, lab[0].to(torch.bool), surface_only=True, dist2=True)
    c = dv.calls[-1]
    assert c["flags"] == hip.NEAREST_SEED_ONE and d2.dtype == torch.int32 and c["dist2"] == d2.data_ptr() and c["dist2_strides"] == (1, 7, 42)
    # bits: 32 voxels per word along x; float32 with a level; permuted out and dist2
    bits = torch.zeros((5, 6, 2), dtype=torch.int32)
    out = dense.nearest_voxel(dv, bits)
    assert tuple(out.shape) == (5, 6, 64) and dv.calls[-1]["fmt"] == hip.GRID_BITS and dv.calls[-1]["dims"] == (64, 6, 5)
    buf, dbuf = torch.zeros((6, 7, 5), dtype=torch.int32), torch.zeros((7, 5, 6), dtype=torch.int32)
    got, d2 = dense.nearest_voxel(dv, torch.zeros((5, 6, 7)), level=0.5, out=buf.permute(2, 0, 1), dist2=dbuf.permute(1, 2, 0))
    c = dv.calls[-1]
    assert got.data_ptr() == buf.data_ptr() and d2.data_ptr() == dbuf.data_ptr()
    assert (c["fmt"], c["level"], c["nearest_strides"], c["dist2_strides"]) == (hip.GRID_F32_BELOW, 0.5, (5, 35, 1), (30, 1, 6))
    assert dense.nearest_voxel(dv, lab[1], dist2=False).dtype == torch.int32   # (no tuple)


_U8 = torch.zeros((4, 4, 4), dtype=torch.uint8)
_I32 = torch.zeros((4, 4, 4), dtype=torch.int32)


@pytest.mark.parametrize("fn, args, kw, exc", [
    (dense.nearest_voxel, (torch.zeros((4, 4, 4), dtype=torch.int64),), {}, TypeError),
    (dense.nearest_voxel, (torch.zeros((4, 4), dtype=torch.uint8),), {}, ValueError),
    (dense.nearest_voxel, (torch.zeros((4, 0, 4), dtype=torch.uint8),), {}, ValueError),
    (dense.nearest_voxel, (torch.zeros((4, 4, 4), device="meta", dtype=torch.uint8),), {}, ValueError),
    (dense.nearest_voxel, (torch.zeros((4, 4, 4)),), {}, ValueError),                                        # float32 without a level
    (dense.nearest_voxel, (_U8,), dict(level=0.0), ValueError),
    (dense.nearest_voxel, (torch.zeros((4, 4, 4)),), dict(level=0.0, surface_only=True), ValueError),
    (dense.nearest_voxel, (_I32,), dict(surface_only=True), ValueError),
    (dense.nearest_voxel, (torch.zeros((1, 1, 46342), dtype=torch.uint8),), {}, ValueError),                  # the distance limit
    (dense.nearest_voxel, (_U8,), dict(out=torch.zeros((4, 4, 4))), TypeError),
    (dense.nearest_voxel, (_U8,), dict(out=torch.zeros((4, 4, 5), dtype=torch.int32)), ValueError),
    (dense.nearest_voxel, (_U8,), dict(dist2=torch.zeros((4, 4, 4))), TypeError),
    (dense.nearest_voxel, (_U8,), dict(dist2=torch.zeros((5, 4, 4), dtype=torch.int32)), ValueError),
    (dense.nearest_voxel, (torch.zeros((4, 4, 1), dtype=torch.int32),), dict(out=torch.zeros((4, 4, 4), dtype=torch.int32)), ValueError),
    (dense.spread_colors, (_U8, torch.zeros((4, 4, 4))), {}, TypeError),
    (dense.spread_colors, (_U8, torch.zeros((4, 4, 5), dtype=torch.int32)), {}, ValueError),
    (dense.spread_colors, (_U8, torch.zeros((4, 4, 4), device="meta", dtype=torch.int32)), {}, ValueError),
    (dense.spread_colors, (_U8, _I32), dict(inside_only=True), ValueError),
    (dense.spread_colors, (torch.zeros((4, 4, 4)), _I32), dict(level=0.0, surface_only=True, inside_only=True), ValueError),
    (dense.spread_colors, (_U8, _I32), dict(max_distance=-1), ValueError),
    (dense.spread_colors, (_U8, _I32), dict(max_distance=float("nan")), ValueError),
    (dense.spread_colors, (_U8, _I32), dict(max_distance=True), ValueError),
    (dense.spread_colors, (_U8, _I32), dict(max_distance="3"), ValueError),
    (dense.spread_colors, (_U8, _I32), dict(out=torch.zeros((4, 4, 4))), TypeError),
    (dense.spread_colors, (_U8, _I32), dict(out=torch.zeros((4, 5, 4), dtype=torch.int32)), ValueError),
])
def test_rejects_before_any_device_call(fn, args, kw, exc):
    dv = NearStub()
    with pytest.raises(exc):
        fn(dv, *args, **kw)
    assert not dv.calls


def test_outputs_in_the_seeds_storage_are_refused():
    dv = NearStub()
    grid = torch.zeros((4, 4, 1), dtype=torch.int32)
    big = torch.zeros(1024, dtype=torch.int32)
    seeds, out = big[:16].view(4, 4, 1), big[512:].view(4, 4, 32)
    for call in (lambda: dense.nearest_voxel(dv, seeds, out=out),
                 lambda: dense.nearest_voxel(dv, seeds, dist2=out),
                 lambda: dense.spread_colors(dv, seeds, torch.zeros((4, 4, 32), dtype=torch.int32), out=out),
                 lambda: dense.spread_colors(dv, seeds, out, out=out)):
        with pytest.raises(ValueError, match="storage"):
            call()
    both = torch.zeros((2, 4, 4, 32), dtype=torch.int32)
    with pytest.raises(ValueError, match="storage"):
        dense.nearest_voxel(dv, grid, out=both[0], dist2=both[1])
    assert not dv.calls
    dense.spread_colors(dv, seeds, out)   # (a painted copy: colors is only read, wherever it lives)
    assert dv.calls[-1]["values"] not in (None, out.data_ptr())


def test_spread_colors_clone_in_place_and_copy_then_paint():
    dv = NearStub()
    lab = torch.zeros((3, 4, 5), dtype=torch.uint8)
    colors = torch.arange(60, dtype=torch.int32).view(3, 4, 5)
    # out=None: a painted clone; colors is not handed to the device
    got = dense.spread_colors(dv, lab, colors)
    c = dv.calls[-1]
    assert got.data_ptr() != colors.data_ptr() and torch.equal(got, colors) and c["values"] == got.data_ptr()
    assert c["value_strides"] == (1, 5, 20) and c["flags"] == 0 and c["max_dist2"] == 0x7FFFFFFF and c["dist2"] is None
    assert c["nearest"] not in (None, got.data_ptr(), colors.data_ptr()) and c["nearest_strides"] == (1, 5, 20)
    # a clone of a permuted view is contiguous
    view = torch.arange(60, dtype=torch.int32).view(5, 3, 4).permute(1, 2, 0)
    got = dense.spread_colors(dv, lab, view)
    assert got.is_contiguous() and torch.equal(got, view) and dv.calls[-1]["value_strides"] == (1, 5, 20)
    # out is colors: in place, as it is
    got = dense.spread_colors(dv, lab, view, surface_only=True, inside_only=True, out=view)
    c = dv.calls[-1]
    assert got is view and c["values"] == view.data_ptr() and c["value_strides"] == (12, 1, 4)
    assert c["flags"] == hip.NEAREST_SEED_ONE | hip.NEAREST_VALUES_INSIDE
    # another tensor: filled with colors, then painted
    batch = torch.full((2, 3, 4, 5), -7, dtype=torch.int32)
    got = dense.spread_colors(dv, lab, colors, surface_only=True, out=batch[1])
    c = dv.calls[-1]
    assert got.data_ptr() == batch[1].data_ptr() and torch.equal(batch[1], colors) and bool((batch[0] == -7).all())
    assert c["values"] == batch[1].data_ptr() and c["flags"] == hip.NEAREST_SEED_ONE
    assert len(dv.calls) == 4


@pytest.mark.parametrize("r, want", [(0, 0), (1, 1), (2.5, 6), (3, 9), (4.5, 20), (1.9999, 3), (46341.0, 0x7FFFFFFF), (1e30, 0x7FFFFFFF),
                                     (float("inf"), 0x7FFFFFFF), (None, 0x7FFFFFFF)])
def test_max_distance_becomes_floor_of_its_square(r, want):
    dv = NearStub()
    dense.spread_colors(dv, _U8, _I32, max_distance=r)
    assert dv.calls[-1]["max_dist2"] == want


def test_nearest_coords():
    near = torch.tensor([[[0, 5, -1], [3, 11, 7]], [[6, -1, 2], [9, 10, 1]]], dtype=torch.int32)   # [z, y, x] = (2, 2, 3)
    xyz = dense.nearest_coords(near)
    assert xyz.dtype == torch.int32 and tuple(xyz.shape) == (2, 2, 3, 3)
    assert xyz[0, 0].tolist() == [[0, 0, 0], [2, 1, 0], [-1, -1, -1]]
    assert xyz[0, 1].tolist() == [[0, 1, 0], [2, 1, 1], [1, 0, 1]]
    assert xyz[1, 0].tolist() == [[0, 0, 1], [-1, -1, -1], [2, 0, 0]]
    assert xyz[1, 1].tolist() == [[0, 1, 1], [1, 1, 1], [1, 0, 0]]
    with pytest.raises(TypeError):
        dense.nearest_coords(near.to(torch.int64))
    with pytest.raises(ValueError):
        dense.nearest_coords(near[0])


def test_scratch_is_the_distance_transform_s():
    L = hip._bind()
    for dims in ((1024, 1024, 1024), (4096, 4096, 1), (1, 1, 46341), (300, 7, 129), (5, 0, 5)):
        d = (hip.C.c_uint32 * 3)(*dims)
        assert L.o2v_hip_nearest_scratch_bytes(d) == L.o2v_hip_distance_scratch_bytes(d, hip.DIST_SQ_I32)
    assert L.o2v_hip_nearest_scratch_bytes((hip.C.c_uint32 * 3)(1024, 1024, 1024)) == 8 * (1 << 17) * 1024
