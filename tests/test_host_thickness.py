"""Local thickness and ball morphology without a GPU: the numpy reference of tests/thickness_ref.py against a
brute force of the definition and against a sweep over the levels; the library's cover table (host code, no device) against
enumeration; the pruning rule; the torch layer of obj2voxel_amd.dense against a stand-in for the device; the scratch formula;
closed forms; what the GPU cases at the call's limits rest on: tiles with an empty outer layer do not see each other, and sets that are
constant over a box's cross-section reduce to a line."""
import math

import numpy as np
import pytest
import torch

from obj2voxel_amd import dense, hip
from tests import thickness_ref as TR
from tests.test_host_dense import StubVoxelizer, on_cpu  # noqa: F401

CAPS = (1, 2, 3, 5, 9, 16, 50)


def grids():
    rng = np.random.default_rng(24)
    return {"random": rng.random((12, 12, 12)) < 0.8, "sparse": rng.random((6, 7, 5)) < 0.4, "full": np.ones((5, 12, 7), bool),
            "ball": TR.digital_ball((12, 12, 12), (6, 5, 6), 5.3), "plate": TR.plate((9, 12, 4), 1, 3, 5) | TR.plate((9, 12, 4), 0, 7, 1),
            "line": rng.random((1, 1, 40)) < 0.9}


GRIDS = grids()


# ---- the reference against the definition --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(GRIDS))
@pytest.mark.parametrize("border", [False, True])
@pytest.mark.parametrize("background", [False, True])
def test_reference_against_the_definition(name, border, background):
    S = ~GRIDS[name] if background else GRIDS[name]
    want, depth = TR.brute(S, CAPS, border)
    d2 = TR.depth2(S, border)
    assert np.array_equal(d2, depth) and d2.dtype == np.int32
    assert (d2[~S] == 0).all() and (S.all() and not border) == bool((d2 == TR.INF).any())
    for cap in CAPS:
        T = TR.thickness(S, cap, border, d2)
        assert T.dtype == np.int32 and np.array_equal(T, want[cap]), (name, cap)
        assert (T[~S] == 0).all() and (T[S] >= 1).all() and (T <= cap).all() and (T >= np.minimum(d2, cap)).all()
        # T == cap exactly in the opening by {|q|^2 < cap}; OPEN_ONLY is a lower bound that agrees there
        low = TR.open_only(S, cap, border, d2)
        assert np.array_equal(low == cap, T == cap) and (low <= T).all() and np.array_equal(low > 0, S)


@pytest.mark.parametrize("name", ["random", "ball", "plate", "sparse"])
@pytest.mark.parametrize("border", [False, True])
def test_reference_against_a_sweep_over_the_levels(name, border):
    for cap in (2, 9, 50):
        assert np.array_equal(TR.thickness(GRIDS[name], cap, border), TR.by_levels(GRIDS[name], cap, border)), cap


def test_scatter_takes_the_same_balls_either_way():
    """Per centre or per ball offset: the reference picks by cost, so both are held against each other."""
    rng = np.random.default_rng(5)
    Rc = np.where(rng.random((9, 10, 11)) < 0.5, rng.integers(1, 30, (9, 10, 11)), 0)
    nz, ny, nx = Rc.shape
    want = np.zeros(Rc.shape, np.int64)
    for z, y, x in np.argwhere(Rc > 0).tolist():
        p = np.indices(Rc.shape)
        inside = (p[0] - z) ** 2 + (p[1] - y) ** 2 + (p[2] - x) ** 2 < Rc[z, y, x]
        want[inside] = np.maximum(want[inside], Rc[z, y, x])
    assert np.array_equal(TR.scatter(Rc), want)
    dense_R = np.full((3, 2, 50), 7)      # many centres of one small ball: the per-offset route, offsets past a 2- and 3-voxel axis
    want = np.full(dense_R.shape, 7)
    assert np.array_equal(TR.scatter(dense_R), want)


# ---- the cover table --------------------------------------------------------------------------------------------------------------------

def test_cover_table_values():
    t = hip.thickness_cover_table(7)
    assert t.dtype == np.uint32 and t.shape == (3, 8)
    assert t[:, 1:].tolist() == [[2, 5, 6, 7, 10, 11, 12], [3, 6, 9, 10, 11, 14, 15], [4, 7, 10, 13, 13, 15, 18]] and t[:, 0].tolist() == [0, 0, 0]


def test_cover_table_against_enumeration():
    want = TR.cover_table(300)
    assert np.array_equal(hip.thickness_cover_table(300), want)
    for cap in (1, 2, 17, 299):           # a table is the head of every longer one
        assert np.array_equal(hip.thickness_cover_table(cap), want[:, :cap + 1])
    assert want[0, 1:].tolist() == [TR.cover_entry(R)[0] for R in range(1, 301)]


def test_cover_table_at_the_largest_cap():
    cap = hip.THICK_MAX_RADIUS2
    assert cap == 1 << 14
    t = hip.thickness_cover_table(cap).astype(np.int64)
    R = np.arange(1, cap + 1)
    assert (t[:, 1:] > R).all()                                            # chains of covered balls end
    assert (np.diff(t[:, 1:], axis=1) >= 0).all() and (t[0] <= t[1]).all() and (t[1] <= t[2]).all()
    # a neighbour at distance |v| needs no more than the triangle inequality asks: sqrt(L - 1) <= sqrt(R - 1) + |v|
    for k in range(3):
        assert (np.sqrt(t[k, 1:] - 1) <= np.sqrt(R - 1) + math.sqrt(k + 1) + 1e-9).all()
    for r in (301, 1000, 4097, 10000, 16383, 16384):
        assert tuple(t[:, r]) == TR.cover_entry(r), r


@pytest.mark.parametrize("bad", [0, -1, (1 << 14) + 1, 2.0, True, None])
def test_cover_table_refuses(bad):
    with pytest.raises(ValueError):
        hip.thickness_cover_table(bad)


# ---- pruning ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(GRIDS))
@pytest.mark.parametrize("border", [False, True])
def test_pruning_leaves_the_result_unchanged(name, border):
    for background in (False, True):
        S = ~GRIDS[name] if background else GRIDS[name]
        for cap in CAPS:
            table = hip.thickness_cover_table(cap)
            assert np.array_equal(TR.pruned(S, cap, border, table), TR.thickness(S, cap, border)), (name, cap, background)
            cand, kept = TR.kept_centres(S, cap, border, table)
            assert not (kept & ~cand).any() and np.array_equal(cand, S & (TR.depth2(S, border) < cap))


def test_pruning_counts_of_a_digital_ball():
    """The ball of DESIGN.md section 24: what the device's counters must show for it."""
    S = TR.digital_ball((96, 96, 96), (48, 48, 48), 43.2)
    assert int(S.sum()) == 337987
    d2 = TR.depth2(S, True)
    for cap, want in ((16, (78298, 15584)), (64, (151574, 17660))):
        cand, kept = TR.kept_centres(S, cap, True, hip.thickness_cover_table(cap), d2)
        assert (int(cand.sum()), int(kept.sum())) == want


# ---- closed forms -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", range(1, 10))
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_plate_reads_its_half_width_squared(w, axis):
    dims = [30, 30, 30]
    dims[axis] = 14
    S = TR.plate(tuple(dims), axis, 2, w)
    half = ((w + 1) // 2) ** 2
    for cap in (3, 9, 50):
        T = TR.pruned(S, cap, False, hip.thickness_cover_table(cap))      # border off: the plate goes on past the box
        assert (T[S] == min(half, cap)).all() and (T[~S] == 0).all()
        f = TR.as_float(T)
        if half <= cap:
            assert (f[S] == (w if w % 2 else w - 1)).all()                # 2 sqrt(T) - 1: w for odd w, w - 1 for even w


def test_full_and_empty_grids():
    full, empty = np.ones((4, 6, 5), bool), np.zeros((4, 6, 5), bool)
    for cap in CAPS:
        assert (TR.thickness(full, cap, False) == cap).all() and (TR.depth2(full, False) == TR.INF).all()
        assert (TR.thickness(empty, cap, False) == 0).all() and (TR.thickness(empty, cap, True) == 0).all()
        assert TR.thickness(full, cap, True).max() == min(cap, 4) and TR.depth2(full, True).max() == 4    # 2 from the z faces
    assert TR.as_float(np.array([0, 1, 2, 4, 5], np.int32)).tolist() == [0.0, 1.0, np.float32(2 * math.sqrt(2) - 1), 3.0, np.float32(2 * math.sqrt(5) - 1)]


def test_the_derived_grids_nest():
    S = GRIDS["random"] | GRIDS["ball"]
    for r in (0, 1, 1.5, 3):
        er, op, cl, di = TR.erode(S, r), TR.opening(S, r), TR.closing(S, r), TR.dilate(S, r)
        assert not (er & ~op).any() and not (op & ~S).any() and not (S & ~cl).any() and not (cl & ~di).any()
        assert np.array_equal(op, TR.thickness(S, TR.cap_of(r), True) == TR.cap_of(r))
        assert np.array_equal(TR.thin_regions(S, 2 * r + 1), S & ~op)
    assert np.array_equal(TR.erode(S, 0), S) and np.array_equal(TR.dilate(S, 0), S) and TR.cap_of(2) == 5 and TR.cap_of(2.5) == 7


# ---- the torch layer against a stub -------------------------------------------------------------------------------------------------

class ThickStub(StubVoxelizer):
    """Computes with the reference, on the tensors' own memory (CPU)."""

    def thickness_dense(self, grid_ptr, fmt, strides, dims, level, flags, cap, dst_ptr, dst_strides, depth2_ptr=None, depth2_strides=None):
        self.calls.append(("thickness", grid_ptr, fmt, tuple(strides), tuple(dims), level, flags, cap, dst_ptr, tuple(dst_strides), depth2_ptr,
                           None if depth2_strides is None else tuple(depth2_strides)))
        C = hip.C
        assert fmt == hip.GRID_U8
        nx, ny, nz = dims

        def view(ptr, ctype, st, elem):
            span = sum((d - 1) * s for d, s in zip(dims, st)) + 1
            raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (span,))
            return np.lib.stride_tricks.as_strided(raw, (nz, ny, nx), tuple(elem * s for s in (st[2], st[1], st[0])))
        S = view(grid_ptr, C.c_uint8, strides, 1) != 0
        if flags & hip.THICK_BACKGROUND:
            S = ~S
        border = bool(flags & hip.THICK_BORDER)
        T = TR.open_only(S, cap, border) if flags & hip.THICK_OPEN_ONLY else TR.thickness(S, cap, border)
        if flags & hip.THICK_F32:
            view(dst_ptr, C.c_float, dst_strides, 4)[...] = TR.as_float(T)
        else:
            view(dst_ptr, C.c_int32, dst_strides, 4)[...] = T
        if depth2_ptr:
            view(depth2_ptr, C.c_int32, depth2_strides, 4)[...] = TR.depth2(S, border)


SOLID = GRIDS["random"] | GRIDS["ball"]


def test_local_thickness_arguments():
    dv = ThickStub()
    grid = torch.from_numpy(SOLID.astype(np.uint8))
    t = dense.local_thickness(dv, grid, 2)
    c = dv.calls[-1]
    assert c[2:8] == (hip.GRID_U8, (1, 12, 144), (12, 12, 12), 0.0, hip.THICK_BORDER, 5) and c[8:] == (t.data_ptr(), (1, 12, 144), None, None)
    assert t.dtype == torch.int32 and t.is_contiguous() and np.array_equal(t.numpy(), TR.thickness(SOLID, 5, True))
    # radius -> cap = floor(r^2) + 1
    for radius, cap in ((0, 1), (0.99, 1), (1, 2), (1.5, 3), (2.0, 5), (3, 10), (127.99, 16382), (math.sqrt(16383), 16384), (np.float32(2.5), 7)):
        rec = RecordOnly()
        dense.local_thickness(rec, grid, radius)
        assert rec.calls[-1][7] == cap, radius
    # the float format, the background, no border; depth2 on request
    f, d2 = dense.local_thickness(dv, grid, 3, fmt="thickness", background=True, border=False, depth2=True)
    c = dv.calls[-1]
    assert c[6] == hip.THICK_BACKGROUND | hip.THICK_F32 and c[7] == 10 and c[10] == d2.data_ptr() and c[11] == (1, 12, 144)
    assert f.dtype == torch.float32 and d2.dtype == torch.int32 and np.array_equal(d2.numpy(), TR.depth2(~SOLID, False))
    assert np.array_equal(f.numpy().view(np.uint32), TR.as_float(TR.thickness(~SOLID, 10, False)).view(np.uint32))
    assert not isinstance(dense.local_thickness(dv, grid, 3, depth2=False), tuple) and dv.calls[-1][10] is None
    # out= and depth2= are written as they are
    wide = torch.full((12, 12, 24), -7, dtype=torch.int32)
    deep = torch.full((12, 36, 12), -7, dtype=torch.int32)
    got, gd = dense.local_thickness(dv, grid, 2, out=wide[:, :, ::2], depth2=deep[:, 1::3, :])
    c = dv.calls[-1]
    assert got.data_ptr() == wide.data_ptr() and c[9] == (2, 24, 288) and c[11] == (1, 36, 432) and gd.data_ptr() == deep[:, 1::3, :].data_ptr()
    assert bool((wide[:, :, 1::2] == -7).all()) and bool((deep[:, 0::3, :] == -7).all())
    assert np.array_equal(wide[:, :, ::2].numpy(), TR.thickness(SOLID, 5, True)) and np.array_equal(deep[:, 1::3, :].numpy(), TR.depth2(SOLID, True))
    # a float grid with a level, a bits grid
    any_dv = RecordOnly()
    dense.local_thickness(any_dv, torch.where(torch.from_numpy(SOLID), -1.0, 1.0), 2, level=0.0)
    assert any_dv.calls[-1][2] == hip.GRID_F32_BELOW
    dense.local_thickness(any_dv, torch.zeros((4, 4, 2), dtype=torch.int32), 2)
    assert any_dv.calls[-1][2] == hip.GRID_BITS and any_dv.calls[-1][4] == (64, 4, 4)
    for text in ("section 24", "at least", "odd", "mandatory"):
        assert text in " ".join(dense.local_thickness.__doc__.split())


class RecordOnly(StubVoxelizer):
    def thickness_dense(self, *args):
        self.calls.append(("thickness",) + args)


def test_the_derived_functions():
    dv = ThickStub()
    grid = torch.from_numpy(SOLID)
    d = dense.inner_distance(dv, grid)
    c = dv.calls[-1]
    assert c[6] == hip.THICK_BORDER | hip.THICK_OPEN_ONLY and c[7] == 1 and c[10] == d.data_ptr() and d.dtype == torch.int32
    assert np.array_equal(d.numpy(), TR.depth2(SOLID, True))
    out = torch.full((12, 12, 24), -7, dtype=torch.int32)
    assert dense.inner_distance(dv, grid, background=True, border=False, out=out[:, :, ::2]).data_ptr() == out.data_ptr()
    assert dv.calls[-1][6] == hip.THICK_BACKGROUND | hip.THICK_OPEN_ONLY and dv.calls[-1][11] == (2, 24, 288)
    assert np.array_equal(out[:, :, ::2].numpy(), TR.depth2(~SOLID, False)) and bool((out[:, :, 1::2] == -7).all())
    for r in (0, 1, 1.5, 3):
        n = len(dv.calls)
        got = {"erode": dense.erode(dv, grid, r), "opening": dense.opening(dv, grid, r), "dilate": dense.dilate(dv, grid, r), "closing": dense.closing(dv, grid, r)}
        want = {"erode": TR.erode(SOLID, r), "opening": TR.opening(SOLID, r), "dilate": TR.dilate(SOLID, r), "closing": TR.closing(SOLID, r)}
        for k in got:
            assert got[k].dtype == torch.bool and np.array_equal(got[k].numpy(), want[k]), (k, r)
        flags = [c[6] for c in dv.calls[n:]]
        assert flags == [hip.THICK_BORDER | hip.THICK_OPEN_ONLY] * 2 + [hip.THICK_BACKGROUND | hip.THICK_OPEN_ONLY] * 2     # dilate, closing: no border
        assert [c[7] for c in dv.calls[n:]] == [1, TR.cap_of(r), 1, TR.cap_of(r)]
        assert np.array_equal(dense.erode(dv, grid, r, border=False, background=True).numpy(), TR.erode(~SOLID, r, False))
    for t in (1, 2, 3, 4.5, 7):
        thin = dense.thin_regions(dv, grid, t)
        c = dv.calls[-1]
        assert c[6] == hip.THICK_BORDER | hip.THICK_OPEN_ONLY and c[7] == TR.cap_of((t - 1) / 2) and thin.dtype == torch.bool
        assert np.array_equal(thin.numpy(), TR.thin_regions(SOLID, t)), t
    assert np.array_equal(dense.thin_regions(dv, grid, 3, border=False, background=True).numpy(), TR.thin_regions(~SOLID, 3, False))
    for fn in (dense.inner_distance, dense.erode, dense.opening, dense.thin_regions):
        assert "section 24" in fn.__doc__
    assert "border=False" in dense.dilate.__doc__ and "border=False" in dense.closing.__doc__ and "past the box" in dense.dilate.__doc__


U8 = torch.zeros((4, 4, 4), dtype=torch.uint8)


@pytest.mark.parametrize("kw, exc", [
    (dict(grid=torch.zeros((4, 4, 4), dtype=torch.float64)), TypeError), (dict(grid=torch.zeros((4, 4))), ValueError), (dict(grid=np.zeros((4, 4, 4), np.uint8)), ValueError),
    (dict(grid=torch.zeros((4, 4, 4))), ValueError), (dict(grid=torch.zeros((4, 4, 4)), level=float("nan")), ValueError), (dict(level=0.0), ValueError),
    (dict(grid=torch.zeros((4, 4, 8), dtype=torch.int32)[:, :, ::2]), ValueError), (dict(grid=torch.zeros((4, 0, 4), dtype=torch.uint8)), ValueError),
    (dict(grid=torch.zeros((4, 4, 4), dtype=torch.uint8, device="meta")), ValueError),
    (dict(grid=torch.zeros((1, 1, 1), dtype=torch.uint8).expand(1, 1, 65537)), ValueError),
    (dict(grid=torch.zeros((1, 1, 1), dtype=torch.uint8).expand(2048, 1024, 1024)), ValueError),
    (dict(grid=torch.zeros((1, 1, 1), dtype=torch.uint8).expand(1, 1, 46342)), ValueError),
    (dict(max_radius=-1), ValueError), (dict(max_radius=128), ValueError), (dict(max_radius=float("nan")), ValueError), (dict(max_radius=float("inf")), ValueError),
    (dict(max_radius=True), ValueError), (dict(max_radius="2"), ValueError), (dict(max_radius=None), ValueError),
    (dict(fmt="float"), ValueError), (dict(fmt=None), ValueError),
    (dict(out=torch.zeros((4, 4, 4), dtype=torch.int64)), TypeError), (dict(out=torch.zeros((4, 4, 4))), TypeError), (dict(out=torch.zeros((4, 4, 5), dtype=torch.int32)), ValueError),
    (dict(fmt="thickness", out=torch.zeros((4, 4, 4), dtype=torch.int32)), TypeError),
    (dict(out=torch.zeros((4, 4, 4), dtype=torch.int32, device="meta")), ValueError), (dict(out=np.zeros((4, 4, 4), np.int32)), ValueError),
    (dict(depth2=torch.zeros((4, 4, 4))), TypeError), (dict(depth2=torch.zeros((4, 5, 4), dtype=torch.int32)), ValueError), (dict(depth2=np.zeros((4, 4, 4), np.int32)), ValueError),
    (dict(depth2=torch.zeros((4, 4, 4), dtype=torch.int32, device="meta")), ValueError),
])
def test_local_thickness_rejects(kw, exc):
    dv = RecordOnly()
    args = dict(grid=U8, max_radius=2)
    args.update(kw)
    with pytest.raises(exc):
        dense.local_thickness(dv, args.pop("grid"), args.pop("max_radius"), **args)
    assert not dv.calls


def test_outputs_in_the_grid_or_in_each_other_are_refused():
    dv = RecordOnly()
    both = torch.zeros((2, 4, 4, 4), dtype=torch.int32)
    bits = torch.zeros((2, 4, 4, 1), dtype=torch.int32)
    with pytest.raises(ValueError, match="storage"):
        dense.local_thickness(dv, bits[0], 2, out=bits[1].expand(4, 4, 32))
    wide = torch.zeros((4, 4, 8), dtype=torch.int32)
    for out, depth2 in ((both[0], both[0]), (wide[:, :, ::2], wide[:, :, 1::2]), (both.view(-1)[:64].view(4, 4, 4), both.view(-1)[63:127].view(4, 4, 4))):
        with pytest.raises(ValueError, match="depth2 must not overlap out"):
            dense.local_thickness(dv, U8, 2, out=out, depth2=depth2)
    with pytest.raises(ValueError, match="storage"):
        dense.inner_distance(dv, bits[0], out=bits[1].expand(4, 4, 32))
    with pytest.raises(TypeError, match="out must be"):     # (inner_distance names its own argument)
        dense.inner_distance(dv, U8, out=torch.zeros((4, 4, 4)))
    assert not dv.calls
    # two slices of one batch tensor share a storage and do not overlap: accepted, as the library accepts them
    dense.local_thickness(dv, U8, 2, out=both[0], depth2=both[1])
    assert dv.calls[-1][8] == both[0].data_ptr() and dv.calls[-1][10] == both[1].data_ptr()


@pytest.mark.parametrize("fn, kw", [(dense.erode, dict(radius=-1)), (dense.erode, dict(radius=128)), (dense.opening, dict(radius=None)), (dense.dilate, dict(radius=True)),
                                    (dense.closing, dict(radius=200)), (dense.thin_regions, dict(min_thickness=0.5)), (dense.thin_regions, dict(min_thickness=257)),
                                    (dense.thin_regions, dict(min_thickness="3")), (dense.thin_regions, dict(min_thickness=float("nan")))])
def test_the_derived_functions_reject(fn, kw):
    dv = RecordOnly()
    with pytest.raises(ValueError):
        fn(dv, U8, **kw)
    assert not dv.calls


def test_refused_when_the_library_came_first(monkeypatch):
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: False)
    with pytest.raises(RuntimeError, match="before torch"):
        dense.local_thickness(RecordOnly(), U8, 2)
    with pytest.raises(RuntimeError, match="before torch"):
        dense.thin_regions(RecordOnly(), U8, 3)


def test_a_wait_comes_before_the_library(monkeypatch):
    """As tests/test_host_dense.py holds it for the other functions: the library call comes behind a wait on the voxelizer's own device."""
    for call in (lambda dv: dense.local_thickness(dv, U8 + 1, 2), lambda dv: dense.inner_distance(dv, U8 + 1), lambda dv: dense.closing(dv, U8 + 1, 1)):
        dv = RecordOnly()
        own = torch.device("cpu")
        monkeypatch.setattr(dense, "_device", lambda v: own)
        monkeypatch.setattr(dense, "_sync", lambda device: dv.calls.append(("sync", device)))
        call(dv)
        names = [c[0] for c in dv.calls]
        assert "thickness" in names and "sync" in names[:names.index("thickness")] and all(c[1] is own for c in dv.calls if c[0] == "sync")


# ---- the scratch formula ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(1, 1, 1), (64, 8, 8), (65, 9, 9), (1024, 1024, 1024), (46341, 1, 7), (1000, 999, 17)])
def test_scratch_bytes_formula(dims):
    voxels = math.prod(dims)
    k8 = int(hip._bind().o2v_hip_distance_scratch_bytes(hip._u32x3(dims), 0))   # (K8's envelope stacks)
    assert k8 == 8 * max(min(dims[0] * dims[2], 1 << 17) * dims[1], min(dims[0] * dims[1], 1 << 17) * dims[2])
    for cap in (1, 5, 1 << 14):
        want = k8 + 8 * (-(-voxels // 256) + 1) + 12 * (cap + 1) + 64
        assert hip.thickness_scratch_bytes(dims, cap, True) == want and hip.thickness_scratch_bytes(dims, cap) == want + 4 * voxels
        assert hip.DeviceVoxelizer.thickness_scratch_bytes(None, dims, cap, False) == want + 4 * voxels
    assert hip.thickness_scratch_bytes((4, 0, 4), 5) == 0 and hip.thickness_scratch_bytes(dims, 0) == 0 and hip.thickness_scratch_bytes(dims, (1 << 14) + 1) == 0


# ---- tiles that do not see each other: what the GPU cases past 2^28 voxels rest on -------------------------------------------------

TILES = {(11, 9, 7): (((4, 4, 3), 2.5), ((8, 3, 3), 1.5)), (13, 8, 9): (((5, 4, 4), 3.0), ((10, 3, 5), 1.8))}   # dims (x, y, z): the balls
TILE_CAPS = (1, 2, 5, 17, 26, 65, 400)


def check_tiles(P, reps, caps=TILE_CAPS):
    """All five quantities of np.tile(P, reps) by the literal reference, both borders, against the tile's (border off) repeated."""
    G = np.tile(P, reps)
    n = int(np.prod(reps))
    d2 = TR.depth2(P, False)
    for border in (False, True):
        D2 = TR.depth2(G, border)
        assert np.array_equal(D2, np.tile(d2, reps)), ("depth2", border)
        for cap in caps:
            table = hip.thickness_cover_table(cap)
            assert np.array_equal(TR.thickness(G, cap, border, D2), np.tile(TR.thickness(P, cap, False, d2), reps)), ("T", cap, border)
            assert np.array_equal(TR.open_only(G, cap, border, D2), np.tile(TR.open_only(P, cap, False, d2), reps)), ("open", cap, border)
            for got, want in zip(TR.kept_centres(G, cap, border, table, D2), TR.kept_centres(P, cap, False, table, d2)):
                assert np.array_equal(got, np.tile(want, reps)), ("centres", cap, border)
            assert TR.visited(G, cap, border, table) == n * TR.visited(P, cap, False, table), ("visited", cap, border)


@pytest.mark.parametrize("dims, reps", [((11, 9, 7), (2, 3, 2)), ((13, 8, 9), (3, 2, 2))])
def test_tiles_with_an_empty_outer_layer_do_not_see_each_other(dims, reps):
    P = TR.tile(dims, 5, seed=sum(dims), balls=TILES[dims], noise=0.05, holes=0.02)
    top = int(TR.depth2(P, False).max())
    assert TR.outer_layer_empty(P) and min(TILE_CAPS) < top < max(TILE_CAPS) and any(1 < c <= top for c in TILE_CAPS), top
    check_tiles(P, reps)
    # what the cases compare against is the same thing
    cap = 5
    table = hip.thickness_cover_table(cap)
    want, G = TR.tiled(P, reps, cap, table), np.tile(P, reps)
    cand, kept = TR.kept_centres(G, cap, True, table)
    assert (want["candidates"], want["kept"], want["visited"]) == (int(cand.sum()), int(kept.sum()), TR.visited(G, cap, True, table))
    assert want["last"] == int(np.flatnonzero(kept)[-1]) and np.array_equal(np.tile(want["T"], reps), TR.thickness(G, cap, True))


@pytest.mark.parametrize("face", range(6))
def test_a_tile_that_touches_its_face_fails_the_tile_check(face):
    """The property needs the empty layer: a ball through one face of the tile joins its neighbour's, and the check says so."""
    dims = (11, 9, 7)
    centre = [5, 4, 3]
    centre[face // 2] = 0 if face % 2 == 0 else dims[face // 2] - 1
    P = TR.tile(dims, 5, seed=27, balls=TILES[dims], noise=0.05, holes=0.02) | TR.digital_ball(dims, centre, 2.5)
    assert not TR.outer_layer_empty(P)
    with pytest.raises(AssertionError):
        check_tiles(P, (2, 3, 2), caps=(5, 17))
    with pytest.raises(AssertionError):
        TR.tiled(P, (2, 3, 2), 5)


@pytest.mark.parametrize("dims", [(12, 7, 5), (9, 9, 9), (20, 3, 6), (1, 8, 8), (15, 14, 13)])
def test_full_box_by_levels_in_closed_form(dims):
    S = np.ones(dims[::-1], bool)
    for cap in (1, 2, 5, 10, 17, 36, 37, 50):
        assert np.array_equal(TR.full_box_thickness(dims, cap), TR.thickness(S, cap, True)), (dims, cap)


# ---- sets constant over the cross-section: the reduction to a line, what the GPU case on the longest axes rests on ------------------

@pytest.fixture(scope="module")
def short_line():
    line = TR.runs_line(640, seed=7, longest=120)
    line[400:] = False
    line[404:] = True      # the last run, 236 long, through the far end: its depth passes 128, a core at cap 2^14
    return line


def line_against_the_literal_reference(line, axis, shape, caps):
    """The reduction of `line` against the literal reference on the box of `shape` with the line along `axis`, all five quantities
    and the ball voxels at every cap; returns, per cap, whether depths below it, depths at or above it and kept centres occur."""
    S = TR.along(line, shape, axis)
    cross = tuple(n for a, n in enumerate(shape) if a != axis)
    d2 = TR.depth2(S, False)
    depths = np.unique(d2[S])
    seen = set()
    for cap in caps:
        table = hip.thickness_cover_table(cap)
        red = TR.line_reduction(line, cap, table)
        for key, want in (("depth2", d2), ("T", TR.thickness(S, cap, False, d2)), ("open", TR.open_only(S, cap, False, d2))):
            assert red[key].dtype == np.int32 and np.array_equal(TR.along(red[key], shape, axis), want), (key, cap)
        for key, want in zip(("candidates", "kept"), TR.kept_centres(S, cap, False, table, d2)):
            assert np.array_equal(TR.along(red[key], shape, axis), want), (key, cap)
        assert TR.line_visited(red, cross) == TR.visited(S, cap, False, table), cap
        seen.add((bool((depths < cap).any()), bool((depths >= cap).any()), bool(red["kept"].any())))
    return seen


@pytest.mark.parametrize("axis, shape", list(zip((2, 1, 0), TR.SHORT_SHAPES)))
def test_line_reduction_against_the_literal_reference(short_line, axis, shape):
    # caps below, among (twice) and - but for the run through the end, which gives cap 2^14 its core - above the run depths
    seen = line_against_the_literal_reference(short_line, axis, shape, (1, 5, 401, hip.THICK_MAX_RADIUS2))
    assert {s[:2] for s in seen} == {(False, True), (True, True)} and (True, True, True) in seen
    # without that run every depth is below 2^14 (the run from position 0 reaches 120^2): a cap above them all, no core, no opening
    inner = short_line[:403]
    assert inner[0] and not inner[-1] and len(inner) > 128
    short = tuple(len(inner) if a == axis else n for a, n in enumerate(shape))
    assert line_against_the_literal_reference(inner, axis, short, (401, hip.THICK_MAX_RADIUS2)) == {(True, True, True), (True, False, True)}
    red = TR.line_reduction(inner, hip.THICK_MAX_RADIUS2, hip.thickness_cover_table(hip.THICK_MAX_RADIUS2))
    assert not (red["open"] == hip.THICK_MAX_RADIUS2).any() and np.array_equal(red["open"], red["depth2"])
    S = TR.along(short_line, shape, axis)
    d2 = TR.depth2(S, False)
    # with the border on depth2' is the line's, min the border term: at most 4 on these cross-sections
    want = TR.depth2(S, True)
    assert np.array_equal(np.where(S, np.minimum(d2, TR.border_term(shape)), 0), want) and int(want.max()) == 4
    table = hip.thickness_cover_table(401)
    _, kept = TR.kept_centres(S, 401, True, table, want)
    assert kept.any() and TR.visited_small(want, kept) == TR.visited(S, 401, True, table)
