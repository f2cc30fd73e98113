"""Surface extraction without a GPU: the numpy reference (tests/surface_ref.py) against a scalar restatement of the header's
definition, the properties of the meshes it gives, its round trip through the project's own distance and parity definitions,
the argument checks and call sequence of dense.extract_surface with the device calls stubbed, and a static check of the K10
kernels in the gfx950 code object."""
import math
import re

import numpy as np
import pytest

from obj2voxel_amd import meshes
from tests import fill_ref
from tests import mesh_distance_ref
from tests import surface_ref as R

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_dense import StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401

F = np.float32


# ---- the reference against a scalar restatement ------------------------------------------------------------------------

def scalar_extract(f, level, origin):
    """include/o2v_hip.h, word by word: per cell, per edge, in loops; every float a numpy float32 scalar."""
    nz, ny, nx = f.shape
    level = F(level)

    def inside(x, y, z):
        return bool(f[z, y, x] < level)
    number, positions = {}, []
    with np.errstate(all="ignore"):
        for k in range(nz - 1):
            for j in range(ny - 1):
                for i in range(nx - 1):
                    ins = [inside(i + a, j + b, k + c) for c in (0, 1) for b in (0, 1) for a in (0, 1)]
                    if all(ins) or not any(ins):
                        continue
                    edges = ([((0, b, c), (1, b, c), 0) for b, c in ((0, 0), (1, 0), (0, 1), (1, 1))] +
                             [((a, 0, c), (a, 1, c), 1) for a, c in ((0, 0), (1, 0), (0, 1), (1, 1))] +
                             [((a, b, 0), (a, b, 1), 2) for a, b in ((0, 0), (1, 0), (0, 1), (1, 1))])
                    s, n = [F(0), F(0), F(0)], 0
                    for p, q, axis in edges:
                        if inside(i + p[0], j + p[1], k + p[2]) == inside(i + q[0], j + q[1], k + q[2]):
                            continue
                        fp, fq = f[k + p[2], j + p[1], i + p[0]], f[k + q[2], j + q[1], i + q[0]]
                        t = F(F(level - fp) / F(fq - fp))
                        if not (t >= 0 and t <= 1):
                            t = F(0.5)
                        point = [F(p[0]), F(p[1]), F(p[2])]
                        point[axis] = t
                        s = [F(s[m] + point[m]) for m in range(3)]
                        n += 1
                    local = [F(s[m] / F(n)) for m in range(3)]
                    number[(i, j, k)] = len(positions)
                    positions.append([F(F(F(origin[m] + (i, j, k)[m]) + F(0.5)) + local[m]) for m in range(3)])
    faces = []
    dims = (nx, ny, nz)
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                for ax in range(3):
                    c = (x, y, z)
                    u, v = (ax + 1) % 3, (ax + 2) % 3
                    if c[ax] + 1 >= dims[ax] or not (1 <= c[u] <= dims[u] - 2 and 1 <= c[v] <= dims[v] - 2):
                        continue
                    d = [0, 0, 0]
                    d[ax] = 1
                    if inside(x, y, z) == inside(x + d[0], y + d[1], z + d[2]):
                        continue

                    def cell(du, dv):
                        e = list(c)
                        e[u] -= du
                        e[v] -= dv
                        return number[tuple(e)]
                    q = [cell(1, 1), cell(0, 1), cell(0, 0), cell(1, 0)]
                    if not inside(x, y, z):
                        q = [q[0], q[3], q[2], q[1]]
                    faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return np.array(positions, F).reshape(-1, 3), np.array(faces, np.int32).reshape(-1, 3)


@pytest.mark.parametrize("dims, seed", [((5, 6, 7), 0), ((4, 3, 9), 1), ((2, 2, 2), 2), ((3, 2, 5), 3), ((6, 1, 4), 4), ((2, 7, 2), 5)])
def test_reference_equals_the_scalar_restatement(dims, seed):
    rng = np.random.default_rng(seed)
    for kind in range(4):
        f = rng.normal(size=dims).astype(F)
        if kind == 1:      # NaN and infinities
            f[rng.random(dims) < 0.1] = np.nan
            f[rng.random(dims) < 0.1] = np.inf
            f[rng.random(dims) < 0.1] = -np.inf
        elif kind == 2:    # exact ties with the level, t exactly 0 and 1
            f = rng.integers(-1, 2, size=dims).astype(F)
        elif kind == 3:    # any bit pattern
            f = rng.integers(0, 2 ** 32, size=dims, dtype=np.uint64).astype(np.uint32).view(F)
        for level, origin in ((0.0, (0, 0, 0)), (0.25, (3, 65000, 17)), (-1.0, (1, 2, 3))):
            got_p, got_f = R.extract(f, level, origin)
            want_p, want_f = scalar_extract(f, level, origin)
            assert got_p.shape == want_p.shape and np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32)), (kind, level)
            assert np.array_equal(got_f, want_f), (kind, level)
            assert np.isfinite(got_p).all()
            if min(dims) == 1:
                assert len(got_p) == 0 and len(got_f) == 0


def test_single_cell_and_flat_grids():
    one = np.ones((2, 2, 2), F)
    one[1, 1, 1] = -1
    p, f = R.extract(one, 0.0, (10, 20, 30))
    # the three edges at the inside corner cross at t = 0.5: s = 2.5 per axis, n = 3
    assert len(f) == 0 and p.shape == (1, 3)
    assert [float(v) for v in p[0]] == [float(F(o + 0.5) + F(F(2.5) / F(3))) for o in (10, 20, 30)]
    for dims in ((9, 9, 1), (1, 9, 9), (9, 1, 9)):
        p, f = R.extract(np.random.default_rng(0).normal(size=dims).astype(F), 0.0)
        assert p.shape == (0, 3) and f.shape == (0, 3) and p.dtype == F and f.dtype == np.int32


# ---- the pieces the large device cases are built from: layer ranges, strided views of a 1-D array, closed forms ---------------

def strided_view(base, dims, sx, s1, s2):
    """f(x, y, z) = base[sx x + s1 y + s2 z] as an array [z, y, x] that shares base's memory."""
    nx, ny, nz = dims
    assert sx * (nx - 1) + s1 * (ny - 1) + s2 * (nz - 1) < len(base)
    e = base.strides[0]
    return np.lib.stride_tricks.as_strided(base, (nz, ny, nx), (s2 * e, s1 * e, sx * e), writeable=False)


STRIDED = [((5, 40, 37), 1, 3, 5), ((3, 70, 29), 1, 5, 3), ((6, 33, 41), 2, 3, 7), ((2, 50, 50), 1, 2, 3), ((8, 2, 90), 3, 5, 2),
           ((4, 90, 2), 1, 1, 1), ((7, 31, 30), 1, 0, 4), ((7, 31, 30), 0, 3, 1)]


def strided_base(dims, sx, s1, s2, seed):
    rng = np.random.default_rng(seed)
    n = sx * (dims[0] - 1) + s1 * (dims[1] - 1) + s2 * (dims[2] - 1) + 1
    base = (0.3 + np.abs(rng.normal(size=n))).astype(F)
    busy = (np.arange(n) // 37) % 2 == 1                     # quiet and busy stretches
    base[busy & (rng.random(n) < 0.3)] *= F(-1)
    return base


@pytest.mark.parametrize("dims,sx,s1,s2", STRIDED)
def test_strided_views_count_and_extract_as_their_copies(dims, sx, s1, s2):
    base = strided_base(dims, sx, s1, s2, 7)
    view = strided_view(base, dims, sx, s1, s2)
    copy = np.ascontiguousarray(view)
    assert not view.flags.c_contiguous and np.shares_memory(view, base)
    level, origin, nz = 0.125, (3, 4, 5), dims[2]
    ins_view = strided_view(base < F(level), dims, sx, s1, s2)
    v_layers, q_layers = R.counts_per_layer(ins_view)
    v_copy, q_copy = R.counts_per_layer(R.inside(copy, level))
    assert np.array_equal(v_layers, v_copy) and np.array_equal(q_layers, q_copy) and v_layers.sum() > 0
    whole_p, whole_f = R.extract(copy, level, origin)
    assert (len(whole_p), len(whole_f)) == (int(v_layers.sum()), 2 * int(q_layers.sum()))
    for z0, z1 in ((0, nz - 1), (0, 1), (nz // 3, nz // 3 + 5), (nz - 2, nz - 1)):
        if not 0 <= z0 < z1 < nz:
            continue
        got = R.extract_layers(view, level, origin, z0, z1, v_layers, q_layers)
        want = R.extract_layers(copy, level, origin, z0, z1, v_layers, q_layers)
        assert got[0] == want[0] and got[2] == want[2]
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and np.array_equal(got[3], want[3])
        assert np.array_equal(whole_p[got[0]:got[0] + len(got[1])].view(np.uint32), got[1].view(np.uint32))
        assert np.array_equal(whole_f[got[2]:got[2] + len(got[3])], got[3])


@pytest.mark.parametrize("n", [2, 3, 7, 64])
def test_chained_overlapping_ranges_give_every_vertex_and_triangle(n):
    """Ranges laid end to end (z1, then z1 again) would leave out the quads of sample layer z1; layer_chunks overlaps them."""
    rng = np.random.default_rng(n)
    f = rng.normal(size=(23, 14, 9)).astype(F)
    level, origin = 0.2, (1, 2, 3)
    want_p, want_f = R.extract(f, level, origin)
    v_layers, q_layers = R.counts_per_layer(R.inside(f, level))
    got_p, got_f = np.full(want_p.shape, np.nan, F), np.full(want_f.shape, -1, np.int32)
    v_end = t_end = new_v = 0
    chunks = R.layer_chunks(f.shape[0], n)
    assert chunks[0][0] == 0 and chunks[-1][1] == f.shape[0] - 1 and all(b[0] == a[1] - 1 for a, b in zip(chunks, chunks[1:]))
    for z0, z1 in chunks:
        v0, p, t0, t = R.extract_layers(f, level, origin, z0, z1, v_layers, q_layers)
        assert v0 <= v_end and t0 == t_end           # no vertex left out; the triangles follow on exactly
        got_p[v0:v0 + len(p)], got_f[t0:t0 + len(t)] = p, t
        new_v += v0 + len(p) - v_end
        v_end, t_end = v0 + len(p), t0 + len(t)
    assert (new_v, v_end, t_end) == (len(want_p), len(want_p), len(want_f)) and len(want_f) > 1000
    assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32)) and np.array_equal(got_f, want_f)
    # ... and end to end they do not: layer 8 of 23 has quads that neither (0, 8) nor (8, 22) gives
    a, b = R.extract_layers(f, level, origin, 0, 8, v_layers, q_layers), R.extract_layers(f, level, origin, 8, 22, v_layers, q_layers)
    assert a[2] + len(a[3]) < b[2]


@pytest.mark.parametrize("dims", [(2, 2, 2), (2, 9, 7), (9, 2, 7), (9, 7, 2), (5, 6, 7), (70, 4, 4), (3, 3, 3), (1, 5, 5), (130, 3, 5)])
def test_checkerboard_closed_form(dims):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ins = (x + y + z) % 2 == 1
    v_layers, q_layers = R.counts_per_layer(ins)
    assert R.checkerboard_counts(nx, ny, nz) == (int(v_layers.sum()), int(q_layers.sum()))
    # the same grid as a view of an alternating 1-D array with strides (1, 1, 1)
    alt = np.where(np.arange(nx + ny + nz) % 2 == 1, F(-1), F(1))
    view = strided_view(alt, dims, 1, 1, 1)
    assert np.array_equal(R.inside(view, 0.0), ins)
    # per block of 256 words: at most 2^14 vertices and 3 x 2^14 quads, what the packed 16-bit prefixes hold
    v_blocks, q_blocks = R.per_block_counts(ins)
    assert v_blocks.sum() == v_layers.sum() and q_blocks.sum() == q_layers.sum() and v_blocks.max() <= 2 ** 14 and q_blocks.max() <= 3 * 2 ** 14


@pytest.mark.parametrize("dims,sx,s1,s2", STRIDED)
def test_row_tables_against_the_grid(dims, sx, s1, s2):
    nx, ny, nz = dims
    base = strided_base(dims, sx, s1, s2, 11)
    level = 0.125
    ins = np.ascontiguousarray(strided_view(base < F(level), dims, sx, s1, s2))
    tables = R.row_tables(base < F(level), nx, sx, s1, s2)
    v_rows, q_rows = R.row_counts(tables, ny, nz, s1, s2, 0, nz)
    want_v = np.zeros((nz, ny), np.int64)
    want_v[:nz - 1, :ny - 1] = R.active_cells(ins).sum(axis=2)
    assert np.array_equal(v_rows, want_v) and np.array_equal(q_rows, R.quad_edges(ins).sum(axis=(2, 3))) and want_v.sum() > 0
    for block, layers, workers in ((256, 64, 1), (16, 3, 4), (7, 5, 3)):
        v_layers, q_layers, v_blocks, q_blocks = R.grid_counts(tables, ny, nz, s1, s2, block, layers, workers)
        want_layers = R.counts_per_layer(ins)
        in_slabs = R.counts_per_layer_slabs(ins, layers, workers)
        assert np.array_equal(in_slabs[0], want_layers[0]) and np.array_equal(in_slabs[1], want_layers[1])
        assert np.array_equal(v_layers, want_layers[0]) and np.array_equal(q_layers, want_layers[1])
        want_blocks = R.per_block_counts(ins, block)
        assert np.array_equal(v_blocks, want_blocks[0]) and np.array_equal(q_blocks, want_blocks[1])


# ---- properties ----------------------------------------------------------------------------------------------------------

FIELDS = {"sphere": (lambda: R.sphere_field(48, 15.2), (2,)), "torus": (lambda: R.torus_field(48, 13, 5), (0,)),
          "two spheres": (lambda: R.two_spheres_field(48, 9, 14), (2, 4))}


@pytest.mark.parametrize("name", sorted(FIELDS))
@pytest.mark.parametrize("level", [0.0, 1.5, -2.0])
def test_closed_surfaces_are_closed_oriented_manifolds(name, level):
    make, euler = FIELDS[name]
    p, f = R.extract(make(), level)
    assert len(p) > 1000 and f.min() == 0 and f.max() == len(p) - 1 and len(np.unique(f)) == len(p)
    und, direct = R.edge_uses(f)
    assert (und == 2).all() and (direct == 1).all()
    assert R.euler(p, f) in euler
    assert R.signed_volume(p, f) > 0       # (the normals point from inside to outside)


def test_sphere_volume():
    p, f = R.extract(R.sphere_field(48, 15.2), 0.0)
    ball = 4 / 3 * math.pi * 15.2 ** 3
    assert abs(R.signed_volume(p, f) - ball) < 0.01 * ball


def test_a_surface_that_leaves_the_box_is_open_there():
    p, f = R.extract(R.sphere_field((20, 30, 40), 17.3), 0.0, (1, 2, 3))
    assert len(f) > 0 and f.min() >= 0 and f.max() < len(p)
    und, direct = R.edge_uses(f)
    assert set(np.unique(und)) == {1, 2} and (direct == 1).all()
    assert len(np.unique(f)) <= len(p)     # (a vertex of a border cell may be used by no face)


# ---- round trip through the project's own definitions --------------------------------------------------------------------

def _vertex_distance(p, sv):
    """sqrt of the smallest d2 (tests/mesh_distance_ref.py) from every point of p [n, 3] to the triangles sv [T, 3, 3]."""
    out = np.empty(len(p))
    for lo in range(0, len(p), 512):
        q = p[lo:lo + 512].astype(np.float64)[:, None, :]
        out[lo:lo + 512] = np.sqrt(mesh_distance_ref.d2(q, sv[None, :, 0], sv[None, :, 1], sv[None, :, 2]).min(axis=1))
    return out


@pytest.mark.parametrize("level", [0.0, 1.5, -1.5])
def test_round_trip_mesh_distance_surface_parity(level):
    """The extracted surface of a signed TSDF, filled by the parity definition of the solid fill, is the set {f < level}
    exactly, and its vertices lie within sqrt(3) voxels of the level set: a vertex lies in its cell, the field is 1-Lipschitz
    and the level set passes through the cell.  (Not for fields with exact ties: an integer-valued field puts vertices on
    voxel centres, where the parity definition's perturbation decides, so such fields are kept out of this assertion.)"""
    G = 40
    verts = fill_ref.weld(meshes.uv_sphere(12))
    sv = (verts.reshape(-1, 3, 3).astype(np.float64) * 13.3 + np.array([20.2, 19.7, 20.4])).astype(F)   # sample space, ss 1
    assert not fill_ref.odd_edges(sv)
    field, _ = mesh_distance_ref.mesh_distance(sv, G, 1, 3.0, True)
    assert (field < 0).any() and (field == F(3)).any() and (field == F(-3)).any()
    assert not (field == F(level)).any()
    p, f = R.extract(field, level)
    und, direct = R.edge_uses(f)
    assert (und == 2).all() and (direct == 1).all()
    keys = fill_ref.parity_keys(p[f], G, 1)
    z, y, x = np.nonzero(field < F(level))
    assert len(keys) > 5000 and np.array_equal(np.sort((x.astype(np.int64) * G + y) * G + z), keys)
    worst = np.abs(_vertex_distance(p, sv) - abs(level)).max()
    print("level", level, "voxels", len(keys), "largest | distance - |level| |", worst)
    assert worst <= math.sqrt(3)


@pytest.mark.parametrize("make", [lambda: R.sphere_field(40, 12.7), lambda: R.torus_field(40, 11, 4.3)])
def test_round_trip_analytic_fields(make):
    field = make()
    for level in (0.0, 1.5, -1.5):
        assert not (field == F(level)).any()
        p, f = R.extract(field, level)
        z, y, x = np.nonzero(field < F(level))
        assert np.array_equal(np.sort((x.astype(np.int64) * 40 + y) * 40 + z), fill_ref.parity_keys(p[f], 40, 1))


# ---- dense.extract_surface against a stub --------------------------------------------------------------------------------

class SurfaceStub(StubVoxelizer):
    """surface_count answers (v, t); surface_write fills the two arrays (the stub's "device" is the host) with a ramp."""

    def __init__(self, v=5, t=4):
        super().__init__()
        self.v, self.t = v, t

    def surface_count(self, field_ptr, strides, dims, level):
        self.calls.append(("count", field_ptr, tuple(strides), tuple(dims), level))
        return self.v, self.t

    def surface_write(self, field_ptr, strides, dims, level, origin, positions_ptr, vertex_capacity, faces_ptr, triangle_capacity):
        self.calls.append(("write", field_ptr, tuple(strides), tuple(dims), level, tuple(origin), positions_ptr, vertex_capacity, faces_ptr,
                           triangle_capacity))
        C = hip.C
        pos = np.ctypeslib.as_array(C.cast(positions_ptr, C.POINTER(C.c_float)), (vertex_capacity * 3,))
        pos[:] = np.arange(vertex_capacity * 3, dtype=F) * F(0.25) + F(1)
        if triangle_capacity:
            fac = np.ctypeslib.as_array(C.cast(faces_ptr, C.POINTER(C.c_int32)), (triangle_capacity * 3,))
            fac[:] = np.arange(triangle_capacity * 3) % vertex_capacity


def test_extract_surface_counts_allocates_and_writes():
    dv = SurfaceStub(v=5, t=4)
    field = torch.zeros((6, 7, 8))
    p, f = dense.extract_surface(dv, field, 1.5, origin=(1, 2, 3))
    assert p.dtype == torch.float32 and tuple(p.shape) == (5, 3) and p.is_contiguous()
    assert f.dtype == torch.int32 and tuple(f.shape) == (4, 3) and f.is_contiguous()
    assert [c[0] for c in dv.calls] == ["count", "write"]
    assert dv.calls[0][1:] == (field.data_ptr(), (1, 8, 56), (8, 7, 6), 1.5)
    w = dv.calls[1]
    assert w[1:6] == (field.data_ptr(), (1, 8, 56), (8, 7, 6), 1.5, (1, 2, 3))
    assert w[6] == p.data_ptr() and w[7] == 5 and w[8] == f.data_ptr() and w[9] == 4
    assert p[1, 0] == 1.75 and f[1, 1] == 4
    # the level is the float32 the call takes
    dense.extract_surface(dv, field, 0.1)
    assert dv.calls[-1][4] == float(F(0.1)) and dv.calls[-2][4] == float(F(0.1))


def test_extract_surface_strided_field():
    dv = SurfaceStub()
    batch = torch.zeros((2, 6, 7, 5))
    field = batch[1].permute(1, 0, 2)          # [z = 7, y = 6, x = 5], strides (5, 35, 1)
    dense.extract_surface(dv, field)
    assert dv.calls[0][1:] == (batch[1].data_ptr(), (1, 35, 5), (5, 6, 7), 0.0)
    assert dv.calls[1][5] == (0, 0, 0)


def test_extract_surface_empty_result():
    dv = SurfaceStub(v=0, t=0)
    p, f = dense.extract_surface(dv, torch.zeros((3, 3, 3)))
    assert tuple(p.shape) == (0, 3) and tuple(f.shape) == (0, 3) and p.dtype == torch.float32 and f.dtype == torch.int32
    assert [c[0] for c in dv.calls] == ["count"]
    # vertices without faces (one cell): positions are written, no face array is passed
    dv = SurfaceStub(v=1, t=0)
    p, f = dense.extract_surface(dv, torch.zeros((2, 2, 2)))
    assert tuple(p.shape) == (1, 3) and tuple(f.shape) == (0, 3) and dv.calls[-1][8] is None and dv.calls[-1][9] == 0


def test_extract_surface_transform_maps_back_to_model_space():
    dv = SurfaceStub(v=6, t=2)
    xf = np.array([3.5, 0.25, 0, 0, -2.0, 0.5, 1.0, 0, 4.0, 10.0, -3.0, 0.75], F)
    voxel, _ = dense.extract_surface(dv, torch.zeros((4, 4, 4)))
    for ss in (1, 2):
        model, faces = dense.extract_surface(dv, torch.zeros((4, 4, 4)), transform=xf, supersampling=ss)
        assert model.dtype == torch.float32 and tuple(model.shape) == (6, 3) and model.is_contiguous()
        # pushed forward by hand: A m + t is the sample-space point ss * p
        a, t = xf[:9].reshape(3, 3).astype(np.float64), xf[9:].astype(np.float64)
        forward = model.numpy().astype(np.float64) @ a.T + t
        assert np.allclose(forward, voxel.numpy().astype(np.float64) * ss, rtol=0, atol=1e-5)
        exact = np.linalg.solve(a, (voxel.numpy().astype(np.float64) * ss - t).T).T
        assert np.abs(model.numpy() - exact).max() <= 2.0 ** -23 * np.abs(exact).max()
    assert torch.equal(dense.extract_surface(dv, torch.zeros((4, 4, 4)), transform=torch.tensor(xf))[0],
                       dense.extract_surface(dv, torch.zeros((4, 4, 4)), transform=list(xf))[0])


@pytest.mark.parametrize("kw, exc", [
    (dict(level=float("nan")), ValueError), (dict(level=float("inf")), ValueError), (dict(level="0"), ValueError),
    (dict(level=True), ValueError), (dict(level=1e39), ValueError),
    (dict(field=torch.zeros((4, 4, 4), dtype=torch.float64)), TypeError),
    (dict(field=torch.zeros((4, 4))), ValueError),
    (dict(field=np.zeros((4, 4, 4), F)), ValueError),
    (dict(field=torch.zeros((4, 4, 4), device="meta")), ValueError),
    (dict(field=torch.zeros((4, 0, 4))), ValueError),
    (dict(origin=(0, 0)), ValueError), (dict(origin=(0, -1, 0)), ValueError),
    (dict(origin=(65533, 0, 0)), ValueError), (dict(origin=(0, 0, 65533)), ValueError),
    (dict(transform=np.zeros(9, F)), ValueError),
    (dict(supersampling=3), ValueError),
])
def test_extract_surface_rejects(kw, exc):
    dv = SurfaceStub()
    args = dict(field=torch.zeros((4, 4, 4)), level=0.0)
    args.update(kw)
    with pytest.raises(exc):
        dense.extract_surface(dv, args.pop("field"), args.pop("level"), **args)
    assert not dv.calls


def test_extract_surface_accepts_the_last_origin():
    dv = SurfaceStub()
    dense.extract_surface(dv, torch.zeros((4, 4, 4)), origin=(65532, 0, 65532))
    assert dv.calls[1][5] == (65532, 0, 65532)


def test_refused_when_the_library_came_first(monkeypatch):
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: False)
    with pytest.raises(RuntimeError, match="before torch"):
        dense.extract_surface(SurfaceStub(), torch.zeros((4, 4, 4)))


# ---- the code object -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["k_surf_signsE", "k_surf_countE", "k_surf_verticesILb0E", "k_surf_verticesILb1E", "k_surf_facesE"])
def test_k10_kernels_in_the_code_object_without_scratch(device_asm, kernel):  # noqa: F811
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    body = m.group(2)
    scratch = re.findall(r"; ScratchSize: (\d+)", device_asm[m.end():m.end() + 4000])
    assert scratch and scratch[0] == "0", scratch[:1]
    assert "scratch_" not in body and "buffer_store_dword v" not in body.replace("buffer_store_dwordx", "")
    assert re.search(r"^\s*\.set " + re.escape(m.group(1)) + r"\.private_seg_size, 0$", device_asm, re.M)
    assert "atomic" not in body            # (every order comes from the scans)
