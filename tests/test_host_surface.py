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
