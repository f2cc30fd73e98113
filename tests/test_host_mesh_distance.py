"""The narrow-band distance to the triangles without a GPU: the numpy reference's d2 against exact rational arithmetic, the
band-culled reference against the unculled one, the argument checks and call sequence of dense.mesh_distance with the device
call stubbed, and a static check of the K9 kernels in the gfx950 code object."""
import re
from fractions import Fraction

import numpy as np
import pytest

from obj2voxel_amd import meshes
from tests import fill_ref
from tests import mesh_distance_ref as R

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_dense import StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401


# ---- d2 against exact arithmetic ---------------------------------------------------------------------------------------

def _fdot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _fsub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _fcross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _fseg(p, u, v):
    e, w = _fsub(v, u), _fsub(p, u)
    ee = _fdot(e, e)
    t = Fraction(0) if ee == 0 else min(max(_fdot(w, e) / ee, Fraction(0)), Fraction(1))
    q = [w[k] - t * e[k] for k in range(3)]
    return _fdot(q, q)


def exact_d2(p, a, b, c):
    """The squared distance from p to the closed triangle abc in rationals: the projection if it lies inside, else the nearest
    edge (a degenerate triangle is its edges)."""
    p, a, b, c = ([Fraction(float(x)) for x in v] for v in (p, a, b, c))
    n = _fcross(_fsub(b, a), _fsub(c, a))
    nn = _fdot(n, n)
    if nn > 0:
        s = [_fdot(n, _fcross(_fsub(v, u), _fsub(p, u))) for u, v in ((a, b), (b, c), (c, a))]
        if all(x >= 0 for x in s):
            h = _fdot(n, _fsub(p, a))
            return h * h / nn
    return min(_fseg(p, a, b), _fseg(p, b, c), _fseg(p, c, a))


def _cases(rng):
    """(p, a, b, c) with float32 vertices: random, over the face, near each edge and vertex, and degenerate triangles."""
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)   # noqa: E731
    out = []
    for _ in range(200):
        a, b, c = (f32(rng.uniform(0, 64, 3)) for _ in range(3))
        out.append((rng.uniform(-8, 72, 3), a, b, c))
        n = np.cross(b - a, c - a)
        n = n / np.linalg.norm(n)
        w = rng.dirichlet([1, 1, 1])
        over = w[0] * a + w[1] * b + w[2] * c
        out.append((over + n * rng.uniform(0.5, 4), a, b, c))                           # over the face
        out.append((over, a, b, c))                                                     # on the face
        for u, v in ((a, b), (b, c), (c, a)):
            t = rng.uniform(0.05, 0.95)
            e = u + t * (v - u)
            out.append((e + rng.normal(0, 1, 3), a, b, c))                              # near an edge
            out.append((u + rng.normal(0, 0.5, 3), a, b, c))                            # near a vertex
            out.append((u + (u - v) * rng.uniform(0.1, 1), a, b, c))                    # beyond a vertex along the edge line
    for _ in range(100):
        a, d = f32(rng.uniform(0, 64, 3)), f32(rng.uniform(-4, 4, 3))
        p = rng.uniform(-8, 72, 3)
        out.append((p, a, f32(a + d), f32(a + 2 * d)))                                  # collinear (up to float32 rounding)
        out.append((p, a, a, f32(a + 3 * d)))                                           # two equal vertices
        out.append((p, a, a, a))                                                        # all equal
        out.append((p, a, f32(a + np.array([4, 0, 0])), f32(a + np.array([8, 0, 0]))))  # exactly collinear
    return out


def test_d2_against_exact_arithmetic():
    rng = np.random.default_rng(2024)
    cases = _cases(rng)
    p = np.array([c[0] for c in cases])
    a, b, c = (np.array([x[k] for x in cases]) for k in (1, 2, 3))
    got = R.d2(p, a, b, c)
    # relative 1e-12; within 0.1 sample of a face h = n.ap cancels to a few ulps of |n||ap| (vertices up to 64 samples apart):
    # there the bound is absolute, 1e-14 squared samples
    worst = 0.0
    for i, case in enumerate(cases):
        e = exact_d2(*case)
        err = abs(Fraction(float(got[i])) - e)
        if e >= Fraction(1, 100):
            assert err <= Fraction(1, 10 ** 12) * e, (i, case, float(got[i]), float(e))
            worst = max(worst, float(err / e))
        else:
            assert err <= Fraction(1, 10 ** 14), (i, case, float(got[i]), float(e))
    assert 0 < worst < 1e-12


def test_d2_single_values():
    a, b, c = np.array([0., 0, 0]), np.array([4., 0, 0]), np.array([0., 4, 0])
    assert R.d2(np.array([1., 1, 3]), a, b, c) == 9.0         # over the face
    assert R.d2(np.array([-3., 0, 4]), a, b, c) == 25.0       # off a vertex
    assert R.d2(np.array([2., -1, 0]), a, b, c) == 1.0        # off an edge, in the plane
    assert R.d2(np.array([1., 1, 0]), a, b, c) == 0.0
    assert R.d2(np.array([1., 1, 1]), a, a, a) == 3.0         # a point triangle


# ---- band culling ------------------------------------------------------------------------------------------------------

def _mixed_soup():
    rng = np.random.default_rng(9)
    v = meshes.random_soup(60, seed=4).reshape(-1, 3, 3) * 20 + 16
    deg = np.array([[[3, 3, 3], [9, 9, 9], [15, 15, 15]],       # collinear
                    [[20, 5, 7], [20, 5, 7], [26, 9, 7]],       # two equal vertices
                    [[12, 24, 18], [12, 24, 18], [12, 24, 18]]], np.float32)
    return np.concatenate([v.astype(np.float32), deg, rng.uniform(0, 32, (6, 3, 3)).astype(np.float32)])


@pytest.mark.parametrize("band", [0.5, 1.0, 2.5, 8.0])
@pytest.mark.parametrize("ss", [1, 2])
def test_culled_reference_equals_unculled(band, ss):
    sv = _mixed_soup() * ss
    G = 24
    got = R.mesh_distance(sv, G, ss, band, signed=False)
    want = R.mesh_distance(sv, G, ss, band, signed=False, cull=False)
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)) and np.array_equal(got[1], want[1])
    assert (got[0] < band).any() and (got[0] == np.float32(band)).any()


def test_band_is_a_float32():
    """The call takes the band as a float and widens that: 2.6 means float32(2.6) = 2.599999904..., which is the distance of
    voxel (1, 1, 0) from the plane z = float32(3.1), so that voxel is at the band, not inside it."""
    z = np.float32(3.1)
    sv = np.array([[[0, 0, z], [4, 0, z], [0, 4, z]]], np.float32)
    a = R.mesh_distance(sv, 8, 1, 2.6, False)
    b = R.mesh_distance(sv, 8, 1, float(np.float32(2.6)), False)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])
    assert a[1][0, 1, 1] == -1 and a[0][0, 1, 1] == np.float32(2.6)
    assert int((a[0] < np.float32(2.6)).sum()) == int((a[1] >= 0).sum()) == 116
    pts = np.array([[1, 1, 0], [1, 1, 1], [7, 7, 7]])
    for band in (2.6, float(np.float32(2.6))):
        v, i = R.point_distance(pts, sv, 1, band)
        assert i.tolist() == [-1, 0, -1] and v.tolist() == [np.float32(2.6), np.float32(z - np.float32(1.5)), np.float32(2.6)]
    lo, hi = R.dilated_aabb(sv, 2.6, 2)
    assert lo[0, 0] == -(np.float64(np.float32(2.6)) * 2 + 2) and hi[0, 2] == np.float64(z) + (np.float64(np.float32(2.6)) * 2 + 2)


def test_threshold_band():
    for D in (6.25, 2.0, 7.3, 1e-6, 63.999):
        f, narrow = R.threshold_band(D)
        g = np.nextafter(f, np.float32(0))
        assert f.dtype == np.float32 and np.float64(f) * np.float64(f) > D >= np.float64(g) * np.float64(g)
        assert narrow == (np.float64(np.float32(f * f)) <= D)
    assert R.threshold_band(6.25)[0] == np.nextafter(np.float32(2.5), np.float32(3))


def test_reference_box_equals_grid_and_sign():
    sv = fill_ref.sample_vertices(fill_ref.weld(meshes.uv_sphere(10)), _xform(20))
    G, band = 20, 2.5
    vals, idx = R.mesh_distance(sv, G, 1, band, signed=True)
    assert (vals < 0).any() and (vals > 0).any() and (idx >= 0).any() and (idx == -1).any()
    sub = R.mesh_distance(sv, G, 1, band, signed=True, origin=(3, 5, 7), dims=(9, 4, 11))
    assert np.array_equal(sub[0].view(np.int32), vals[7:18, 5:9, 3:12].view(np.int32)) and np.array_equal(sub[1], idx[7:18, 5:9, 3:12])
    uns = R.mesh_distance(sv, G, 1, band, signed=False)[0]
    assert np.array_equal(np.abs(vals).view(np.int32), uns.view(np.int32))
    # an empty mesh: +band everywhere
    e, ei = R.mesh_distance(np.zeros((0, 3, 3), np.float32), 4, 1, 1.5, signed=True)
    assert (e == np.float32(1.5)).all() and (ei == -1).all()


def _xform(G):
    """A mesh transform of the unit sphere into a G^3 grid (scale and offset only)."""
    s = np.float32((G - 0.5) / 2)
    return np.array([s, 0, 0, 0, s, 0, 0, 0, s, s + 0.25, s + 0.25, s + 0.25], np.float32)


# ---- dense.mesh_distance against a stub --------------------------------------------------------------------------------

class MeshDistStub(StubVoxelizer):
    def mesh_distance_dense(self, resolution, band, fmt, origin, dims, dst_ptr, dst_strides, closest_ptr=None, closest_strides=None,
                            **kw):
        self.calls.append(("meshdist", resolution, band, fmt, tuple(origin), tuple(dims), dst_ptr, tuple(dst_strides), closest_ptr,
                           None if closest_strides is None else tuple(closest_strides), kw))


def test_mesh_distance_whole_grid_and_formats():
    dv = MeshDistStub()
    out, origin = dense.mesh_distance(dv, 12, band=2)
    assert out.dtype == torch.float32 and tuple(out.shape) == (12, 12, 12) and origin == (0, 0, 0)
    c = dv.calls[-1]
    assert c[:6] == ("meshdist", 12, 2.0, hip.MESH_DIST_SIGNED_F32, (0, 0, 0), (12, 12, 12))
    assert c[6] == out.data_ptr() and c[7] == (1, 12, 144) and c[8] is None and c[9] is None
    assert c[10] == dict(supersampling=1, unit_transform=None, bounds=None)
    out, idx, origin = dense.mesh_distance(dv, 12, band=0.5, signed=False, closest=True, origin=(2, 3, 4), supersampling=2,
                                           bounds=np.zeros(6, np.float32))
    assert tuple(out.shape) == (8, 9, 10) and idx.dtype == torch.int32 and tuple(idx.shape) == (8, 9, 10) and origin == (2, 3, 4)
    c = dv.calls[-1]
    assert c[3] == hip.MESH_DIST_UNSIGNED_F32 and c[4] == (2, 3, 4) and c[5] == (10, 9, 8) and c[8] == idx.data_ptr()
    assert c[10]["supersampling"] == 2 and c[10]["bounds"] is not None


def test_mesh_distance_strided_out_and_closest():
    dv = MeshDistStub()
    batch = torch.zeros((2, 6, 7, 5))
    out = batch[1].permute(1, 0, 2)                      # [z=7, y=6, x=5], strides (5, 35, 1)
    idx = torch.zeros((5, 7, 6), dtype=torch.int32).permute(1, 2, 0)   # [7, 6, 5]
    got, ci, origin = dense.mesh_distance(dv, 16, band=3, out=out, closest=idx, origin=(1, 2, 3))
    assert got.data_ptr() == out.data_ptr() and ci is idx and origin == (1, 2, 3)
    c = dv.calls[-1]
    assert c[4] == (1, 2, 3) and c[5] == (5, 6, 7) and c[6] == batch[1].data_ptr()
    assert c[7] == (1, 35, 5) and c[9] == (42, 1, 6)


def test_mesh_distance_max_layers_origins():
    dv = MeshDistStub()
    out = torch.zeros((10, 3, 4))
    idx = torch.zeros((10, 3, 4), dtype=torch.int32)
    dense.mesh_distance(dv, 32, band=1, out=out, closest=idx, origin=(5, 6, 7), max_layers=4)
    calls = [c for c in dv.calls if c[0] == "meshdist"]
    assert [c[4] for c in calls] == [(5, 6, 7), (5, 6, 11), (5, 6, 15)]
    assert [c[5] for c in calls] == [(4, 3, 4), (4, 3, 4), (4, 3, 2)]
    assert [c[6] for c in calls] == [out[z].data_ptr() for z in (0, 4, 8)]
    assert [c[8] for c in calls] == [idx[z].data_ptr() for z in (0, 4, 8)]


@pytest.mark.parametrize("kw, exc", [
    (dict(band=0), ValueError), (dict(band=-1.0), ValueError), (dict(band=float("nan")), ValueError),
    (dict(band=32.5), ValueError), (dict(band=float("inf")), ValueError), (dict(band="2"), ValueError),
    (dict(band=1, out=torch.zeros((4, 4, 4), dtype=torch.float64)), TypeError),
    (dict(band=1, out=torch.zeros((4, 4)), ), ValueError),
    (dict(band=1, out=torch.zeros((4, 4, 4), device="meta")), ValueError),
    (dict(band=1, out=torch.zeros((4, 0, 4))), ValueError),
    (dict(band=1, out=torch.zeros((4, 4, 4)), origin=(0, 0, 13)), ValueError),
    (dict(band=1, closest=torch.zeros((16, 16, 16))), TypeError),
    (dict(band=1, out=torch.zeros((4, 4, 4)), closest=torch.zeros((4, 4, 5), dtype=torch.int32)), ValueError),
    (dict(band=1, supersampling=3), ValueError),
    (dict(band=1, max_layers=0), ValueError),
    (dict(band=1e-46), ValueError),   # (0 as a float32: refused here like every other bad band, not by the device call)
])
def test_mesh_distance_rejects(kw, exc):
    dv = MeshDistStub()
    with pytest.raises(exc):
        dense.mesh_distance(dv, 16, **kw)
    assert not dv.calls


def test_mesh_distance_rejects_closest_in_out_storage():
    dv = MeshDistStub()
    buf = torch.zeros((2, 4, 4, 4))
    with pytest.raises(ValueError, match="storage"):
        dense.mesh_distance(dv, 16, band=1, out=buf[0], closest=buf[1].view(torch.int32))
    assert not dv.calls


# ---- the code object ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["k_meshdist_bin_countE", "k_meshdist_tile_sumsE", "k_meshdist_tile_offsetsE", "k_meshdist_bin_scatterE",
                                    "k_meshdist_tilesE"])
def test_k9_kernels_in_the_code_object_without_scratch(device_asm, kernel):  # noqa: F811
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    body = m.group(2)
    scratch = re.findall(r"; ScratchSize: (\d+)", device_asm[m.end():m.end() + 4000])
    assert scratch and scratch[0] == "0", scratch[:1]
    assert "scratch_" not in body and "buffer_store_dword v" not in body.replace("buffer_store_dwordx", "")
    assert re.search(r"^\s*\.set " + re.escape(m.group(1)) + r"\.private_seg_size, 0$", device_asm, re.M)
