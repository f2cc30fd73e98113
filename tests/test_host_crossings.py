"""Signed crossing numbers without a GPU: the vectorised numpy reference (tests/crossings_ref.py) against the definition as a
scalar loop over voxels, rays and triangles; properties and known answers of the reference; the plain C++ of
o2v_dev_k18_crossings.hpp compiled for the host and run against the reference (and one mutation seen to fail); the argument
checks and the calls of obj2voxel_amd.dense.crossing_numbers / winding_fill with the device calls stubbed; the C refusals that
need no device; the K18 kernels in the gfx950 code object."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests import crossings_ref as R
from tests import fill_ref

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip, meshes  # noqa: E402
from tests.test_host_dense import HIPCC, SRC, StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401

K18 = os.path.join(SRC, "o2v_dev_k18_crossings.hpp")
SUBSETS = ("x", "y", "z", "xy", "yz", "zx", "xyz")


def sphere24():
    """weld(uv_sphere(8)) in the sample space of a 24^3 grid (wound inwards)"""
    return (fill_ref.weld(meshes.uv_sphere(8)) * 10.3 + 12.1).astype(np.float32).reshape(-1, 3, 3)


def cube_soup():
    """an open box, a closed tetrahedron, a triangle with vertices on line centres, a degenerate and a non-finite triangle"""
    box = (meshes.unit_cube().reshape(-1, 3, 3) * 3.0 + 0.8)[:10]
    a, b, c, d = np.array([[1.2, 0.7, 0.9], [4.6, 1.1, 1.3], [2.2, 4.4, 0.6], [2.9, 2.1, 4.7]])
    tetra = np.array([[a, b, c], [a, d, b], [a, c, d], [b, d, c]])
    flat = np.array([[[0.5, 0.5, 2.5], [3.5, 0.5, 2.5], [3.5, 3.5, 2.5]], [[1.5, 2.5, 1.5], [1.5, 2.5, 1.5], [4.0, 1.0, 2.0]],
                     [[np.nan, 1.0, 1.0], [2.0, 3.0, 1.0], [4.0, 1.0, 4.0]]])
    return np.concatenate([box, tetra, flat]).astype(np.float32)


# ---- the reference ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ss", [1, 2])
def test_reference_against_a_scalar_loop(ss):
    G = 5
    sv = cube_soup() * ss
    rays = R.crossing_numbers_scalar(sv, G, ss, rays=True)
    for a in "xyz":
        D, U = R.ray_sums(sv, G, ss, a)
        assert np.array_equal(D, rays[a][0]) and np.array_equal(U, rays[a][1]), a
        assert np.abs(D).max() > 0 and np.abs(U).max() > 0
    for axes in SUBSETS:
        want = sum(rays[a][0] + rays[a][1] for a in axes)
        assert np.array_equal(R.crossing_numbers(sv, G, ss, axes), want), axes
    rng = np.random.default_rng(18)
    soup = (rng.uniform(-1.5, 6.5, (9, 3, 3)) * ss).astype(np.float32)
    soup[3] = np.round(soup[3]) + 0.5 * ss   # (vertices on centres)
    for axes in ("xyz", "y"):
        assert np.array_equal(R.crossing_numbers(soup, G, ss, axes), R.crossing_numbers_scalar(soup, G, ss, axes)), axes


def test_closed_meshes_all_six_rays_agree_and_z_is_the_parity_set():
    cube = meshes.unit_cube().reshape(-1, 3, 3)
    tetra_in_cube = np.concatenate([cube * 9.2 + 3.37, cube_soup()[10:14] * 1.3 + 4.1]).astype(np.float32)
    for sv, G, ss in ((sphere24(), 24, 1), (sphere24() * 2, 24, 2), (tetra_in_cube, 16, 1)):
        assert fill_ref.odd_edges(sv) == []
        sums = [s for a in "xyz" for s in R.ray_sums(sv, G, ss, a)]
        assert all(np.array_equal(s, sums[0]) for s in sums)
        Sz = R.crossing_numbers(sv, G, ss, "z")
        assert np.array_equal(Sz, 2 * sums[0])
        odd = np.argwhere((Sz // 2) % 2 != 0)   # [z, y, x]
        keys = np.sort((odd[:, 2] * G + odd[:, 1]) * G + odd[:, 0])
        assert len(keys) > 100 and np.array_equal(keys, fill_ref.parity_keys(sv, G, ss))


def test_flipping_every_triangle_negates():
    sv = cube_soup()[:15]
    for axes in ("xyz", "x", "yz"):
        S = R.crossing_numbers(sv, 6, 1, axes)
        assert np.abs(S).max() > 0 and np.array_equal(R.crossing_numbers(sv[:, ::-1], 6, 1, axes), -S)


def test_a_coordinate_permuted_mesh_gives_the_permuted_grid():
    """(x', y', z') = (y, z, x): the voxel (x', y', z') is the old voxel (z', x', y'), and the rays along x' are the old rays
    along y - with their (u, v, w) = (z, x, y) = (y', z', x'), which pins the convention per axis."""
    sv = np.random.default_rng(21).uniform(-1.0, 7.0, (8, 3, 3)).astype(np.float32)
    G = 6
    old = {a: R.ray_sums(sv, G, 1, a) for a in "xyz"}
    assert len({old[a][0].tobytes() for a in "xyz"}) == 3   # (the soup tells the axes apart)
    new_sv = sv[:, :, [1, 2, 0]]
    for new_axis, old_axis in (("x", "y"), ("y", "z"), ("z", "x")):
        D, U = R.ray_sums(new_sv, G, 1, new_axis)
        assert np.array_equal(D, old[old_axis][0].transpose(2, 0, 1)) and np.array_equal(U, old[old_axis][1].transpose(2, 0, 1)), new_axis
    assert np.array_equal(R.crossing_numbers(new_sv, G), R.crossing_numbers(sv, G).transpose(2, 0, 1))


# ---- known answers ----------------------------------------------------------------------------------------------------------------

def test_known_answer_closed_sphere():
    S = R.crossing_numbers(sphere24(), 24)
    assert int((S == -6).sum()) == 4289 and int((S == 0).sum()) == 24 ** 3 - 4289   # (uv_sphere is wound inwards)
    assert int(R.inside(S, 3).sum()) == 4289 and int(R.inside(S, 3, "positive").sum()) == 0
    assert int(R.inside(-S, 3, "positive").sum()) == 4289


def two_cubes():
    cube = meshes.unit_cube()
    return np.concatenate([cube * 16 + 4.03, cube * 16 + 10.07]).astype(np.float32)


def cpu_solidify(surface):
    """dense.solidify's labels on the host: the empty voxels that no 6-connected path of empty voxels joins to the border are 2"""
    empty = ~surface
    ext = np.zeros(surface.shape, bool)
    ext[0], ext[-1], ext[:, 0], ext[:, -1], ext[:, :, 0], ext[:, :, -1] = True, True, True, True, True, True
    ext &= empty
    while True:
        grown = ext.copy()
        grown[1:] |= ext[:-1]
        grown[:-1] |= ext[1:]
        grown[:, 1:] |= ext[:, :-1]
        grown[:, :-1] |= ext[:, 1:]
        grown[:, :, 1:] |= ext[:, :, :-1]
        grown[:, :, :-1] |= ext[:, :, 1:]
        grown &= empty
        if np.array_equal(grown, ext):
            break
        ext = grown
    return np.where(surface, 1, np.where(ext, 0, 2)).astype(np.uint8)


def test_known_answer_two_cubes_and_the_fill_is_solidify_s():
    """The README's two cubes at resolution 40, with the oracle's surface voxels: the vote's labels are the flood's, 33 636
    interior voxels, (15, 15, 15) among them; parity (S_z / 2 odd) hollows the overlap out."""
    G = 40
    v = two_cubes()
    p = v.reshape(-1, 3)
    xf = oracle.mesh_transform(np.concatenate([p.min(axis=0), p.max(axis=0)]), G)
    sv = fill_ref.sample_vertices(v, xf)
    S = R.crossing_numbers(sv, G)
    assert [int((S == k).sum()) for k in (0, 6, 12)] == [21054, 37114, 5832] and int(np.isin(S, (0, 6, 12)).sum()) == G ** 3
    Sz = R.crossing_numbers(sv, G, 1, "z")
    assert int(((Sz // 2) % 2 != 0).sum()) == 37114 and int(R.inside(S, 3).sum()) == 42946
    vox = oracle.voxelize(v, G)
    surface = np.zeros((G, G, G), bool)
    surface[vox[:, 2], vox[:, 1], vox[:, 0]] = True
    labels = R.labels(S, surface, 3)
    assert np.array_equal(labels, cpu_solidify(surface))
    assert labels[15, 15, 15] == 2 and int((labels == 2).sum()) == 33636


def test_known_answer_sphere_with_one_triangle_removed():
    """Under the default vote the sphere without a triangle that faces z is the closed sphere's set: the hole is seen by one
    ray of six.  (A hole in an oblique triangle is seen by three rays from the few voxels right behind it.)  The z rays
    alone, and the parity rule, lose the columns over the hole; so does the flood of the oracle's surface voxels."""
    closed, hole = sphere24(), np.delete(sphere24(), R.R_HOLE, axis=0)
    S, H = R.crossing_numbers(closed, 24), R.crossing_numbers(hole, 24)
    assert np.array_equal(R.inside(H, 3), R.inside(S, 3)) and int(R.inside(H, 3).sum()) == 4289
    assert int((H != S).sum()) > 0 and set(np.unique(np.abs(H))) == {0, 1, 5, 6}
    Hz = R.crossing_numbers(hole, 24, 1, "z")
    assert int(R.inside(Hz, 1).sum()) < 4289
    odd = np.argwhere((R.crossing_numbers(closed, 24, 1, "z") // 2) % 2 != 0)
    assert len(fill_ref.parity_keys(hole, 24, 1)) < len(odd)
    # the same on the grid the device sees (the mesh scaled to fill 24^3), with the oracle's surface voxels
    model = fill_ref.weld(meshes.uv_sphere(8))
    p = model.reshape(-1, 3)
    xf = oracle.mesh_transform(np.concatenate([p.min(axis=0), p.max(axis=0)]), 24)
    grids = {}
    for name, v in (("closed", model), ("hole", np.delete(model, R.R_HOLE, axis=0))):
        vox = oracle.voxelize(v, 24, bounds=np.concatenate([p.min(axis=0), p.max(axis=0)]))
        surface = np.zeros((24, 24, 24), bool)
        surface[vox[:, 2], vox[:, 1], vox[:, 0]] = True
        vote = R.labels(R.crossing_numbers(fill_ref.sample_vertices(v, xf), 24), surface, 3)
        grids[name] = (vote, cpu_solidify(surface))
    assert np.array_equal(*grids["closed"])
    vote, flood = grids["hole"]
    assert int((flood == 2).sum()) < int((vote == 2).sum()) and bool((vote[grids["closed"][0] == 2] == 2).all())


def test_known_answer_open_box():
    """A cube without its +z face: five rays of six see it closed, so the vote fills it; the z rays alone do not."""
    cube = meshes.unit_cube().reshape(-1, 3, 3) * 9.0 + 3.2
    top = np.all(cube[:, :, 2] == cube[:, :, 2].max(), axis=1)
    assert int(top.sum()) == 2
    closed, open_box = cube.astype(np.float32), cube[~top].astype(np.float32)
    want = R.inside(R.crossing_numbers(closed, 16), 3)
    assert int(want.sum()) == 729   # (the centres 3.5 ... 11.5 per axis)
    S = R.crossing_numbers(open_box, 16)
    assert np.array_equal(R.inside(S, 3), want) and set(np.unique(S[want])) == {5}
    assert int(R.inside(R.crossing_numbers(open_box, 16, 1, "z"), 1).sum()) == 0


# ---- the kernel's own plain C++ on the host ------------------------------------------------------------------------------------------

HOST_CR = r"""
#include <cmath>
#include <cstdint>
#define O2V_CR_HOST
#define O2V_CR_FN static inline
using std::floor; using std::fmax; using std::fmin;
%s
// One line as k_cross_mark and k_cross_prefix treat it: n crossings (height, sigma) added to the deltas of a box of nw layers
// from w0 and to the line's total, then the walk along w.
extern "C" void cr_line_host(const double *hgt, const int32_t *sigma, uint32_t n, uint32_t w0, uint32_t nw, uint32_t ss, int32_t *delta, int32_t *out)
{
    int32_t total = 0;
    for (uint32_t k = 0; k < nw; ++k) delta[k] = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const CrAdd a = cr_add(hgt[i], sigma[i], w0, nw, ss);
        if (a.layer < nw) delta[a.layer] += a.delta;
        total += a.total;
    }
    int32_t d = 0;
    for (uint32_t k = 0; k < nw; ++k) {
        d += delta[k];
        out[k] = cr_value(d, total);
    }
}
extern "C" uint32_t cr_layer_host(double hgt, uint32_t w0, uint32_t nw, uint32_t ss) { return cr_layer(hgt, w0, nw, ss); }
"""


@pytest.fixture(scope="module")
def host_cr(tmp_path_factory):
    """build(defines) -> the library: the plain C++ part of o2v_dev_k18_crossings.hpp, compiled for the host."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    if not shutil.which(cxx) and not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    k18 = open(K18).read()
    text = k18[k18.index("// The layer of a box of nw layers"):k18.index("// ---- kernels")]
    tmp = tmp_path_factory.mktemp("host_cr")

    def build(defines=()):
        name = "cr_%d" % len(list(tmp.iterdir()))
        (tmp / (name + ".cpp")).write_text(HOST_CR % text)
        subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC"] + ["-D" + d for d in defines] +
                       [str(tmp / (name + ".cpp")), "-o", str(tmp / (name + ".so"))], check=True, capture_output=True)
        L = C.CDLL(str(tmp / (name + ".so")))
        L.cr_line_host.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p]
        L.cr_line_host.restype = None
        L.cr_layer_host.argtypes = [C.c_double] + [C.c_uint32] * 3
        L.cr_layer_host.restype = C.c_uint32
        return L
    return build


def line_want(hgt, sigma, w0, nw, ss):
    """D + U at the centres of the layers w0 ... w0 + nw - 1 of one line, by the definition"""
    centres = (np.arange(w0, w0 + nw) * ss + 0.5 * ss)[:, None]
    below = centres > np.asarray(hgt)[None, :]
    s = np.asarray(sigma)[None, :]
    return (-(s * below).sum(axis=1) + (s * ~below).sum(axis=1)).astype(np.int32)


def run_line(L, hgt, sigma, w0, nw, ss):
    hgt, sigma = np.ascontiguousarray(hgt, np.float64), np.ascontiguousarray(sigma, np.int32)
    delta, out = np.zeros(nw, np.int32), np.full(nw, 77, np.int32)
    L.cr_line_host(hgt.ctypes.data, sigma.ctypes.data, len(hgt), w0, nw, ss, delta.ctypes.data, out.ctypes.data)
    return out


def test_lines_on_the_host(host_cr):
    L = host_cr()
    # k0: the first k with k ss + ss/2 > height, clamped to the box; heights on centres, below 0, far above
    for ss in (1, 2):
        h = 0.5 * ss
        for w0, nw in ((0, 8), (3, 4), (7, 1), (65000, 535)):
            for hgt in (-1e30, -3.0, 0.0, h, np.nextafter(h, 0), np.nextafter(h, 9), w0 * ss + h, np.nextafter(w0 * ss + h, 0), (w0 + 1) * ss,
                        (w0 + nw - 1) * ss + h, np.nextafter((w0 + nw - 1) * ss + h, 0), (w0 + nw) * ss + 3.0, 1e30):
                centres = np.arange(w0, w0 + nw) * ss + h
                want = int(np.argmax(centres > hgt)) if (centres > hgt).any() else nw
                assert L.cr_layer_host(hgt, w0, nw, ss) == want, (ss, w0, nw, hgt)
    rng = np.random.default_rng(181)
    for trial in range(300):
        ss = 1 + trial % 2
        w0, nw = int(rng.integers(0, 9)), int(rng.integers(1, 12))
        n = int(rng.integers(0, 9))
        hgt = rng.uniform(-3, (w0 + nw + 3) * ss, n)
        on = rng.random(n) < 0.3   # some on centres
        hgt[on] = rng.integers(0, w0 + nw + 2, int(on.sum())) * ss + 0.5 * ss
        sigma = rng.choice([-1, 1], n)
        assert np.array_equal(run_line(L, hgt, sigma, w0, nw, ss), line_want(hgt, sigma, w0, nw, ss)), (trial, hgt, sigma, w0, nw, ss)
    # a closed outward pair around the box's middle: 2 inside, 0 outside, whatever part of the line the box is
    for w0, nw in ((0, 10), (4, 3), (0, 3), (8, 2)):
        want = np.where((np.arange(w0, w0 + nw) >= 3) & (np.arange(w0, w0 + nw) < 7), 2, 0)
        assert np.array_equal(run_line(L, [2.9, 6.9], [-1, 1], w0, nw, 1), want), (w0, nw)


def test_the_dropped_crossings_above_the_box_are_caught_on_the_host(host_cr):
    """With O2V_CR_MUTATE_DROP_ABOVE a crossing above the box's last centre is lost from T.  A box that ends below the mesh's
    top then differs; one that reaches above every crossing does not."""
    good, bad = host_cr(), host_cr(("O2V_CR_MUTATE_DROP_ABOVE",))
    hgt, sigma = [2.9, 6.9], [-1, 1]
    assert np.array_equal(run_line(bad, hgt, sigma, 0, 10, 1), run_line(good, hgt, sigma, 0, 10, 1))
    want = line_want(hgt, sigma, 0, 5, 1)
    assert np.array_equal(run_line(good, hgt, sigma, 0, 5, 1), want) and list(want) == [0, 0, 0, 2, 2]
    assert not np.array_equal(run_line(bad, hgt, sigma, 0, 5, 1), want)


# ---- dense.crossing_numbers / winding_fill against a stub --------------------------------------------------------------------------

class CrossStub(StubVoxelizer):
    """crossings_dense records its arguments and writes `value` into every voxel of the box through the strides."""

    def __init__(self, value=0, **kw):
        super().__init__(**kw)
        self.value, self.tensors = value, {}

    def crossings_dense(self, resolution, axes, origin, dims, dst_ptr, dst_strides, *, supersampling=1, unit_transform=None, bounds=None):
        self.calls.append(dict(res=resolution, axes=axes, origin=tuple(origin), dims=tuple(dims), dst=dst_ptr, strides=tuple(dst_strides),
                               ss=supersampling, unit=unit_transform, bounds=bounds))

    def write_dense(self, ptr, code, origin, dims, strides):
        self.calls.append(("write", ptr, code, tuple(origin), tuple(dims), tuple(strides)))
        return 0

    def cross_calls(self):
        return [c for c in self.calls if isinstance(c, dict)]


def test_crossing_numbers_arguments_strides_and_ranges(on_cpu):  # noqa: F811
    dv = CrossStub()
    S, origin = dense.crossing_numbers(dv, 8)
    c = dv.calls[-1]
    assert origin == (0, 0, 0) and S.dtype == torch.int32 and tuple(S.shape) == (8, 8, 8) and S.is_contiguous() and len(dv.calls) == 1
    assert (c["res"], c["axes"], c["origin"], c["dims"], c["dst"], c["strides"], c["ss"]) == (8, 7, (0, 0, 0), (8, 8, 8), S.data_ptr(), (1, 8, 64), 1)
    for axes, mask in (("x", 1), ("y", 2), ("z", 4), ("xy", 3), ("zx", 5), ("zy", 6), ("zyx", 7)):
        dense.crossing_numbers(dv, 8, axes=axes)
        assert dv.calls[-1]["axes"] == mask
    # origin without out: the grid from there on; the sampling arguments reach the library
    S, origin = dense.crossing_numbers(dv, 9, origin=(1, 2, 3), supersampling=2, unit_transform=[1, 0, 0, 0, 0, 1, 0, 1, 0], bounds=[0, 0, 0, 1, 1, 1])
    c = dv.calls[-1]
    assert origin == (1, 2, 3) and tuple(S.shape) == (6, 7, 8) and c["dims"] == (8, 7, 6) and c["origin"] == (1, 2, 3)
    assert c["ss"] == 2 and c["unit"] == [1, 0, 0, 0, 0, 1, 0, 1, 0] and c["bounds"] == [0, 0, 0, 1, 1, 1]
    # permuted and sliced outputs, written as they are
    buf = torch.zeros((5, 7, 6), dtype=torch.int32)          # [x][z][y]
    view = buf.permute(1, 2, 0)                              # [z, y, x]
    S, _ = dense.crossing_numbers(dv, 8, out=view, origin=(1, 0, 1))
    c = dv.calls[-1]
    assert S is view and c["dst"] == buf.data_ptr() and c["strides"] == (42, 1, 6) and c["dims"] == (5, 6, 7)
    batch = torch.zeros((2, 4, 4, 8), dtype=torch.int32)
    dense.crossing_numbers(dv, 8, out=batch[1][:, :, ::2])
    c = dv.calls[-1]
    assert c["dst"] == batch[1].data_ptr() and c["strides"] == (2, 8, 32) and c["dims"] == (4, 4, 4)
    # max_layers: z ranges into the one tensor
    n = len(dv.calls)
    out = torch.zeros((7, 3, 4), dtype=torch.int32)
    dense.crossing_numbers(dv, 8, out=out, origin=(0, 1, 1), max_layers=3)
    got = dv.calls[n:]
    assert [(c["origin"], c["dims"]) for c in got] == [((0, 1, 1), (4, 3, 3)), ((0, 1, 4), (4, 3, 3)), ((0, 1, 7), (4, 3, 1))]
    assert [c["dst"] for c in got] == [out[0].data_ptr(), out[3].data_ptr(), out[6].data_ptr()] and all(c["strides"] == (1, 4, 12) for c in got)


def test_winding_fill_votes_on_the_two_grids(on_cpu, monkeypatch):  # noqa: F811
    calls = []
    surface = torch.zeros((4, 4, 4), dtype=torch.uint8)
    surface[1, 1, 1] = 1
    S = torch.zeros((4, 4, 4), dtype=torch.int32)
    S[1, 1, 1], S[2, 2, 2], S[2, 2, 1], S[0, 0, 0], S[3, 3, 3] = 6, 4, 3, -4, -6

    def voxelize_dense(dv, resolution, **kw):
        calls.append(("voxelize_dense", resolution, kw))
        if kw["out"] is not None:
            kw["out"].copy_(surface)
            return kw["out"], (0, 0, 0)
        return surface.clone(), (1, 2, 3) if kw["box"] == "tight" else (0, 0, 0)

    def crossing_numbers(dv, resolution, **kw):
        calls.append(("crossing_numbers", resolution, kw))
        kw["out"].copy_(S)
        return kw["out"], kw["origin"]
    monkeypatch.setattr(dense, "voxelize_dense", voxelize_dense)
    monkeypatch.setattr(dense, "crossing_numbers", crossing_numbers)
    dv = CrossStub()
    got = dense.winding_fill(dv, 4)
    assert len(got) == 2 and got[1] == (0, 0, 0) and got[0].dtype == torch.uint8
    want = surface.clone()
    want[2, 2, 2] = want[0, 0, 0] = want[3, 3, 3] = 2
    assert torch.equal(got[0], want)                      # (the surface voxel keeps 1; |S| = 3 is below len(axes) + 1)
    v, c = calls[0], calls[1]
    assert v[2]["fmt"] == "labels" and v[2]["box"] == "grid" and "fill" not in v[2] and c[2]["axes"] == "xyz" and c[2]["origin"] == (0, 0, 0)
    assert tuple(c[2]["out"].shape) == (4, 4, 4) and c[2]["out"].dtype == torch.int32
    pos = dense.winding_fill(dv, 4, rule="positive")[0]
    assert int(pos[2, 2, 2]) == 2 and int(pos[0, 0, 0]) == 0 and int(pos[3, 3, 3]) == 0
    low = dense.winding_fill(dv, 4, min_sum=3)[0]
    assert int(low[2, 2, 1]) == 2
    one = dense.winding_fill(dv, 4, axes="z", min_sum=2)[0]
    assert calls[-1][2]["axes"] == "z" and int(one[2, 2, 1]) == 2
    with pytest.raises(ValueError):
        dense.winding_fill(dv, 4, axes="z", min_sum=3)
    # the sampling arguments go to both; the tight box's origin goes to the crossing numbers
    calls.clear()
    _, origin = dense.winding_fill(dv, 9, box="tight", supersampling=2, strategy="blend", unit_transform=[1] * 9, bounds=[0] * 6, max_layers=5)
    assert origin == (1, 2, 3) and calls[1][2]["origin"] == (1, 2, 3)
    for _, res, kw in calls:
        assert res == 9 and kw["supersampling"] == 2 and kw["unit_transform"] == [1] * 9 and kw["bounds"] == [0] * 6 and kw["max_layers"] == 5
    assert calls[0][2]["strategy"] == "blend" and calls[0][2]["box"] == "tight"
    # out: cleared, written and returned
    out = torch.full((2, 4, 4, 4), 9, dtype=torch.uint8)
    got, _ = dense.winding_fill(dv, 8, out=out[1], origin=(1, 1, 1))
    assert got.data_ptr() == out[1].data_ptr() and torch.equal(out[1], want) and bool((out[0] == 9).all())


def test_the_wait_comes_before_the_library_call(monkeypatch):
    dv = CrossStub()
    order = []
    monkeypatch.setattr(dense, "_device", lambda dv: torch.device("cpu"))
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: True)
    monkeypatch.setattr(dense, "_sync", lambda device: order.append("sync"))
    monkeypatch.setattr(dv, "crossings_dense", lambda *a, **kw: order.append("crossings"))
    dense.crossing_numbers(dv, 4, max_layers=2)
    assert order == ["sync", "crossings", "crossings"]
    order.clear()
    monkeypatch.setattr(dv, "voxelize", lambda *a, **kw: order.append("voxelize") or 1)
    monkeypatch.setattr(dv, "write_dense", lambda *a, **kw: order.append("write") or 0)
    dense.winding_fill(dv, 4)
    assert order == ["sync", "voxelize", "write", "sync", "crossings"]


_I32 = torch.zeros((4, 4, 4), dtype=torch.int32)
_U8 = torch.zeros((4, 4, 4), dtype=torch.uint8)


@pytest.mark.parametrize("fn, kw, exc", [
    ("crossing_numbers", dict(axes=7), TypeError),
    ("crossing_numbers", dict(axes=("x", "y")), TypeError),
    ("crossing_numbers", dict(axes=""), ValueError),
    ("crossing_numbers", dict(axes="xw"), ValueError),
    ("crossing_numbers", dict(axes="xx"), ValueError),
    ("crossing_numbers", dict(axes="XYZ"), ValueError),
    ("crossing_numbers", dict(resolution=0), ValueError),
    ("crossing_numbers", dict(supersampling=3), ValueError),
    ("crossing_numbers", dict(max_layers=0), ValueError),
    ("crossing_numbers", dict(origin=(0, 0)), ValueError),
    ("crossing_numbers", dict(origin=(0, -1, 0)), ValueError),
    ("crossing_numbers", dict(origin=(0, 0, 8)), ValueError),
    ("crossing_numbers", dict(out=torch.zeros((4, 4, 4))), TypeError),
    ("crossing_numbers", dict(out=torch.zeros((4, 4), dtype=torch.int32)), ValueError),
    ("crossing_numbers", dict(out=torch.zeros((4, 0, 4), dtype=torch.int32)), ValueError),
    ("crossing_numbers", dict(out=torch.zeros((4, 4, 4), device="meta", dtype=torch.int32)), ValueError),
    ("crossing_numbers", dict(out=_I32, origin=(5, 0, 0)), ValueError),
    ("crossing_numbers", dict(out=torch.zeros((9, 4, 4), dtype=torch.int32)), ValueError),
    ("winding_fill", dict(axes=None), TypeError),
    ("winding_fill", dict(axes="zz"), ValueError),
    ("winding_fill", dict(rule="parity"), ValueError),
    ("winding_fill", dict(min_sum=0), ValueError),
    ("winding_fill", dict(min_sum=7), ValueError),
    ("winding_fill", dict(axes="xy", min_sum=5), ValueError),
    ("winding_fill", dict(min_sum=4.0), TypeError),
    ("winding_fill", dict(min_sum=True), TypeError),
    ("winding_fill", dict(min_sum="4"), TypeError),
    ("winding_fill", dict(box="loose"), ValueError),
    ("winding_fill", dict(strategy="min"), ValueError),
    ("winding_fill", dict(resolution=0), ValueError),
    ("winding_fill", dict(supersampling=4), ValueError),
    ("winding_fill", dict(max_layers=0), ValueError),
    ("winding_fill", dict(resolution=40000, supersampling=2), ValueError),
    ("winding_fill", dict(box="tight", origin=(0, 0, 0)), ValueError),
    ("winding_fill", dict(out=_I32), TypeError),
    ("winding_fill", dict(out=torch.zeros((4, 4), dtype=torch.uint8)), ValueError),
    ("winding_fill", dict(out=torch.zeros((4, 0, 4), dtype=torch.uint8)), ValueError),
    ("winding_fill", dict(out=torch.zeros((4, 4, 4), device="meta", dtype=torch.uint8)), ValueError),
    ("winding_fill", dict(out=_U8, origin=(5, 0, 0)), ValueError),
    ("winding_fill", dict(out=_U8, origin=(0, -1, 0)), ValueError),
])
def test_rejects_before_any_device_call(on_cpu, fn, kw, exc):  # noqa: F811
    dv = CrossStub()
    kw = dict(kw)
    res = kw.pop("resolution", 8)
    with pytest.raises(exc):
        getattr(dense, fn)(dv, res, **kw)
    assert not dv.calls
    assert bool((_U8 == 0).all())


def test_the_docstrings_say_what_the_numbers_mean():
    doc = " ".join(dense.winding_fill.__doc__.split())
    assert "|S| >= min_sum" in doc and "S >= min_sum" in doc and "len(axes) + 1" in doc and "fill=True" in doc
    assert "2 len(axes) inside and 0 outside" in " ".join(dense.crossing_numbers.__doc__.split())
    assert "winding_fill" in dense.__doc__ and "section 21" in dense.__doc__


# ---- the C refusals that need no device ------------------------------------------------------------------------------------------------

def test_c_refusals_without_a_context():
    L = hip._bind()
    ms = (C.c_float * 3)(5, 5, 5)
    assert L.o2v_hip_crossings_times(None, ms) == hip.ERR_BAD_ARGUMENT and list(ms) == [5, 5, 5]
    p = hip.DeviceVoxelizer._params(8, 1, 0, None, None, (0, 0))
    dst = np.full(8, 7, np.int32)
    u3, u6 = C.c_uint32 * 3, C.c_uint64 * 3
    rc = L.o2v_hip_crossings_dense(None, C.byref(p), 7, u3(0, 0, 0), u3(2, 2, 2), dst.ctypes.data, u6(1, 2, 4))
    assert rc == hip.ERR_BAD_ARGUMENT and (dst == 7).all()
    header = open(os.path.join(SRC, "..", "..", "include", "o2v_hip.h")).read()
    assert "int o2v_hip_crossings_dense(o2v_hip_ctx *ctx, const o2v_hip_params *params, uint32_t axes" in header
    assert "int o2v_hip_crossings_times(const o2v_hip_ctx *ctx, float out_ms[3]);" in header


# ---- the kernels in the code object ------------------------------------------------------------------------------------------------

K18_KERNELS = ["k_cross_countILi0E", "k_cross_countILi1E", "k_cross_countILi2E", "k_cross_markILi0E", "k_cross_markILi1E", "k_cross_markILi2E",
               "k_cross_prefixILb0E", "k_cross_prefixILb1E", "k_cross_prefix_tileILb0E", "k_cross_prefix_tileILb1E"]


@pytest.mark.parametrize("kernel", K18_KERNELS)
def test_k18_kernels_in_the_code_object(device_asm, kernel):  # noqa: F811
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    name, body = m.group(1), m.group(2)
    entry = [e for e in device_asm[device_asm.index("amdhsa.kernels:"):].split("\n  - ") if re.search(r"\.name: +" + re.escape(name) + r"\n", e)]
    assert len(entry) == 1
    assert re.search(r"\.wavefront_size: +64\b", entry[0]) and re.search(r"\.max_flat_workgroup_size: +256\b", entry[0])
    if "mark" in kernel:
        assert len(re.findall(r"global_atomic_add\w*\s", body)) == 2   # the delta and the line's total
    else:
        assert "atomic" not in body
    if "prefix" in kernel:
        assert re.search(r"\.private_segment_fixed_size: +0\b", entry[0]) and "scratch_" not in body
        lds = 4 * 64 * 33 * 4 + 4 * 64 * 8 if "tile" in kernel else 0   # per wave a tile of 64 lines x (32 + 1) layers and 64 row offsets
        assert re.search(r"\.group_segment_fixed_size: +%d\b" % lds, entry[0])
