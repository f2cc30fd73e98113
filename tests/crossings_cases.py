"""The GPU cases of tests/test_gpu_crossings.py, each run in a child process of its own:
`python -m tests.crossings_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison is np.array_equal against the
numpy restatement (tests/crossings_ref.py), which takes its sample-space vertices from the transform o2v_hip_voxelize reports
for the same params.  Outputs are filled with a guard value before a call.  A case prints "ok" last when everything held."""
import os
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import crossings_ref as R
from tests import fill_ref
from tests.fill_cases import exact_sign_set, power_of_two_bounds, to_model

DEV = torch.device("cuda", 0)
GUARD = 0x5A5A5A5A
SUBSETS = ("x", "y", "z", "xy", "yz", "zx", "xyz")
MIRROR = [0, 0, -1, 0, 1, 0, -1, 0, 0]   # (a permutation with a reflection, determinant -1: the mesh's orientation changes sign)


def upload(dv, verts):
    dense.set_mesh(dv, torch.from_numpy(np.ascontiguousarray(verts, np.float32).reshape(-1, 9)).to(DEV))


def sample_space(dv, verts, res, ss=1, **kw):
    """The sample-space vertices o2v_hip_voxelize's transform gives for these params (needs finite vertices in the context)."""
    dv.voxelize(res, read=False, supersampling=ss, **kw)
    return fill_ref.sample_vertices(verts, dv.transform())


def per_axis(sv, res, ss):
    """{axis: D + U of the whole grid}"""
    out = {}
    for a in "xyz":
        D, U = R.ray_sums(sv, res, ss, a)
        out[a] = D + U
    return out


def want_of(per, axes, origin=(0, 0, 0), dims=None):
    S = sum(per[a] for a in axes)
    if dims is None:
        return S
    (ox, oy, oz), (nx, ny, nz) = origin, dims
    return S[oz:oz + nz, oy:oy + ny, ox:ox + nx]


def run(dv, res, axes, origin=(0, 0, 0), dims=None, ss=1, **kw):
    """One o2v_hip_crossings_dense call into a guard-filled contiguous tensor; its values on the host."""
    dims = dims or (res, res, res)
    out = torch.full(tuple(dims[::-1]), GUARD, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    dv.crossings_dense(res, R.axes_mask(axes), origin, dims, out.data_ptr(), (1, dims[0], dims[0] * dims[1]), supersampling=ss, **kw)
    return out.cpu().numpy()


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), (what, int((got != want).sum()), got[got != want][:5], want[got != want][:5])


# ---- axes ------------------------------------------------------------------------------------------------------------------------

def case_axes():
    dv = hip.DeviceVoxelizer(0)
    n = 0
    for name, verts in (("sphere 8", fill_ref.weld(meshes.uv_sphere(8))), ("sphere 12", meshes.uv_sphere(12))):
        assert len(verts) == (224 if name == "sphere 8" else 528)
        upload(dv, verts)
        for res in (16, 24):
            for ss in (1, 2):
                for unit in (None, MIRROR):
                    sv = sample_space(dv, verts, res, ss, unit_transform=unit)
                    per = per_axis(sv, res, ss)
                    for axes in SUBSETS:
                        same(run(dv, res, axes, ss=ss, unit_transform=unit), want_of(per, axes), (name, res, ss, unit, axes))
                        n += 1
                    full = want_of(per, "xyz")
                    if name == "sphere 8":   # closed: six rays agree; uv_sphere is wound inwards, the mirror turns it round
                        assert set(np.unique(full)) == {0, 6 if unit else -6}, (np.unique(full), unit)
                    ms = dv.crossings_times()
                    assert len(ms) == 3 and all(t > 0 for t in ms), ms
    same(run(dv, 16, "y"), want_of(per_axis(sample_space(dv, verts, 16), 16, 1), "y"), "y alone")
    ms = dv.crossings_times()
    assert ms[0] == 0.0 and ms[2] == 0.0 and ms[1] > 0, ms
    # soups of open and closed pieces
    for seed in range(6):
        rng = np.random.default_rng(51000 + seed)
        verts = R.pieces(rng).astype(np.float32)
        res, ss = (16, 24, 33)[seed % 3], 1 + seed % 2
        kw = {}
        if seed % 2:
            kw["unit_transform"] = R.PERMS[seed % len(R.PERMS)]
        if seed >= 3:
            kw["bounds"] = [0.2, 0.15, 0.25, 0.8, 0.9, 0.75]   # (cuts the pieces on every side: crossings outside the grid)
        upload(dv, verts)
        per = per_axis(sample_space(dv, verts, res, ss, **kw), res, ss)
        for axes in SUBSETS:
            same(run(dv, res, axes, ss=ss, **kw), want_of(per, axes), ("soup", seed, axes))
            n += 1
        assert np.abs(want_of(per, "xyz")).max() > 0
    # an empty mesh gives 0
    dense.set_mesh(dv, torch.zeros((0, 9), device=DEV))
    assert not run(dv, 8, "xyz").any()
    print("axes: compared", n, "grids")


# ---- boxes -----------------------------------------------------------------------------------------------------------------------

def case_boxes():
    dv = hip.DeviceVoxelizer(0)
    verts = fill_ref.weld(meshes.uv_sphere(8))
    upload(dv, verts)
    res = 24
    kw = dict(bounds=[-1.7, -2.0, -2.4, 2.1, 2.0, 1.9])   # (the sphere takes about the middle half of the grid, off centre)
    sv = sample_space(dv, verts, res, **kw)
    per = per_axis(sv, res, 1)
    full = want_of(per, "xyz")
    lo = np.floor(sv.reshape(-1, 3).min(axis=0)).astype(int)
    hi = np.ceil(sv.reshape(-1, 3).max(axis=0)).astype(int)
    assert (lo >= 3).all() and (hi <= res - 3).all(), (lo, hi)
    mid = [int(v) for v in (lo + hi) // 2]
    n = 0
    boxes = [(tuple(mid), (1, 1, 1)), ((0, 0, 0), (1, 1, 1)), ((res - 1,) * 3, (1, 1, 1))]
    for a in range(3):
        o, line, layer = list(mid), [1, 1, 1], [res, res, res]
        o[a], line[a], layer[a] = 0, res, 1
        boxes.append((tuple(o), tuple(line)))                                      # one line along axis a, through the sphere
        boxes.append((tuple(mid[b] if b == a else 0 for b in range(3)), tuple(layer)))   # one layer across axis a
        for first, count in ((int(hi[a]) + 1, res - int(hi[a]) - 1),                # begins above the mesh
                             (0, mid[a]),                                          # ends below the mesh's top: crossings above the box
                             (mid[a], 2),                                          # inside: crossings below and above the box
                             (0, int(lo[a]) - 1)):                                 # wholly beside (below) the mesh
            o, d = [0, 0, 0], [res, res, res]
            o[a], d[a] = first, count
            boxes.append((tuple(o), tuple(d)))
        o, d = [2, 2, 2], [res - 5, res - 4, res - 3]                               # beside along the other two axes
        o[(a + 1) % 3], d[(a + 1) % 3] = 0, int(lo[(a + 1) % 3]) - 1
        boxes.append((tuple(o), tuple(d)))
    for origin, dims in boxes:
        for axes in ("xyz", "x", "y", "z"):
            same(run(dv, res, axes, origin, dims, **kw), want_of(per, axes, origin, dims), ("box", origin, dims, axes))
            n += 1
    # the whole grid cut into ranges along each axis: the bits of one call
    one = run(dv, res, "xyz", **kw)
    same(one, full, "one call")
    for a in range(3):
        for step in (1, 5, res):
            got = np.full((res, res, res), GUARD, np.int32)
            for first in range(0, res, step):
                o, d = [0, 0, 0], [res, res, res]
                o[a], d[a] = first, min(step, res - first)
                part = run(dv, res, "xyz", tuple(o), tuple(d), **kw)
                got[o[2]:o[2] + d[2], o[1]:o[1] + d[1], o[0]:o[0] + d[0]] = part
                n += 1
            same(got, one, ("ranges", a, step))
    # max_layers through dense
    for layers in (1, 5, 7, None):
        out = torch.full((res - 3, res, res), GUARD, dtype=torch.int32, device=DEV)
        S, origin = dense.crossing_numbers(dv, res, out=out, origin=(0, 0, 2), max_layers=layers, **kw)
        assert S is out and origin == (0, 0, 2)
        same(S.cpu().numpy(), full[2:res - 1], ("max_layers", layers))
    S, origin = dense.crossing_numbers(dv, res, axes="zx", origin=(1, 2, 3), **kw)
    assert origin == (1, 2, 3) and S.dtype == torch.int32 and S.is_contiguous()
    same(S.cpu().numpy(), want_of(per, "zx")[3:, 2:, 1:], "dense without out")
    print("boxes: compared", n, "calls")


# ---- strided outputs -------------------------------------------------------------------------------------------------------------

def case_strided():
    dv = hip.DeviceVoxelizer(0)
    verts = meshes.uv_sphere(12)
    upload(dv, verts)
    res = 20
    per = per_axis(sample_space(dv, verts, res), res, 1)
    n = 0
    for axes in ("xyz", "x", "y", "z"):
        want = want_of(per, axes)
        # a slice of a batch
        batch = torch.full((3, res, res, res), GUARD, dtype=torch.int32, device=DEV)
        dense.crossing_numbers(dv, res, axes=axes, out=batch[1])
        got = batch.cpu().numpy()
        same(got[1], want, ("batch", axes))
        assert (got[0] == GUARD).all() and (got[2] == GUARD).all()
        # [x][z][y] storage inside a larger buffer: the bands around it stay
        o, d = (2, 1, 3), (res - 5, res - 3, res - 7)   # x, y, z
        buf = torch.full((d[0] + 2, d[2] + 4, d[1] + 6), GUARD, dtype=torch.int32, device=DEV)
        view = buf[1:-1, 2:-2, 3:-3].permute(1, 2, 0)   # [z, y, x]
        assert tuple(view.shape) == d[::-1]
        dense.crossing_numbers(dv, res, axes=axes, out=view, origin=o)
        got = buf.cpu().numpy()
        same(got[1:-1, 2:-2, 3:-3].transpose(1, 2, 0), want_of(per, axes, o, d), ("xzy", axes))
        inner = np.zeros(got.shape, bool)
        inner[1:-1, 2:-2, 3:-3] = True
        assert (got[~inner] == GUARD).all(), "the bands were written"
        # every second element
        wide = torch.full((res, res, 2 * res), GUARD, dtype=torch.int32, device=DEV)
        dense.crossing_numbers(dv, res, axes=axes, out=wide[:, :, ::2])
        got = wide.cpu().numpy()
        same(got[:, :, ::2], want, ("every second", axes))
        assert (got[:, :, 1::2] == GUARD).all()
        n += 3
    # A/B: without the LDS-staged tile (the rays along the tensor's unit stride) the same bits
    os.environ["O2V_CROSS_NO_TILE"] = "1"
    try:
        for axes in ("xyz", "x"):
            same(run(dv, res, axes), want_of(per, axes), ("no tile", axes))
            o, d = (2, 1, 3), (res - 5, res - 3, res - 7)
            buf = torch.full((d[0], d[2], d[1]), GUARD, dtype=torch.int32, device=DEV)   # [x][z][y]: the y rays run along the unit stride
            dense.crossing_numbers(dv, res, axes=axes, out=buf.permute(1, 2, 0), origin=o)
            same(buf.cpu().numpy().transpose(1, 2, 0), want_of(per, axes, o, d), ("no tile, xzy", axes))
            n += 2
    finally:
        del os.environ["O2V_CROSS_NO_TILE"]
    print("strided: compared", n, "outputs")


# ---- exact signs -----------------------------------------------------------------------------------------------------------------

def _square(c0, c1, hgt):
    """two triangles of the square [c0, c1]^2 at the height hgt: vertices on centres, the diagonal through centres"""
    a, b, c, d = (c0, c0, hgt), (c1, c0, hgt), (c1, c1, hgt), (c0, c1, hgt)
    return np.array([a + b + c, a + c + d], np.float32).reshape(-1, 3, 3)


def case_exact():
    dv = hip.DeviceVoxelizer(0)
    n = 0
    for G, ss in ((96, 1), (64, 2)):
        upload(dv, meshes.unit_cube())
        bounds, m = power_of_two_bounds(dv, G, ss)
        base, _ = exact_sign_set(23 + ss, G, ss)
        h = 0.5 * ss
        flat = np.concatenate([_square(2 * ss + h, 9 * ss + h, 5 * ss + h), _square(3 * ss + h, 7 * ss + h, 6 * ss + h)[:, ::-1]])
        rng = np.random.default_rng(61000 + ss)
        lattice = R.lattice(R.pieces(rng), G * ss, ss).reshape(-1, 3, 3).astype(np.float32)
        for what, sv0 in (("exact set", base), ("on centres", flat), ("lattice", lattice)):
            for shift in range(3):   # the cyclic coordinate permutations: each axis meets the exact zeros
                sv = np.ascontiguousarray(np.roll(sv0, shift, axis=2))
                v = to_model(sv, m)
                upload(dv, v)
                dv.voxelize(G, read=False, supersampling=ss, bounds=bounds)
                assert np.array_equal(fill_ref.sample_vertices(v, dv.transform()), sv)
                fill_ref.EXACT.update(calls=0, nonzero=0)
                per = per_axis(sv, G, ss)
                if what == "exact set":
                    assert fill_ref.EXACT["nonzero"] >= len(sv0), fill_ref.EXACT   # only the exact value decides these signs
                else:
                    assert fill_ref.EXACT["calls"] > fill_ref.EXACT["nonzero"], fill_ref.EXACT   # exact zeros: the perturbation
                for axes in ("xyz", "x", "y", "z"):
                    same(run(dv, G, axes, ss=ss, bounds=bounds), want_of(per, axes), (what, G, ss, shift, axes))
                    n += 1
                assert np.abs(want_of(per, "xyz")).max() > 0
    print("exact: compared", n, "grids")


# ---- many triangles, one large triangle ------------------------------------------------------------------------------------------

def case_many():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(71000)
    T = 66000   # (258 blocks of 256 triangles: the block-sum scan's second trip)
    c = rng.random((T, 1, 3))
    verts = (c + 0.09 * (rng.random((T, 3, 3)) - 0.5)).astype(np.float32).reshape(T, 9)
    upload(dv, verts)
    res = 16
    per = per_axis(sample_space(dv, verts, res), res, 1)
    for axes in ("xyz", "x", "y", "z"):
        same(run(dv, res, axes), want_of(per, axes), ("many", axes))
    assert np.abs(want_of(per, "xyz")).max() > 3
    for origin, dims in (((3, 4, 5), (9, 8, 7)), ((0, 0, 8), (16, 16, 8))):
        same(run(dv, res, "xyz", origin, dims), want_of(per, "xyz", origin, dims), ("many", origin))
    # one triangle as large as the box, cut by the user bounds on every side
    big = np.array([[-1.0, -1.2, 0.2, 3.1, -0.9, 0.45, -0.8, 3.3, 0.8]], np.float32)
    upload(dv, big)
    res, kw = 64, dict(bounds=[0, 0, 0, 1, 1, 1])
    per = per_axis(sample_space(dv, big, res, **kw), res, 1)
    for axes in ("xyz", "x", "y", "z"):
        same(run(dv, res, axes, **kw), want_of(per, axes), ("large", axes))
    assert set(np.unique(want_of(per, "z"))) == {-1, 1} or set(np.unique(want_of(per, "z"))) == {-1, 0, 1}
    print("many: 66000 triangles and one large one")


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def expect_code(code, fn, what):
    try:
        fn()
    except hip.DeviceError as e:
        assert f"code {code}" in str(e) and "o2v_hip_crossings_dense" in str(e), (what, str(e))
        return what + ": " + str(e)
    raise AssertionError(what + " was accepted")


def case_refusals():
    dv = hip.DeviceVoxelizer(0)
    verts = fill_ref.weld(meshes.uv_sphere(8))
    upload(dv, verts)
    n = 40
    dims, st = (n, n, n), (1, n, n * n)
    want = want_of(per_axis(sample_space(dv, verts, n), n, 1), "xyz")
    full = torch.full((n, n, n), GUARD, dtype=torch.int32, device=DEV)
    short = torch.full((n // 2, n, n), GUARD, dtype=torch.int32, device=DEV)
    line = torch.full((65536,), GUARD, dtype=torch.int32, device=DEV)
    host = np.zeros((n, n, n), np.int32)
    torch.cuda.synchronize()
    F = full.data_ptr()

    def good():
        """After a refusal nothing was written and the context still works."""
        assert bool((full == GUARD).all()) and bool((short == GUARD).all()) and bool((line == GUARD).all()) and not host.any()
        same(run(dv, n, "xyz"), want, "after a refusal")

    def c(dst=F, axes=7, origin=(0, 0, 0), d=dims, strides=st, res=n, **kw):
        return lambda: dv.crossings_dense(res, axes, origin, d, dst, strides, **kw)

    def raw(params=True, origin=True, d=True, dst=True, strides=True, zslab=(0, 0)):
        """the C call itself: a null argument, a slab field of params"""
        def fn():
            p = dv._params(n, 1, 0, None, None, zslab)
            u3, u6 = hip.C.c_uint32 * 3, hip.C.c_uint64 * 3
            dv._check(dv._L.o2v_hip_crossings_dense(dv._ctx, hip.C.byref(p) if params else None, 7, u3(0, 0, 0) if origin else None,
                                                    u3(*dims) if d else None, F if dst else None, u6(*st) if strides else None),
                      "o2v_hip_crossings_dense")
        return fn

    refusals = [
        (3, raw(params=False), "null params"),
        (3, raw(origin=False), "null origin"),
        (3, raw(d=False), "null dims"),
        (3, raw(dst=False), "null dst"),
        (3, raw(strides=False), "null strides"),
        (3, raw(zslab=(0, 8)), "a slab in params"),
        (3, c(axes=0), "axes 0"),
        (3, c(axes=8), "axes 8"),
        (3, c(res=0, d=(1, 1, 1)), "resolution 0"),
        (3, c(supersampling=3), "supersampling 3"),
        (3, c(d=(n, 0, n)), "zero dims"),
        (3, c(origin=(1, 0, 0)), "box past the grid along x"),
        (3, c(origin=(0, 0, n), d=(n, n, 1)), "box past the grid along z"),
        (3, c(strides=(1, n // 2, n * n)), "y inside x"),
        (3, c(strides=(0, 1, n)), "a stride of 0"),
        (3, c(dst=short.data_ptr()), "short dst"),
        (3, c(dst=host.ctypes.data), "host dst"),
        (5, c(dst=line.data_ptr(), res=70000, d=(65536, 1, 1), strides=(1, 65536, 65536)), "65 536 voxels along x"),
        (5, c(dst=line.data_ptr(), res=70000, d=(1, 1, 65536), strides=(1, 1, 1)), "65 536 voxels along z"),
    ]
    msgs = []
    for code, fn, what in refusals:
        msgs.append(expect_code(code, fn, what))
        good()
    assert all("one element" in t for t in msgs if t.startswith(("y inside x", "a stride of 0"))), msgs
    # through dense: an expand()ed out
    try:
        dense.crossing_numbers(dv, n, out=line[:n].view(1, 1, n).expand(n, n, n))
        raise AssertionError("an expanded out was accepted")
    except hip.DeviceError as e:
        assert "code 3" in str(e), str(e)
    good()
    # 65 535 voxels along an axis are accepted
    dv.crossings_dense(70000, 7, (0, 0, 0), (65535, 1, 1), line.data_ptr(), (1, 65536, 65536))
    torch.cuda.synchronize()
    assert int(line[65535]) == GUARD and not bool((line[:65535] == GUARD).any())
    line.fill_(GUARD)
    # 2 x 3 rays x triangles above 2^31 - 1: all three axes are refused, one axis is within the limit
    T = (2 ** 31 - 1) // 6 + 1
    faces = torch.zeros((T, 3), dtype=torch.int32, device=DEV)
    dense.set_mesh(dv, torch.zeros((1, 3), device=DEV), faces)
    del faces
    msgs.append(expect_code(5, c(axes=7), "2 x 3 x %d triangles" % T))
    assert bool((full == GUARD).all())
    dv.crossings_dense(n, 4, (0, 0, 0), (2, 2, 2), full.data_ptr(), st)   # (degenerate triangles: no crossing)
    torch.cuda.synchronize()
    assert not bool(full[:2, :2, :2].any()) and int((full == GUARD).sum()) == n ** 3 - 8
    full.fill_(GUARD)
    upload(dv, verts)
    good()
    print("\n".join(msgs))
    print("refused", len(msgs) + 1)


# ---- the fill --------------------------------------------------------------------------------------------------------------------

def host(t):
    return t.cpu().numpy()


def case_fill():
    dv = hip.DeviceVoxelizer(0)
    # the README's two cubes: the overlap stays
    cube = meshes.unit_cube()
    two = np.concatenate([cube * 16 + 4.03, cube * 16 + 10.07]).astype(np.float32)
    upload(dv, two)
    labels, origin = dense.winding_fill(dv, 40)
    assert origin == (0, 0, 0) and labels.dtype == torch.uint8 and tuple(labels.shape) == (40, 40, 40)
    surface, _ = dense.voxelize_dense(dv, 40, fmt="labels")
    solid = dense.solidify(dv, surface)
    assert torch.equal(labels, solid), int((labels != solid).sum())
    assert int(labels[15, 15, 15]) == 2 and int((labels == 2).sum()) == 33636, int((labels == 2).sum())
    parity, _ = dense.voxelize_dense(dv, 40, fmt="labels", fill=True)
    assert int(parity[15, 15, 15]) == 0 and int((parity == 2).sum()) == 29540
    S = R.crossing_numbers(sample_space(dv, two, 40), 40)
    same(host(labels), R.labels(S, host(surface) != 0, 3), "two cubes")
    tight, o = dense.winding_fill(dv, 40, box="tight", max_layers=8)
    (ox, oy, oz), (nz, ny, nx) = o, tight.shape
    same(host(tight), host(labels)[oz:oz + nz, oy:oy + ny, ox:ox + nx], "tight")
    assert int((tight == 2).sum()) == 33636
    print("fill: two cubes, 33636 interior voxels, the parity rule 29540")
    # the closed sphere: fill=True's labels
    sphere = fill_ref.weld(meshes.uv_sphere(8))
    upload(dv, sphere)
    for res, ss in ((24, 1), (16, 2)):
        labels, _ = dense.winding_fill(dv, res, supersampling=ss)
        parity, _ = dense.voxelize_dense(dv, res, fmt="labels", fill=True, supersampling=ss)
        assert torch.equal(labels, parity) and int((labels == 2).sum()) > 500
        for axes in ("z", "xy"):
            assert torch.equal(dense.winding_fill(dv, res, axes=axes, supersampling=ss)[0], parity), axes
    out = torch.full((2, 24, 24, 24), 9, dtype=torch.uint8, device=DEV)
    got, _ = dense.winding_fill(dv, 24, out=out[1])
    assert got.data_ptr() == out[1].data_ptr() and torch.equal(out[1], dense.voxelize_dense(dv, 24, fmt="labels", fill=True)[0]) and bool((out[0] == 9).all())
    # one triangle removed: the vote fills what the closed sphere holds; the flood leaks and the parity rule differs
    closed, _ = dense.winding_fill(dv, 24)
    hole = np.delete(sphere, R.R_HOLE, axis=0)
    upload(dv, hole)
    labels, _ = dense.winding_fill(dv, 24)
    surface, _ = dense.voxelize_dense(dv, 24, fmt="labels")
    S = R.crossing_numbers(sample_space(dv, hole, 24), 24)
    same(host(labels), R.labels(S, host(surface) != 0, 3), "hole")
    n_vote = int((labels == 2).sum())
    leak = dense.solidify(dv, surface)
    parity, _ = dense.voxelize_dense(dv, 24, fmt="labels", fill=True)
    assert int((leak == 2).sum()) < n_vote and not torch.equal(parity, labels), (int((leak == 2).sum()), n_vote)
    assert n_vote >= int((closed == 2).sum())   # (the missing triangle's surface voxels are interior now)
    assert torch.equal(dense.winding_fill(dv, 24, min_sum=6)[0] == 2, (torch.from_numpy(np.abs(S) >= 6).to(DEV)) & (surface == 0))
    print("fill: hole", n_vote, "by the vote,", int((leak == 2).sum()), "by the flood,", int((parity == 2).sum()), "by parity")
    # rule="positive": an inward-wound sphere inside an outward-wound one carves a cavity
    inward = fill_ref.weld(meshes.uv_sphere(8)).reshape(-1, 3, 3)
    outward = inward[:, ::-1]
    shell = np.concatenate([outward, inward * 0.5]).reshape(-1, 9).astype(np.float32)
    upload(dv, shell)
    pos, _ = dense.winding_fill(dv, 32, rule="positive")
    S = R.crossing_numbers(sample_space(dv, shell, 32), 32)
    surface, _ = dense.voxelize_dense(dv, 32, fmt="labels")
    same(host(pos), R.labels(S, host(surface) != 0, 3, "positive"), "positive")
    assert int(pos[16, 16, 16]) == 0 and int(pos[16, 16, 5]) == 2 and set(np.unique(S)) == {0, 6}
    both = np.concatenate([outward, outward * 0.5]).reshape(-1, 9).astype(np.float32)
    upload(dv, both)
    kept, _ = dense.winding_fill(dv, 32, rule="positive")
    assert int(kept[16, 16, 16]) == 2 and int((kept == 2).sum()) > int((pos == 2).sum())
    # the mesh turned inside out: the nonzero rule does not mind, the positive rule finds nothing
    upload(dv, shell.reshape(-1, 3, 3)[:, ::-1].reshape(-1, 9))
    assert torch.equal(dense.winding_fill(dv, 32)[0], pos) and int((dense.winding_fill(dv, 32, rule="positive")[0] == 2).sum()) == 0
    # the labels are fill=True's format
    sdf = dense.distance_transform(dv, pos, "sdf")
    assert torch.equal(sdf < 0, pos == 2) and float(sdf[16, 16, 16]) > 0
    print("fill: positive rule", int((pos == 2).sum()), "in the shell,", int((kept == 2).sum()), "without the cavity")


CASES = {"axes": case_axes, "boxes": case_boxes, "strided": case_strided, "exact": case_exact, "many": case_many,
         "refusals": case_refusals, "fill": case_fill}

if __name__ == "__main__":
    t0 = time.time()
    CASES[sys.argv[1]]()
    print("case", sys.argv[1], "took %.1f s" % (time.time() - t0))
    print("ok")
