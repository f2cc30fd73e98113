"""The GPU cases of tests/test_gpu_surface.py, each run in a child process of its own: `python -m tests.surface_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison with the reference
(tests/surface_ref.py) is bit for bit: positions as the uint32 bits of their float32 (so -0.0 and NaN count), faces exactly.
A case prints what it covered and "ok" last when everything held."""
import sys

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import fill_ref
from tests import surface_ref as R
from tests.dense_cases import expect_code3

DEV = torch.device("cuda", 0)
F = np.float32


def check(dv, field, level, origin=(0, 0, 0), what=""):
    """extract_surface of a device tensor [z, y, x] of any strides against the reference on its host copy; returns both results'
    sizes (V, T)."""
    positions, faces = dense.extract_surface(dv, field, level, origin=origin)
    assert positions.dtype == torch.float32 and faces.dtype == torch.int32 and positions.is_contiguous() and faces.is_contiguous()
    want_p, want_f = R.extract(field.cpu().numpy(), level, origin)
    got_p, got_f = positions.cpu().numpy(), faces.cpu().numpy()
    assert got_p.shape == want_p.shape and got_f.shape == want_f.shape, (what, level, got_p.shape, want_p.shape, got_f.shape, want_f.shape)
    bad = got_p.view(np.uint32) != want_p.view(np.uint32)
    assert not bad.any(), (what, level, origin, int(bad.sum()), got_p[bad.any(axis=1)][:4], want_p[bad.any(axis=1)][:4])
    assert np.array_equal(got_f, want_f), (what, level, origin, int((got_f != want_f).sum()))
    return len(got_p), len(got_f)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).to(DEV)


def case_shapes():
    dv = hip.DeviceVoxelizer(0)
    n = 0
    fields = (("sphere", R.sphere_field(48, 15.2)), ("torus", R.torus_field(48, 13, 5)), ("two spheres", R.two_spheres_field(48, 9, 14)))
    for name, f in fields:   # (48 x 48 rows of one word: 9 blocks of words, so the block offsets are used)
        t = dev(f)
        for level in (0.0, 1.5, -2.0):
            for origin in ((0, 0, 0), (5, 7, 11), (65536 - 48, 0, 65000)):
                v, tris = check(dv, t, level, origin, name)
                assert v > 0 and tris > 0
                n += 1
    # a sphere cut by the box: open at the border
    v, tris = check(dv, dev(R.sphere_field((20, 30, 40), 17.3)), 0.0, (1, 2, 3), "cut sphere")
    assert v > 0 and tris > 0
    n += 1
    # x extents that are and are not multiples of the word; 2 and 1 along each axis
    rng = np.random.default_rng(11)
    for dims in ((9, 11, 63), (9, 11, 64), (9, 11, 65), (9, 11, 129), (5, 7, 67), (3, 2, 130), (2, 9, 9), (9, 2, 9), (9, 9, 2),
                 (2, 2, 2), (2, 2, 200), (1, 9, 9), (9, 1, 9), (9, 9, 1), (1, 1, 1), (1, 1, 300), (3, 300, 3), (300, 3, 3)):
        smooth = R.sphere_field(dims, min(dims) * 0.8 + 0.3)
        noise = rng.normal(size=dims).astype(F)
        for f in (smooth, noise):
            v, tris = check(dv, dev(f), 0.0, (3, 1, 2), dims)
            if min(dims) == 1:
                assert v == 0 and tris == 0
            n += 1
    one = np.ones((2, 2, 2), F)
    one[1, 1, 1] = -1
    assert check(dv, dev(one), 0.0) == (1, 0)
    # a grid of more than 2^16 words and 256 blocks of them
    v, tris = check(dv, dev(R.torus_field((100, 120, 330), 40, 11.5)), 0.5, (0, 0, 0), "wide torus")
    n += 2
    print("compared", n, "last", v, tris, "times", dv.surface_times())


def case_strides():
    dv = hip.DeviceVoxelizer(0)
    f = R.two_spheres_field((40, 50, 70), 11, 17)
    want = R.extract(f, 0.5, (2, 3, 4))
    n = 0
    for perm in ((0, 1, 2), (2, 1, 0), (1, 0, 2), (0, 2, 1), (1, 2, 0), (2, 0, 1)):
        # a tensor stored with its axes in another order, seen as [z, y, x]
        inverse = np.argsort(perm)
        t = dev(f.transpose(perm)).permute(*[int(a) for a in inverse])
        assert tuple(t.shape) == f.shape and (perm == (0, 1, 2) or not t.is_contiguous())
        p, fa = dense.extract_surface(dv, t, 0.5, origin=(2, 3, 4))
        assert np.array_equal(p.cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and np.array_equal(fa.cpu().numpy(), want[1]), perm
        n += 1
    # a slice of a batch, every second sample along x of a wider tensor, a box inside a larger tensor
    batch = torch.full((3, 40, 50, 70), 99.0, device=DEV)
    batch[1] = dev(f)
    check(dv, batch[1], 0.5, (2, 3, 4), "slice of a batch")
    wide = torch.full((40, 50, 140), -99.0, device=DEV)
    wide[:, :, ::2] = dev(f)
    check(dv, wide[:, :, ::2], 0.5, (2, 3, 4), "every second sample")
    big = dev(R.sphere_field((60, 64, 90), 25.5))
    check(dv, big[7:41, 5:60, 13:88], 0.0, (13, 5, 7), "a box of a larger tensor")
    # samples that share elements (the field is only read): a layer expanded along z, a plane expanded along x
    layer = dev(f[17:18]).expand(40, -1, -1)
    assert layer.stride(0) == 0 and check(dv, layer, 0.5, (2, 3, 4), "stride 0 along z")[0] > 0
    plane = dev(f[:, :, 30:31]).expand(-1, -1, 70)
    assert plane.stride(2) == 0 and check(dv, plane, 0.5, (2, 3, 4), "stride 0 along x")[0] > 0
    print("compared", n + 5)


def case_rounding():
    """The division and the clamp rule: fields of random bit patterns (every exponent, denormals, +-inf, NaN), fields with
    exact ties f == level and t exactly 0 and 1, denormal and huge levels."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2025)
    dims = (24, 28, 70)
    n = 0
    bits = rng.integers(0, 2 ** 32, size=dims, dtype=np.uint64).astype(np.uint32).view(F)
    assert np.isnan(bits).any() and (np.abs(bits[np.isfinite(bits)]) < 1.2e-38).any()
    special = bits.copy()
    special[rng.random(dims) < 0.05] = np.inf
    special[rng.random(dims) < 0.05] = -np.inf
    special[rng.random(dims) < 0.05] = np.nan
    den = (rng.integers(-2 ** 23, 2 ** 23, size=dims).astype(np.int64) * 2.0 ** -149).astype(F)   # denormals only
    assert ((den != 0) & (np.abs(den) < 1.2e-38)).any()
    near = (1.0 + rng.integers(-40, 40, size=dims) * 2.0 ** -23).astype(F)                          # a few ulps around 1
    ints = rng.integers(-2, 3, size=dims).astype(F)                                                 # ties, t exactly 0 and 1
    spread = (rng.normal(size=dims) * 10.0 ** rng.uniform(-30, 30, size=dims)).astype(F)
    for name, f, levels in (("bit patterns", bits, (0.0, 1.5, -3e-39, 1e30, -7.25)), ("specials", special, (0.0, 1.0)),
                            ("denormals", den, (0.0, 3e-39, -1e-40)), ("near 1", near, (1.0, float(F(1.0 + 2.0 ** -22)))),
                            ("small integers", ints, (0.0, 1.0, -1.0, 0.5)), ("spread", spread, (0.0, 1e-20, -1e20))):
        t = dev(f)
        for level in levels:
            v, tris = check(dv, t, level, (7, 8, 9), name)
            assert v > 0
            n += 1
    # t exactly 0 (p on the level, q inside) and exactly 1 (p inside, q on the level) on one edge each
    f = np.full((3, 3, 4), 2.0, F)
    f[1, 1, 1], f[1, 1, 2] = 0.0, -1.0      # level 0: sample 1 is outside (a tie), sample 2 inside: t = -0.0 from 1 to 2
    p, fa = dense.extract_surface(dv, dev(f), 0.0)
    want = R.extract(f, 0.0)
    assert np.array_equal(p.cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and np.array_equal(fa.cpu().numpy(), want[1])
    assert np.isfinite(want[0]).all()
    print("compared", n + 1)


def sphere_mesh(nv=24):
    verts = fill_ref.weld(meshes.uv_sphere(nv))
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    return verts, positions.view(F), faces.reshape(-1, 3).astype(np.int32)


def case_pipeline():
    """mesh -> TSDF -> mesh -> voxels without leaving the device."""
    dv = hip.DeviceVoxelizer(0)
    res = 96
    _, positions, faces = sphere_mesh()
    dense.set_mesh(dv, torch.from_numpy(positions).to(DEV), torch.from_numpy(faces).to(DEV))
    room = np.array([-1.2, -1.2, -1.2, 1.2, 1.2, 1.2], F)   # (the sphere 8 voxels inside the grid: the shell at +1.5 stays closed)
    tsdf, origin = dense.mesh_distance(dv, res, band=3.0, bounds=room)
    host = tsdf.cpu().numpy()
    for level in (0.0, 1.5, -1.5):
        p, f = dense.extract_surface(dv, tsdf, level, origin=origin)
        want_p, want_f = R.extract(host, level, origin)
        assert np.array_equal(p.cpu().numpy().view(np.uint32), want_p.view(np.uint32)) and np.array_equal(f.cpu().numpy(), want_f), level
        und, direct = R.edge_uses(want_f)
        assert (und == 2).all() and (direct == 1).all() and R.signed_volume(want_p, want_f) > 0
        # the extracted mesh back into the context, its signed distance on the same grid
        dense.set_mesh(dv, p, f)
        bounds = np.array([0, 0, 0, res, res, res], F)
        again, _ = dense.mesh_distance(dv, res, band=3.0, bounds=bounds)
        dv.voxelize(res, read=False, bounds=bounds)
        xf = dv.transform()
        tris = want_p[want_f].reshape(-1, 9)
        keys = fill_ref.parity_keys(fill_ref.sample_vertices(tris, xf), res, 1)
        z, y, x = np.nonzero(np.signbit(again.cpu().numpy()))
        assert np.array_equal(np.sort((x.astype(np.int64) * res + y) * res + z), keys), level
        identity = bool(np.array_equal(xf, np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F)))
        if identity:   # voxel space is sample space bit for bit: the set is the TSDF's own
            z, y, x = np.nonzero(host < F(level))
            assert np.array_equal(np.sort((x.astype(np.int64) * res + y) * res + z), keys), level
        print("pipeline level", level, "vertices", len(want_p), "triangles", len(want_f), "negative voxels", len(keys), "identity transform",
              identity)
        dense.set_mesh(dv, torch.from_numpy(positions).to(DEV), torch.from_numpy(faces).to(DEV))


def case_dense_field():
    """Every cell active: the densest output the scans and stores can meet; and fields without a surface."""
    dv = hip.DeviceVoxelizer(0)
    nz, ny, nx = 33, 17, 150
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    f = np.where((x + y + z) % 2 == 0, 1.0, -1.0).astype(F)
    v, tris = check(dv, dev(f), 0.0, (0, 0, 0), "alternating")
    assert v == (nz - 1) * (ny - 1) * (nx - 1)
    # every edge crosses: the interior ones give a quad each
    assert tris == 2 * ((nx - 1) * (ny - 2) * (nz - 2) + (nx - 2) * (ny - 1) * (nz - 2) + (nx - 2) * (ny - 2) * (nz - 1))
    print("dense_field vertices", v, "triangles", tris)
    for name, value in (("all inside", -1.0), ("all outside", 1.0), ("all NaN", np.nan), ("all on the level", 0.0)):
        p, fa = dense.extract_surface(dv, torch.full((9, 10, 70), value, device=DEV), 0.0)
        assert tuple(p.shape) == (0, 3) and tuple(fa.shape) == (0, 3) and p.dtype == torch.float32 and fa.dtype == torch.int32, name
    print("ok empty")


def case_refusals():
    dv = hip.DeviceVoxelizer(0)
    n = 40
    f = dev(R.sphere_field(n, 13.3))
    dims, st = (n, n, n), (1, n, n * n)
    V, T = dv.surface_count(f.data_ptr(), st, dims, 0.0)
    want_p, want_f = R.extract(f.cpu().numpy(), 0.0)
    assert (V, T) == (len(want_p), len(want_f)) and V > 0
    pos = torch.full((V, 3), 7.0, device=DEV)
    fac = torch.full((T, 3), 7, dtype=torch.int32, device=DEV)
    short_p = torch.full((V // 2, 3), 7.0, device=DEV)
    short_f = torch.full((T // 2, 3), 7, dtype=torch.int32, device=DEV)
    both = torch.full((V * 3 + T * 3,), 7, dtype=torch.int32, device=DEV)
    host = np.zeros((V, 3), F)
    torch.cuda.synchronize()

    def write(p=None, vc=V, fa=None, tc=T, level=0.0, origin=(0, 0, 0), field=None, d=dims, strides=st):
        return lambda: dv.surface_write((field if field is not None else f).data_ptr(), strides, d, level, origin,
                                        pos.data_ptr() if p is None else p, vc, fac.data_ptr() if fa is None else fa, tc)
    msgs = [
        expect_code3(write(vc=V - 1), "vertex capacity below the count"),
        expect_code3(write(tc=T - 1), "triangle capacity below the count"),
        expect_code3(write(p=short_p.data_ptr()), "short positions"),
        expect_code3(write(fa=short_f.data_ptr()), "short faces"),
        expect_code3(write(p=host.ctypes.data), "host positions"),
        expect_code3(write(level=0.5), "another level"),
        expect_code3(write(d=(n, n, n - 1)), "other dims"),
        expect_code3(write(strides=(1, n, 2 * n * n), d=(n, n, n // 2)), "other strides"),
        expect_code3(write(field=dev(np.zeros((n, n, n)))), "another field"),
        expect_code3(write(level=float("nan")), "level nan"),
        expect_code3(write(p=both.data_ptr(), fa=both.data_ptr() + V * 12 - 4), "positions and faces overlap"),
        expect_code3(write(p=f.data_ptr()), "positions in the field"),
        expect_code3(write(fa=f.data_ptr() + 64), "faces in the field"),
        expect_code3(write(p=0), "null positions"),
        expect_code3(lambda: dv.surface_count(f.data_ptr(), st, dims, float("inf")), "count: level inf"),
    ]
    # a refused count leaves nothing to write
    V2, T2 = dv.surface_count(f.data_ptr(), st, dims, 0.0)
    assert (V2, T2) == (V, T)
    msgs += [
        expect_code3(lambda: dv.surface_count(f.data_ptr(), st, dims, float("nan")), "count: level nan"),
        expect_code3(write(), "write after a refused count"),
        expect_code3(lambda: dv.surface_count(f.data_ptr(), st, (n, 0, n), 0.0), "count: zero dims"),
        expect_code3(lambda: dv.surface_count(host.ctypes.data, st, dims, 0.0), "count: host field"),
        expect_code3(lambda: dv.surface_count(f.data_ptr(), st, (n, n, 2 * n), 0.0), "count: field past its allocation"),
        expect_code3(lambda: dv.surface_count(0, st, dims, 0.0), "count: null field"),
    ]
    assert any("no matching o2v_hip_surface_count" in m for m in msgs)
    # origin past the limit: O2V_HIP_ERR_LIMIT
    assert dv.surface_count(f.data_ptr(), st, dims, 0.0) == (V, T)
    try:
        write(origin=(65536 - n + 1, 0, 0))()
        raise AssertionError("an origin past 65 536 was accepted")
    except hip.DeviceError as e:
        assert "code 5" in str(e), str(e)
    torch.cuda.synchronize()
    assert bool((pos == 7).all()) and bool((fac == 7).all()) and bool((both == 7).all()) and bool((short_p == 7).all())
    # the context still works; the count above is still the matching one; side by side in one allocation is accepted
    write(origin=(65536 - n, 0, 0))()
    write(p=both.data_ptr(), fa=both.data_ptr() + V * 12)()
    write()()
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy().view(np.uint32), want_p.view(np.uint32)) and np.array_equal(fac.cpu().numpy(), want_f)
    assert np.array_equal(both[V * 3:].view(T, 3).cpu().numpy(), want_f)
    assert all(t >= 0 for t in dv.surface_times()) and len(dv.surface_times()) == 4
    # the field changed between count and write: values may be meaningless, every index stays below V
    dv.surface_count(f.data_ptr(), st, dims, 0.0)
    f.copy_(dev(np.random.default_rng(3).normal(size=(n, n, n))))
    torch.cuda.synchronize()
    write()()
    torch.cuda.synchronize()
    assert int(fac.min()) >= 0 and int(fac.max()) < V and np.array_equal(fac.cpu().numpy(), want_f)
    assert bool(torch.isfinite(pos).all())
    print("\n".join(msgs))
    print("ok refusals")


def case_bench_mesh():
    """scan_like at 512 with band 3: the counts against the reference's (from the sign grid, layer by layer), positions and
    faces on seeded z ranges (the whole reference would need the grid several times over in host memory)."""
    dv = hip.DeviceVoxelizer(0)
    verts = meshes.scan_like()
    positions, faces = np.unique(verts.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    dense.set_mesh(dv, torch.from_numpy(positions.view(F)).to(DEV), torch.from_numpy(faces.reshape(-1, 3).astype(np.int32)).to(DEV))
    res = 512
    tsdf, origin = dense.mesh_distance(dv, res, band=3.0)
    host = tsdf.cpu().numpy()
    rng = np.random.default_rng(512)
    for level in (0.0, 1.5):
        p, f = dense.extract_surface(dv, tsdf, level, origin=origin)
        v_layers, q_layers = R.counts_per_layer(R.inside(host, level))
        assert len(p) == int(v_layers.sum()) and len(f) == 2 * int(q_layers.sum()), (len(p), int(v_layers.sum()), len(f), 2 * int(q_layers.sum()))
        assert int(f.min()) >= 0 and int(f.max()) < len(p)
        got_p, got_f = p.cpu().numpy(), f.cpu().numpy()
        busy = np.nonzero(v_layers)[0]
        starts = sorted({0, res - 13, int(busy[0]), int(busy[-1]) - 11} | {int(z) for z in rng.choice(busy[:-12], 6, replace=False)})
        nv = nt = 0
        for z0 in starts:
            z0 = max(0, min(z0, res - 13))
            v0, want_p, t0, want_f = R.extract_layers(host, level, origin, z0, z0 + 12, v_layers, q_layers)
            assert np.array_equal(got_p[v0:v0 + len(want_p)].view(np.uint32), want_p.view(np.uint32)), (level, z0)
            assert np.array_equal(got_f[t0:t0 + len(want_f)], want_f), (level, z0)
            nv, nt = nv + len(want_p), nt + len(want_f)
        print("bench_mesh level", level, "vertices", len(p), "triangles", len(f), "compared", nv, "vertices and", nt, "triangles in", len(starts),
              "ranges of 12 layers; times", dv.surface_times())


# ---- the documented limits, reached with small fields: a field is only read, so its samples may share elements ----------------

TURN = 2 ** 20    # kSurfMaxGrid: the workgroups of k_surf_count / _vertices / _faces; block b is taken by workgroup b % TURN
BLOCK = 256       # kBlock: words per block
WORKERS = 8       # threads of the reference over a grid of 10^9 samples


def strided(base, dims, sx, s1, s2):
    """f(x, y, z) = base[sx x + s1 y + s2 z] as [z, y, x]: a torch view of a device tensor or a numpy view of a host array;
    neither holds the grid."""
    nx, ny, nz = dims
    assert sx * (nx - 1) + s1 * (ny - 1) + s2 * (nz - 1) < len(base)
    if isinstance(base, torch.Tensor):
        return torch.as_strided(base, (nz, ny, nx), (s2, s1, sx))
    e = base.strides[0]
    return np.lib.stride_tricks.as_strided(base, (nz, ny, nx), (s2 * e, s1 * e, sx * e), writeable=False)


def turns_base(n, seed):
    """n float32: stretches of 300 to 3 000 elements, in turn quiet (all above the level 0.125) and busy (a share p of the
    samples below it, p drawn per stretch between 1e-4 and 8e-3; in every eighth busy stretch half of the first 150 samples,
    for blocks with more outputs than threads)."""
    rng = np.random.default_rng(seed)
    base = (0.3 + np.abs(rng.normal(size=n))).astype(F)
    at, stretch = 0, 0
    while at < n:
        length = int(rng.integers(300, 3000))
        if stretch % 2:
            part = base[at:at + length]
            part[rng.random(len(part)) < float(np.exp(rng.uniform(np.log(1e-4), np.log(8e-3))))] *= F(-1)
            if stretch % 16 == 1:
                part[:150][rng.random(len(part[:150])) < 0.5] *= F(-1)
        at, stretch = at + length, stretch + 1
    return base


def turn_kinds(per_block):
    """How many workgroups with two turns have output in neither turn, in the second only, in the first only, in both: [4]."""
    second = per_block[TURN:] > 0
    first = per_block[:len(second)] > 0
    return np.bincount(2 * first.astype(np.int64) + second, minlength=4)


def case_in_turns():
    """More than 2^20 blocks of words: the workgroups with a low number take two blocks, one after the other.  The grid is a
    strided view of a 1-D tensor of 190 000 floats (the field is only read, so its samples may share elements); what it costs is
    the context's 20 bytes per word.  nx = 3 keeps quads along all three axes at a word per row; ny = nz = 18 400 gives 1.26 x 2^20
    blocks; the base's density was chosen for about 10 M vertices, at which comparing every output against the reference takes
    about as long as the reference's passes over the 1 G samples alone."""
    import time
    t_start = time.time()
    dv = hip.DeviceVoxelizer(0)
    level, origin = 0.125, (40000, 123, 7)
    ny = nz = 18400
    host = turns_base(190000, 2028)
    base = torch.from_numpy(host).to(DEV)
    free0, total = torch.cuda.mem_get_info(DEV)
    ins = host < F(level)

    # the smaller run first: an x stride of 2 (k_surf_vertices<false>), totals and seeded ranges of 12 layers
    dims, (sx, s1, s2) = (5, ny, nz), (2, 3, 7)
    n_blocks = -(-ny * nz // BLOCK)
    assert n_blocks > TURN and 1.25 * 2 ** 28 <= ny * nz <= 1.5 * 2 ** 28
    v_layers, q_layers, v_blocks, q_blocks = R.grid_counts(R.row_tables(ins, dims[0], sx, s1, s2), ny, nz, s1, s2, workers=WORKERS)
    kinds_v, kinds_q = turn_kinds(v_blocks), turn_kinds(q_blocks)
    assert kinds_v.min() >= 1000 and kinds_q.min() >= 1000, (kinds_v, kinds_q)
    V, T = int(v_layers.sum()), 2 * int(q_layers.sum())
    p, f = dense.extract_surface(dv, strided(base, dims, sx, s1, s2), level, origin=origin)
    assert (len(p), len(f)) == (V, T), (len(p), V, len(f), T)
    assert int(f.min()) >= 0 and int(f.max()) < V
    got_p, got_f = p.cpu().numpy(), f.cpu().numpy()
    view = strided(host, dims, sx, s1, s2)
    rng = np.random.default_rng(77)
    first_late = TURN * BLOCK // ny + 1          # the first layer whose blocks are all taken in a second turn
    starts = sorted(int(z) for z in np.concatenate([rng.choice(first_late - 12, 4, replace=False),
                                                    first_late + rng.choice(nz - 13 - first_late, 3, replace=False), [nz - 13]]))
    assert sum(z * ny // BLOCK >= TURN for z in starts) >= 4 and len(starts) == 8
    nv = nt = 0
    for z0 in starts:
        v0, want_p, t0, want_f = R.extract_layers(view, level, origin, z0, z0 + 12, v_layers, q_layers)
        assert len(want_p) > 0 and len(want_f) > 0, z0
        assert np.array_equal(got_p[v0:v0 + len(want_p)].view(np.uint32), want_p.view(np.uint32)), ("x stride 2", z0)
        assert np.array_equal(got_f[t0:t0 + len(want_f)], want_f), ("x stride 2", z0)
        nv, nt = nv + len(want_p), nt + len(want_f)
    print("in_turns x stride 2: dims", dims, "strides", (sx, s1, s2), "blocks", n_blocks, "vertices", V, "triangles", T, "workgroups with two turns"
          " (neither turn with output, the second only, the first only, both): vertices", kinds_v.tolist(), "quads", kinds_q.tolist(), "compared", nv, "vertices and", nt,
          "triangles in 8 ranges of 12 layers from", starts, "times", dv.surface_times(), "wall %.1f s" % (time.time() - t_start), flush=True)
    del p, f, got_p, got_f

    # every output compared: x stride 1 (k_surf_vertices<true>)
    t_main = time.time()
    dims, (sx, s1, s2) = (3, ny, nz), (1, 3, 5)
    tables = R.row_tables(ins, dims[0], sx, s1, s2)
    t_layers, tq_layers, v_blocks, q_blocks = R.grid_counts(tables, ny, nz, s1, s2, workers=WORKERS)
    kinds_v, kinds_q = turn_kinds(v_blocks), turn_kinds(q_blocks)
    assert kinds_v.min() >= 1000 and kinds_q.min() >= 1000, (kinds_v, kinds_q)
    v_layers, q_layers = R.counts_per_layer_slabs(strided(ins, dims, sx, s1, s2), 64, WORKERS)
    assert np.array_equal(v_layers, t_layers) and np.array_equal(q_layers, tq_layers)
    V, T = int(v_layers.sum()), 2 * int(q_layers.sum())
    assert 2_000_000 <= V <= 40_000_000, V
    t_counts = time.time()
    p, f = dense.extract_surface(dv, strided(base, dims, sx, s1, s2), level, origin=origin)
    times = dv.surface_times()
    used = total - torch.cuda.mem_get_info(DEV)[0]
    assert (len(p), len(f)) == (V, T), (len(p), V, len(f), T)
    assert int(f.min()) >= 0 and int(f.max()) < V
    got_p, got_f = p.cpu().numpy(), f.cpu().numpy()
    t_device = time.time()
    view = strided(host, dims, sx, s1, s2)
    v_end = t_end = 0
    chunks = R.layer_chunks(nz, 64)
    for at in range(0, len(chunks), 4 * WORKERS):   # (a few ranges at a time: the host holds their meshes only)
        some = chunks[at:at + 4 * WORKERS]
        wants = R.each(lambda z0, z1: R.extract_layers(view, level, origin, z0, z1, v_layers, q_layers), some, WORKERS)
        for (z0, z1), (v0, want_p, t0, want_f) in zip(some, wants):
            assert v0 <= v_end and t0 == t_end, (z0, v0, v_end, t0, t_end)
            bad = (got_p[v0:v0 + len(want_p)].view(np.uint32) != want_p.view(np.uint32)).any(axis=1)
            assert not bad.any(), ("vertices", z0, z1, int(bad.sum()), "first at", v0 + int(np.argmax(bad)), "of block",
                                   int(np.searchsorted(np.cumsum(v_blocks), v0 + int(np.argmax(bad)), side="right")))
            bad = (got_f[t0:t0 + len(want_f)] != want_f).any(axis=1)
            assert not bad.any(), ("triangles", z0, z1, int(bad.sum()), "first at", t0 + int(np.argmax(bad)), "of block",
                                   int(np.searchsorted(np.cumsum(q_blocks), (t0 + int(np.argmax(bad))) // 2, side="right")))
            v_end, t_end = v0 + len(want_p), t0 + len(want_f)
    assert (v_end, t_end) == (V, T)
    print("in_turns: dims", dims, "strides", (sx, s1, s2), "origin", origin, "blocks", n_blocks, "of which", n_blocks - TURN, "in a second turn; vertices", V,
          "triangles", T, "all compared; most per block", int(v_blocks.max()), "vertices", int(q_blocks.max()), "quads; workgroups with two turns"
          " (neither turn with output, the second only, the first only, both): vertices", kinds_v.tolist(), "quads", kinds_q.tolist(), "times", times,
          "device memory in use after the call %.2f GB (%.2f GB before the context's arrays)" % (used / 1e9, (total - free0) / 1e9),
          "wall: counts %.1f s, device and copy %.1f s, compare %.1f s, case %.1f s" %
          (t_counts - t_main, t_device - t_counts, time.time() - t_device, time.time() - t_start))


def checkerboard(dims):
    """f = (-1)^(x + y + z) as a view with strides (1, 1, 1) of an alternating device tensor: every cell is active."""
    base = torch.ones(sum(dims), device=DEV)
    base[1::2] = -1
    return base


def case_vertex_limit():
    """2^31 vertices are refused, 2^31 - 2^21 are counted and their triangles are above 2^32: count only (the mesh would be over
    150 GB).  The limit itself, 2^31 - 1, is a prime and no box has that many cells, so which of > and >= the check uses is not
    tested here."""
    dv = hip.DeviceVoxelizer(0)
    st = (1, 1, 1)
    dims = (2049, 1025, 1025)
    base = checkerboard(dims)
    torch.cuda.synchronize()
    assert R.checkerboard_counts(*dims)[0] == 2 ** 31
    try:
        dv.surface_count(base.data_ptr(), st, dims, 0.0)
        raise AssertionError("2^31 vertices were accepted")
    except hip.DeviceError as e:
        assert "code 5" in str(e) and str(2 ** 31) + " vertices" in str(e), str(e)
        print(e)
    out = torch.full((64,), 7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    msg = expect_code3(lambda: dv.surface_write(base.data_ptr(), st, dims, 0.0, (0, 0, 0), out.data_ptr(), 1, out.data_ptr() + 128, 1),
                       "write after a refused count")
    assert "no matching o2v_hip_surface_count" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    # the context still works
    check(dv, dev(R.sphere_field(24, 8.3)), 0.0, (1, 2, 3), "after the refusal")
    dims = (2049, 1025, 1024)
    want_v, want_q = R.checkerboard_counts(*dims)
    assert want_v == 2 ** 31 - 2 ** 21 and 2 * want_q > 2 ** 32 and want_q > 2 ** 32
    V, T = dv.surface_count(base.data_ptr(), st, dims, 0.0)
    assert (V, T) == (want_v, 2 * want_q), (V, T, want_v, 2 * want_q)
    print("vertex_limit: dims (2049, 1025, 1025) refused at", 2 ** 31, "vertices; dims", dims, "counted", V, "vertices,", T // 2, "quads,", T,
          "triangles; times", dv.surface_times())


def case_full_blocks():
    """Blocks with 2^14 vertices and 3 x 2^14 quads, the most the packed 16-bit prefixes of a block are documented for; and the
    longest axes: 65 536 samples along x, y and z, positions up to 65 535.5."""
    dv = hip.DeviceVoxelizer(0)
    dims = (65536, 4, 4)
    field = strided(checkerboard(dims), dims, 1, 1, 1)
    v_blocks, q_blocks = R.per_block_counts(R.inside(field.cpu().numpy(), 0.0))
    assert int(v_blocks.max()) == 2 ** 14 and int(q_blocks.max()) == 3 * 2 ** 14
    v, tris = check(dv, field, 0.0, (0, 0, 0), "full blocks")
    assert (v, tris) == (R.checkerboard_counts(*dims)[0], 2 * R.checkerboard_counts(*dims)[1])
    print("full_blocks: dims", dims, "vertices", v, "triangles", tris, "blocks with 16 384 vertices:", int((v_blocks == 2 ** 14).sum()),
          "with 49 152 quads:", int((q_blocks == 3 * 2 ** 14).sum()))
    rng = np.random.default_rng(65536)
    for dims in ((65536, 2, 2), (2, 65536, 2), (2, 2, 65536), (65536, 3, 3)):
        nx, ny, nz = dims
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        smooth = (np.sin(0.05 * (x + 2 * y + 3 * z)) + 0.2 * np.cos(0.31 * (x - y + z)) + 0.4 * np.sin(1.3 * x + 2.1 * y + 0.7 * z)).astype(F)
        noise = rng.normal(size=(nz, ny, nx)).astype(F)
        for name, f in (("smooth", smooth), ("noise", noise)):
            t = dev(f)
            v, tris = check(dv, t, 0.0, (0, 0, 0), (name, dims))
            p, _ = dense.extract_surface(dv, t, 0.0)
            top = float(p.max())
            assert v > 1000 and 65500 < top <= 65535.5 and (tris > 0) == (min(dims) > 2), (name, dims, v, tris, top)
            print("longest axes:", name, dims, "vertices", v, "triangles", tris, "largest coordinate", top)


CASES = {"shapes": case_shapes, "strides": case_strides, "rounding": case_rounding, "pipeline": case_pipeline, "dense_field": case_dense_field,
         "refusals": case_refusals, "bench_mesh": case_bench_mesh, "in_turns": case_in_turns, "vertex_limit": case_vertex_limit,
         "full_blocks": case_full_blocks}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
