"""The GPU cases of tests/test_gpu_label_stats.py, each run in a child process of its own: `python -m tests.label_stats_cases <case>`.

torch is imported before the library is loaded (the grids are torch tensors; see tests/dense_cases.py).  Every comparison is
np.array_equal on int64 against the numpy reference of tests/label_stats_ref.py or against closed forms in Python ints, never
against the code under test, and there is no tolerance anywhere.  A case prints what it covered and "ok" last when everything
held."""
import os
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import components_ref as CR
from tests import label_stats_ref as R

DEV = torch.device("cuda", 0)
I32, U8 = hip.LABELS_I32, hip.LABELS_U8
GUARD = -7
BITS = (R.BOX, R.SUMS, R.MOMENTS, R.FACES)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def st(t):
    """(x, y, z) element strides of a tensor [z, y, x]."""
    return t.stride(2), t.stride(1), t.stride(0)


def call(dv, t, n, origin=(0, 0, 0), which=R.ALL, table=None):
    """dv.label_stats at the C level on the tensor view t [z, y, x] into a table filled with a guard value; (table, outside)."""
    if table is None:
        table = torch.full((n + 1, R.COLUMNS), GUARD, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    nz, ny, nx = t.shape
    outside = dv.label_stats(t.data_ptr(), I32 if t.dtype == torch.int32 else U8, st(t), (nx, ny, nz), origin, n, which, table.data_ptr())
    return table.cpu().numpy(), outside


def same(got, want, what):
    assert got[1] == want[1], (what, "outside", got[1], want[1])
    assert got[0].dtype == np.int64 and got[0].shape == want[0].shape, what
    bad = np.argwhere(got[0] != want[0])
    assert not len(bad), (what, len(bad), "elements differ, the first at", bad[0].tolist(), int(got[0][tuple(bad[0])]), int(want[0][tuple(bad[0])]))


# ---- shapes and layouts -----------------------------------------------------------------------------------------------------------

def layouts(g):
    """name -> (tensor view on the device, the numpy grid it holds): the grid g [z, y, x] in every layout the call takes."""
    nz, ny, nx = g.shape
    t = dev(g)
    out = {"contiguous": (t, g)}
    flat = torch.zeros(g.size + 8, dtype=t.dtype, device=DEV)
    flat[1:1 + g.size] = t.reshape(-1)
    out["one element into an allocation"] = (flat[1:1 + g.size].view(g.shape), g)     # (rows not aligned for 16-byte loads)
    wide = torch.zeros((nz, ny, 2 * nx), dtype=t.dtype, device=DEV)
    wide[:, :, ::2] = t
    out["x stride 2"] = (wide[:, :, ::2], g)
    out["x and z swapped"] = (t.permute(2, 1, 0).contiguous().permute(2, 1, 0), g)
    out["a slice of a batch"] = (torch.stack([torch.ones_like(t), t, torch.zeros_like(t)])[1], g)
    padded = torch.ones((nz, ny + 1, nx + 5), dtype=t.dtype, device=DEV)
    padded[:, :ny, :nx] = t
    out["padded rows"] = (padded[:, :ny, :nx], g)
    out["a plane expanded along z"] = (t[:1].expand(nz, ny, nx), np.broadcast_to(g[:1], g.shape))
    return out


def case_shapes_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(192)
    shapes = [(x, 3, 2) for x in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257)] + [(70, 50, 40), (65, 9, 9), (1, 9, 7), (9, 1, 7), (9, 7, 1)]
    calls = grids = 0
    for i, dims in enumerate(shapes):
        for kind in ("int32", "uint8", "bool"):
            n = {"int32": (1, 7, 255, 1000)[i % 4], "uint8": (1, 7, 255)[i % 3], "bool": 1}[kind]
            g = R.blobs(rng, dims, n).astype({"int32": np.int32, "uint8": np.uint8, "bool": np.bool_}[kind])
            origin = tuple(int(v) for v in rng.integers(0, 1000, 3))
            wants = {}
            for name, (t, held) in layouts(g).items():
                assert t.shape == g.shape and np.array_equal(t.cpu().numpy(), held), (dims, kind, name)
                key = "expanded" if name.startswith("a plane") else "grid"
                if key not in wants:
                    wants[key] = R.label_stats(held, n, origin)
                same(call(dv, t, n, origin), wants[key], (dims, kind, name))
                calls += 1
                if name in ("contiguous", "one element into an allocation"):
                    for which in BITS + (0,):
                        same(call(dv, t, n, origin, which), R.label_stats(held, n, origin, which), (dims, kind, name, which))
                        calls += 1
            grids += 1
    # through dense: the same numbers in LabelStats' fields
    g = R.blobs(rng, (70, 50, 40), 7)
    s = dense.label_stats(dv, dev(g), 7, origin=(5, 6, 7), moments=True, faces=True)
    want, _ = R.label_stats(g, 7, (5, 6, 7))
    assert np.array_equal(s.count.cpu().numpy(), want[:, 0]) and np.array_equal(s.lo.cpu().numpy(), want[:, 1:4]) and (want[:, 0] > 0).all()
    assert np.array_equal(s.hi.cpu().numpy(), want[:, 4:7] + 1) and np.array_equal(s.sum.cpu().numpy(), want[:, 7:10])
    assert np.array_equal(s.moment.cpu().numpy(), want[:, 10:16]) and np.array_equal(s.faces.cpu().numpy(), want[:, 16])
    assert len(dv.label_stats_times()) == 2 and all(v >= 0 for v in dv.label_stats_times())
    print("shapes_and_layouts: compared", calls, "calls on", grids, "grids in 7 layouts")


# ---- many labels ------------------------------------------------------------------------------------------------------------------

def case_many_labels():
    mode = "every run to global memory" if os.environ.get("O2V_LS_NO_TABLE") == "1" else "the table in LDS"
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(193)
    own = np.arange(40 * 24 * 16, dtype=np.int32).reshape(16, 24, 40)
    z, y, x = np.indices((9, 10, 37))
    grids = [("every voxel its own label", own, own.size - 1), ("random labels out of 5000", rng.integers(0, 5000, (48, 64, 96)).astype(np.int32), 4999),
             ("checkerboard", ((x + y + z) & 1).astype(np.int32), 1), ("checkerboard, uint8", ((x + y + z) & 1).astype(np.uint8), 1),
             ("one label everywhere", np.full((64, 128, 256), 3, np.int32), 3), ("one label everywhere, uint8", np.full((64, 128, 256), 3, np.uint8), 3)]
    for name, g, n in grids:
        origin = (11, 65536 - g.shape[1], 3)
        same(call(dv, dev(g), n, origin), R.label_stats(g, n, origin), (name, mode))
    t = call(dv, dev(grids[4][1]), 3, (0, 0, 0))[0]
    assert t[3].tolist() == R.box_row((256, 128, 64), (0, 0, 0))
    print("many_labels:", len(grids), "grids with", mode)


# ---- out of range -----------------------------------------------------------------------------------------------------------------

def case_out_of_range():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(194)
    n_calls = 0
    for dims in ((33, 9, 5), (70, 50, 40)):
        for n in (0, 1, 7, 1000):
            g = R.blobs(rng, dims, n, outside=0.1)
            want = R.label_stats(g, n, (1, 2, 3))
            assert want[1] > 0 and {-1, n + 1, -2 ** 31, 2 ** 31 - 1} <= set(np.unique(g).tolist())
            same(call(dv, dev(g), n, (1, 2, 3)), want, (dims, n))
            s = dense.label_stats(dv, dev(g), n)
            assert s.outside == want[1] and int(s.count.sum()) + s.outside == g.size
            n_calls += 1
        # uint8: everything above n is outside
        g = rng.integers(0, 256, dims[::-1]).astype(np.uint8)
        for n in (0, 7, 254, 255):
            want = R.label_stats(g, n)
            assert (want[1] == 0) == (n == 255)
            same(call(dv, dev(g), n), want, (dims, n, "uint8"))
            n_calls += 1
    # rows without voxels: the sentinels where the box is asked for, 0 where it is not
    g = np.full((4, 5, 6), 2, np.int32)
    t, outside = call(dv, dev(g), 4)
    assert outside == 0 and t[2].tolist() == R.box_row((6, 5, 4), (0, 0, 0))
    for row in (0, 1, 3, 4):
        assert t[row].tolist() == [0] + [2 ** 31 - 1] * 3 + [-1] * 3 + [0] * 10
    t, _ = call(dv, dev(g), 4, which=R.SUMS)
    assert not t[[0, 1, 3, 4]].any() and t[2, 1:7].tolist() == [0] * 6
    s = dense.label_stats(dv, dev(g), 4)
    assert s.lo[[0, 1, 3, 4]].abs().sum() == 0 and s.hi[[0, 1, 3, 4]].abs().sum() == 0 and s.hi[2].tolist() == [6, 5, 4]
    # n = 0 on a grid of zeros, and on a grid without any
    assert call(dv, dev(np.zeros((3, 3, 3), np.int32)), 0)[0][0, 0] == 27
    t, outside = call(dv, dev(np.full((3, 3, 3), 9, np.int32)), 0)
    assert outside == 27 and t[0].tolist() == [0] + [2 ** 31 - 1] * 3 + [-1] * 3 + [0] * 10
    print("out_of_range: compared", n_calls, "calls")


# ---- magnitudes -------------------------------------------------------------------------------------------------------------------

def case_magnitudes():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(195)
    for dims in ((70, 50, 40), (257, 3, 2)):
        g = R.blobs(rng, dims, 7)
        origin = tuple(65536 - d for d in dims)
        same(call(dv, dev(g), 7, origin), R.label_stats(g, 7, origin), (dims, "origin at 65 536 - dims"))
    # one row of one label expanded to 2 047 x 1 024 x 1 024 [z, y, x], 2 146 435 072 voxels, at the far corner
    nx, ny, nz = 1024, 1024, 2047
    row = torch.full((1, 1, nx), 3, dtype=torch.uint8, device=DEV)
    big = row.expand(nz, ny, nx)
    origin = (65536 - nx, 65536 - ny, 65536 - nz)
    assert origin[0] == 64512 and big.numel() == 2146435072
    t0 = time.time()
    s = dense.label_stats(dv, big, 3, origin=origin, moments=True, faces=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    ms = dv.label_stats_times()
    want = R.box_row((nx, ny, nz), origin)
    got = [int(s.count[3])] + s.lo[3].tolist() + (s.hi[3] - 1).tolist() + s.sum[3].tolist() + s.moment[3].tolist() + [int(s.faces[3])]
    assert got == want, (got, want)
    assert want[16] == 2 * (nx * ny + ny * nz + nx * nz) and want[0] > 2 ** 30 and max(want) > 2 ** 62 and s.outside == 0
    assert not s.count[:3].any() and not s.faces[:3].any()
    print(f"magnitudes: 2 146 435 072 voxels, the largest sum {max(want)} = 2^{np.log2(float(max(want))):.2f}; device ms {ms[0]:.3f} + {ms[1]:.3f}, wall {wall:.2f} s")


# ---- faces ------------------------------------------------------------------------------------------------------------------------

def case_faces():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(196)
    z, y, x = np.indices((24, 24, 24))
    ball = (x - 11.5) ** 2 + (y - 11.5) ** 2 + (z - 11.5) ** 2 <= 10.5 ** 2
    hollow = np.ones((10, 10, 10), bool)
    hollow[1:-1, 1:-1, 1:-1] = False
    grids = [ball, hollow] + [rng.random(d[::-1]) < p for d in ((70, 50, 40), (17, 3, 2), (64, 5, 4), (1, 9, 7)) for p in (0.1, 0.5, 0.9)]
    for g in grids:
        t = dev(g)
        s = dense.label_stats(dv, t, faces=True, box=False, sums=False)
        n_faces = dense.count_faces(dv, t, merge="none")
        assert int(s.faces[1]) == n_faces == int(R.label_stats(g, 1, which=R.FACES)[0][1, 16]), (g.shape, int(s.faces[1]), n_faces)
    assert int(dense.label_stats(dv, dev(ball), faces=True).faces[1]) == 1992 and int(dense.label_stats(dv, dev(hollow), faces=True).faces[1]) == 984
    # the labels of components: a face between two components, or towards the background, is a face of both sides
    for conn in (6, 26):
        g = rng.random((40, 50, 70)) < 0.25
        labels, n, s = dense.component_stats(dv, dev(g), connectivity=conn, moments=True, faces=True)
        want_labels, want_n = CR.label(g, conn)
        assert n == want_n and np.array_equal(labels.cpu().numpy(), want_labels)
        want, _ = R.label_stats(want_labels, n)
        got = torch.cat([s.count[:, None], s.sum, s.moment, s.faces[:, None]], dim=1).cpu().numpy()
        assert np.array_equal(got, want[:, [0] + list(range(7, 17))]), conn
        assert int(s.faces[1:].sum()) == dense.count_faces(dv, dev(g), merge="none")
        print("faces: connectivity", conn, ":", n, "components,", int(s.faces[1:].sum()), "faces")
    print("faces: compared", len(grids), "0 / 1 grids with count_faces")


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------

def indexed(verts):
    positions, faces = np.unique(np.asarray(verts, np.float32).reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    return dev(positions.view(np.float32)), dev(faces.reshape(-1, 3).astype(np.int32))


def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    c = meshes.unit_cube().reshape(-1, 9)
    dense.set_mesh(dv, *indexed(np.concatenate([c * 16 + 4.03, c * 16 + 10.07])))
    surface, origin = dense.voxelize_dense(dv, 40, fmt="labels")
    solid = dense.solidify(dv, surface)
    s = dense.label_stats(dv, solid, 2, origin=origin, moments=True, faces=True)
    g = solid.cpu().numpy()
    want, _ = R.label_stats(g, 2, origin)
    got = torch.cat([s.count[:, None], s.lo, s.hi - 1, s.sum, s.moment, s.faces[:, None]], dim=1).cpu().numpy()
    assert np.array_equal(got, want)
    n_surface = int((g == 1).sum())
    assert int(s.count[2]) == 33636 and int(s.count[1]) == n_surface and int(s.count[1] + s.count[2]) == 33636 + n_surface
    volume, centre, inertia = dense.mass_properties(s, (1, 2), transform=dv.transform())
    zz, yy, xx = np.nonzero(g)
    p = np.stack([xx, yy, zz], 1) + 0.5
    d = p - p.mean(0)
    second = d.T @ d + np.eye(3) * len(p) / 12
    v_vol, v_centre, v_inertia = dense.mass_properties(s, (1, 2))
    assert v_vol == len(p) and np.allclose(v_centre.numpy(), p.mean(0), rtol=0, atol=1e-9)
    assert np.allclose(v_inertia.numpy(), np.eye(3) * np.trace(second) - second, rtol=1e-12)
    # model space: the voxel volume over |det A| of the run's transform (model to voxel space), the centre mapped back
    A, t = np.asarray(dv.transform(), np.float64)[:9].reshape(3, 3), np.asarray(dv.transform(), np.float64)[9:]
    assert np.isclose(volume, v_vol / abs(np.linalg.det(A)), rtol=1e-12, atol=0) and np.allclose(A @ centre.numpy() + t, v_centre.numpy(), rtol=1e-12)
    labels, n, cs = dense.component_stats(dv, solid, connectivity=6)
    assert n == 1 and int(cs.count[1]) == 33636 + n_surface
    print("pipeline: two cubes at 40:", int(s.count[1]), "surface +", int(s.count[2]), "interior voxels; model volume %.1f" % volume, flush=True)
    # the largest piece of a scan
    dense.set_mesh(dv, *indexed(meshes.scan_like()))
    occ, _ = dense.voxelize_dense(dv, 256)
    labels, n = dense.components(dv, occ, connectivity=26)
    sizes = dense.component_sizes(labels, n)
    largest = int(sizes[1:].max())
    kept = dense.keep_largest(dv, occ, connectivity=26)
    if int((sizes[1:] == largest).sum()) == 1:
        assert torch.equal(kept, dense.remove_small(dv, occ, largest, connectivity=26))
    assert int(kept.sum()) == largest and torch.equal(kept, labels == int(sizes[1:].argmax()) + 1)
    # every component cropped: the crop holds all of it, and nothing of it lies outside
    s = dense.label_stats(dv, labels, n)
    assert np.array_equal(s.count.cpu().numpy(), sizes.cpu().numpy())
    total = 0
    for L in range(1, min(n, 40) + 1):
        view, o = dense.crop(labels, s, L)
        inside = int((view == L).sum())
        assert inside == int(sizes[L]) and o == tuple(s.lo[L].tolist())
        if view.numel() > 1:   # the box is tight: the label touches every face of it
            assert bool((view[0] == L).any()) and bool((view[-1] == L).any()) and bool((view[:, 0] == L).any()) and bool((view[:, :, -1] == L).any())
        total += inside
    print("pipeline: scan_like at 256:", n, "components, the largest", largest, "voxels;", min(n, 40), "crops hold", total, "voxels")
    # ... and the components of a random grid, many and small: every 50th
    g = dev(np.random.default_rng(198).random((40, 50, 70)) < 0.2)
    labels, n, s = dense.component_stats(dv, g, connectivity=6, origin=(100, 200, 300))
    sizes = dense.component_sizes(labels, n)
    crops = 0
    for L in range(1, n + 1, 50):
        view, o = dense.crop(labels, s, L)
        lo = s.lo[L].tolist()
        assert o == tuple(lo) and tuple(view.shape) == tuple((s.hi[L] - s.lo[L]).tolist()[::-1])
        assert view.data_ptr() == labels[lo[2] - 300, lo[1] - 200, lo[0] - 100:].data_ptr()
        assert int((view == L).sum()) == int(sizes[L]) == int((labels == L).sum())        # all of it inside, so none outside
        assert bool((view[0] == L).any()) and bool((view[-1] == L).any()) and bool((view[:, 0] == L).any()) and bool((view[:, -1] == L).any())
        assert bool((view[:, :, 0] == L).any()) and bool((view[:, :, -1] == L).any())
        crops += 1
    assert n > 1000 and crops > 20
    print("pipeline: random grid:", n, "components,", crops, "cropped")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def expect_code(code, fn, what):
    try:
        fn()
    except hip.DeviceError as e:
        assert f"code {code}" in str(e) and "o2v_hip_label_stats" in str(e), (what, str(e))
        return what + ": " + str(e)
    raise AssertionError(what + " was accepted")


def case_refusals():
    """Every refusal of the header's list but the failed scratch allocation (the scratch is one counter).  This child runs with
    torch's caching allocator off: each tensor is an allocation of its own, so a short one is short."""
    dv = hip.DeviceVoxelizer(0)
    L = hip._bind()
    n, k = 48, 7
    dims, s = (n, n, n), (1, n, n * n)
    rng = np.random.default_rng(197)
    g_np = R.blobs(rng, dims, k)
    want = R.label_stats(g_np, k)
    lab, lab8 = dev(g_np), dev(g_np.astype(np.uint8))
    table = torch.full((k + 1, R.COLUMNS), GUARD, dtype=torch.int64, device=DEV)
    short_table = torch.full((k // 2, R.COLUMNS), GUARD, dtype=torch.int64, device=DEV)
    short = torch.full((n // 2, n, n), 5, dtype=torch.int32, device=DEV)
    shared = torch.full((n ** 3 + (k + 1) * R.COLUMNS * 2 + 2,), 5, dtype=torch.int32, device=DEV)   # the grid and a table in one allocation
    byte = torch.zeros((1, 1, 1), dtype=torch.uint8, device=DEV)
    host_grid, host_table = g_np.copy(), np.zeros((k + 1, R.COLUMNS), np.int64)
    torch.cuda.synchronize()
    G, T, S = lab.data_ptr(), table.data_ptr(), shared.data_ptr()

    def good():
        """After a refusal the context still works, and the refusal wrote nothing."""
        assert bool((table == GUARD).all()) and bool((short_table == GUARD).all()) and bool((shared == 5).all()) and np.array_equal(lab.cpu().numpy(), g_np)
        same(call(dv, lab, k), want, "after a refusal")

    def c(grid=G, fmt=I32, strides=s, dm=dims, origin=(0, 0, 0), n_labels=k, which=R.ALL, tab=T):
        return lambda: dv.label_stats(grid, fmt, strides, dm, origin, n_labels, which, tab)

    refusals = [
        (3, c(grid=None), "null grid"),
        (3, c(strides=None), "null strides"),
        (3, c(tab=None), "null table"),
        (3, c(dm=(n, 0, n)), "zero dims"),
        (3, c(fmt=2), "unknown format"),
        (3, c(which=16), "unknown which bit"),
        (3, c(which=0x80000001), "unknown high which bit"),
        (3, c(grid=lab8.data_ptr(), fmt=U8, n_labels=256), "n_labels 256 for U8"),
        (3, c(tab=T + 4), "a table that is not 8-byte aligned"),
        (3, c(grid=G + 2), "an int32 grid that is not 4-byte aligned"),
        (3, c(grid=S, tab=S + 4 * n ** 3 - 8), "the table overlaps the grid's last two elements"),
        (3, c(grid=S + 8 * (k + 1) * R.COLUMNS - 4, tab=S), "the grid overlaps the table's last four bytes"),
        (3, c(grid=short.data_ptr()), "short grid"),
        (3, c(tab=short_table.data_ptr()), "short table"),
        (3, c(grid=host_grid.ctypes.data), "host grid"),
        (3, c(tab=host_table.ctypes.data), "host table"),
        (5, c(dm=(65537, 1, 1), strides=(0, 0, 0)), "65 537 voxels along x"),
        (5, c(dm=(1, 1, 65537), strides=(0, 0, 0)), "65 537 voxels along z"),
        (5, c(origin=(65536 - n + 1, 0, 0)), "origin + dims above 65 536 along x"),
        (5, c(origin=(0, 0, 65536)), "origin + dims above 65 536 along z"),
        (5, c(grid=byte.data_ptr(), fmt=U8, dm=(1024, 1024, 2048), strides=(0, 0, 0)), "2^31 voxels"),
        (5, c(n_labels=2 ** 31 - 1), "n_labels 2^31 - 1"),
    ]
    msgs = []
    for code, fn, what in refusals:
        msgs.append(expect_code(code, fn, what))
        good()
    assert all("overlap" in t.split(": ", 1)[1] for t in msgs if "overlaps" in t.split(":")[0]), msgs
    # null dims, origin and out_outside, and a null context, at the ctypes level
    u3 = lambda v: (hip.C.c_uint32 * 3)(*v)   # noqa: E731
    u64 = lambda v: (hip.C.c_uint64 * 3)(*v)  # noqa: E731
    out = hip.C.c_uint64(99)
    base = [dv._ctx, G, I32, u64(s), u3(dims), u3((0, 0, 0)), k, R.ALL, T, hip.C.byref(out)]
    for i in (0, 4, 5, 9):
        args = list(base)
        args[i] = None
        assert L.o2v_hip_label_stats(*args) == 3 and out.value == 99, i
        good()
    # then correct calls: the table beside the grid in one allocation (the table 8-byte aligned), and U8 with n_labels 255
    shared[:n ** 3] = lab.reshape(-1)
    tab_at = S + 4 * n ** 3 + (4 * n ** 3) % 8
    torch.cuda.synchronize()
    assert dv.label_stats(S, I32, s, dims, (0, 0, 0), k, R.ALL, tab_at) == 0
    first = (tab_at - S) // 4
    got = shared[first:first + (k + 1) * R.COLUMNS * 2].cpu().numpy().view(np.int64).reshape(k + 1, R.COLUMNS)
    assert np.array_equal(got, want[0]) and bool((shared[first + (k + 1) * R.COLUMNS * 2:] == 5).all())
    same(call(dv, lab8, 255), R.label_stats(g_np.astype(np.uint8), 255), "U8 with n_labels 255")
    print("\n".join(msgs))
    print("refused", len(msgs) + 4)


# ---- one call per case and its wall time ------------------------------------------------------------------------------------------

CASES = {"shapes_and_layouts": case_shapes_and_layouts, "many_labels": case_many_labels, "out_of_range": case_out_of_range,
         "magnitudes": case_magnitudes, "faces": case_faces, "pipeline": case_pipeline, "refusals": case_refusals}

if __name__ == "__main__":
    t0 = time.time()
    CASES[sys.argv[1]]()
    print("case", sys.argv[1], "took %.1f s" % (time.time() - t0))
    print("ok")
