"""The GPU cases of tests/test_gpu_topology.py, each run in a child process of its own: `python -m tests.topology_cases <case>`.

torch is imported before the library is loaded (the grids are torch tensors; see tests/dense_cases.py).  Every comparison is
np.array_equal on int64 against the numpy reference of tests/topology_ref.py or against closed forms in Python ints, never against
the code under test, and there is no tolerance anywhere.  The tables are filled with a guard value before every call.  A case
prints what it covered and "ok" last when everything held."""
import os
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import topology_ref as R

DEV = torch.device("cuda", 0)
I32, U8 = hip.LABELS_I32, hip.LABELS_U8
GUARD = -7


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def st(t):
    """(x, y, z) element strides of a tensor [z, y, x]."""
    return t.stride(2), t.stride(1), t.stride(0)


def call(dv, t, n, table=None):
    """dv.euler_stats at the C level on the tensor view t [z, y, x] into a table filled with a guard value; (table, outside)."""
    if table is None:
        table = torch.full((n + 1, R.COLUMNS), GUARD, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    nz, ny, nx = t.shape
    outside = dv.euler_stats(t.data_ptr(), I32 if t.dtype == torch.int32 else U8, st(t), (nx, ny, nz), n, table.data_ptr())
    return table.cpu().numpy(), outside


def same(got, want, what):
    assert got[1] == want[1], (what, "outside", got[1], want[1])
    assert got[0].dtype == np.int64 and got[0].shape == want[0].shape, what
    bad = np.argwhere(got[0] != want[0])
    assert not len(bad), (what, len(bad), "elements differ, the first at", bad[0].tolist(), int(got[0][tuple(bad[0])]), int(want[0][tuple(bad[0])]))


def table_of(s):
    """An EulerStats as the table [n + 1, 7], on the host."""
    return torch.stack([s.voxels, s.faces, s.edges, s.vertices, s.inner_faces, s.inner_edges, s.inner_vertices], dim=1).cpu().numpy()


# ---- shapes and layouts -----------------------------------------------------------------------------------------------------------

def layouts(g):
    """name -> tensor view on the device: the grid g [z, y, x] in every layout of the case."""
    nz, ny, nx = g.shape
    t = dev(g)
    out = {"contiguous": t}
    flat = torch.zeros(g.size + 8, dtype=t.dtype, device=DEV)
    flat[1:1 + g.size] = t.reshape(-1)
    out["one element into an allocation"] = flat[1:1 + g.size].view(g.shape)     # (rows not aligned for 16-byte loads)
    wide = torch.zeros((nz, ny, 2 * nx), dtype=t.dtype, device=DEV)
    wide[:, :, ::2] = t
    out["x stride 2"] = wide[:, :, ::2]
    out["x and z swapped"] = t.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    out["a slice of a batch"] = torch.stack([torch.ones_like(t), t, torch.zeros_like(t)])[1]
    return out


def case_shapes_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(292)
    yz = [(1, 1), (2, 3), (3, 2), (1, 3), (3, 1), (2, 2), (3, 3), (1, 2), (2, 1)]
    shapes = [(x,) + yz[i % 9] for i, x in enumerate((1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025))] + [(70, 50, 40)]
    calls = grids = 0
    for i, dims in enumerate(shapes):
        for kind in ("int32", "uint8", "bool"):
            n = {"int32": (1, 7, 255, 1000)[i % 4], "uint8": (1, 7, 255, 0)[i % 4], "bool": 1}[kind]
            if kind == "bool":
                g = rng.random(dims[::-1]) < 0.5 if i % 2 else R.blobs(rng, dims, 1) != 0
            else:
                g = R.blobs(rng, dims, n, outside=0.1)                                                 # blobs, with values below 0 and above n
                if i % 3 == 2:
                    g = rng.integers(-1 if kind == "int32" else 0, n + 2, g.shape).astype(np.int32)    # noise
                g = g if kind == "int32" else (g & 255).astype(np.uint8)
            want = R.euler_stats(g, n)
            for name, t in layouts(g).items():
                assert t.shape == g.shape and np.array_equal(t.cpu().numpy(), g), (dims, kind, name)
                same(call(dv, t, n), want, (dims, kind, name))
                calls += 1
            grids += 1
    # through dense: the same numbers in EulerStats' fields
    g = R.blobs(rng, (70, 50, 40), 7, 0.1)
    s = dense.euler_stats(dv, dev(g), 7)
    want = R.euler_stats(g, 7)
    assert np.array_equal(table_of(s), want[0]) and s.outside == want[1] and s.n == 7
    assert np.array_equal(dense.euler_numbers(s).cpu().numpy(), R.euler_numbers(want[0])) and np.array_equal(dense.intrinsic_volumes(s).cpu().numpy(), R.intrinsic_volumes(want[0]))
    assert len(dv.euler_stats_times()) == 2 and all(v >= 0 for v in dv.euler_stats_times())
    print("shapes_and_layouts: compared", calls, "calls on", grids, "grids in 5 layouts")


# ---- row ends ---------------------------------------------------------------------------------------------------------------------

def case_row_ends():
    dv = hip.DeviceVoxelizer(0)
    n_calls = 0
    for dims in ((5, 3, 2), (17, 2, 3), (5, 2, 2), (17, 3, 3)):
        nx, ny, nz = dims
        g = np.arange(1, nx * ny * nz + 1, dtype=np.int32).reshape(nz, ny, nx)
        for t in layouts(g).values():
            table, outside = call(dv, t, g.size)
            assert outside == 0 and not table[0].any() and (table[1:] == np.array(R.SINGLE_VOXEL)).all(), (dims, table[:3].tolist())
            n_calls += 1
    print("row_ends: compared", n_calls, "calls with the single-voxel row")


# ---- many labels ------------------------------------------------------------------------------------------------------------------

def case_many_labels():
    mode = "every row to global memory" if os.environ.get("O2V_EU_NO_TABLE") == "1" else "the table in LDS"
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(293)
    own = np.arange(40 * 24 * 16, dtype=np.int32).reshape(16, 24, 40)
    table, outside = call(dv, dev(own), own.size - 1)
    assert outside == 0 and (table == np.array(R.SINGLE_VOXEL)).all(), mode
    same((table, outside), R.euler_stats(own, own.size - 1), ("every voxel its own label", mode))
    g = rng.integers(0, 5000, (48, 64, 96)).astype(np.int32)
    same(call(dv, dev(g), 4999), R.euler_stats(g, 4999), ("random labels out of 5000", mode))
    for dtype in (np.int32, np.uint8):
        board = R.checkerboard(4).astype(dtype)
        table, outside = call(dv, dev(board), 1)
        assert table[1].tolist() == [32, 192, 276, 121, 0, 0, 0] and outside == 0, mode
        z, y, x = np.indices((9, 10, 37))
        board = ((x + y + z) & 1).astype(dtype)
        same(call(dv, dev(board), 1), R.euler_stats(board, 1), ("checkerboard", dtype, mode))
        table, outside = call(dv, dev(np.full((64, 128, 256), 3, dtype)), 3)
        assert table[3].tolist() == R.box_row(256, 128, 64) and not table[:3].any() and outside == 0, mode
    print("many_labels: 8 grids with", mode)


# ---- hot rows ---------------------------------------------------------------------------------------------------------------------

def case_hot_rows():
    dv = hip.DeviceVoxelizer(0)
    n_calls = 0
    want = [32 * v for v in R.box_row(1, 64, 64)]
    for dtype in (torch.int32, torch.uint8):
        row = (torch.arange(64, device=DEV) % 2 + 1).to(dtype).reshape(1, 1, 64)
        t = row.expand(64, 64, 64)
        assert st(t) == (1, 0, 0)
        table, outside = call(dv, t, 2)
        assert outside == 0 and not table[0].any() and table[1].tolist() == want == table[2].tolist(), (dtype, table.tolist(), want)
        n_calls += 1
    print("hot_rows:", n_calls, "calls on 64^3")


# ---- magnitudes -------------------------------------------------------------------------------------------------------------------

def case_magnitudes():
    dv = hip.DeviceVoxelizer(0)
    nx, ny, nz = 1024, 1024, 2047
    row = torch.full((1, 1, nx), 3, dtype=torch.uint8, device=DEV)
    big = row.expand(nz, ny, nx)
    assert big.numel() == 2146435072
    t0 = time.time()
    s = dense.euler_stats(dv, big, 3)
    torch.cuda.synchronize()
    wall = time.time() - t0
    ms = dv.euler_stats_times()
    want = R.box_row(nx, ny, nz)
    got = table_of(s)
    assert got[3].tolist() == want and not got[:3].any() and s.outside == 0, (got.tolist(), want)
    assert want[1] > 2 ** 32 and want[2] > 2 ** 32 and max(want) < 2 ** 36
    assert int(dense.euler_numbers(s)[3]) == 1 == int(dense.euler_numbers(s, 6)[3]) and dense.intrinsic_volumes(s)[3].tolist() == [1, nx + ny + nz, nx * ny + ny * nz + nx * nz, nx * ny * nz]
    print(f"magnitudes: 2 146 435 072 voxels, {want[2]} closed-in edges; device ms {ms[0]:.3f} + {ms[1]:.3f}, wall {wall:.2f} s")


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------

def indexed(verts):
    positions, faces = np.unique(np.asarray(verts, np.float32).reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    return dev(positions.view(np.float32)), dev(faces.reshape(-1, 3).astype(np.int32))


def torus(x, y, z, centre, axis, R_, r):
    """The solid torus around `centre` whose circle of radius R_ lies across `axis`, with tube radius r (torch)."""
    d = [x - centre[0], y - centre[1], z - centre[2]]
    along = d.pop(axis)
    return (torch.sqrt(d[0] ** 2 + d[1] ** 2) - R_) ** 2 + along ** 2 < r * r


def analytic_grids():
    """name -> (bool grid on the device, (b0, b1, b2)): shapes thick enough that 6 and 26 agree."""
    z, y, x = torch.meshgrid(*(torch.arange(64, dtype=torch.float32, device=DEV),) * 3, indexing="ij")
    c = (31.5, 31.5, 31.5)
    r2 = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
    return {
        "ball": (r2 < 20 ** 2, (1, 0, 0)),
        "torus": (torus(x, y, z, c, 2, 18, 6), (1, 1, 0)),
        "hollow sphere": ((r2 < 26 ** 2) & (r2 > 18 ** 2), (1, 0, 1)),
        "two linked tori": (torus(x, y, z, (24.5, 31.5, 31.5), 2, 14, 4) | torus(x, y, z, (38.5, 31.5, 31.5), 1, 14, 4), (2, 2, 0)),
        "a ball with a torus-shaped cavity": ((r2 < 28 ** 2) & ~torus(x, y, z, c, 2, 14, 5), (1, 1, 1)),
    }


def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    for name, (grid, want) in analytic_grids().items():
        g = grid.cpu().numpy()
        same(call(dv, grid.to(torch.uint8), 1), R.euler_stats(g, 1), name)                          # (the arbiter for K25)
        for conn in (26, 6):
            got = dense.betti_numbers(dv, grid, connectivity=conn)
            assert got == want, (name, conn, got, want)
            # the per-component Euler numbers of the components' labels add up to the set's
            labels, n = dense.components(dv, grid, connectivity=conn)
            per = dense.euler_numbers(dense.euler_stats(dv, labels, n), conn)
            whole = dense.euler_numbers(dense.euler_stats(dv, grid), conn)
            assert int(per[1:].sum()) == int(whole[1]) == want[0] - want[1] + want[2], (name, conn, per.tolist(), whole.tolist())
        print(f"pipeline: {name} at 64^3: betti {want} at 26 and at 6", flush=True)
    # a random grid: many components, the rows add; K25 against the reference on the components' labels
    noise = dev(np.random.default_rng(294).random((40, 50, 70)) < 0.3)
    for conn in (26, 6):
        labels, n = dense.components(dv, noise, connectivity=conn)
        s = dense.euler_stats(dv, labels, n)
        want = R.euler_stats(labels.cpu().numpy(), n)
        assert np.array_equal(table_of(s), want[0]) and s.outside == 0 == want[1]
        assert int(dense.euler_numbers(s, conn)[1:].sum()) == int(dense.euler_numbers(dense.euler_stats(dv, noise), conn)[1]), conn
    # the filled bench mesh: the exposed faces are label_stats' faces
    dense.set_mesh(dv, *indexed(meshes.scan_like()))
    small, _ = dense.voxelize_dense(dv, 64, fmt="labels", fill=True)
    same(call(dv, small, 2), R.euler_stats(small.cpu().numpy(), 2), "scan_like at 64, filled")       # (the arbiter for K25)
    filled, _ = dense.voxelize_dense(dv, 256, fmt="labels", fill=True)
    assert filled.dtype == torch.uint8 and int(filled.max()) == 2
    s = dense.euler_stats(dv, filled, 2)
    ls = dense.label_stats(dv, filled, 2, faces=True)
    assert torch.equal(6 * s.voxels - 2 * s.inner_faces, ls.faces) and torch.equal(s.voxels, ls.count) and s.outside == 0
    print(f"pipeline: scan_like at 256, filled: exposed faces {ls.faces.tolist()} = 6 voxels - 2 inner faces; chi_26 {dense.euler_numbers(s).tolist()}", flush=True)
    # thinning keeps components, tunnels and cavities: a thick ring with one spur, and the filled bench mesh
    z, y, x = np.indices((9, 48, 64))
    r = np.hypot(x - 24, y - 24)
    ring = dev(((r > 12) & (r < 19) | (abs(y - 24) < 3) & (x >= 40) & (x < 60)) & (abs(z - 4) < 3))
    solid, _ = dense.voxelize_dense(dv, 128, fill=True)
    for name, grid in (("a ring with a spur", ring), ("scan_like at 128, filled", solid)):
        before = dense.betti_numbers(dv, grid)
        after = dense.betti_numbers(dv, dense.skeletonize(dv, grid, mode="ultimate"))
        print(f"pipeline: {name}: betti {before} before and {after} after skeletonize(mode='ultimate')", flush=True)
        assert before == after, (name, before, after)
    assert dense.betti_numbers(dv, ring) == (1, 1, 0)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list but the failed scratch allocation (the scratch is one counter).  This child runs with
    torch's caching allocator off: each tensor is an allocation of its own, so a short one is short."""
    dv = hip.DeviceVoxelizer(0)
    L = hip._bind()
    C = hip.C
    n, k = 48, 7
    dims, s = (n, n, n), (1, n, n * n)
    rng = np.random.default_rng(295)
    g_np = R.blobs(rng, dims, k)
    want = R.euler_stats(g_np, k)
    lab, lab8 = dev(g_np), dev(g_np.astype(np.uint8))
    table = torch.full((k + 1, R.COLUMNS), GUARD, dtype=torch.int64, device=DEV)
    short_table = torch.full((k // 2, R.COLUMNS), GUARD, dtype=torch.int64, device=DEV)
    short = torch.full((n // 2, n, n), 5, dtype=torch.int32, device=DEV)
    shared = torch.full((n ** 3 + (k + 1) * R.COLUMNS * 2 + 2,), 5, dtype=torch.int32, device=DEV)   # the grid and a table in one allocation
    byte = torch.zeros((1, 1, 1), dtype=torch.uint8, device=DEV)
    host_grid, host_table = g_np.copy(), np.zeros((k + 1, R.COLUMNS), np.int64)
    torch.cuda.synchronize()
    G, T, S = lab.data_ptr(), table.data_ptr(), shared.data_ptr()
    u3 = lambda a: None if a is None else (C.c_uint32 * 3)(*a)    # noqa: E731
    u64 = lambda a: None if a is None else (C.c_uint64 * 3)(*a)   # noqa: E731
    msgs = []

    def good():
        """After a refusal the context still works, and the refusal wrote nothing."""
        assert bool((table == GUARD).all()) and bool((short_table == GUARD).all()) and bool((shared == 5).all()) and np.array_equal(lab.cpu().numpy(), g_np)
        same(call(dv, lab, k), want, "after a refusal")

    def refused(code, what, ctx=dv._ctx, grid=G, fmt=I32, strides=s, dm=dims, n_labels=k, tab=T, out=True):
        outside = C.c_uint64(99)
        rc = L.o2v_hip_euler_stats(ctx, grid, fmt, u64(strides), u3(dm), n_labels, tab, C.byref(outside) if out else None)
        assert rc == code and outside.value == 99, (what, rc, outside.value)
        if ctx:
            msgs.append(what + ": " + L.o2v_hip_last_error(ctx).decode())
            assert "o2v_hip_euler_stats" in msgs[-1], msgs[-1]
        good()

    for what, kw in [
        ("null context", dict(ctx=None)), ("null grid", dict(grid=None)), ("null strides", dict(strides=None)), ("null dims", dict(dm=None)),
        ("null table", dict(tab=None)), ("null out_outside", dict(out=False)), ("zero dims", dict(dm=(n, 0, n))), ("unknown format", dict(fmt=2)),
        ("n_labels 256 for U8", dict(grid=lab8.data_ptr(), fmt=U8, n_labels=256)), ("a table that is not 8-byte aligned", dict(tab=T + 4)),
        ("an int32 grid that is not 4-byte aligned", dict(grid=G + 2)),
        ("the table overlaps the grid's last two elements", dict(grid=S, tab=S + 4 * n ** 3 - 8)),
        ("the grid overlaps the table's last four bytes", dict(grid=S + 8 * (k + 1) * R.COLUMNS - 4, tab=S)),
        ("short grid", dict(grid=short.data_ptr())), ("short table", dict(tab=short_table.data_ptr())),
        ("host grid", dict(grid=host_grid.ctypes.data)), ("host table", dict(tab=host_table.ctypes.data)),
    ]:
        refused(3, what, **kw)
    for what, kw in [
        ("65 537 voxels along x", dict(dm=(65537, 1, 1), strides=(0, 0, 0))), ("65 537 voxels along z", dict(dm=(1, 1, 65537), strides=(0, 0, 0))),
        ("2^31 voxels", dict(grid=byte.data_ptr(), fmt=U8, dm=(1024, 1024, 2048), strides=(0, 0, 0))),   # (an expanded byte that is never read)
        ("n_labels 2^31 - 1", dict(n_labels=2 ** 31 - 1)),
        ("the limit before the pointer", dict(grid=host_grid.ctypes.data, dm=(65537, 1, 1), strides=(0, 0, 0))),
    ]:
        refused(5, what, **kw)
    assert all("overlap" in t.split(": ", 1)[1] for t in msgs if "overlaps" in t.split(":")[0]), msgs
    assert L.o2v_hip_euler_stats_times(None, None) == 3
    # then correct calls: the table beside the grid in one allocation (the table 8-byte aligned), and U8 with n_labels 255
    shared[:n ** 3] = lab.reshape(-1)
    tab_at = S + 4 * n ** 3 + (4 * n ** 3) % 8
    torch.cuda.synchronize()
    assert dv.euler_stats(S, I32, s, dims, k, tab_at) == 0
    first = (tab_at - S) // 4
    got = shared[first:first + (k + 1) * R.COLUMNS * 2].cpu().numpy().view(np.int64).reshape(k + 1, R.COLUMNS)
    assert np.array_equal(got, want[0]) and bool((shared[first + (k + 1) * R.COLUMNS * 2:] == 5).all())
    same(call(dv, lab8, 255), R.euler_stats(g_np.astype(np.uint8), 255), "U8 with n_labels 255")
    print("\n".join(msgs))
    print("refused", len(msgs) + 1, "calls")


# ---- one call per case and its wall time ------------------------------------------------------------------------------------------

CASES = {"shapes_and_layouts": case_shapes_and_layouts, "row_ends": case_row_ends, "many_labels": case_many_labels, "hot_rows": case_hot_rows,
         "magnitudes": case_magnitudes, "pipeline": case_pipeline, "refusals": case_refusals}

if __name__ == "__main__":
    t0 = time.time()
    CASES[sys.argv[1]]()
    print("case", sys.argv[1], "took %.1f s" % (time.time() - t0))
    print("ok")
