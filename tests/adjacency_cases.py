"""The GPU cases of tests/test_gpu_adjacency.py, each run in a child process of its own: `python -m tests.adjacency_cases <case>`.

torch is imported before the library is loaded (the grids are torch tensors; see tests/dense_cases.py).  Every comparison is
np.array_equal against the numpy reference of tests/adjacency_ref.py or against closed forms in Python ints, never against the
code under test, and there is no tolerance anywhere.  A case prints what it covered and "ok" last when everything held."""
import os
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from obj2voxel_amd import watershed as WS
from tests import adjacency_ref as R
from tests import label_stats_ref as LR
from tests import watershed_ref as WR

DEV = torch.device("cuda", 0)
I32, U8 = hip.LABELS_I32, hip.LABELS_U8
GUARD = -7
TIMES = hip.FLAG_STAGE_TIMES


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def st(t):
    """(x, y, z) element strides of a tensor [z, y, x]."""
    return t.stride(2), t.stride(1), t.stride(0)


def switch(name, value):
    """An environment switch for the calls that follow (the library reads its switches at every call); None: unset."""
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)


def call(dv, t, n, conn=6, zero=False, values=None, flags=0):
    """adjacency_count and adjacency_write at the C level on the tensor view t [z, y, x], into arrays with two guard rows behind
    the list; (pairs, table, outside)."""
    torch.cuda.synchronize()
    nz, ny, nx = t.shape
    m, outside = dv.adjacency_count(t.data_ptr(), I32 if t.dtype == torch.int32 else U8, st(t), (nx, ny, nz), n, conn, flags | (hip.ADJ_ZERO if zero else 0),
                                    None if values is None else values.data_ptr(), None if values is None else st(values))
    pairs = torch.full((m + 2, 2), GUARD, dtype=torch.int32, device=DEV)
    table = torch.full((m + 2, R.COLUMNS), GUARD, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    dv.adjacency_write(pairs.data_ptr(), table.data_ptr(), m)
    assert bool((pairs[m:] == GUARD).all()) and bool((table[m:] == GUARD).all())
    return pairs[:m].cpu().numpy(), table[:m].cpu().numpy(), outside


def same(got, want, what):
    assert got[2] == want[2], (what, "outside", got[2], want[2])
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64, what
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), (what, "pairs", got[0].shape, want[0].shape, got[0][:6].tolist(), want[0][:6].tolist())
    bad = np.argwhere(got[1] != want[1])
    assert not len(bad), (what, len(bad), "elements differ, the first at", bad[0].tolist(), int(got[1][tuple(bad[0])]), int(want[1][tuple(bad[0])]))


# ---- shapes and layouts -----------------------------------------------------------------------------------------------------------

def layouts(g):
    """name -> (tensor view on the device, the numpy grid it holds): the grid g [z, y, x] in every layout the call takes."""
    nz, ny, nx = g.shape
    t = dev(g)
    out = {"contiguous": (t, g)}
    out["x and z swapped"] = (t.permute(2, 1, 0).contiguous().permute(2, 1, 0), g)
    wide = torch.zeros((nz, ny, 2 * nx), dtype=t.dtype, device=DEV)
    wide[:, :, ::2] = t
    out["x stride 2"] = (wide[:, :, ::2], g)
    out["a plane expanded along z"] = (t[:1].expand(nz, ny, nx), np.broadcast_to(g[:1], g.shape))
    flat = torch.zeros(g.size + 8, dtype=t.dtype, device=DEV)
    flat[1:1 + g.size] = t.reshape(-1)
    out["one element into an allocation"] = (flat[1:1 + g.size].view(g.shape), g)     # (rows not aligned for 16-byte loads)
    return out


def case_shapes_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(243)
    yz = [(1, 1), (2, 3), (3, 2), (1, 3), (3, 1), (2, 2), (3, 3), (1, 2), (2, 1)]
    shapes = [(x, *yz[(2 * i + k) % 9]) for i, x in enumerate((1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025)) for k in (0, 1)]
    combos = [(conn, zero, vals) for conn in (6, 18, 26) for zero in (False, True) for vals in (False, True)]
    calls = grids = 0
    seen = set()
    for i, dims in enumerate(shapes):
        for kind in ("int32", "uint8", "bool"):
            n = {"int32": (1, 7, 255, 1000)[i % 4], "uint8": (1, 7, 254)[i % 3], "bool": 1}[kind]
            if grids % 2:
                g = LR.blobs(rng, dims, n, 0.1 if kind == "int32" else 0.0)
                if kind == "uint8":
                    g[rng.random(g.shape) < 0.1] = n + 1   # (above n)
            else:   # pure noise, with values below 0 and above n among them
                g = rng.integers(-1 if kind == "int32" else 0, 2 if kind == "bool" else n + 2, dims[::-1])
            g = g.astype({"int32": np.int32, "uint8": np.uint8, "bool": np.bool_}[kind])
            v = rng.integers(-1000, 1000, g.shape).astype(np.int32)
            v_views = layouts(v)
            v_names = list(v_views)
            wants = {}
            for k, (name, (t, held)) in enumerate(layouts(g).items()):
                assert t.shape == g.shape and np.array_equal(t.cpu().numpy(), held), (dims, kind, name)
                todo = [combos[(grids + k) % 12]]
                if name == "contiguous":   # ... and every connectivity, with the other flags flipped
                    conn0, zero0, vals0 = todo[0]
                    todo += [(c, not zero0, not vals0) for c in (6, 18, 26)]
                for conn, zero, vals in todo:
                    vt, vheld = v_views[v_names[(k + 1) % len(v_names)]] if vals else (None, None)   # (values in a layout of their own)
                    key = (name.startswith("a plane"), conn, zero, None if not vals else v_names[(k + 1) % len(v_names)].startswith("a plane"))
                    if key not in wants:
                        wants[key] = R.adjacency(held, n, conn, zero, vheld)
                    same(call(dv, t, n, conn, zero, vt), wants[key], (dims, kind, name, conn, zero, vals))
                    seen.add((conn, zero, vals, kind))
                    calls += 1
            grids += 1
    assert len(seen) == 36 and grids == 78
    # through dense: the same numbers in LabelAdjacency's fields
    g = LR.blobs(rng, (70, 50, 40), 7)
    v = rng.integers(0, 100, g.shape).astype(np.int32)
    adj = dense.label_adjacency(dv, dev(g), 7, connectivity=26, background=True, values=dev(v))
    want = R.adjacency(g, 7, 26, True, v)
    assert np.array_equal(adj.pairs.cpu().numpy(), want[0]) and len(want[0]) > 10 and adj.outside == want[2] == 0
    assert np.array_equal(torch.stack([adj.faces, adj.edges, adj.corners, adj.pass_high.to(torch.int64), adj.pass_low.to(torch.int64)], 1).cpu().numpy(), want[1])
    assert len(dv.adjacency_times()) == 4 and all(x >= 0 for x in dv.adjacency_times()) and dv.adjacency_counters() == (0, 0, 0, 0)
    assert dv.adjacency_scratch_bytes(10) == 48 * 10 + 64
    print("shapes_and_layouts: compared", calls, "calls on", grids, "grids in 5 layouts")


# ---- row ends ---------------------------------------------------------------------------------------------------------------------

def case_row_ends():
    dv = hip.DeviceVoxelizer(0)
    n_calls = 0
    for dims in ((5, 3, 2), (17, 2, 3), (5, 2, 2), (17, 3, 3)):
        nx, ny, nz = dims
        g = np.arange(1, nx * ny * nz + 1, dtype=np.int32).reshape(nz, ny, nx)
        for conn, want_pairs in zip((6, 18, 26), R.grid_pair_counts(*dims)):
            for t in (dev(g), dev(g.astype(np.uint8))) if g.size < 256 else (dev(g),):
                got = call(dv, t, g.size, conn)
                same(got, R.adjacency(g, g.size, conn), ("row ends", dims, conn))
                assert len(got[0]) == want_pairs and (got[1][:, :3].sum(1) == 1).all(), (dims, conn, len(got[0]), want_pairs)
                # the last voxel of a row and the first of the next follow each other in memory and are no neighbours (nx > 2)
                ends = {(i, i + 1) for i in range(nx, g.size, nx)}
                assert len(ends) == ny * nz - 1 and not ends & {tuple(p) for p in got[0].tolist()}
                n_calls += 1
    print("row_ends: compared", n_calls, "calls with the closed forms")


# ---- many pairs -------------------------------------------------------------------------------------------------------------------

def case_many_pairs():
    no_table = os.environ.get("O2V_ADJ_NO_TABLE") == "1"
    assert int(os.environ.get("O2V_ADJ_TABLE_LOG2", "0")) == 10
    dv = hip.DeviceVoxelizer(0)
    nx, ny, nz = 64, 32, 16
    g = np.arange(1, nx * ny * nz + 1, dtype=np.int32).reshape(nz, ny, nx)
    v = np.random.default_rng(244).integers(0, 2 ** 31 - 1, g.shape).astype(np.int32)
    want = R.adjacency(g, g.size, 26, False, v)
    assert len(want[0]) == R.grid_pair_counts(nx, ny, nz)[2] == 394396
    t0 = time.time()
    got = call(dv, dev(g), g.size, 26, False, dev(v), TIMES)
    wall = time.time() - t0
    same(got, want, "many pairs")
    to_lds, to_global, growths, table_bytes = dv.adjacency_counters()
    assert growths >= 9 and table_bytes == 48 << (10 + growths), (growths, table_bytes)
    if no_table:
        assert to_lds == 0 and to_global >= len(want[0])
    else:
        assert to_lds > 0 and to_global > 0      # (256 slots a workgroup: the probes run out)
    print(f"many_pairs: {len(want[0])} pairs, {'every flush to global memory' if no_table else 'with the table in LDS'}: {to_lds} flushes into LDS, "
          f"{to_global} to global memory, {growths} growths to {table_bytes} bytes; wall {wall:.2f} s, stages {dv.adjacency_times()}")


# ---- hot pair ---------------------------------------------------------------------------------------------------------------------

def alternating(nx, ny, nz, dtype):
    """Two labels alternating along x, broadcast over y and z by strides of 0."""
    row = ((torch.arange(nx, device=DEV) & 1) + 1).to(dtype).reshape(1, 1, nx)
    return row.expand(nz, ny, nx)


def case_hot_pair():
    dv = hip.DeviceVoxelizer(0)
    n_calls = 0
    for dtype in (torch.int32, torch.uint8):
        t = alternating(64, 64, 64, dtype)
        assert st(t) == (1, 0, 0)
        for off in (None, 1):
            switch("O2V_ADJ_NO_TABLE", off)
            for conn in (6, 18, 26):
                pairs, table, outside = call(dv, t, 2, conn, flags=TIMES)
                want = R.alternating_row(64, 64, 64)
                want = [want[0], want[1] if conn > 6 else 0, want[2] if conn > 18 else 0, 0, 0]
                assert pairs.tolist() == [[1, 2]] and table.tolist() == [want] and outside == 0, (dtype, off, conn, table.tolist(), want)
                to_lds, to_global, growths, _ = dv.adjacency_counters()
                assert growths == 0 and (to_lds == 0) == bool(off) and (to_global == 0) != bool(off)
                n_calls += 1
            switch("O2V_ADJ_NO_TABLE", None)
    print("hot_pair:", n_calls, "calls on 64^3, with and without the table in LDS")


# ---- magnitudes -------------------------------------------------------------------------------------------------------------------

def case_magnitudes():
    dv = hip.DeviceVoxelizer(0)
    nx, ny, nz = 2048, 1024, 1023
    t = alternating(nx, ny, nz, torch.int32)
    assert t.numel() == 2145386496
    t0 = time.time()
    adj = dense.label_adjacency(dv, t, 2, connectivity=26)
    torch.cuda.synchronize()
    wall = time.time() - t0
    ms = dv.adjacency_times()
    want = [2144338944, 8568975358, 8560603128]
    assert want == R.alternating_row(nx, ny, nz) and want[1] > 2 ** 32 and want[2] > 2 ** 32
    got = [int(adj.faces[0]), int(adj.edges[0]), int(adj.corners[0])]
    assert adj.pairs.tolist() == [[1, 2]] and got == want and adj.outside == 0, (adj.pairs.tolist(), got, want)
    assert int(adj.contacts[0]) == sum(want)
    print(f"magnitudes: 2 145 386 496 voxels, one pair, {sum(want)} contacts; device ms {ms[0]:.3f} + {ms[1]:.3f} + {ms[2]:.3f} + {ms[3]:.3f}, wall {wall:.2f} s")


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------

def indexed(verts):
    positions, faces = np.unique(np.asarray(verts, np.float32).reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    return dev(positions.view(np.float32)), dev(faces.reshape(-1, 3).astype(np.int32))


def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    # two balls sintered at a neck: two parts, one pair, and the neck's depth is watershed's merge threshold
    solid = dev(WR.dumbbell())
    labels, n = dense.split_parts(dv, solid, min_depth=1.0)
    relief = WS.scaled_root(dense.inner_distance(dv, solid), 4)
    adj = dense.label_adjacency(dv, labels, n, connectivity=26, values=relief)
    want = R.adjacency(labels.cpu().numpy(), n, 26, False, relief.cpu().numpy())
    assert n == 2 and adj.pairs.tolist() == [[1, 2]] and np.array_equal(adj.pairs.cpu().numpy(), want[0])
    assert [int(adj.faces[0]), int(adj.edges[0]), int(adj.corners[0]), int(adj.pass_high[0]), int(adj.pass_low[0])] == want[1][0].tolist()
    _, heights = dense.watershed_peaks(labels, relief, n)
    depth = int(heights.min()) - int(adj.pass_high[0])
    assert depth > 0
    assert dense.watershed(dv, relief, min_depth=depth + 1)[1] == 1 and dense.watershed(dv, relief, min_depth=depth)[1] == 2
    assert dense.coordination(adj).tolist() == [0, 1, 1]
    print(f"pipeline: two balls: the neck {int(adj.faces[0])} faces wide, pass_high {int(adj.pass_high[0])}, {depth} below the lower top", flush=True)
    # fill=True labels with the background: a label's faces are its contacts and its share of the box's six sides
    dense.set_mesh(dv, *indexed(meshes.scan_like()))
    filled, _ = dense.voxelize_dense(dv, 64, fill=True)
    top = int(filled.max())
    stats = dense.label_stats(dv, filled, top, faces=True)
    adj = dense.label_adjacency(dv, filled, top, connectivity=6, background=True)
    want = R.adjacency(filled.cpu().numpy(), top, 6, True)
    assert np.array_equal(adj.pairs.cpu().numpy(), want[0]) and np.array_equal(adj.faces.cpu().numpy(), want[1][:, 0]) and len(want[0]) >= 1
    contact = torch.zeros(top + 1, dtype=torch.int64, device=DEV)
    contact.index_add_(0, adj.pairs[:, 0].to(torch.int64), adj.faces)
    contact.index_add_(0, adj.pairs[:, 1].to(torch.int64), adj.faces)
    sides = sum(torch.bincount(s.reshape(-1).to(torch.int64), minlength=top + 1)
                for s in (filled[0], filled[-1], filled[:, 0], filled[:, -1], filled[:, :, 0], filled[:, :, -1]))
    assert torch.equal(contact + sides, stats.faces), (contact.tolist(), sides.tolist(), stats.faces.tolist())
    print(f"pipeline: scan_like at 64, filled: labels 0 ... {top}, {len(want[0])} pairs, faces {stats.faces.tolist()} = contacts + box sides", flush=True)
    # the graph of a device-made skeleton: a thick ring with one spur
    z, y, x = np.indices((9, 48, 64))
    r = np.hypot(x - 24, y - 24)
    shape = ((r > 12) & (r < 19) | (abs(y - 24) < 3) & (x >= 40) & (x < 60)) & (abs(z - 4) < 3)
    degree = dense.skeletonize(dv, dev(shape), fmt="degree")
    graph = dense.skeleton_graph(dv, degree)
    labels, n_nodes, n_branches, incidence, contacts = R.skeleton_graph(degree.cpu().numpy())
    assert np.array_equal(graph.labels.cpu().numpy(), labels) and (graph.n_nodes, graph.n_branches) == (n_nodes, n_branches)
    assert np.array_equal(graph.incidence.cpu().numpy(), incidence) and np.array_equal(graph.node_contacts.cpu().numpy(), contacts)
    count = np.bincount(labels.reshape(-1), minlength=n_nodes + n_branches + 1)
    assert graph.node_voxels.tolist() == count[1:n_nodes + 1].tolist() and graph.branch_voxels.tolist() == count[n_nodes + 1:].tolist()
    assert n_nodes >= 2 and n_branches >= 2 and len(incidence) >= 3
    print(f"pipeline: a ring with a spur: {n_nodes} nodes, {n_branches} branches, {len(incidence)} incidences")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list.  This child runs with torch's caching allocator off: each tensor is an allocation of
    its own, so a short one is short."""
    dv = hip.DeviceVoxelizer(0)
    L = hip._bind()
    C = hip.C
    n, k = 40, 7
    dims, s = (n, n, n), (1, n, n * n)
    rng = np.random.default_rng(245)
    g_np = LR.blobs(rng, dims, k)
    v_np = rng.integers(0, 50, g_np.shape).astype(np.int32)
    want = R.adjacency(g_np, k, 26, False, v_np)
    m = len(want[0])
    lab, lab8, val = dev(g_np), dev(g_np.astype(np.uint8)), dev(v_np)
    short = torch.full((n // 2, n, n), 5, dtype=torch.int32, device=DEV)
    byte = torch.zeros((1, 1, 1), dtype=torch.uint8, device=DEV)
    host_grid = g_np.copy()
    torch.cuda.synchronize()
    G, V = lab.data_ptr(), val.data_ptr()
    u3 = lambda a: None if a is None else (C.c_uint32 * 3)(*a)    # noqa: E731
    u64 = lambda a: None if a is None else (C.c_uint64 * 3)(*a)   # noqa: E731
    msgs = []

    def good():
        same(call(dv, lab, k, 26, False, val), want, "after a refusal")

    def count(code, what, ctx=dv._ctx, grid=G, fmt=I32, strides=s, dm=dims, n_labels=k, conn=26, flags=0, values=V, vstrides=s, out=(True, True)):
        """The call is refused with `code`, its outputs are untouched, and a write behind it is refused too."""
        pairs, outside = C.c_uint64(99), C.c_uint64(98)
        rc = L.o2v_hip_adjacency_count(ctx, grid, fmt, u64(strides), u3(dm), n_labels, conn, flags, values, u64(vstrides), C.byref(pairs) if out[0] else None,
                                       C.byref(outside) if out[1] else None)
        assert rc == code and pairs.value == 99 and outside.value == 98, (what, rc, pairs.value, outside.value)
        if ctx:
            msgs.append(what + ": " + L.o2v_hip_last_error(ctx).decode())
            assert "o2v_hip_adjacency_count" in msgs[-1], msgs[-1]
            assert L.o2v_hip_adjacency_write(ctx, None, None, 1 << 40) == 3, what     # (a refused count is no count)
        good()

    fresh = hip.DeviceVoxelizer(0)
    assert L.o2v_hip_adjacency_write(fresh._ctx, None, None, 0) == 3                    # no count before it
    fresh.close()
    for what, kw in [
        ("null context", dict(ctx=None)), ("null grid", dict(grid=None)), ("null strides", dict(strides=None)), ("null dims", dict(dm=None)),
        ("null out_pairs", dict(out=(False, True))), ("null out_outside", dict(out=(True, False))), ("values without strides", dict(vstrides=None)),
        ("zero dims", dict(dm=(n, 0, n))), ("unknown format", dict(fmt=2)), ("connectivity 8", dict(conn=8)), ("connectivity 0", dict(conn=0)),
        ("unknown flag bit", dict(flags=32)), ("unknown high flag bit", dict(flags=0x80000000)),
        ("n_labels 256 for U8", dict(grid=lab8.data_ptr(), fmt=U8, n_labels=256)), ("an int32 grid that is not 4-byte aligned", dict(grid=G + 2)),
        ("values that are not 4-byte aligned", dict(values=V + 2)), ("short grid", dict(grid=short.data_ptr())), ("short values", dict(values=short.data_ptr())),
        ("host grid", dict(grid=host_grid.ctypes.data)), ("host values", dict(values=host_grid.ctypes.data)),
    ]:
        count(3, what, **kw)
    for what, kw in [
        ("65 537 voxels along x", dict(dm=(65537, 1, 1), strides=(0, 0, 0), vstrides=(0, 0, 0))),
        ("65 537 voxels along z", dict(dm=(1, 1, 65537), strides=(0, 0, 0), vstrides=(0, 0, 0))),
        ("2^31 voxels", dict(grid=byte.data_ptr(), fmt=U8, dm=(1024, 1024, 2048), strides=(0, 0, 0), values=None, vstrides=None)),
        ("n_labels 2^31 - 1", dict(n_labels=2 ** 31 - 1)),
        ("the limit before the pointer", dict(grid=host_grid.ctypes.data, dm=(65537, 1, 1), strides=(0, 0, 0), vstrides=(0, 0, 0))),
    ]:
        count(5, what, **kw)
    # the write: after a count of m pairs
    torch.cuda.synchronize()
    assert dv.adjacency_count(G, I32, s, dims, k, 26, 0, V, s) == (m, want[2]) and m > 4
    pairs = torch.full((m, 2), GUARD, dtype=torch.int32, device=DEV)
    table = torch.full((m, R.COLUMNS), GUARD, dtype=torch.int64, device=DEV)
    both = torch.full((m * 6,), GUARD, dtype=torch.int64, device=DEV)
    short_pairs = torch.full((m - 1, 2), GUARD, dtype=torch.int32, device=DEV)
    short_table = torch.full((m - 1, R.COLUMNS), GUARD, dtype=torch.int64, device=DEV)
    host_pairs, host_table = np.zeros((m, 2), np.int32), np.zeros((m, R.COLUMNS), np.int64)
    torch.cuda.synchronize()
    P, T, B = pairs.data_ptr(), table.data_ptr(), both.data_ptr()
    writes = [("capacity below the pairs", (P, T, m - 1)), ("null pairs", (None, T, m)), ("null table", (P, None, m)), ("pairs not 4-byte aligned", (P + 2, T, m)),
              ("table not 8-byte aligned", (P, T + 4, m)), ("short pairs", (short_pairs.data_ptr(), T, m)), ("short table", (P, short_table.data_ptr(), m)),
              ("host pairs", (host_pairs.ctypes.data, T, m)), ("host table", (P, host_table.ctypes.data, m)),
              ("table overlaps the pairs' last bytes", (B, B + 8 * m - 8, m)), ("pairs overlap the table's last bytes", (B + 40 * m - 8, B, m))]
    for what, args in writes:
        assert L.o2v_hip_adjacency_write(dv._ctx, *args) == 3, what
        torch.cuda.synchronize()
        assert bool((pairs == GUARD).all()) and bool((table == GUARD).all()) and bool((both == GUARD).all()) and bool((short_pairs == GUARD).all()), what
        assert bool((short_table == GUARD).all())
    assert L.o2v_hip_adjacency_write(None, P, T, m) == 3
    # ... and the correct write still follows, twice: pairs and table side by side in one allocation
    dv.adjacency_write(P, T, m)
    dv.adjacency_write(B + 40 * m, B, m)
    assert np.array_equal(pairs.cpu().numpy(), want[0]) and np.array_equal(table.cpu().numpy(), want[1])
    assert np.array_equal(both[:5 * m].cpu().numpy().reshape(m, 5), want[1]) and np.array_equal(both[5 * m:].cpu().numpy().view(np.int32).reshape(m, 2), want[0])
    # no pairs: both pointers may be null
    assert dv.adjacency_count(G, I32, s, dims, 0, 6, 0) == (0, int((g_np != 0).sum()))
    dv.adjacency_write(None, None, 0)
    good()
    print("\n".join(msgs))
    print("refused", len(msgs) + 1, "counts and", len(writes) + 2, "writes")


# ---- one call per case and its wall time ------------------------------------------------------------------------------------------

CASES = {"shapes_and_layouts": case_shapes_and_layouts, "row_ends": case_row_ends, "many_pairs": case_many_pairs, "hot_pair": case_hot_pair,
         "magnitudes": case_magnitudes, "pipeline": case_pipeline, "refusals": case_refusals}

if __name__ == "__main__":
    t0 = time.time()
    CASES[sys.argv[1]]()
    print("case", sys.argv[1], "took %.1f s" % (time.time() - t0))
    print("ok")
