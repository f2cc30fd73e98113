"""The GPU cases of tests/test_gpu_watershed.py, each run in a child process of its own: `python -m tests.watershed_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison with the reference
(tests/watershed_ref.py) is np.array_equal / torch.equal on the labels and equality of the count; every raw call is made with
O2V_HIP_FLAG_STAGE_TIMES so that the counters are compared too: peaks and survivors always, boundary pairs seen and distinct pairs
where the pair stage ran.  The shapes are the smallest at which the passes can go wrong - rows of more than one word, more than one
tile along every axis, sizes that are no multiple of a word or a tile -, not workload sizes; a reference is computed once per
(relief, connectivity) and gives the labels of every min_depth.  A case prints what it covered and "ok" last when everything held."""
import os
import re
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from obj2voxel_amd import watershed as WS
from tests import watershed_ref as WR
from tests.components_cases import indexed
from tests.raycast_cases import dev, expect_code

DEV = torch.device("cuda", 0)
GUARD = -7
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "obj2voxel_amd", "csrc")


def switch(name, value):
    """An environment switch for the calls that follow (the library reads its switches at every call); None: unset."""
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)


def raw(dv, t, connectivity, min_depth, out):
    """One o2v_hip_watershed_dense call on tensor views [z, y, x], with O2V_HIP_FLAG_STAGE_TIMES: (count, the six counters)."""
    nz, ny, nx = t.shape
    torch.cuda.synchronize()
    n = dv.watershed_dense(t.data_ptr(), dense._strides(t), (nx, ny, nz), connectivity, min_depth, hip.FLAG_STAGE_TIMES, out.data_ptr(), dense._strides(out))
    return n, dv.watershed_counters()


def check(dv, t, w, min_depth, out=None, what=""):
    """One call against the reference w (a WR.Watershed of the relief t holds): labels, count and counters."""
    if out is None:
        out = torch.full(w.H.shape, GUARD, dtype=torch.int32, device=DEV)
    n, counters = raw(dv, t, w.connectivity, min_depth, out)
    want, count = w.labels(min_depth)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), (what, w.connectivity, min_depth, int((got != want).sum()), "voxels differ")
    assert n == count == counters[5] and counters[0] == len(w.peaks), (what, w.connectivity, min_depth, n, count, counters)
    if min_depth > 0 and len(w.peaks) >= 2:
        assert counters[1:3] == (w.seen, len(w.a)) and counters[4] >= 12 * len(w.a), (what, counters, w.seen, len(w.a))
    else:
        assert counters[1:5] == (0, 0, 0, 0), (what, counters)
    return out, counters


# ---- formats_and_layouts ---------------------------------------------------------------------------------------------------------------

def relief_layouts(t):
    """(layout, view) of a contiguous int32 device tensor [z, y, x]: the same elements stored in other ways."""
    nz, ny, nx = t.shape
    wide = torch.full((nz, ny, 2 * nx), 2 ** 31 - 1, dtype=torch.int32, device=DEV)       # (what lies between must not be read as a voxel)
    wide[:, :, ::2] = t
    batch = torch.full((3, nz, ny, nx), 2 ** 31 - 1, dtype=torch.int32, device=DEV)
    batch[1] = t
    big = torch.full((nz + 3, ny + 5, nx + 7), 2 ** 31 - 1, dtype=torch.int32, device=DEV)
    big[2:2 + nz, 3:3 + ny, 5:5 + nx] = t
    out = [("every second element along x", wide[:, :, ::2]), ("x and z swapped in memory", t.permute(2, 1, 0).contiguous().permute(2, 1, 0)),
           ("y and z swapped in memory", t.permute(1, 0, 2).contiguous().permute(1, 0, 2)), ("slice of a batch", batch[1]),
           ("box inside a larger tensor", big[2:2 + nz, 3:3 + ny, 5:5 + nx])]
    assert all(torch.equal(v, t) for _, v in out)
    return out


def case_formats_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2026)
    shape = (21, 19, 70)
    reliefs = [("values 0 .. 5", rng.integers(0, 6, shape).astype(np.int32)), ("the whole int32 range", rng.integers(-2 ** 31, 2 ** 31, shape).astype(np.int32))]
    depths = (0, 1, 2, 2 ** 31 - 1)
    n = 0
    for name, H in reliefs:
        t = dev(H)
        for connectivity in (6, 18, 26):
            w = WR.Watershed(H, connectivity)
            for h in depths:
                check(dv, t, w, h, what=name)
                n += 1
            for layout, view in relief_layouts(t):
                check(dv, view, w, 2, what=(name, layout))
                n += 1
            # out= views: every second element along x, a slice of a batch, y and z swapped in memory
            wide = torch.full(shape[:2] + (2 * shape[2],), 9, dtype=torch.int32, device=DEV)
            check(dv, t, w, 1, out=wide[:, :, ::2], what=(name, "strided out"))
            assert bool((wide[:, :, 1::2] == 9).all())
            batch = torch.full((3,) + shape, 9, dtype=torch.int32, device=DEV)
            check(dv, t, w, 2, out=batch[1], what=(name, "out in a batch"))
            assert bool((batch[0] == 9).all()) and bool((batch[2] == 9).all())
            swapped = torch.full((shape[1], shape[0], shape[2]), 9, dtype=torch.int32, device=DEV).permute(1, 0, 2)
            check(dv, t, w, 0, out=swapped, what=(name, "swapped out"))
            n += 3
        print(f"{name}: {len(w.peaks)} peaks and {len(w.a)} adjacent pairs at 26 neighbours, {[w.labels(h)[1] for h in depths]} parts at min_depth {depths}")
    # the torch layer: a new contiguous tensor, out=, the peaks
    H = reliefs[0][1]
    w = WR.Watershed(H, 26)
    L, count = dense.watershed(dv, dev(H), min_depth=2)
    assert L.dtype == torch.int32 and L.is_contiguous() and np.array_equal(L.cpu().numpy(), w.labels(2)[0]) and count == w.labels(2)[1]
    assert dv.watershed_counters() == (0,) * 6 and len(dv.watershed_times()) == 5                  # (counted only on request)
    xyz, heights = dense.watershed_peaks(L, dev(H), count)
    ref = WR.part_peaks(w.labels(2)[0], H, count)
    assert np.array_equal(xyz.cpu().numpy(), ref[0]) and np.array_equal(heights.cpu().numpy(), ref[1])
    print(f"{n} calls compared with the reference, bit for bit")


# ---- known_shapes ----------------------------------------------------------------------------------------------------------------------

def case_known_shapes():
    """The pinned results of the definition, on the device."""
    dv = hip.DeviceVoxelizer(0)

    def parts(w, t, h):
        out, counters = check(dv, t, w, h, what="known shape")
        return np.bincount(out.cpu().numpy().ravel())[1:].tolist(), counters
    S = WR.dumbbell()
    H = WR.squared_edt(S)
    t = dev(H)
    depth2 = dense.inner_distance(dv, dev(S))
    assert int(S.sum()) == 7827 and np.array_equal(depth2.cpu().numpy(), H)                        # the relief is the toolkit's own depth map
    w = WR.Watershed(H, 26)
    for h in (0, 1, 49):
        sizes, counters = parts(w, depth2, h)
        assert sizes == [3833, 3994] and counters[0] == 2 and (h == 0 or counters[1:3] == (1413, 1))
    assert parts(w, t, 50)[0] == [7827]
    w = WR.Watershed(H, 6)
    assert len(parts(w, t, 0)[0]) == 6 and sorted(w.pers)[:5] == [0, 0, 0, 0, 49]
    for h in (1, 49):
        assert parts(w, t, h)[0] == [3832, 3995]
    U = WR.flat_u()
    w = WR.Watershed(U, 26)
    assert [len(parts(w, dev(U), h)[0]) for h in (0, 1)] == [2, 1]
    R = WR.random_relief()
    t = dev(R)
    w = WR.Watershed(R, 6)
    assert [len(parts(w, t, h)[0]) for h in (1, 2, 3, 6)] == [2554, 852, 111, 1]
    counters = parts(w, t, 1)[1]
    assert (counters[0], counters[2]) == (3183, 13042)
    assert parts(WR.Watershed(R, 18), t, 0)[1][0] == 897 and parts(WR.Watershed(R, 26), t, 0)[1][0] == 523
    B = np.full((3, 4, 5), 7, np.int32)
    L, n = dense.watershed(dv, dev(B))
    xyz, heights = dense.watershed_peaks(L, dev(B), n)
    assert n == 1 and bool((L == 1).all()) and xyz.tolist() == [[4, 3, 2]] and heights.tolist() == [7]       # a flat box: its last voxel
    for h in (0, 3):
        L, n = dense.watershed(dv, torch.zeros((3, 4, 5), dtype=torch.int32, device=DEV), min_depth=h)
        assert n == 0 and not bool(L.any())
        L, n = dense.watershed(dv, torch.full((1, 1, 1), 5, dtype=torch.int32, device=DEV), min_depth=h)
        assert n == 1 and L.tolist() == [[[1]]]
    print("dumbbell, flat U, random 70 x 19 x 17, flat box, empty relief and single voxel: the pinned results")


# ---- tile_borders ----------------------------------------------------------------------------------------------------------------------

def staircases():
    """A one-voxel staircase ramp y = z = min(x // 7, 19) with H = x + 1 in 140 x 21 x 21, and the same descending."""
    x = np.arange(140)
    for name, h in (("staircase up", x + 1), ("staircase down", 140 - x)):
        H = np.zeros((21, 21, 140), np.int32)
        H[np.minimum(x // 7, 19), np.minimum(x // 7, 19), x] = h
        yield name, H


def case_tile_borders():
    """What crosses tile borders, with the tile pass and with O2V_WS_NO_TILES=1, each twice: the same bits, the reference's."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(31)
    reliefs = [("random 130 x 19 x 17", rng.integers(0, 6, (17, 19, 130)).astype(np.int32))] + list(staircases())
    for name, H in reliefs:
        t = dev(H)
        for connectivity in (6, 26):
            w = WR.Watershed(H, connectivity)
            for h in (0, 2):
                outs = []
                for off in (None, 1):
                    switch("O2V_WS_NO_TILES", off)
                    a, ca = check(dv, t, w, h, what=(name, off))
                    b, cb = check(dv, t, w, h, what=(name, off, "again"))
                    assert torch.equal(a, b) and ca[:4] == cb[:4] and ca[5] == cb[5]
                    outs.append(a)
                switch("O2V_WS_NO_TILES", None)
                assert torch.equal(outs[0], outs[1])
            if "staircase" in name and connectivity == 26:
                L, n = w.labels(0)
                assert n == 1 and WR.part_peaks(L, H, 1)[0].tolist() == [[139, 19, 19] if "up" in name else [0, 0, 0]]
        print(f"{name}: {len(w.peaks)} peaks at 26 neighbours")
    print("with and without the tile pass: the same bits")


# ---- long_chains -----------------------------------------------------------------------------------------------------------------------

def case_long_chains():
    """Ramps H = position + 1 along x, y and z: one part whose peak is the far end, the flatten finishing - 2 050 voxels in a box
    of 3 x 2 across, and 65 536 voxels, the documented limit of an axis."""
    dv = hip.DeviceVoxelizer(0)
    for length, across in ((2050, (3, 2)), (65536, (1, 1))):
        for axis in (2, 1, 0):                                  # x, y, z of [z, y, x]
            shape = [0, 0, 0]
            shape[axis] = length
            shape[(axis + 1) % 3], shape[(axis + 2) % 3] = across
            pos = np.arange(length, dtype=np.int32).reshape([length if a == axis else 1 for a in range(3)])
            for name, H in (("up", np.broadcast_to(pos + 1, shape)), ("down", np.broadcast_to(length - pos, shape))):
                H = np.ascontiguousarray(H)
                w = WR.Watershed(H, 26)
                assert len(w.peaks) == 1
                for off in (None, 1):
                    switch("O2V_WS_NO_TILES", off)
                    for h in (0, 5):
                        out, counters = check(dv, dev(H), w, h, what=("ramp", length, "xyz"[2 - axis], name, off))
                switch("O2V_WS_NO_TILES", None)
                xyz, heights = dense.watershed_peaks(out, dev(H), 1)
                far = [s - 1 for s in shape[::-1]] if name == "up" else [(s - 1 if a != 2 - axis else 0) for a, s in enumerate(shape[::-1])]
                assert xyz.tolist() == [far] and heights.tolist() == [length], (xyz.tolist(), far)
        print(f"ramps of {length} voxels along x, y and z, up and down: one part, its peak at the far end")


# ---- many_peaks ------------------------------------------------------------------------------------------------------------------------

def case_many_peaks():
    """H = 2 where x, y and z are all even and 1 elsewhere, at 6 neighbours: every even voxel a part at min_depth 0, one part at 2.
    The box is sized from the source's constants: the peak words span more than one turn of the block scan (kBlock words a block,
    kBlock blocks a turn), and the peak count is no multiple of kBlock."""
    dv = hip.DeviceVoxelizer(0)
    block = int(re.search(r"constexpr uint32_t kBlock = (\d+);", open(os.path.join(SRC, "o2v_dev_common.hpp")).read()).group(1))
    side = 1
    while side * side <= block * block:
        side += 2
    nx, ny, nz = 5, side, side                                  # (odd sides: the last voxel is even, so no plateau of 1 ends in a peak of its own)
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx]
    H = np.where((x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0), 2, 1).astype(np.int32)
    even = 3 * ((side + 1) // 2) ** 2
    assert ny * nz > block * block and even % block and even > block * block // 2
    w = WR.Watershed(H, 6)
    t = dev(H)
    out, counters = check(dv, t, w, 0, what="many peaks")
    assert counters[0] == even and int(out.max()) == even
    assert np.array_equal(out.cpu().numpy()[H == 2], np.arange(1, even + 1))                        # every even voxel a part, numbered by its index
    out, counters = check(dv, t, w, 2, what="many peaks merged")
    assert counters[5] == 1 and bool((out == 1).all())
    out, counters = check(dv, t, w, 1, what="many peaks, min_depth 1")
    assert counters[5] == even
    print(f"{nx} x {ny} x {nz}: {even} peaks in {ny * nz} words ({block} words a block, {block} blocks a turn), {len(w.a)} adjacent pairs; min_depth 0, 1 and 2")


# ---- table_growth ----------------------------------------------------------------------------------------------------------------------

def case_table_growth():
    dv = hip.DeviceVoxelizer(0)
    R = WR.random_relief()
    w = WR.Watershed(R, 6)
    t = dev(R)
    free, c0 = check(dv, t, w, 2, what="table sized from the peaks")
    for log2 in (4, 9, 11):
        switch("O2V_WS_TABLE_LOG2", log2)
        small, c1 = check(dv, t, w, 2, what=("table forced", log2))
        switch("O2V_WS_TABLE_LOG2", None)
        assert torch.equal(free, small) and c1[:3] == c0[:3] == (3183, w.seen, 13042) and c0[3] == 0 and c1[3] >= 2 and c1[4] == 12 << (log2 + c1[3])
        print(f"table_growth: 2^{log2} slots at first, {c1[3]} growths to {c1[4]} bytes; unforced {c0[4]} bytes; 13042 distinct pairs from {c1[1]} boundary pairs")
    assert c0[4] == 12 << 16                                    # 16 slots a peak: 2^16 for 3 183 peaks


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------

def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, *indexed(meshes.scan_like()))
    solid, _ = dense.voxelize_dense(dv, 64, fill=True)
    S = solid.cpu().numpy().astype(bool)
    assert S.sum() > 1000
    relief = WS.scaled_root(dense.inner_distance(dv, solid), 4)
    R = relief.cpu().numpy()
    assert np.array_equal(R > 0, S)
    w = WR.Watershed(R, 26)
    finer = None
    for min_depth in (0.5, 2.0):
        t0 = time.time()
        L, n = dense.split_parts(dv, solid, min_depth=min_depth)
        ms = (time.time() - t0) * 1e3
        want, count = w.labels(int(np.ceil(min_depth * 4)))
        assert np.array_equal(L.cpu().numpy(), want) and n == count
        stats = dense.label_stats(dv, L, n)
        assert int(stats.count[1:].sum()) == int(S.sum()) and int(stats.count[1:].min()) >= 1 and stats.outside == 0
        if finer is not None:   # nesting: every finer part lies in one coarser part
            pairs = torch.unique(torch.stack([finer[finer > 0], L[finer > 0]], 1), dim=0)
            assert len(pairs) == len(torch.unique(pairs[:, 0]))
        finer = L
        print(f"pipeline: scan_like at 64, min_depth {min_depth}: {int(S.sum())} voxels, {len(w.peaks)} peaks -> {n} parts, {ms:.1f} ms")


# ---- call_sequence ---------------------------------------------------------------------------------------------------------------------

def case_call_sequence():
    """One context through boxes of different sizes and connectivities, with and without the pair stage: the scratch is grown on
    demand and reused, and every call gives what a fresh context gives."""
    rng = np.random.default_rng(61)
    reliefs = {"big": rng.integers(0, 6, (40, 37, 130)).astype(np.int32), "small": rng.integers(0, 6, (21, 19, 70)).astype(np.int32),
               "dumbbell": WR.squared_edt(WR.dumbbell()), "flat": np.full((9, 9, 70), 3, np.int32)}
    tensors = {k: dev(v) for k, v in reliefs.items()}
    refs = {}
    # (relief, connectivity, min_depth, no tiles)
    calls = [("big", 6, 2, None), ("small", 26, 0, None), ("big", 26, 1, 1), ("flat", 18, 3, None), ("dumbbell", 26, 49, None), ("small", 6, 2 ** 31 - 1, None),
             ("big", 6, 0, None)]

    def call(dv, name, connectivity, h, off):
        w = refs.setdefault((name, connectivity), WR.Watershed(reliefs[name], connectivity))
        switch("O2V_WS_NO_TILES", off)
        out, counters = check(dv, tensors[name], w, h, what=("call_sequence", name, connectivity, h))
        switch("O2V_WS_NO_TILES", None)
        return out, counters
    one = hip.DeviceVoxelizer(0)
    for i, c in enumerate(calls):
        a, ca = call(one, *c)
        fresh = hip.DeviceVoxelizer(0)
        b, cb = call(fresh, *c)
        fresh.close()
        assert torch.equal(a, b) and ca == cb, (i, c, ca, cb)
        print(f"call_sequence {i + 1}: {c[0]} {reliefs[c[0]].shape[::-1]}, {c[1]} neighbours, min_depth {c[2]}{', no tiles' if c[3] else ''}: counters {ca}")
    print("call_sequence: seven calls on one context, each equal to the reference and to a fresh context")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list, in its order, by code and words, made before any launch, the outputs untouched; the
    context stays usable.  (This child runs with torch's caching allocator off: each tensor is an allocation of its own, so a short
    one is short.)  One is not here: a failed allocation, for K12's reason (tests/components_cases.py)."""
    dv = hip.DeviceVoxelizer(0)
    N = 64
    R = np.random.default_rng(1).integers(0, 6, (N, N, N)).astype(np.int32)
    relief = dev(R)
    half = torch.full((N // 2, N, N), GUARD, dtype=torch.int32, device=DEV)
    labels = torch.full((N, N, N), GUARD, dtype=torch.int32, device=DEV)
    big = torch.full((2 * N, N, N), GUARD, dtype=torch.int32, device=DEV)
    host = np.zeros((N, N, N), np.int32)
    one = torch.zeros((1,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st, dims = (1, N, N * N), (N, N, N)

    def ws(ptr=relief.data_ptr(), strides=st, d=dims, connectivity=26, h=1, flags=0, op=labels.data_ptr(), os_=st):
        return lambda: dv.watershed_dense(ptr, strides, d, connectivity, h, flags, op, os_)

    def words_of(m, what, *parts):
        assert all(p in m for p in parts), (what, m)
        return m
    msgs = [
        words_of(expect_code(3, ws(op=None), "null labels"), "null labels", "null argument"),
        words_of(expect_code(3, ws(os_=None), "null labels strides"), "null labels strides", "null argument"),
        words_of(expect_code(3, ws(ptr=None), "null relief"), "null relief", "null argument"),
        words_of(expect_code(3, ws(strides=None), "null strides"), "null strides", "null argument"),
        words_of(expect_code(3, ws(d=(N, 0, N)), "zero dims"), "zero dims", "zero dims"),
        words_of(expect_code(3, ws(connectivity=8), "connectivity 8"), "connectivity", "connectivity must be 6, 18 or 26, not 8"),
        words_of(expect_code(3, ws(connectivity=0), "connectivity 0"), "connectivity", "not 0"),
        words_of(expect_code(3, ws(flags=256), "unknown flag bits"), "flags", "unknown flag bits in 256"),
        words_of(expect_code(3, ws(flags=hip.CC_INVERT), "a flag of components"), "flags", "unknown flag bits in 16"),
        words_of(expect_code(3, ws(ptr=relief.data_ptr() + 2), "relief off by two bytes"), "alignment", "4-byte aligned"),
        words_of(expect_code(5, ws(ptr=one.data_ptr(), d=(65537, 1, 1), strides=(0, 0, 0)), "an axis of 65 537"), "axis", "more than 65 536 voxels along an axis"),
        words_of(expect_code(5, ws(ptr=one.data_ptr(), d=(1024, 1024, 2048), strides=(0, 0, 0)), "2^31 voxels"), "voxels", "2147483648 voxels do not fit an int32 index"),
        words_of(expect_code(3, ws(ptr=host.ctypes.data), "host relief"), "host relief", "relief"),
        words_of(expect_code(3, ws(ptr=half.data_ptr()), "short relief"), "short relief", "relief", "extend past its allocation"),
        words_of(expect_code(3, ws(op=host.ctypes.data), "host labels"), "host labels", "labels"),
        words_of(expect_code(3, ws(op=half.data_ptr()), "short labels"), "short labels", "labels", "extend past its allocation"),
        words_of(expect_code(3, ws(os_=(1, N, 0)), "labels strides that map two voxels to one element"), "labels strides", "labels: strides map two voxels"),
        words_of(expect_code(3, ws(op=relief.data_ptr()), "labels in the relief"), "overlap", "labels and relief overlap"),
        words_of(expect_code(3, ws(op=relief.data_ptr(), os_=(N, 1, N * N)), "labels in the relief, other strides"), "overlap", "labels and relief overlap"),
        words_of(expect_code(3, ws(ptr=big.data_ptr(), op=big.data_ptr() + 4 * N), "labels a row into the relief"), "overlap", "labels and relief overlap"),
    ]
    assert all("o2v_hip_watershed_dense: " in m for m in msgs)
    torch.cuda.synchronize()
    assert bool((labels == GUARD).all()) and bool((big == GUARD).all()) and bool((half == GUARD).all()) and torch.equal(relief, dev(R))
    # the order: null arguments, the connectivity, the flags, the limits, the memory, shared elements, the overlap
    assert "null argument" in expect_code(3, ws(op=None, connectivity=8), "null before connectivity")
    assert "connectivity" in expect_code(3, ws(connectivity=8, flags=256), "connectivity before flags")
    assert "unknown flag bits" in expect_code(3, ws(flags=256, ptr=one.data_ptr(), d=(65537, 1, 1), strides=(0, 0, 0)), "flags before the limits")
    assert "along an axis" in expect_code(5, ws(ptr=one.data_ptr(), d=(65537, 1, 1), strides=(0, 0, 0), op=host.ctypes.data), "the limits before the memory")
    assert "labels: strides map" in expect_code(3, ws(op=relief.data_ptr(), os_=(1, N, 0)), "shared elements before the overlap")
    # a relief may share elements (it is only read); the context still works
    w = WR.Watershed(R, 26)
    n = dv.watershed_dense(relief.data_ptr(), st, dims, 26, 2, hip.FLAG_STAGE_TIMES, labels.data_ptr(), st)
    want, count = w.labels(2)
    assert np.array_equal(labels.cpu().numpy(), want) and n == count and dv.watershed_counters()[0] == len(w.peaks) and dv.watershed_counters()[5] == count
    plane = WR.Watershed(np.broadcast_to(R[:1], R.shape), 6)
    n = dv.watershed_dense(relief.data_ptr(), (1, N, 0), dims, 6, 1, 0, labels.data_ptr(), st)
    assert np.array_equal(labels.cpu().numpy(), plane.labels(1)[0]) and n == plane.labels(1)[1]
    assert dv.watershed_counters() == (0,) * 6                                                        # (counted only on request)
    assert len(dv.watershed_times()) == 5 and all(ms >= 0 for ms in dv.watershed_times()) and sum(dv.watershed_times()) > 0
    print("\n".join(msgs))
    print("ok refusals")


CASES = {"formats_and_layouts": case_formats_and_layouts, "known_shapes": case_known_shapes, "tile_borders": case_tile_borders,
         "long_chains": case_long_chains, "many_peaks": case_many_peaks, "table_growth": case_table_growth, "pipeline": case_pipeline,
         "call_sequence": case_call_sequence, "refusals": case_refusals}

if __name__ == "__main__":
    t0 = time.time()
    CASES[sys.argv[1]]()
    print(f"wall time {time.time() - t0:.1f} s")
    print("ok")
