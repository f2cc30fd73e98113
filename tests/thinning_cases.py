"""The GPU cases of tests/test_gpu_thinning.py, each run in a child process of its own: `python -m tests.thinning_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison with the reference
(tests/thinning_ref.py) is np.array_equal on the skeleton's bits or its degree grid, and every call is made with
O2V_HIP_FLAG_STAGE_TIMES so that the counters are compared too: iterations and removed voxels must be the reference's, the
launches nine per iteration.  The shapes are the smallest at which the passes can go wrong - rows of more than one word, more
than one tile along every axis, sizes that are no multiple of a word or a tile -, not workload sizes; a reference is computed
once per (set, mode, keep, cap) and shared.  A case prints what it covered and "ok" last when everything held."""
import os
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import thinning_ref as TR
from tests import thinning_sets as TS
from tests.components_cases import indexed, set_of
from tests.dense_cases import expect_code3
from tests.raycast_cases import dev, expect_code, formats, layouts

DEV = torch.device("cuda", 0)
MODES = {TR.ULTIMATE: "ultimate", TR.CURVE: "curve"}


def no_tiles(on):
    """O2V_THIN_NO_TILES for the calls that follow (the library reads its switches at every call)."""
    if on:
        os.environ["O2V_THIN_NO_TILES"] = "1"
    else:
        os.environ.pop("O2V_THIN_NO_TILES", None)


class Ref:
    """The reference's results of one set, each computed once: (skeleton, iterations, removed) per (mode, keep, cap)."""

    def __init__(self, S):
        self.S, self.memo = np.asarray(S, bool), {}

    def get(self, mode, keep=None, cap=0, key=None):
        k = (mode, key if keep is not None else None, cap)
        if k not in self.memo:
            self.memo[k] = TR.thin(self.S, mode, keep, cap)
        return self.memo[k]


def raw(dv, t, level, mode, flags, cap, keep, out, dst_format):
    """One o2v_hip_thin_dense call on tensors, with O2V_HIP_FLAG_STAGE_TIMES; the counters."""
    _, fmt, lvl, dims = dense._set_grid(dv, t, level, dense._limit_voxels)
    torch.cuda.synchronize()
    dv.thin_dense(t.data_ptr(), fmt, dense._strides(t), dims, 0.0 if lvl is None else lvl, flags | hip.FLAG_STAGE_TIMES, mode, cap,
                  None if keep is None else keep.data_ptr(), None if keep is None else dense._strides(keep), out.data_ptr(), dense._strides(out), dst_format)
    return dv.thin_counters()


def check(dv, t, ref, mode, level=None, invert=False, keep=None, keep_np=None, keep_key=None, cap=0, degree=False, out=None, what=""):
    """One call against the reference of the set (ref: a Ref of S, or of its complement with invert): the bits or the degree
    grid, and the counters."""
    if out is None:
        out = torch.full(ref.S.shape, 7, dtype=torch.uint8, device=DEV)
    counters = raw(dv, t, level, mode, hip.CC_INVERT if invert else 0, cap, keep, out, hip.THIN_DST_DEGREE if degree else hip.THIN_DST_MASK)
    K, iterations, removed = ref.get(mode, keep_np, cap, keep_key)
    got = out.cpu().numpy()
    want = TR.degree(K) if degree else K.astype(np.uint8)
    assert np.array_equal(got, want), (what, MODES[mode], invert, cap, degree, int((got != want).sum()), "voxels differ")
    assert (counters[0], counters[3]) == (iterations, removed) and counters[1] == 9 * iterations, (what, MODES[mode], counters, iterations, removed)
    return out, counters


# ---- formats_and_layouts ---------------------------------------------------------------------------------------------------------------

def case_formats_and_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2026)
    n = 0
    for density in (0.3, 0.6):
        solid = TR.random_grid(rng, (70, 19, 21), density)
        refs = {}
        for fmt, t, level in formats(solid, rng):
            S = set_of(fmt, t, level)                       # (bits: 32 voxels per word, the padding is empty - and set under INVERT)
            for invert in (False, True):
                ref = refs.setdefault((S.shape, invert), Ref(~S if invert else S))
                for mode in MODES:
                    for degree in (False, True):
                        check(dv, t, ref, mode, level, invert, degree=degree, what=(fmt, density))
                        n += 1
            ref = refs[S.shape, False]
            for layout, view in layouts(fmt, t):
                check(dv, view, ref, TR.CURVE, level, what=(fmt, layout))
                n += 1
            # out= views: every second element along x, a slice of a batch, y and z swapped in memory
            wide = torch.full(S.shape[:2] + (2 * S.shape[2],), 9, dtype=torch.uint8, device=DEV)
            check(dv, t, ref, TR.CURVE, level, degree=True, out=wide[:, :, ::2], what=(fmt, "strided out"))
            assert bool((wide[:, :, 1::2] == 9).all())
            batch = torch.full((3,) + S.shape, 9, dtype=torch.uint8, device=DEV)
            check(dv, t, ref, TR.ULTIMATE, level, out=batch[1], what=(fmt, "out in a batch"))
            assert bool((batch[0] == 9).all()) and bool((batch[2] == 9).all())
            swapped = torch.full((S.shape[1], S.shape[0], S.shape[2]), 9, dtype=torch.uint8, device=DEV).permute(1, 0, 2)
            check(dv, t, ref, TR.CURVE, level, out=swapped, what=(fmt, "swapped out"))
            n += 3
        # in place: dst is the grid itself, contiguous and as a view; through dense.skeletonize with out=grid as well
        S = solid
        ref = refs[S.shape, False]
        own = dev(S.astype(np.uint8) * 200)
        check(dv, own, ref, TR.CURVE, out=own, what="in place")
        wide = torch.full(S.shape[:2] + (2 * S.shape[2],), 9, dtype=torch.uint8, device=DEV)
        wide[:, :, ::2] = dev(S.astype(np.uint8))
        check(dv, wide[:, :, ::2], ref, TR.ULTIMATE, degree=True, out=wide[:, :, ::2], what="in place, strided")
        assert bool((wide[:, :, 1::2] == 9).all())
        grid = dev(S)
        assert dense.skeletonize(dv, grid, out=grid) is grid and np.array_equal(grid.cpu().numpy(), ref.get(TR.CURVE)[0])
        n += 3
    # the torch layer: dtypes, the background, the float grid with a level
    S = solid
    K = dense.skeletonize(dv, dev(S), mode="ultimate", background=True)
    assert K.dtype == torch.bool and K.is_contiguous() and np.array_equal(K.cpu().numpy(), TR.thin(~S, TR.ULTIMATE)[0])
    field = dev(np.where(S, -1.0, 1.0).astype(np.float32))
    D = dense.skeletonize(dv, field, level=0.0, fmt="degree")
    assert D.dtype == torch.uint8 and np.array_equal(D.cpu().numpy(), TR.degree(TR.thin(S, TR.CURVE)[0]))
    assert dv.thin_counters() == (0, 0, 0, 0) and len(dv.thin_times()) == 3                       # (counted only on request)
    print(f"{n} calls compared with the reference, bit for bit")


# ---- known_shapes ----------------------------------------------------------------------------------------------------------------------

def case_known_shapes():
    """The pinned results of the definition, on the device."""
    dv = hip.DeviceVoxelizer(0)

    def thin(S, mode, degree=False):
        out, counters = check(dv, dev(S.astype(np.uint8)), Ref(S), mode, degree=degree, what="known shape")
        return out.cpu().numpy(), counters[0]
    K, it = thin(TR.box(), TR.ULTIMATE)
    assert (int(K.sum()), it) == (1, 5)
    D, it = thin(TR.box(), TR.CURVE, True)
    assert int((D > 0).sum()) == 25 and int((D == 2).sum()) == 8
    K, it = thin(TR.ball(), TR.ULTIMATE)
    assert (int(K.sum()), it) == (1, 13)
    for mode in MODES:
        K, it = thin(TR.shell(), mode)
        assert (int(K.sum()), it) == (1142, 3)
        labels, n = dense.components(dv, dev(K), background=True, connectivity=6)
        assert n == 2                                                                   # the cavity stays closed
    D, it = thin(TR.torus(), TR.ULTIMATE, True)
    assert int((D > 0).sum()) == 56 and set(D[D > 0].tolist()) == {3}                   # a closed loop
    for S in (TR.line("x", 130), TR.line("x", 130, 1)):
        K, it = thin(S, TR.ULTIMATE)
        assert np.argwhere(K).tolist() == [[1, 1, 65]] and it == 34
    K, it = thin(TR.line("x", 130), TR.CURVE)
    assert np.array_equal(K != 0, TR.line("x", 130)) and it == 1
    for axis, at in (("y", [1, 10, 1]), ("z", [10, 1, 1])):
        K, it = thin(TR.line(axis, 20), TR.ULTIMATE)
        assert np.argwhere(K).tolist() == [at] and it == 6
    S = np.ones((5, 5, 21), bool)
    for mode in MODES:
        a, b = thin(S, mode), thin(np.pad(S, 2), mode)
        assert np.array_equal(a[0], b[0][2:-2, 2:-2, 2:-2]) and a[1] == b[1]            # outside the box is background
    print("box, ball, shell, torus, lines and the unpadded box: the pinned results")


# ---- tile_borders ----------------------------------------------------------------------------------------------------------------------

def case_tile_borders():
    """What crosses tile borders, with the tile pass and with O2V_THIN_NO_TILES=1, each twice: the same bits, the reference's."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(31)
    sets = [("line 130", TR.line("x", 130)), ("line 129", TR.line("x", 130, 1)), ("line y", TR.line("y", 20)), ("line z", TR.line("z", 20)),
            ("staircase", TR.staircase())] + [(f"random {d}", TR.random_grid(rng, (130, 19, 17), d)) for d in (0.3, 0.6)]
    for name, S in sets:
        ref, t = Ref(S), dev(S.astype(np.uint8))
        for mode in ((TR.ULTIMATE,) if "line" in name or name == "staircase" else tuple(MODES)):
            turns = {}
            for off in (False, True):
                no_tiles(off)
                a, counters = check(dv, t, ref, mode, what=(name, off))
                b, again = check(dv, t, ref, mode, what=(name, off, "again"))
                assert torch.equal(a, b) and counters[:2] == again[:2] and counters[3] == again[3]
                turns[off] = counters[2]
                if name == "staircase":
                    assert np.argwhere(a.cpu().numpy()).tolist() == [[9, 9, 65]] and counters[0] == 34
            no_tiles(False)
            K, it, removed = ref.get(mode)
            print(f"{name} ({MODES[mode]}): {int(S.sum())} -> {int(K.sum())} voxels in {it} iterations; tile turns {turns[False]}, without the tile rule {turns[True]}")
            assert turns[False] <= turns[True]
    print("with and without the tile pass: the same bits")


# ---- keep_and_caps ---------------------------------------------------------------------------------------------------------------------

def case_keep_and_caps():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(41)
    S = TR.random_grid(rng, (70, 19, 21), 0.7)
    S[4:17, 3:16, 5:60] = True
    ref, t = Ref(S), dev(S.astype(np.uint8))
    keep_np = rng.random(S.shape) < 0.02
    # keep as a strided view, and as a bool tensor through the torch layer
    wide = torch.zeros(S.shape[:2] + (2 * S.shape[2],), dtype=torch.uint8, device=DEV)
    wide[:, :, 1::2] = 1
    wide[:, :, ::2] = dev(keep_np.astype(np.uint8) * 3)
    for mode in MODES:
        out, _ = check(dv, t, ref, mode, keep=wide[:, :, ::2], keep_np=keep_np, keep_key="k", what="keep")
        assert bool(out[dev(keep_np & S)].all())
        K = dense.skeletonize(dv, dev(S), mode=MODES[mode], keep=dev(keep_np))
        assert np.array_equal(K.cpu().numpy(), ref.get(mode, keep_np, 0, "k")[0])
    assert not np.array_equal(ref.get(TR.ULTIMATE, keep_np, 0, "k")[0], ref.get(TR.ULTIMATE)[0])
    # max_iterations 1, 2, 3: each result holds the next, and the counters stop there
    last = S
    for cap in (1, 2, 3):
        out, counters = check(dv, t, ref, TR.ULTIMATE, cap=cap, what=("cap", cap))
        K = out.cpu().numpy() != 0
        assert counters[0] == cap and not (K & ~last).any() and K.sum() < last.sum()
        last = K
        assert np.array_equal(dense.skeletonize(dv, dev(S), mode="ultimate", max_iterations=cap).cpu().numpy(), K)
    check(dv, dev(TR.box().astype(np.uint8)), Ref(TR.box()), TR.ULTIMATE, cap=1, what="the box, one iteration")
    check(dv, dev(TR.box().astype(np.uint8)), Ref(TR.box()), TR.CURVE, cap=1, what="the box, one iteration")
    print("keep (strided, bool) and max_iterations 1, 2, 3")


# ---- degree ----------------------------------------------------------------------------------------------------------------------------

def case_degree():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(51)
    for S in (TR.random_grid(rng, (70, 19, 21), 0.5), TR.cross(), np.ones((3, 5, 70), bool)):
        for mode in MODES:
            check(dv, dev(S.astype(np.uint8)), Ref(S), mode, degree=True, what="degree")
    # the degree grid is a convolution of the result: also where nothing is removed (a full box, capped)
    full = np.ones((9, 9, 70), bool)
    check(dv, dev(full), Ref(full), TR.CURVE, cap=1, degree=True, what="degree of a nearly full box")
    deg = dense.skeletonize(dv, dev(TR.cross()), fmt="degree")
    ends, junctions = dense.skeleton_nodes(deg)
    want = TR.nodes(TR.degree(TR.thin(TR.cross(), TR.CURVE)[0]))
    assert ends.dtype == junctions.dtype == torch.int32 and ends.device == deg.device
    assert np.array_equal(ends.cpu().numpy(), want[0]) and np.array_equal(junctions.cpu().numpy(), want[1])
    assert len(want[0]) == 24 and [16, 16, 16] in want[1].tolist()                      # four spurs per bar end; the centre is a junction
    print(f"degree grids; the cross: {len(want[0])} end points, {len(want[1])} junction voxels")


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------

def case_pipeline():
    dv = hip.DeviceVoxelizer(0)
    dense.set_mesh(dv, *indexed(meshes.scan_like()))
    solid, _ = dense.voxelize_dense(dv, 64, fill=True)
    S = solid.cpu().numpy().astype(bool)
    assert S.sum() > 1000
    for background in (False, True):
        t0 = time.time()
        K = dense.skeletonize(dv, solid, background=background)
        ms = (time.time() - t0) * 1e3
        want = TR.thin(~S if background else S, TR.CURVE)
        assert K.dtype == torch.bool and np.array_equal(K.cpu().numpy(), want[0])
        # (objects are 26-connected: the thinned set - the solid, or the empty space - before and after)
        before26 = dense.components(dv, solid, connectivity=26, background=background)[1]
        after26 = dense.components(dv, K, connectivity=26)[1]
        assert after26 == before26 >= 1
        print(f"pipeline: scan_like at 64, {'background' if background else 'solid'}: {int((~S if background else S).sum())} -> {int(K.sum())} voxels in "
              f"{want[1]} iterations, {after26} components, {ms:.1f} ms")


# ---- sets of isolated objects (tests/thinning_sets.py: the lemma is tests/test_host_thinning.py's) ----------------------------------------

def cus():
    """The CU count the library reads for its choice of tiles per workgroup."""
    return torch.cuda.get_device_properties(0).multi_processor_count


class Isolated(Ref):
    """The reference of a set of isolated objects, object by object: the Ref that check() takes, key "k" for the objects' keep."""

    def __init__(self, dims, objects):
        super().__init__(TS.grid_of(dims, TS.set_of(objects)))
        self.dims, self.objects = dims, objects
        self.bare = [(o, A, None) for o, A, _ in objects]
        self.keep = TS.grid_of(dims, TS.keep_of(objects))

    def get(self, mode, keep=None, cap=0, key=None):
        assert cap == 0
        k = (mode, key if keep is not None else None, 0)
        if k not in self.memo:
            _, skeleton, iterations, removed = TS.isolated_objects(self.objects if keep is not None else self.bare, mode)
            self.memo[k] = (TS.grid_of(self.dims, skeleton), iterations, removed)
        return self.memo[k]


class FixedRef(Ref):
    """A Ref with one result that needs no computing."""

    def __init__(self, S, mode, K, iterations, removed):
        super().__init__(S)
        self.memo[mode, None, 0] = (np.asarray(K, bool), iterations, removed)


def chunk_grid(name, with_keep=False):
    """Grid (a), (b) or (c) of tile_chunks for this device: (dims, what, its Isolated reference)."""
    want, nx = {"a": (3, 3), "b": (3, 70), "c": (32, 3)}[name]
    dims = TS.dims_for_chunk(cus(), want, nx)
    objects, what = TS.tile_chunks_objects(dims, cus(), 7, with_keep=with_keep)
    assert what["chunk"] == want and what["tiles"] % want and what["list_tiles"] == what["list_tiles_hit"]
    return dims, what, Isolated(dims, objects)


def turns_within(counters, what, tiled=True):
    """The tile-turn counter: every tile has a candidate in iteration 1, and none runs more than 8 sub-steps an iteration."""
    assert what["tiles"] <= counters[2] <= 8 * counters[0] * what["tiles"] and (tiled or counters[2] == 8 * counters[0] * what["tiles"]), (counters, what)


# ---- tile_chunks -----------------------------------------------------------------------------------------------------------------------

def case_tile_chunks():
    """Several tiles per workgroup (the host's own choice for boxes of this many tiles), ragged lists, LDS rows reused from tile
    to tile: a lattice object in every tile and random objects across the tiles, against the objects' references."""
    dv = hip.DeviceVoxelizer(0)
    for name in ("a", "b", "c"):
        dims, what, ref = chunk_grid(name, with_keep=name == "a")
        t = dev(ref.S.astype(np.uint8))
        for mode in MODES:
            for off in ((False, True) if name != "c" else (False,)):
                no_tiles(off)
                _, counters = check(dv, t, ref, mode, what=(name, off))
                turns_within(counters, what, not off)
                print(f"tile_chunks ({name}) {dims[0]} x {dims[1]} x {dims[2]}, {cus()} CUs: {what['tiles']} tiles, chunk {what['chunk']}, {what['chunks']} chunks, "
                      f"{what['lattice']} + {what['random']} objects, {what['list_tiles']} tiles of whole lists under random objects; {MODES[mode]}"
                      f"{', no tiles' if off else ''}: {counters[0]} iterations, {counters[3]} removed, {counters[2]} tile turns")
            no_tiles(False)
        if name == "a":
            keep = dev(ref.keep.astype(np.uint8))
            out, counters = check(dv, t, ref, TR.ULTIMATE, keep=keep, keep_np=ref.keep, keep_key="k", what="(a) with keep")
            turns_within(counters, what)
            assert bool(out[keep != 0].all()) and not np.array_equal(ref.get(TR.ULTIMATE, ref.keep, 0, "k")[0], ref.get(TR.ULTIMATE)[0])
            print(f"tile_chunks (a) with keep on {int(ref.keep.sum())} lattice voxels: {counters[0]} iterations, {counters[3]} removed")
        del t
    print("tile_chunks: chunk 3 and 32, ragged, both modes")


# ---- grid_turns ------------------------------------------------------------------------------------------------------------------------

def case_grid_turns():
    """More than 2^20 chunks: the chunk loop's second turn, words and voxels near 2^31, in place on a uint8 grid."""
    dims = TS.GRID_TURNS_DIMS
    objects, required, what = TS.grid_turns_objects(dims, cus())
    assert (what["tiles"], what["chunk"], what["chunks"], what["grid"], what["second_turn"]) == (33558849, 32, 1048715, 1 << 20, 139)
    words = dims[1] * dims[2]
    assert hip.thin_scratch_bytes(dims) == 16 * words + 8 * what["tiles"] + 64
    dv = hip.DeviceVoxelizer(0)

    def paint(t, placed):
        z, y, x = TS.coords(placed)
        t.view(-1)[torch.from_numpy((z * dims[1] + y) * dims[0] + x).to(DEV)] = 1

    grid = torch.zeros((dims[2], dims[1], dims[0]), dtype=torch.uint8, device=DEV)
    want = torch.zeros_like(grid)
    for mode in MODES:
        _, skeleton, iterations, removed = TS.isolated_objects(objects, mode)
        grid.zero_(), want.zero_()
        paint(grid, TS.set_of(objects)), paint(want, skeleton)
        t0 = time.time()
        counters = raw(dv, grid, None, mode, 0, 0, None, grid, hip.THIN_DST_MASK)
        seconds = time.time() - t0
        assert torch.equal(grid, want), (MODES[mode], int((grid != want).sum()), "voxels differ")
        assert (counters[0], counters[3]) == (iterations, removed) and counters[1] == 9 * iterations, (MODES[mode], counters, iterations, removed)
        assert counters[2] <= 8 * iterations * what["tiles"]
        print(f"grid_turns 1 x {dims[1]} x {dims[2]} ({words} words, scratch {hip.thin_scratch_bytes(dims)} B): {what['tiles']} tiles, chunk {what['chunk']}, "
              f"{what['chunks']} chunks on {what['grid']} workgroups, {what['second_turn']} second-turn chunks with {what['required'] - 2} tiles under objects, "
              f"{len(objects)} objects; {MODES[mode]}: {counters[0]} iterations, {counters[3]} removed, {counters[2]} tile turns, call {seconds:.2f} s "
              f"(classify, iterate, write: {', '.join('%.1f' % ms for ms in dv.thin_times())} ms)")


# ---- long_runs -------------------------------------------------------------------------------------------------------------------------

def case_long_runs():
    """Hundreds of iterations: the stamps' two slots by the parity of the iteration, tiles that sleep until the front arrives."""
    dv = hip.DeviceVoxelizer(0)
    diagonal = np.zeros((74, 74, 74), bool)
    diagonal[np.arange(1, 73), np.arange(1, 73), np.arange(1, 73)] = True
    sets = [(f"line {axis}", TR.line(axis, 2051, 1)) for axis in "xyz"] + [("diagonal", diagonal)]
    for name, S in sets:
        if "line" in name:
            S = np.pad(S, [(0, n == 2051) for n in S.shape])                                         # voxels 1 ... 2050 of 2052
            assert int(S.sum()) == 2050 and sorted(S.shape) == [3, 3, 2052]
        ref, t = Ref(S), dev(S.astype(np.uint8))
        turns = {}
        for off in (False, True):
            no_tiles(off)
            a, counters = check(dv, t, ref, TR.ULTIMATE, what=(name, off))
            b, again = check(dv, t, ref, TR.ULTIMATE, what=(name, off, "again"))
            assert torch.equal(a, b) and counters[:2] == again[:2] and counters[3] == again[3]
            turns[off] = counters[2]
        no_tiles(False)
        K, it, removed = ref.get(TR.ULTIMATE)
        at = np.argwhere(K)[:, ::-1].tolist()
        print(f"long_runs {name} (ultimate): {int(S.sum())} -> {at} (x, y, z) in {it} iterations, {removed} removed; tile turns {turns[False]}, without the tile rule {turns[True]}")
        assert len(at) == 1 and removed == int(S.sum()) - 1
        if name == "line x":
            assert (at, it, removed) == ([[1025, 1, 1]], 514, 2049)
        if name == "diagonal":
            assert (at, it, removed) == ([[36, 36, 36]], 19, 71) and turns[False] * 4 < turns[True]
        else:
            assert it > 500 and turns[False] * 20 < turns[True]
            for off in (False, True):
                no_tiles(off)
                _, counters = check(dv, t, FixedRef(S, TR.CURVE, S, 1, 0), TR.CURVE, what=(name, "curve", off))
                assert counters[0] == 1
            no_tiles(False)
    print("long_runs: lines of 2050 voxels along x, y and z and the diagonal of 72")


# ---- long_axes -------------------------------------------------------------------------------------------------------------------------

def case_long_axes():
    """65 536 voxels along an axis - the documented limit -, segments at both ends of it and across its middle."""
    dv = hip.DeviceVoxelizer(0)
    n = TS.LONG_AXIS
    for axis in "xyz":
        S = TS.long_axis_set(axis)
        ref, t = Ref(S), dev(S.astype(np.uint8))
        K, it, removed = ref.get(TR.ULTIMATE)
        survivors = np.argwhere(K)[:, {"x": 2, "y": 1, "z": 0}[axis]].tolist()
        assert (survivors, it, removed) == ([20, 32767, 65472, 65516], 11, 134), (axis, survivors, it, removed)
        for off in (False, True):
            no_tiles(off)
            for mode in MODES:
                for degree in (False, True):
                    check(dv, t, ref, mode, degree=degree, what=(axis, off))
        no_tiles(False)
        print(f"long_axes {axis}: {int(S.sum())} voxels in four segments of a box of {n} along {axis}; ultimate leaves {survivors} in {it} iterations, {removed} removed; "
              f"curve {ref.get(TR.CURVE)[1:]}")
    one = torch.zeros((1,), dtype=torch.uint8, device=DEV)
    expect_code(5, lambda: dv.thin_dense(one.data_ptr(), hip.GRID_U8, (0, 0, 0), (n + 1, 1, 1), 0.0, 0, hip.THIN_CURVE, 0, None, None, one.data_ptr(), (0, 0, 0), hip.THIN_DST_MASK), "65 537")
    print("long_axes: 65 536 along x, y and z, both modes, both tile modes, mask and degree")


# ---- call_sequence ---------------------------------------------------------------------------------------------------------------------

def case_call_sequence():
    """One context through calls of different sizes, with and without keep and tiles: the scratch (set, border and keep bits, the
    stamps) is grown on demand and reused, and every call gives what a fresh context gives."""
    rng = np.random.default_rng(61)
    dims, what, big = chunk_grid("a", with_keep=True)
    small, mid, flat = TR.random_grid(rng, (70, 19, 21), 0.6), TR.random_grid(rng, (130, 19, 17), 0.6), np.ones((9, 9, 70), bool)
    small_keep = rng.random(small.shape) < 0.03
    refs = {"big": big, "small": Ref(small), "mid": Ref(mid), "flat": Ref(flat)}
    tensors = {k: dev(r.S.astype(np.uint8)) for k, r in refs.items()}
    keeps = {"big": (dev(big.keep.astype(np.uint8)), big.keep), "small": (dev(small_keep.astype(np.uint8)), small_keep)}
    # (set, mode, keep, no tiles, cap, degree)
    calls = [("big", TR.ULTIMATE, False, False, 0, False), ("small", TR.CURVE, True, False, 0, False), ("mid", TR.ULTIMATE, False, False, 0, False),
             ("mid", TR.ULTIMATE, False, True, 0, False), ("big", TR.ULTIMATE, True, False, 0, False), ("flat", TR.CURVE, False, False, 1, True)]

    def call(dv, name, mode, keep, off, cap, degree):
        no_tiles(off)
        kt, kn = keeps[name] if keep else (None, None)
        out, counters = check(dv, tensors[name], refs[name], mode, keep=kt, keep_np=kn, keep_key="k", cap=cap, degree=degree, what=("call_sequence", name, keep, off))
        no_tiles(False)
        return out, counters
    one = hip.DeviceVoxelizer(0)
    for i, c in enumerate(calls):
        a, ca = call(one, *c)
        fresh = hip.DeviceVoxelizer(0)
        b, cb = call(fresh, *c)
        fresh.close()
        assert torch.equal(a, b) and ca[:2] == cb[:2] and ca[3] == cb[3], (i, c, ca, cb)
        print(f"call_sequence {i + 1}: {c[0]} {tuple(refs[c[0]].S.shape[::-1])}, {MODES[c[1]]}{', keep' if c[2] else ''}{', no tiles' if c[3] else ''}"
              f"{', 1 iteration, degree' if c[4] else ''}: counters {ca}")
    print(f"call_sequence: six calls on one context, each equal to the reference and to a fresh context ({what['tiles']} tiles, chunk {what['chunk']} in 1 and 5)")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list, by code and words, made before any launch, the outputs untouched; the context stays
    usable.  (This child runs with torch's caching allocator off: each tensor is an allocation of its own, so a short one is
    short.)  One is not here: a failed scratch allocation, for K12's reason (tests/components_cases.py)."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(1)
    N = 64
    S = TR.random_grid(rng, (N, N, N), 0.5)
    grid = dev(S.astype(np.uint8))
    half = torch.zeros((N // 2, N, N), dtype=torch.uint8, device=DEV)
    field = torch.ones((N, N, N), dtype=torch.float32, device=DEV)
    words = torch.zeros((N, N, N // 32), dtype=torch.int32, device=DEV)
    dst = torch.full((N, N, N), 7, dtype=torch.uint8, device=DEV)
    keep = torch.zeros((N, N, N), dtype=torch.uint8, device=DEV)
    big = torch.full((2 * N, N, N), 7, dtype=torch.uint8, device=DEV)
    host = np.zeros((N, N, N), np.uint8)
    one = torch.zeros((1,), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    st, dims = (1, N, N * N), (N, N, N)
    wst = (1, N // 32, N * N // 32)

    def th(ptr=grid.data_ptr(), fmt=hip.GRID_U8, strides=st, d=dims, level=0.0, flags=0, mode=hip.THIN_CURVE, cap=0, kp=keep.data_ptr(), ks=st, op=dst.data_ptr(),
           os_=st, df=hip.THIN_DST_MASK):
        return lambda: dv.thin_dense(ptr, fmt, strides, d, level, flags, mode, cap, kp, ks, op, os_, df)

    def words_of(m, what, *parts):
        assert all(p in m for p in parts), (what, m)
        return m
    msgs = [
        words_of(expect_code3(th(ptr=None), "null grid"), "null grid", "null argument"), words_of(expect_code3(th(op=None), "null dst"), "null dst", "null argument"),
        words_of(expect_code3(th(os_=None), "null dst strides"), "null dst strides", "null argument"),
        words_of(expect_code3(th(ks=None), "keep without strides"), "keep strides", "null argument"),
        words_of(expect_code3(th(d=(N, 0, N)), "zero dims"), "zero dims", "zero dims"), words_of(expect_code3(th(fmt=3), "unknown format"), "format", "unknown format 3"),
        words_of(expect_code3(th(ptr=words.data_ptr(), fmt=hip.GRID_BITS, strides=(2,) + wst[1:]), "bits with an x stride of 2"), "bits", "strides[0] == 1"),
        words_of(expect_code3(th(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("nan")), "level nan"), "level", "level must be finite"),
        expect_code3(th(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("inf")), "level inf"),
        expect_code3(th(ptr=host.ctypes.data), "host grid"), expect_code3(th(ptr=half.data_ptr()), "short grid"),
        expect_code3(th(ptr=grid.data_ptr(), fmt=hip.GRID_F32_BELOW), "short grid (f32)"),
        words_of(expect_code3(th(mode=2), "unknown mode"), "mode", "unknown mode 2"), words_of(expect_code3(th(df=2), "unknown dst_format"), "dst_format", "unknown dst_format 2"),
        words_of(expect_code3(th(flags=256), "unknown flag bits"), "flags", "unknown flag bits in 256"), expect_code3(th(flags=hip.CC_SEED_BORDER), "a flag of flood"),
        words_of(expect_code(5, th(ptr=one.data_ptr(), d=(65537, 1, 1), strides=(0, 0, 0)), "an axis of 65 537"), "axis", "more than 65 536 voxels along an axis"),
        words_of(expect_code(5, th(ptr=one.data_ptr(), d=(1024, 1024, 2048), strides=(0, 0, 0)), "2^31 voxels"), "voxels", "2147483648 voxels do not fit an int32 index"),
        expect_code3(th(op=host.ctypes.data), "host dst"), expect_code3(th(op=half.data_ptr()), "short dst"),
        words_of(expect_code3(th(kp=host.ctypes.data), "host keep"), "host keep", "keep"), words_of(expect_code3(th(kp=half.data_ptr()), "short keep"), "short keep", "keep"),
        words_of(expect_code3(th(os_=(1, N, 0)), "dst strides that map two voxels to one element"), "dst strides", "dst: strides map two voxels"),
        words_of(expect_code3(th(op=grid.data_ptr(), os_=(N, 1, N * N)), "dst in the grid, other strides"), "overlap", "dst and grid overlap"),
        words_of(expect_code3(th(ptr=big.data_ptr(), op=big.data_ptr() + N), "dst a row into the grid"), "overlap", "dst and grid overlap"),
        words_of(expect_code3(th(ptr=dst.data_ptr(), fmt=hip.GRID_BITS, strides=wst), "dst in a bits grid"), "overlap", "dst and grid overlap"),
        words_of(expect_code3(th(op=keep.data_ptr()), "dst in keep"), "overlap", "dst and keep overlap"),
    ]
    assert all("o2v_hip_thin_dense: " in m for m in msgs)
    torch.cuda.synchronize()
    assert bool((dst == 7).all()) and bool((big == 7).all()) and bool((keep == 0).all()) and bool((half == 0).all())
    assert bool((grid == dev(S.astype(np.uint8))).all())
    # a level that is not finite is ignored where the format has none; keep strides without a keep are not read; grid and keep
    # may share memory (both are only read)
    th(level=float("nan"))()
    th(kp=None, ks=None)()
    th(kp=grid.data_ptr(), cap=1)()
    assert np.array_equal(dst.cpu().numpy(), S.astype(np.uint8))                                   # everything kept
    # the order: the set grid's checks before the mode, the mode before the flags, the flags before the sizes, the sizes before the outputs
    assert "unknown format" in expect_code3(th(fmt=3, mode=5, flags=256), "format before mode")
    assert "unknown mode" in expect_code3(th(mode=5, df=9, flags=256), "mode before dst_format")
    assert "unknown dst_format" in expect_code3(th(df=9, flags=256), "dst_format before flags")
    assert "along an axis" in expect_code(5, th(ptr=one.data_ptr(), d=(65537, 1, 1), strides=(0, 0, 0), op=host.ctypes.data), "the sizes before the outputs")
    # the context still works
    r = Ref(S)
    th(kp=None, ks=None, flags=hip.FLAG_STAGE_TIMES)()
    K, iterations, removed = r.get(TR.CURVE)
    assert np.array_equal(dst.cpu().numpy(), K.astype(np.uint8)) and dv.thin_counters()[0] == iterations and dv.thin_counters()[3] == removed
    th(kp=None, ks=None)()
    assert dv.thin_counters() == (0, 0, 0, 0)                                                      # (counted only on request)
    assert len(dv.thin_times()) == 3 and all(ms >= 0 for ms in dv.thin_times()) and sum(dv.thin_times()) > 0
    print("\n".join(msgs))
    print("ok refusals")


CASES = {"formats_and_layouts": case_formats_and_layouts, "known_shapes": case_known_shapes, "tile_borders": case_tile_borders,
         "keep_and_caps": case_keep_and_caps, "degree": case_degree, "pipeline": case_pipeline, "refusals": case_refusals, "tile_chunks": case_tile_chunks,
         "grid_turns": case_grid_turns, "long_runs": case_long_runs, "long_axes": case_long_axes, "call_sequence": case_call_sequence}

if __name__ == "__main__":
    t0 = time.time()
    CASES[sys.argv[1]]()
    print(f"wall time {time.time() - t0:.1f} s")
    print("ok")
