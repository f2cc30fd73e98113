"""The GPU cases of tests/test_gpu_geodesic.py, each run in a child process of its own: `python -m tests.geodesic_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison with the reference
(tests/geodesic_ref.py) is np.array_equal on int32 distances, paths and lengths, `reached` included.  The shapes are the smallest
at which the tile scheme can go wrong, not workload sizes; a reference is computed once per set and shared.  A case prints what it
covered and "ok" last when everything held."""
import os
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import components_ref as CR
from tests import geodesic_ref as GR
from tests.components_cases import SHAPES, indexed, set_of
from tests.dense_cases import expect_code3
from tests.raycast_cases import dev, expect_code, formats, layouts

DEV = torch.device("cuda", 0)
CHAMFER, HOPS6, HOPS26 = (3, 4, 5), (1, 0, 0), (1, 1, 1)


class Voxelizer(hip.DeviceVoxelizer):
    """Keeps what the last geodesic_dense call returned: dense.geodesic_distance does not hand `reached` on."""
    reached = None

    def geodesic_dense(self, *args):
        self.reached = super().geodesic_dense(*args)
        return self.reached


def no_tiles(on):
    """O2V_GEO_NO_TILES for the calls that follow (the library reads its switches at every call)."""
    if on:
        os.environ["O2V_GEO_NO_TILES"] = "1"
    else:
        os.environ.pop("O2V_GEO_NO_TILES", None)


def seeds_in(rng, S, n):
    """n seeds drawn from the set S, as (x, y, z)."""
    z, y, x = np.nonzero(S)
    pick = rng.integers(0, len(x), n) if len(x) else []
    return np.array([(x[i], y[i], z[i]) for i in pick], np.int64).reshape(-1, 3)


def check(dv, t, want, weights, seeds=None, border=False, background=False, cap=None, level=None, out=None, what=""):
    """dense.geodesic_distance of the tensor t against want = (dist, reached, ...) of the reference."""
    sd = None if seeds is None else dev(np.asarray(seeds, np.int32).reshape(-1, 3))
    got = dense.geodesic_distance(dv, t, sd, border=border, weights=weights, background=background, max_distance=cap, level=level, out=out)
    assert got.dtype == torch.int32 and tuple(got.shape) == want[0].shape and (out is None or got is out)
    g = got.cpu().numpy()
    assert np.array_equal(g, want[0]), (what, weights, border, background, cap, int((g != want[0]).sum()), "distances differ")
    assert dv.reached == want[1], (what, weights, dv.reached, want[1])
    return got


# ---- formats_and_layouts ---------------------------------------------------------------------------------------------------------------

def case_formats_and_layouts():
    dv = Voxelizer(0)
    rng = np.random.default_rng(2026)
    n = 0
    for dims in SHAPES:
        solid = CR.random_grid(rng, dims, 0.3)
        big = dims == (130, 70, 67)
        combos = [(CHAMFER, False), (HOPS6, True)] if big else [(w, b) for w in (HOPS6, HOPS26, CHAMFER) for b in (False, True)]
        refs = {}                                              # (the set's bytes, weights, background): one reference each

        def ref(S, weights, background):
            T = ~S if background else S
            key = (T.shape, T.tobytes(), weights)
            if key not in refs:
                sd = seeds_in(np.random.default_rng(len(refs)), T, 3)
                refs[key] = (sd,) + GR.distance(T, weights, sd, big)
            return refs[key]
        for fmt, t, level in formats(solid, rng):
            S = set_of(fmt, t, level)                          # (bits: 32 voxels per word, the padding is empty)
            assert fmt == "bits" or np.array_equal(S, solid)
            for weights, background in (combos[:2] if fmt == "bits" else combos):
                sd, *want = ref(S, weights, background)
                check(dv, t, want, weights, sd, big, background, level=level, what=(dims, fmt))
                n += 1
            if dims in ((65, 9, 9), (130, 70, 67), (70, 50, 40)):
                weights, background = combos[0]
                sd, *want = ref(S, weights, background)
                for layout, v in layouts(fmt, t):
                    check(dv, v, want, weights, sd, big, background, level=level, what=(dims, fmt, layout))
                    n += 1
        # out= with strides: a slice of a batch, every second element along x, axes swapped in memory; what lies between stays
        nz, ny, nx = solid.shape
        t = dev(solid)
        sd, *want = ref(solid, CHAMFER, False)
        batch = torch.full((3, nz, ny, nx), -7, dtype=torch.int32, device=DEV)
        check(dv, t, want, CHAMFER, sd, big, out=batch[1], what=(dims, "out in a batch"))
        assert bool((batch[0] == -7).all()) and bool((batch[2] == -7).all())
        wide = torch.full((nz, ny, 2 * nx), -7, dtype=torch.int32, device=DEV)
        check(dv, t, want, CHAMFER, sd, big, out=wide[:, :, ::2], what=(dims, "out with an x stride of 2"))
        assert bool((wide[:, :, 1::2] == -7).all())
        swapped = torch.empty((nx, ny, nz), dtype=torch.int32, device=DEV).permute(2, 1, 0)
        check(dv, t, want, CHAMFER, sd, big, out=swapped, what=(dims, "out with x and z swapped in memory"))
        n += 3
    print("compared", n, "calls; times", dv.geodesic_times())


# ---- tiles -----------------------------------------------------------------------------------------------------------------------------

def counted(dv, S, weights, seeds, flags=0):
    """(dist, reached, counters) of one o2v_hip_geodesic_dense call with O2V_HIP_FLAG_STAGE_TIMES."""
    t = dev(S.astype(np.uint8))
    out = torch.empty(S.shape, dtype=torch.int32, device=DEV)
    sd = dev(np.asarray(seeds, np.int32).reshape(-1, 3))
    torch.cuda.synchronize()
    reached = dv.geodesic_dense(t.data_ptr(), hip.GRID_U8, dense._strides(t), S.shape[::-1], 0.0, weights, flags | hip.FLAG_STAGE_TIMES,
                                sd.data_ptr() if len(sd) else None, len(sd), hip.GEO_MAX_DISTANCE, out.data_ptr(), dense._strides(out))
    return out.cpu().numpy(), reached, dv.geodesic_counters()


def run_tiles(dv, modes=(False,)):
    """The sets of `tiles` that `no_tiles_ab` runs in both modes."""
    n = 0
    # a corridor that leaves the first tile and comes back into it further on
    S, seed, end = GR.u_corridor()
    want = GR.dijkstra(S, HOPS6, [seed])
    assert want[0][end[2], end[1], end[0]] == S.sum() - 1
    for mode in modes:
        no_tiles(mode)
        check(dv, dev(S), want, HOPS6, [seed], what=("u corridor", mode))
        got, reached, (rounds, visits, sweeps, reads) = counted(dv, S, HOPS6, [seed])
        assert np.array_equal(got, want[0]) and reached == want[1]
        tiles = len({(x // 64, y // 8, z // 8) for z, y, x in zip(*np.nonzero(S))})
        if mode:
            assert (visits, sweeps) == (0, 0) and reads == rounds > 100
        else:
            # the way goes through its tiles one after the other and ends in the first: more rounds than it has tiles, and
            # more visits than tiles - the first tile, converged in round 0, is among them again
            assert rounds > tiles and visits > tiles and sweeps >= visits and reads == rounds + 1, (tiles, rounds, visits, sweeps, reads)
        print(f"u corridor{' (no tiles)' if mode else ''}: {int(S.sum())} voxels in {tiles} tiles; rounds {rounds}, tile visits {visits}, sweeps {sweeps}, "
              f"host reads {reads}", flush=True)
        n += 1
    # two voxels that touch only across a tile's faces, edges and corner: reached exactly when that kind of step has a weight
    for kind, steps in (("x", 1), ("y", 1), ("z", 1), ("xy", 2), ("xz", 2), ("yz", 2), ("xyz", 3)):
        for at in ((64, 8, 8), (128, 16, 8)):
            S, a, b = GR.pair_across(kind, at)
            t = dev(S)
            for weights in (HOPS6, (1, 1, 0), HOPS26, CHAMFER, (0, 4, 0), (0, 0, 5)):
                want = GR.distance(S, weights, [a])
                assert want[1] == (2 if weights[steps - 1] else 1) and want[0][b[2], b[1], b[0]] == (weights[steps - 1] or -1)
                for mode in modes:
                    no_tiles(mode)
                    check(dv, t, want, weights, [a], what=("pair", kind, at, mode))
                    check(dv, t, GR.distance(S, weights, [b]), weights, [b], what=("pair back", kind, at, mode))
                n += 1
    # the serpentine: a round per tile along the way
    S = CR.serpentine((128, 64, 16))
    t = dev(S)
    for weights in (HOPS6, CHAMFER):
        want = GR.dijkstra(S, weights, [(0, 0, 0)])
        assert want[1] == S.sum() and (weights != HOPS6 or want[0].max() == S.sum() - 1)
        for mode in modes:
            no_tiles(mode)
            t0 = time.time()
            check(dv, t, want, weights, [(0, 0, 0)], what=("serpentine", mode))
            print(f"serpentine{' (no tiles)' if mode else ''} {weights}: {int(S.sum())} voxels, d(last) {int(want[0].max())}, {time.time() - t0:.2f} s; ms "
                  + " ".join(f"{v:.3f}" for v in dv.geodesic_times()), flush=True)
        n += 1
    # the door box
    for door, reached in ((True, 15601), (False, 8000)):
        S = GR.door_box(door)
        want = GR.distance(S, CHAMFER, [(0, 0, 0)])
        assert want[1] == reached and (not door or (want[0][3, 4, 20], want[0][19, 19, 39], want[0][0, 0, 21]) == (67, 155, 83))
        for mode in modes:
            no_tiles(mode)
            check(dv, dev(S), want, CHAMFER, [(0, 0, 0)], what=("door", door, mode))
        n += 1
    no_tiles(False)
    return n


def case_tiles():
    dv = Voxelizer(0)
    assert "O2V_GEO_NO_TILES" not in os.environ
    n = run_tiles(dv)
    # empty, full and single-voxel sets
    dims = (150, 90, 70)
    empty, full = np.zeros(dims[::-1], bool), np.ones(dims[::-1], bool)
    single = empty.copy()
    single[33, 44, 77] = True
    none = (np.full(empty.shape, -1, np.int32), 0)
    z, y, x = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    r, q, p = np.sort(np.stack([x, y, z]), axis=0)
    for weights, closed in ((HOPS6, x + y + z), (HOPS26, p), (CHAMFER, 3 * p + q + r)):      # (tests/test_host_geodesic.py: the closed forms)
        check(dv, dev(full), (closed.astype(np.int32), full.size), weights, [(0, 0, 0)], what="full")
        check(dv, dev(full), none, weights, [(0, 0, 0)], background=True, what="full, background")
        check(dv, dev(empty), none, weights, [(5, 5, 5)], border=True, what="empty")
        one = none[0].copy()
        one[33, 44, 77] = 0
        check(dv, dev(single), (one, 1), weights, [(77, 44, 33), (78, 44, 33)], what="single voxel")
        check(dv, dev(single), none, weights, [(78, 44, 33)], border=True, what="single voxel, its seed beside it")
        n += 5
    # seeds: in S, not in S, negative, past the box, 2^31 - 1, int64, a sequence, none at all, border only, both
    rng = np.random.default_rng(17)
    dims = (65, 40, 33)
    S = CR.random_grid(rng, dims, 0.5)
    t = dev(S)
    inside = rng.integers(0, dims, (12, 3))
    in_set = S[inside[:, 2], inside[:, 1], inside[:, 0]]
    assert in_set.any() and not in_set.all()
    seeds = np.concatenate([inside, rng.integers(-3, 0, (5, 3)), inside[:5] + np.array(dims), [[dims[0], 0, 0], [0, -1, 0], [2 ** 31 - 1, 0, 0]]])
    for weights in (HOPS6, CHAMFER):
        for border, sd in ((True, None), (False, seeds), (True, seeds), (False, None), (False, seeds[-8:])):
            want = GR.distance(S, weights, () if sd is None else sd, border)
            check(dv, t, want, weights, sd, border, what=("seeds", border))
            n += 1
        assert GR.distance(S, weights)[1] == 0 and GR.distance(S, weights, seeds[-8:])[1] == 0        # none at all: everything -1
    want = GR.distance(S, CHAMFER, seeds)
    got = dense.geodesic_distance(dv, t, dev(seeds.astype(np.int64)))
    assert np.array_equal(got.cpu().numpy(), want[0]) and dv.reached == want[1]
    got = dense.geodesic_distance(dv, t, [tuple(int(v) for v in s) for s in seeds])
    assert np.array_equal(got.cpu().numpy(), want[0])
    print("compared", n + 3, "sets; times", dv.geodesic_times())


# ---- no_tiles_ab -----------------------------------------------------------------------------------------------------------------------

def case_no_tiles_ab():
    """The sets of `tiles`, two of formats_and_layouts and three random grids with O2V_GEO_NO_TILES=1 (the child's environment has
    it) and without: both equal the reference, so each other."""
    assert os.environ.get("O2V_GEO_NO_TILES") == "1"
    dv = Voxelizer(0)
    n = run_tiles(dv, (True, False))
    rng = np.random.default_rng(2026)
    for dims in ((65, 9, 9), (70, 50, 40)):
        solid = CR.random_grid(rng, dims, 0.3)
        for fmt, t, level in formats(solid, rng):
            S = set_of(fmt, t, level)
            sd = seeds_in(rng, S, 3)
            want, back = GR.distance(S, CHAMFER, sd), GR.distance(~S, HOPS6, (), True)
            for mode in (True, False):
                no_tiles(mode)
                check(dv, t, want, CHAMFER, sd, level=level, what=(dims, fmt, mode))
                check(dv, t, back, HOPS6, None, True, True, level=level, what=(dims, fmt, mode))
            n += 2
    rng = np.random.default_rng(31)
    for density, weights in ((0.4, CHAMFER), (0.6, HOPS6), (0.95, CHAMFER)):
        S = CR.random_grid(rng, (96, 90, 80), density)
        sd = seeds_in(rng, S, 8)
        t0 = time.time()
        want = GR.distance(S, weights, sd)
        ref = time.time() - t0
        ms = []
        for mode in (True, False):
            no_tiles(mode)
            check(dv, dev(S), want, weights, sd, what=("random", density, mode))
            ms.append(dv.geodesic_times())
        print(f"random {density} {weights}: {want[1]} reached, d max {int(want[0].max())}, reference {ref:.1f} s in {want[2]} rounds; ms " +
              "; ".join(("tiles " if i else "no tiles ") + " ".join(f"{v:.3f}" for v in m) for i, m in enumerate(ms)), flush=True)
        n += 1
    no_tiles(True)
    print("compared", n, "sets with and without the tile pass")


# ---- max_distance ----------------------------------------------------------------------------------------------------------------------

def case_max_distance():
    dv = Voxelizer(0)
    rng = np.random.default_rng(5)
    n = 0
    sets = [("door", GR.door_box(), CHAMFER, np.array([[0, 0, 0]]))]
    for dims, density, weights in (((96, 90, 80), 0.6, CHAMFER), ((65, 40, 33), 0.4, HOPS6), ((70, 50, 40), 0.35, HOPS26)):
        S = CR.random_grid(rng, dims, density)
        sets.append((f"random {dims}", S, weights, seeds_in(rng, S, 4)))
    for name, S, weights, sd in sets:
        t = dev(S)
        uncapped = GR.distance(S, weights, sd)
        top = int(uncapped[0].max())
        for cap in (0, 1, 6, 100, top + 1, top, top - 1):
            # the reference computed with the cap (tests/geodesic_ref.py: it masks at the end; the host tests hold that against a
            # Dijkstra that stops at the cap, which is where a cap applied too early or too late would show)
            want = GR.cap(uncapped[0], cap)
            for mode in (False, True):
                no_tiles(mode)
                check(dv, t, want, weights, sd, cap=cap, what=(name, cap, mode))
            n += 1
        no_tiles(False)
        assert GR.cap(uncapped[0], 0)[1] == len(np.unique(sd, axis=0)) and GR.cap(uncapped[0], top + 1)[1] == uncapped[1] > GR.cap(uncapped[0], top - 1)[1]
    small = GR.dijkstra(sets[2][1], HOPS6, sets[2][3], False, 6)                # ... and once against that Dijkstra itself
    check(dv, dev(sets[2][1]), small, HOPS6, sets[2][3], cap=6, what="against the Dijkstra with the cap")
    t = dev(GR.door_box().astype(np.uint8))
    out = torch.full((20, 20, 40), 7, dtype=torch.int32, device=DEV)
    sd = dev(np.array([[0, 0, 0]], np.int32))
    torch.cuda.synchronize()
    msg = expect_code3(lambda: dv.geodesic_dense(t.data_ptr(), hip.GRID_U8, (1, 40, 800), (40, 20, 20), 0.0, CHAMFER, 0, sd.data_ptr(), 1, 2 ** 31 - 1,
                                                 out.data_ptr(), (1, 40, 800)), "a cap of 2^31 - 1")
    assert "max_distance" in msg and bool((out == 7).all())
    try:
        dense.geodesic_distance(dv, t, sd, max_distance=2 ** 31 - 1)
        raise AssertionError("a cap of 2^31 - 1 was accepted")
    except ValueError:
        pass
    print("compared", n, "caps; a cap of 2^31 - 1 is refused:", msg)


# ---- paths -----------------------------------------------------------------------------------------------------------------------------

def check_path_properties(dist, weights, seeds_at, targets, paths, lengths):
    for t, p, n in zip(targets, paths, lengths):
        if n < 0:
            continue
        p = p[:n].astype(np.int64)
        assert tuple(p[0]) == tuple(t) and seeds_at[p[-1][2], p[-1][1], p[-1][0]], "a path starts at its target and ends on a seed"
        if n > 1:
            steps = np.abs(np.diff(p, axis=0))
            kinds = steps.sum(axis=1)
            assert (steps.max(axis=1) == 1).all() and all(weights[k - 1] for k in kinds), "consecutive voxels are a step with a weight apart"
            assert sum(weights[k - 1] for k in kinds) == dist[t[2], t[1], t[0]], "the weights along the path sum to the distance"


def case_paths():
    dv = Voxelizer(0)
    rng = np.random.default_rng(9)
    random = CR.random_grid(rng, (70, 50, 40), 0.4)
    n = 0
    for name, S, weights, seeds in (("door", GR.door_box(), CHAMFER, np.array([[0, 0, 0]])), ("door, hops", GR.door_box(), HOPS26, np.array([[0, 0, 0], [39, 0, 0]])),
                                    ("serpentine", CR.serpentine((128, 64, 16)), HOPS6, np.array([[0, 0, 0]])),
                                    ("random", random, CHAMFER, seeds_in(rng, random, 3)), ("random, 18", random, (2, 3, 0), seeds_in(rng, random, 3))):
        nz, ny, nx = S.shape
        t = dev(S)
        want_d = (GR.dijkstra if name == "serpentine" else GR.distance)(S, weights, seeds)
        dist = check(dv, t, want_d, weights, seeds, what=name)
        last = np.unravel_index(np.argmax(want_d[0]), S.shape)
        few = name == "serpentine"                              # (its paths are thousands of voxels long: the scalar trace takes its time)
        targets = np.concatenate([rng.integers(0, (nx, ny, nz), (8 if few else 40, 3)), seeds_in(rng, want_d[0] >= 0, 4 if few else 20), [[last[2], last[1], last[0]]], seeds[:1],
                                  [[-1, 0, 0], [nx, 0, 0], [0, 0, nz], [2 ** 31 - 1, 1, 1]]])
        L = GR.default_max_len(want_d[0], weights, targets)
        want = GR.paths(want_d[0], weights, targets, L)
        paths, lengths = dense.shortest_paths(dv, dist, dev(targets), weights=weights)
        assert paths.dtype == lengths.dtype == torch.int32 and tuple(paths.shape) == (len(targets), L, 3)
        gp, gl = paths.cpu().numpy(), lengths.cpu().numpy()
        assert np.array_equal(gl, want[1]) and np.array_equal(gp, want[0]), (name, "the paths differ from the scalar trace")
        assert (gl[-4:] == -1).all() and (name != "random" or (gl == -1).sum() > 4)        # outside the box; not reached
        assert gl.max() <= L and gl[-5] == 1 and gl[-6] > 1
        check_path_properties(want_d[0], weights, GR.seed_mask(S, seeds), targets, gp, gl)
        # a max_len shorter than the paths: the true lengths, the rows' tails untouched (-1 from the fill)
        short = dense.shortest_paths(dv, dist, dev(targets), weights=weights, max_len=5)
        keep = np.arange(5)[None, :, None] < want[1][:, None, None]
        assert np.array_equal(short[1].cpu().numpy(), want[1]) and np.array_equal(short[0].cpu().numpy(), np.where(keep, want[0][:, :5], -1))
        # the call itself leaves the tail alone, whatever is there
        tg = dev(targets.clip(-1, 2 ** 31 - 1).astype(np.int32))
        raw = torch.full((len(targets), 5, 3), -7, dtype=torch.int32, device=DEV)
        ln = torch.full((len(targets),), -7, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        dv.geodesic_paths(dist.data_ptr(), dense._strides(dist), (nx, ny, nz), weights, tg.data_ptr(), len(targets), 5, raw.data_ptr(), ln.data_ptr())
        assert np.array_equal(raw.cpu().numpy(), np.where(keep, want[0][:, :5], -7)) and np.array_equal(ln.cpu().numpy(), want[1])
        # a strided dist
        wide = torch.full((nz, ny, 2 * nx), -1, dtype=torch.int32, device=DEV)
        wide[:, :, ::2] = dist
        again = dense.shortest_paths(dv, wide[:, :, ::2], dev(targets), weights=weights)
        assert torch.equal(again[0], paths) and torch.equal(again[1], lengths)
        print(f"{name}: {len(targets)} targets, the longest path {int(gl.max())} voxels, {int((gl == -1).sum())} not reached or outside", flush=True)
        n += 1
    # traced with the wrong weights: -2
    dist = dense.geodesic_distance(dv, dev(GR.door_box()), [(0, 0, 0)])
    targets = [(39, 19, 19), (0, 0, 0), (20, 0, 0), (30, 4, 3)]
    for wrong in (HOPS26, HOPS6, (3, 4, 0)):
        got = dense.shortest_paths(dv, dist, targets, weights=wrong, max_len=60)
        want = GR.paths(dist.cpu().numpy(), wrong, targets, 60)
        assert np.array_equal(got[1].cpu().numpy(), want[1]) and np.array_equal(got[0].cpu().numpy(), want[0]) and want[1][0] == -2 and want[1][1] == 1
    print("compared", n, "sets of paths")


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------

def case_pipeline():
    dv = Voxelizer(0)
    c = meshes.unit_cube().reshape(-1, 9)                  # the two cubes of the README, pushed into each other
    dense.set_mesh(dv, *indexed(np.concatenate([c * 16 + 4.03, c * 16 + 10.07])))
    surface, origin = dense.voxelize_dense(dv, 40, fmt="labels")
    solid = dense.solidify(dv, surface)
    s = solid.cpu().numpy()
    # drain depth: through the air from the border, it reaches exactly the exterior
    drain = dense.geodesic_distance(dv, surface, background=True, border=True, connectivity=6)
    ext = dense.exterior(dv, surface, connectivity=6)
    want = GR.distance(surface.cpu().numpy() == 0, (3, 0, 0), (), True)
    assert np.array_equal(drain.cpu().numpy(), want[0]) and dv.reached == want[1] and np.array_equal((drain >= 0).cpu().numpy(), ext.cpu().numpy())
    assert not (drain >= 0)[15, 15, 15] and int(s[15, 15, 15]) == 2
    # inside the solid, from one seed: exactly that voxel's component
    labels, count = dense.components(dv, solid, connectivity=26)
    inside = dense.geodesic_distance(dv, solid, [(15, 15, 15)])
    want = GR.distance(s != 0, CHAMFER, [(15, 15, 15)])
    assert np.array_equal(inside.cpu().numpy(), want[0]) and dv.reached == want[1]
    assert torch.equal(inside >= 0, labels == labels[15, 15, 15]) and int(labels[15, 15, 15]) > 0
    assert int(inside.max()) == int(want[0].max())
    far = np.unravel_index(np.argmax(want[0]), want[0].shape)                     # the way from the farthest voxel of the solid, and from the air
    air = np.argwhere(s == 0)[0]
    targets = [(int(far[2]), int(far[1]), int(far[0])), (int(air[2]), int(air[1]), int(air[0]))]
    paths, lengths = dense.shortest_paths(dv, inside, targets)
    wp = GR.paths(want[0], CHAMFER, targets, paths.shape[1])
    assert np.array_equal(paths.cpu().numpy(), wp[0]) and np.array_equal(lengths.cpu().numpy(), wp[1])
    assert int(lengths[0]) > 10 and int(lengths[1]) == -1 and paths[0, int(lengths[0]) - 1].tolist() == [15, 15, 15]
    print(f"pipeline: two cubes at 40: the air's drain depth reaches {int((drain >= 0).sum())} voxels, the exterior; from the overlap's centre "
          f"{dv.reached} voxels of the solid, dist.max() {int(inside.max())} = {int(inside.max()) / dense.CHAMFER_UNIT:.1f} voxels; "
          f"times {dv.geodesic_times()}", flush=True)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list for both calls, made before any launch, the outputs untouched; the context stays usable.
    (This child runs with torch's caching allocator off: each tensor is an allocation of its own, so a short one is short.)  One
    is not here: a failed scratch allocation, for K12's reason (tests/components_cases.py)."""
    dv = Voxelizer(0)
    rng = np.random.default_rng(1)
    N = 96
    S = CR.random_grid(rng, (N, N, N), 0.5)
    grid = dev(S.astype(np.uint8))
    half = torch.zeros((N // 2, N, N), dtype=torch.uint8, device=DEV)
    field = torch.ones((N, N, N), dtype=torch.float32, device=DEV)
    words = torch.zeros((N, N, N // 32), dtype=torch.int32, device=DEV)
    dist = torch.full((N, N, N), 7, dtype=torch.int32, device=DEV)
    short = torch.full((N * N * N // 4,), 7, dtype=torch.int32, device=DEV)
    seeds = dev(np.array([[1, 2, 3], [4, 5, 6]], np.int32))
    host = np.zeros((N, N, N), np.int32)
    one = torch.zeros((1,), dtype=torch.int32, device=DEV)
    paths = torch.full((2, 64, 3), 7, dtype=torch.int32, device=DEV)
    lengths = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st, dims = (1, N, N * N), (N, N, N)
    wst = (1, N // 32, N * N // 32)

    def geo(ptr=grid.data_ptr(), fmt=hip.GRID_U8, strides=st, d=dims, level=0.0, w=CHAMFER, flags=0, sp=seeds.data_ptr(), n=2, cap=hip.GEO_MAX_DISTANCE,
            op=dist.data_ptr(), os_=st):
        return lambda: dv.geodesic_dense(ptr, fmt, strides, d, level, w, flags, sp, n, cap, op, os_)

    def walk(dp=dist.data_ptr(), ds=st, d=dims, w=CHAMFER, tp=seeds.data_ptr(), n=2, max_len=64, pp=paths.data_ptr(), lp=lengths.data_ptr()):
        return lambda: dv.geodesic_paths(dp, ds, d, w, tp, n, max_len, pp, lp)
    msgs = [
        expect_code3(geo(ptr=None), "null grid"), expect_code3(geo(op=None), "null dist"), expect_code3(geo(d=(N, 0, N)), "zero dims"),
        expect_code3(geo(fmt=3), "unknown format"), expect_code3(geo(flags=64), "unknown flag bits"), expect_code3(geo(flags=1), "a flag of o2v_hip_voxelize"),
        expect_code3(geo(ptr=words.data_ptr(), fmt=hip.GRID_BITS, strides=(2,) + wst[1:]), "bits with an x stride of 2"),
        expect_code3(geo(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("nan")), "level nan"),
        expect_code3(geo(ptr=field.data_ptr(), fmt=hip.GRID_F32_BELOW, level=float("-inf")), "level -inf"),
        expect_code3(geo(w=(0, 0, 0)), "weights all 0"), expect_code3(geo(w=(65536, 0, 0)), "a weight of 65 536"), expect_code3(geo(w=(1, 1, 1 << 20)), "a weight of 2^20"),
        expect_code3(geo(cap=2 ** 31 - 1), "a cap of 2^31 - 1"), expect_code3(geo(cap=2 ** 32 - 1), "a cap of 2^32 - 1"),
        expect_code3(geo(ptr=host.ctypes.data), "host grid"), expect_code3(geo(ptr=half.data_ptr()), "short grid"),
        expect_code3(geo(ptr=grid.data_ptr(), fmt=hip.GRID_F32_BELOW), "short grid (f32)"),
        expect_code3(geo(ptr=words.data_ptr(), fmt=hip.GRID_BITS, strides=wst, d=(N, N, 8 * N)), "short bits"),
        expect_code(5, geo(d=(N, N, 65537), strides=(1, N, 0)), "a dim above 65 536"),
        expect_code(5, geo(ptr=one.data_ptr(), d=(1024, 1024, 2048), strides=(0, 0, 0), op=one.data_ptr()), "2^31 voxels"),
        expect_code(5, geo(n=1 << 31), "2^31 seeds"),
        expect_code3(geo(op=host.ctypes.data), "host dist"), expect_code3(geo(op=short.data_ptr()), "short dist"), expect_code3(geo(op=dist.data_ptr() + 2), "dist off its alignment"),
        expect_code3(geo(os_=(1, N, 0)), "dist strides that map two voxels to one element"), expect_code3(geo(os_=(1, 1, N * N)), "dist strides (x, y)"),
        expect_code3(geo(ptr=dist.data_ptr(), fmt=hip.GRID_F32_BELOW), "dist in the grid"),
        expect_code3(geo(sp=None), "null seeds"), expect_code3(geo(sp=host.ctypes.data), "host seeds"), expect_code3(geo(n=1 << 20), "short seeds"),
        expect_code3(geo(op=seeds.data_ptr(), d=(4, 1, 1), os_=(1, 4, 4)), "dist over the seeds"),
        # the walk
        expect_code3(walk(dp=None), "paths: null dist"), expect_code3(walk(tp=None), "paths: null targets"), expect_code3(walk(pp=None), "paths: null paths"),
        expect_code3(walk(lp=None), "paths: null lengths"), expect_code3(walk(d=(N, 0, N)), "paths: zero dims"),
        expect_code3(walk(w=(0, 0, 0)), "paths: weights all 0"), expect_code3(walk(w=(0, 65536, 0)), "paths: a weight of 65 536"),
        expect_code3(walk(dp=dist.data_ptr() + 2), "paths: dist off its alignment"),
        expect_code(5, walk(d=(N, N, 65537), ds=(1, N, 0)), "paths: a dim above 65 536"),
        expect_code(5, walk(dp=one.data_ptr(), d=(1024, 1024, 2048), ds=(0, 0, 0)), "paths: 2^31 voxels"), expect_code(5, walk(n=1 << 31), "paths: 2^31 targets"),
        expect_code3(walk(dp=host.ctypes.data), "paths: host dist"), expect_code3(walk(dp=short.data_ptr()), "paths: short dist"),
        expect_code3(walk(tp=host.ctypes.data), "paths: host targets"), expect_code3(walk(n=1 << 20), "paths: short targets, lengths and paths"),
        expect_code3(walk(max_len=1 << 20), "paths: short paths"), expect_code3(walk(n=1 << 30, max_len=1 << 31), "paths: rows past any allocation"),
        expect_code3(walk(pp=dist.data_ptr()), "paths: paths in dist"), expect_code3(walk(lp=dist.data_ptr()), "paths: lengths in dist"),
        expect_code3(walk(pp=seeds.data_ptr(), max_len=1), "paths: paths over the targets"), expect_code3(walk(lp=paths.data_ptr()), "paths: lengths in paths"),
    ]
    assert any("2147483648 voxels" in m for m in msgs)
    torch.cuda.synchronize()
    assert bool((dist == 7).all()) and bool((short == 7).all()) and bool((paths == 7).all()) and bool((lengths == 7).all())
    assert bool((grid == dev(S.astype(np.uint8))).all())
    # a level that is not finite is ignored where the format has none; no seeds or targets: the pointers are not read
    geo(level=float("nan"))()
    assert geo(sp=None, n=0, level=float("inf"))() == 0 and bool((dist == -1).all())
    walk(tp=None, n=0, pp=None, lp=None)()
    # the context still works: both calls, on the same context
    want = GR.distance(S, CHAMFER, [(1, 2, 3), (4, 5, 6)], True)
    assert geo(flags=hip.CC_SEED_BORDER)() == want[1] and np.array_equal(dist.cpu().numpy(), want[0])
    targets = dev(np.array([[N // 2, N // 2, N // 2], [N, 0, 0]], np.int32))
    walk(tp=targets.data_ptr())()
    wp = GR.paths(want[0], CHAMFER, [(N // 2, N // 2, N // 2), (N, 0, 0)], 64)
    got = paths.cpu().numpy()
    keep = np.arange(64)[None, :, None] < wp[1][:, None, None]
    assert np.array_equal(lengths.cpu().numpy(), wp[1]) and np.array_equal(got, np.where(keep, wp[0], 7))
    assert len(dv.geodesic_times()) == 4 and all(ms > 0 for ms in dv.geodesic_times()) and dv.geodesic_counters() == (0, 0, 0, 0)
    print("\n".join(msgs))
    print("ok refusals")


CASES = {"formats_and_layouts": case_formats_and_layouts, "tiles": case_tiles, "no_tiles_ab": case_no_tiles_ab, "max_distance": case_max_distance,
         "paths": case_paths, "pipeline": case_pipeline, "refusals": case_refusals}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
