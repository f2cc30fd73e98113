"""The GPU cases of tests/test_gpu_grow.py, each run in a child process of its own: `python -m tests.grow_cases <case>`.

torch is imported before the library is loaded (see tests/dense_cases.py).  Every comparison with the reference
(tests/grow_ref.py, its frontier form: tests/test_host_grow.py holds it equal to the shifted views) is np.array_equal on int32 labels, levels and ticks, `reached` included.  The shapes are the smallest at which
the tile scheme can go wrong, not workload sizes; a reference is computed once per set and shared.  A case prints what it covered
and "ok" last when everything held."""
import os
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip
from tests import components_ref as CR
from tests import grow_ref as WR
from tests.dense_cases import expect_code3
from tests.raycast_cases import dev, expect_code

DEV = torch.device("cuda", 0)
CHAMFER, HOPS6, HOPS26 = (3, 4, 5), (1, 0, 0), (1, 1, 1)
GUARD = -7


def no_tiles(on):
    """O2V_GROW_NO_TILES for the calls that follow (the library reads its switches at every call)."""
    if on:
        os.environ["O2V_GROW_NO_TILES"] = "1"
    else:
        os.environ.pop("O2V_GROW_NO_TILES", None)


def st(t):
    return dense._strides(t)


def call(dv, h, m, weights, labels, level=None, ticks=None, flags=0):
    """o2v_hip_grow_dense at the C level on tensor views [z, y, x]; returns `reached`."""
    torch.cuda.synchronize()
    nz, ny, nx = h.shape
    return dv.grow_dense(h.data_ptr(), st(h), m.data_ptr(), st(m), (nx, ny, nz), weights, flags, labels.data_ptr(), st(labels),
                         None if level is None else level.data_ptr(), None if level is None else st(level),
                         None if ticks is None else ticks.data_ptr(), None if ticks is None else st(ticks))


def check(dv, H, M, weights, want, what="", outs=(True, True), h=None, m=None, views=None):
    """One call on the grids H, M (numpy; h, m: the tensor views to pass instead of contiguous copies) against want = (labels,
    level, ticks, reached).  outs: level / ticks asked for.  views: three tensor views to write into instead of new tensors."""
    h = dev(H.astype(np.int32)) if h is None else h
    m = dev(M.astype(np.int32)) if m is None else m
    new = lambda: torch.full(H.shape, GUARD, dtype=torch.int32, device=DEV)   # noqa: E731
    lab, lev, tic = views if views is not None else (new(), new(), new())
    reached = call(dv, h, m, weights, lab, lev if outs[0] else None, tic if outs[1] else None)
    assert reached == want[3], (what, weights, "reached", reached, want[3])
    for name, got, ref, asked in (("labels", lab, want[0], True), ("level", lev, want[1], outs[0]), ("ticks", tic, want[2], outs[1])):
        g = got.cpu().numpy()
        if asked:
            assert np.array_equal(g, ref), (what, weights, name, int((g != ref).sum()), "voxels differ")
        elif views is None:
            assert (g == GUARD).all(), (what, name, "was written though not asked for")
    return lab, lev, tic


def counted(dv, H, M, weights):
    """(labels, level, ticks, reached, counters, times) of one call with O2V_HIP_FLAG_STAGE_TIMES."""
    h, m = dev(H.astype(np.int32)), dev(M.astype(np.int32))
    lab, lev, tic = (torch.empty(H.shape, dtype=torch.int32, device=DEV) for _ in range(3))
    reached = call(dv, h, m, weights, lab, lev, tic, hip.FLAG_STAGE_TIMES)
    return lab.cpu().numpy(), lev.cpu().numpy(), tic.cpu().numpy(), reached, dv.grow_counters(), dv.grow_times()


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------

def views_of(t, fill):
    """name -> a view of t's shape that holds t's elements in another layout; `fill` lies between and around them."""
    nz, ny, nx = t.shape
    out = {"contiguous": t}
    wide = torch.full((nz, ny, 2 * nx), fill, dtype=t.dtype, device=DEV)
    wide[:, :, ::2] = t
    out["every second element along x"] = wide[:, :, ::2]
    out["x and z swapped in memory"] = t.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    big = torch.full((nz + 2, ny + 3, nx + 5), fill, dtype=t.dtype, device=DEV)
    big[1:1 + nz, 2:2 + ny, 3:3 + nx] = t
    out["a box inside a larger tensor"] = big[1:1 + nz, 2:2 + ny, 3:3 + nx]
    return out


def case_layouts():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(2028)
    n = 0
    for dims in ((1, 1, 1), (1, 1, 9), (65, 1, 1), (64, 8, 8), (70, 20, 12), (130, 17, 9)):
        H, M = WR.random_case(rng, dims, 8, 6, 0.75)
        if dims == (1, 1, 1):
            H[...], M[...] = 4, 9
        refs = {w: WR.grow_frontier(H, M, w) for w in (CHAMFER, HOPS6, (7, 1, 1))}
        for weights, want in refs.items():
            for outs in ((True, True), (False, False), (True, False), (False, True)):
                check(dv, H, M, weights, want, (dims, outs), outs)
                n += 1
        want = refs[CHAMFER]
        h, m = dev(H), dev(M)
        # each of the five tensors in every layout, the others contiguous; a marker value between the elements must not be read
        for name, v in views_of(h, 9).items():
            check(dv, H, M, CHAMFER, want, (dims, "relief", name), h=v)
            n += 1
        for name, v in views_of(m, 3).items():
            check(dv, H, M, CHAMFER, want, (dims, "markers", name), m=v)
            n += 1
        for which in range(3):
            for name in ("every second element along x", "x and z swapped in memory", "a box inside a larger tensor"):
                outs = [torch.full(H.shape, GUARD, dtype=torch.int32, device=DEV) for _ in range(3)]
                base = torch.full(H.shape, GUARD, dtype=torch.int32, device=DEV)
                view = views_of(base, GUARD)[name]
                store = view._base if view._base is not None else view
                outs[which] = view
                check(dv, H, M, CHAMFER, want, (dims, "output", which, name), views=tuple(outs))
                # what lies between and around the box's elements stays
                assert int((store == GUARD).sum()) == store.numel() - H.size, (dims, which, name)
                n += 1
        # all three strided at once: Q, T and L all in scratch
        outs = tuple(views_of(torch.full(H.shape, GUARD, dtype=torch.int32, device=DEV), GUARD)["every second element along x"] for _ in range(3))
        check(dv, H, M, HOPS6, refs[HOPS6], (dims, "all outputs strided"), views=outs)
        n += 1
    print("compared", n, "calls; times", dv.grow_times())


# ---- tiles -----------------------------------------------------------------------------------------------------------------------------

SIX_WEIGHTS = (HOPS6, (1, 1, 0), HOPS26, CHAMFER, (0, 4, 0), (0, 0, 5))


def serpentine_case():
    S = CR.serpentine((128, 64, 16))
    M = np.zeros(S.shape, np.int32)
    M[0, 0, 0] = 1
    return S.astype(np.int32), M


def run_tiles(dv, modes=(False,)):
    """The sets of `tiles` that `no_tiles_ab` runs in both modes."""
    n = 0
    # two voxels that touch only across a tile's faces, edges and corner, flat and with a descent across the boundary, seeded on either side
    for kind, steps in (("x", 1), ("y", 1), ("z", 1), ("xy", 2), ("xz", 2), ("yz", 2), ("xyz", 3)):
        for descent in (False, True):
            H, M, a, b = WR.pair_across(kind, descent)
            back = np.zeros_like(M)
            back[b[2], b[1], b[0]] = 5
            for weights in SIX_WEIGHTS:
                want, want_back = WR.grow_frontier(H, M, weights), WR.grow_frontier(H, back, weights)
                w = weights[steps - 1]
                assert want[3] == (2 if w else 1) and want[0][b[2], b[1], b[0]] == (5 if w else 0)
                assert want[2][b[2], b[1], b[0]] == ((0 if descent else w) if w else -1) and want[1][b[2], b[1], b[0]] == (1 if w else 0)
                assert want_back[1][a[2], a[1], a[0]] == (1 if w else 0) and want_back[2][a[2], a[1], a[0]] == (w if w else -1)   # uphill: at the lower level
                for mode in modes:
                    no_tiles(mode)
                    check(dv, H, M, weights, want, ("pair", kind, descent, mode))
                    check(dv, H, back, weights, want_back, ("pair back", kind, descent, mode))
                n += 1
    # the serpentine: a round per tile along the way, in each of the three phases
    H, M = serpentine_case()
    for weights, name in ((HOPS6, "serpentine"), ((65535, 0, 0), "saturation serpentine")):
        want = WR.dijkstra(H, M, weights)
        t = want[2][H > 0]
        assert want[3] == H.sum() and (want[0][H > 0] == 1).all() and np.array_equal(np.sort(t), np.minimum(np.arange(H.sum()) * weights[0], WR.CAP))
        assert weights == HOPS6 or (t == WR.CAP).sum() > 100
        for mode in modes:
            no_tiles(mode)
            t0 = time.time()
            got = counted(dv, H, M, weights)
            assert got[3] == want[3] and all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])), (name, mode)
            c = got[4]
            assert all(c[3 * p] >= 1 for p in range(3)) and (mode or all(c[3 * p + 2] >= c[3 * p + 1] >= c[3 * p] for p in range(3)))
            print(f"{name}{' (no tiles)' if mode else ''}: {int(H.sum())} voxels, {time.time() - t0:.2f} s; (rounds, visits, sweeps) level {c[0:3]}, "
                  f"ticks {c[3:6]}, labels {c[6:9]}; ms " + " ".join(f"{v:.3f}" for v in got[5]), flush=True)
        n += 1
    # two hills across a tile boundary: the valley voxels on the boundary go to the smaller label
    H, M = WR.two_hills()
    for weights in (HOPS6, CHAMFER):
        want = WR.grow_frontier(H, M, weights)
        assert want[3] == H.size and set(np.unique(want[0])) == {1, 2} and (want[0][:, :, :64] == 2).all() and (want[0][:, :, 64:] == 1).all()
        for mode in modes:
            no_tiles(mode)
            check(dv, H, M, weights, want, ("two hills", mode))
        n += 1
    # empty, full, single-marker, every-voxel-a-marker and cone boxes at 150 x 90 x 70 against closed forms
    dims = (150, 90, 70)
    shape = dims[::-1]
    z, y, x = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    r, q, p = np.sort(np.stack([x, y, z]), axis=0)
    zero, minus = np.zeros(shape, np.int32), np.full(shape, -1, np.int32)
    corner = zero.copy()
    corner[0, 0, 0] = 7

    def both(*args):
        for mode in modes:
            no_tiles(mode)
            check(dv, *args[:-1], (args[-1], mode))
    every = (1 + x + 150 * (y + 90 * z)).astype(np.int32)
    for weights, closed in ((HOPS6, x + y + z), (HOPS26, p), (CHAMFER, 3 * p + q + r)):      # (tests/test_host_geodesic.py: the closed forms)
        flat = np.full(shape, 3, np.int32)
        both(flat, corner, weights, (np.full(shape, 7, np.int32), flat, closed.astype(np.int32), flat.size), "full, one marker")
        both(flat, zero, weights, (zero, zero, minus, 0), "full, no marker")
        both(zero, corner, weights, (zero, zero, minus, 0), "empty relief")
        both(flat - 4, every, weights, (zero, zero, minus, 0), "a relief below 0 everywhere")
        both(flat, every, weights, (every, flat, zero, flat.size), "every voxel a marker")
        # a cone: downhill from the marker on its top every voxel is a descent - level H, ticks 0
        cone = (1000 - closed).astype(np.int32)
        assert cone.min() > 0
        both(cone, corner, weights, (np.full(shape, 7, np.int32), cone, zero, flat.size), "a cone under its marker")
        n += 6
    no_tiles(False)
    return n


def case_tiles():
    dv = hip.DeviceVoxelizer(0)
    assert "O2V_GROW_NO_TILES" not in os.environ
    n = run_tiles(dv)
    print("compared", n, "sets; times", dv.grow_times())


# ---- no_tiles_ab -----------------------------------------------------------------------------------------------------------------------

def case_no_tiles_ab():
    """The sets of `tiles` and random reliefs with O2V_GROW_NO_TILES=1 (the child's environment has it) and without: both equal
    the reference, so each other."""
    assert os.environ.get("O2V_GROW_NO_TILES") == "1"
    dv = hip.DeviceVoxelizer(0)
    n = run_tiles(dv, (True, False))
    rng = np.random.default_rng(41)
    for density, weights in ((0.5, CHAMFER), (0.8, HOPS6)):
        H, M = WR.random_case(rng, (96, 90, 80), 8, 50, density)
        t0 = time.time()
        want = WR.grow_frontier(H, M, weights)
        ref = time.time() - t0
        lines = []
        for mode in (True, False):
            no_tiles(mode)
            got = counted(dv, H, M, weights)
            assert got[3] == want[3] and all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])), (density, weights, mode)
            lines.append(("tiles " if not mode else "no tiles ") + " ".join(f"{v:.3f}" for v in got[5]) + f" rounds {got[4][0::3]}")
        print(f"random {density} {weights}: {want[3]} reached, {len(np.unique(want[0])) - 1} labels, reference {ref:.1f} s; ms " + "; ".join(lines), flush=True)
        n += 1
    no_tiles(True)
    print("compared", n, "sets with and without the tile pass")


# ---- flat_is_geodesic ------------------------------------------------------------------------------------------------------------------

def case_flat_is_geodesic():
    """grow_labels' dist equals dense.geodesic_distance on the same set and seeds, on the device; labels is the nearest seed."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(7)
    S = CR.random_grid(rng, (96, 70, 40), 0.55)
    z, y, x = np.nonzero(S)
    pick = rng.integers(0, len(x), 9)
    seeds = np.stack([x[pick], y[pick], z[pick]], 1).astype(np.int32)
    sd = dev(seeds)
    n = 0
    for t, level, background in ((dev(S), None, False), (dev(S.astype(np.uint8) * 3), None, False), (dev(np.where(S, -1.0, 1.0).astype(np.float32)), 0.0, False),
                                 (dev(~S), None, True)):
        markers = dense.markers_from_seeds(sd, S.shape, device=DEV)
        assert int((markers > 0).sum()) == len(np.unique(seeds, axis=0))
        for connectivity in (6, 18, 26):
            for metric in ("steps", "chamfer"):
                for cap in (0, 6, None):
                    labels, dist = dense.grow_labels(dv, t, markers, level=level, background=background, max_distance=cap, metric=metric, connectivity=connectivity)
                    geo = dense.geodesic_distance(dv, t, sd, level=level, background=background, max_distance=cap, metric=metric, connectivity=connectivity)
                    assert torch.equal(dist, geo), (connectivity, metric, cap)
                    assert torch.equal(labels > 0, geo >= 0) and (cap != 0 or torch.equal(labels, torch.where(geo == 0, markers, 0)))
                    n += 1
        if level is None and not background and t.dtype == torch.bool:
            labels, dist = dense.grow_labels(dv, t, markers)
            want = WR.grow_frontier(S.astype(np.int32), markers.cpu().numpy(), CHAMFER)
            assert np.array_equal(labels.cpu().numpy(), want[0]) and np.array_equal(dist.cpu().numpy(), want[2])
    print("compared", n, "pairs of grow_labels and geodesic_distance")


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------

def case_pipeline():
    """Two balls of radius 14 whose centres are 22 apart: cores from erode + components, grown through the depth map by face steps.
    (With diagonal steps the same call equals the reference too, but the border is not the mid-plane: DESIGN.md section 32, "what
    the smallest label does on a descent".)"""
    dv = hip.DeviceVoxelizer(0)
    z, y, x = np.meshgrid(np.arange(40), np.arange(40), np.arange(64), indexing="ij")
    ball = lambda cx: (x - cx) ** 2 + (y - 20) ** 2 + (z - 20) ** 2 <= 14 * 14   # noqa: E731
    solid = dev(ball(21) | ball(43))
    cores, n = dense.components(dv, dense.erode(dv, solid, 9), connectivity=26)
    assert n == 2 and int(cores[20, 20, 21]) == 1 and int(cores[20, 20, 43]) == 2
    depth2 = dense.inner_distance(dv, solid)
    labels, level, ticks = dense.seeded_watershed(dv, depth2, cores, connectivity=6, level=True, distance=True)
    want = WR.grow_frontier(depth2.cpu().numpy(), cores.cpu().numpy(), (3, 0, 0))
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((labels, level, ticks), want[:3]))
    L = labels.cpu().numpy()
    assert set(np.unique(L)) == {0, 1, 2} and np.array_equal(L > 0, solid.cpu().numpy())      # two labels, every solid voxel labelled
    assert (L[:, :, :31][L[:, :, :31] > 0] == 1).all() and (L[:, :, 34:][L[:, :, 34:] > 0] == 2).all()   # the border within one voxel of the mid-plane x = 32
    adj = dense.label_adjacency(dv, labels, 2, values=depth2)
    assert adj.pairs.cpu().numpy().tolist() == [[1, 2]]
    only = dense.seeded_watershed(dv, depth2, cores, connectivity=6)
    assert torch.equal(only, labels)
    diagonal = dense.seeded_watershed(dv, depth2, cores)
    want26 = WR.grow_frontier(depth2.cpu().numpy(), cores.cpu().numpy(), CHAMFER)
    assert np.array_equal(diagonal.cpu().numpy(), want26[0])
    print(f"pipeline: two balls, {int((L == 1).sum())} + {int((L == 2).sum())} voxels, x = 32 holds labels {np.unique(L[:, :, 32]).tolist()}; with diagonal steps "
          f"{int((want26[0] == 1).sum())} + {int((want26[0] == 2).sum())}; times {dv.grow_times()}", flush=True)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def case_refusals():
    """Every refusal of the header's list, made before any launch, the outputs untouched; the context stays usable.  (This child
    runs with torch's caching allocator off: each tensor is an allocation of its own, so a short one is short.)  One is not here: a
    failed scratch allocation, for K12's reason (tests/components_cases.py)."""
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(1)
    N = 64
    Hn, Mn = WR.random_case(rng, (N, N, N), 8, 20)
    H, M = dev(Hn), dev(Mn)
    lab, lev, tic = (torch.full((N, N, N), 7, dtype=torch.int32, device=DEV) for _ in range(3))
    short = torch.full((N * N * N // 4,), 7, dtype=torch.int32, device=DEV)
    host = np.zeros((N, N, N), np.int32)
    one = torch.zeros((1,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    s, dims = (1, N, N * N), (N, N, N)

    def grow(hp=H.data_ptr(), hs=s, mp=M.data_ptr(), ms=s, d=dims, w=CHAMFER, flags=0, lp=lab.data_ptr(), ls=s, qp=lev.data_ptr(), qs=s, tp=tic.data_ptr(), ts=s):
        return lambda: dv.grow_dense(hp, hs, mp, ms, d, w, flags, lp, ls, qp, qs, tp, ts)
    L = hip._bind()
    C = hip.C
    n_reached = C.c_uint64(99)
    w3, d3, s3 = (C.c_uint32 * 3)(*CHAMFER), (C.c_uint32 * 3)(*dims), (C.c_uint64 * 3)(*s)
    raw = [dv._ctx, H.data_ptr(), s3, M.data_ptr(), s3, d3, w3, 0, lab.data_ptr(), s3, lev.data_ptr(), s3, tic.data_ptr(), s3, C.byref(n_reached)]
    # the null arguments that the Python binding cannot pass: reached, weights, dims, and the strides of a grid that is given
    for at, what in ((14, "reached"), (6, "weights"), (5, "dims"), (2, "relief strides"), (4, "marker strides"), (9, "labels strides"), (11, "level strides"),
                     (13, "ticks strides")):
        args = list(raw)
        args[at] = None
        assert L.o2v_hip_grow_dense(*args) == 3 and n_reached.value == 99, "null " + what
        assert b"null argument" in L.o2v_hip_last_error(dv._ctx), what
    msgs = [
        expect_code3(grow(hp=None), "null relief"), expect_code3(grow(mp=None), "null markers"), expect_code3(grow(lp=None), "null labels"),
        expect_code3(grow(d=(N, 0, N)), "zero dims"), expect_code3(grow(flags=64), "unknown flag bits"), expect_code3(grow(flags=1), "a flag of o2v_hip_voxelize"),
        expect_code3(grow(w=(0, 0, 0)), "weights all 0"), expect_code3(grow(w=(65536, 0, 0)), "a weight of 65 536"), expect_code3(grow(w=(1, 1, 1 << 20)), "a weight of 2^20"),
        expect_code(5, grow(d=(N, N, 65537), hs=(1, N, 0), ms=(1, N, 0)), "a dim above 65 536"),
        expect_code(5, grow(hp=one.data_ptr(), mp=one.data_ptr(), d=(1024, 1024, 2048), hs=(0, 0, 0), ms=(0, 0, 0)), "2^31 voxels"),
        expect_code3(grow(hp=H.data_ptr() + 2), "relief off its alignment"), expect_code3(grow(mp=M.data_ptr() + 1), "markers off their alignment"),
        expect_code3(grow(lp=lab.data_ptr() + 2), "labels off their alignment"), expect_code3(grow(qp=lev.data_ptr() + 2), "level off its alignment"),
        expect_code3(grow(tp=tic.data_ptr() + 2), "ticks off their alignment"),
        expect_code3(grow(hp=host.ctypes.data), "host relief"), expect_code3(grow(mp=host.ctypes.data), "host markers"), expect_code3(grow(lp=host.ctypes.data), "host labels"),
        expect_code3(grow(qp=host.ctypes.data), "host level"), expect_code3(grow(tp=host.ctypes.data), "host ticks"),
        expect_code3(grow(hp=short.data_ptr()), "short relief"), expect_code3(grow(mp=short.data_ptr()), "short markers"), expect_code3(grow(lp=short.data_ptr()), "short labels"),
        expect_code3(grow(qp=short.data_ptr()), "short level"), expect_code3(grow(tp=short.data_ptr()), "short ticks"),
        expect_code3(grow(ls=(1, N, 0)), "labels strides that map two voxels to one element"), expect_code3(grow(qs=(1, 1, N * N)), "level strides (x, y)"),
        expect_code3(grow(ts=(0, N, N * N)), "ticks strides of 0 along x"),
        expect_code3(grow(lp=H.data_ptr()), "labels in the relief"), expect_code3(grow(lp=M.data_ptr()), "labels in the markers"),
        expect_code3(grow(qp=H.data_ptr()), "level in the relief"), expect_code3(grow(tp=M.data_ptr()), "ticks in the markers"),
        expect_code3(grow(qp=lab.data_ptr()), "level in labels"), expect_code3(grow(tp=lab.data_ptr()), "ticks in labels"), expect_code3(grow(tp=lev.data_ptr()), "ticks in level"),
        expect_code3(grow(qp=lab.data_ptr() + 8, d=(4, 1, 1), qs=(1, 4, 4)), "level two elements into a labels of four"),
    ]
    assert any("2147483648 voxels" in m for m in msgs) and any("overlap" in m for m in msgs)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (lab, lev, tic, short)) and bool((H == dev(Hn)).all()) and bool((M == dev(Mn)).all())
    # relief and markers may share memory (both are only read); level and ticks may be left out
    want = WR.grow_frontier(Hn, Hn, HOPS6)
    assert grow(mp=H.data_ptr(), w=HOPS6, qp=None, qs=None, tp=None, ts=None)() == want[3] and np.array_equal(lab.cpu().numpy(), want[0])
    assert bool((lev == 7).all()) and bool((tic == 7).all())
    # the context still works
    want = WR.grow_frontier(Hn, Mn, CHAMFER)
    assert grow()() == want[3] and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((lab, lev, tic), want[:3]))
    assert len(dv.grow_times()) == 7 and all(ms > 0 for ms in dv.grow_times()) and dv.grow_counters() == (0,) * 9
    print("\n".join(msgs))
    print("ok refusals")


CASES = {"layouts": case_layouts, "tiles": case_tiles, "no_tiles_ab": case_no_tiles_ab, "flat_is_geodesic": case_flat_is_geodesic, "pipeline": case_pipeline,
         "refusals": case_refusals}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("ok")
