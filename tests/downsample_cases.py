"""The GPU cases of tests/test_gpu_downsample.py, each run in a child process of its own: `python -m tests.downsample_cases <case>`.

torch is imported before the library is loaded (the grids are torch tensors; see tests/dense_cases.py).  Every comparison is
np.array_equal against the numpy reference of tests/downsample_ref.py, never against the code under test.  A case prints what it
covered and "ok" last when everything held."""
import sys
import time

import torch  # first

import numpy as np

from obj2voxel_amd import dense, hip, meshes
from tests import downsample_ref as D

DEV = torch.device("cuda", 0)
U8, BITS, F32 = hip.GRID_U8, hip.GRID_BITS, hip.GRID_F32_BELOW
DIMS = [(1, 1, 1), (3, 2, 1), (7, 9, 13), (63, 5, 4), (64, 5, 4), (65, 5, 4), (129, 6, 3), (200, 17, 11)]   # (nx, ny, nz)
DENSITIES = (0.0, 0.02, 0.5, 1.0)
FACTORS = range(2, 9)
KEYS = ("count", "solid", "values", "argb")
DTYPES = dict(count=torch.int16, solid=torch.uint8, values=torch.uint8, argb=torch.int32)
FILL = dict(count=-3, solid=7, values=9, argb=-5)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def st(t):
    """(x, y, z) element strides of a tensor [z, y, x]."""
    return t.stride(2), t.stride(1), t.stride(0)


def labels_grid(rng, dims, density):
    """uint8 [z, y, x]: solid with the density, bytes of {1, 2, 255}."""
    shape = dims[::-1]
    return np.where(rng.random(shape) < density, rng.choice(np.array([1, 2, 255], np.uint8), shape), 0).astype(np.uint8)


def random_colors(rng, shape):
    return rng.integers(-2 ** 31, 2 ** 31, shape).astype(np.int32)


def call(dv, grid_ptr, fmt, strides, dims, level, origin, f, min_count, mode=hip.DOWN_VALUE_MIN, colors=None, keys=KEYS, outs=None):
    """dv.downsample at the C level into new (or the given) tensors filled with a guard value; {key: numpy array}."""
    _, cdims = D.box(origin, dims, f)
    cshape = cdims[::-1]
    t = {}
    for k in keys:
        t[k] = outs[k] if outs and k in outs else torch.full(cshape, FILL[k], dtype=DTYPES[k], device=DEV)
    torch.cuda.synchronize()
    args = {}
    for k, name in (("count", "count"), ("solid", "solid"), ("values", "values"), ("argb", "argb")):
        if k in t:
            args[name + "_ptr"] = t[k].data_ptr()
            args[("value" if k == "values" else name) + "_strides"] = st(t[k])
    if colors is not None:
        args["colors_ptr"], args["color_strides"] = colors.data_ptr(), st(colors)
    dv.downsample(grid_ptr, fmt, strides, dims, level, origin, f, min_count, mode, **args)
    return {k: host(v) for k, v in t.items()}


def same(got, want, what):
    for k, v in got.items():
        w = want[k]
        g = v.view(np.uint32) if k == "argb" else v
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        assert np.array_equal(g, w), (what, k, int((g != w).sum()), "of", w.size, "differ")


# ---- factors ------------------------------------------------------------------------------------------------------------------

def case_factors():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(170)
    n = alone = 0
    for f in FACTORS:
        for dims in DIMS:
            for density in DENSITIES:
                g = labels_grid(rng, dims, density)
                c = random_colors(rng, g.shape)
                origin = tuple(int(v) for v in rng.integers(0, 3 * f, 3))
                mc = int(rng.integers(1, f ** 3 + 1))
                mode = int(rng.integers(0, 2))
                want = D.downsample(g != 0, f, origin, mc, g, mode, c)
                gt, ct = dev(g), dev(c)
                got = call(dv, gt.data_ptr(), U8, st(gt), dims, 0.0, origin, f, mc, mode, ct)
                same(got, want, (f, dims, density, origin, mc, mode))
                n += 1
                if density == 0.5:
                    for k in KEYS:
                        same(call(dv, gt.data_ptr(), U8, st(gt), dims, 0.0, origin, f, mc, mode, ct if k == "argb" else None, keys=(k,)),
                             want, (f, dims, k, "alone"))
                        alone += 1
    # every origin residue on one small box
    dims = (5, 4, 3)
    g = labels_grid(rng, dims, 0.5)
    c = random_colors(rng, g.shape)
    gt, ct = dev(g), dev(c)
    residues = 0
    for f in FACTORS:
        for oz in range(f):
            for oy in range(f):
                for ox in range(f):
                    origin = (ox + f, oy + 2 * f, oz)
                    want = D.downsample(g != 0, f, origin, D.majority(f) if (ox + oy + oz) % 2 else 1, g, D.MIN, c)
                    got = call(dv, gt.data_ptr(), U8, st(gt), dims, 0.0, origin, f, D.majority(f) if (ox + oy + oz) % 2 else 1, D.MIN, ct)
                    same(got, want, (f, origin))
                    residues += 1
    # the scalar loop on the device too, once per factor
    for f in FACTORS:
        origin = (f - 1, 1, 2 * f + 1)
        want = D.downsample_loop(g != 0, f, origin, 2, g, D.MAX, c)
        same(call(dv, gt.data_ptr(), U8, st(gt), dims, 0.0, origin, f, 2, D.MAX, ct), want, (f, "loop"))
    assert all(t >= 0 for t in dv.downsample_times()) and len(dv.downsample_times()) == 1
    print("factors: compared", n, "grids with all four outputs,", alone, "single outputs,", residues, "origin residues")


# ---- formats ------------------------------------------------------------------------------------------------------------------

def case_formats():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(171)
    n = 0
    level = 0.25
    for f in FACTORS:
        for dims in DIMS:
            for density in (0.02, 0.5):
                nx, ny, nz = dims
                g = labels_grid(rng, dims, density)
                s = g != 0
                origin = tuple(int(v) for v in rng.integers(0, 2 * f, 3))
                mc = int(rng.integers(1, f ** 3 + 1))
                want = D.downsample(s, f, origin, mc)
                keys = ("count", "solid")
                gt = dev(g)
                same(call(dv, gt.data_ptr(), U8, st(gt), dims, 0.0, origin, f, mc, keys=keys), want, (f, dims, "u8"))
                # bool, through dense
                solid, cnt, corigin = dense.downsample(dv, dev(s), f, origin=origin, reduce=mc, count=True)
                assert solid.dtype == torch.bool and cnt.dtype == torch.int16 and corigin == want["corigin"]
                assert np.array_equal(host(solid), want["solid"] != 0) and np.array_equal(host(cnt), want["count"]), (f, dims, "bool")
                # bits at the C level: nx voxels over rows of ceil(nx / 32) words; the padding bits set, they are outside the box
                words = D.pack_bits(s)
                nw = words.shape[2]
                if nx % 32:
                    words.view(np.uint32)[:, :, -1] |= np.uint32((0xffffffff << (nx % 32)) & 0xffffffff)
                bt = dev(words)
                same(call(dv, bt.data_ptr(), BITS, (1, nw, nw * ny), dims, 0.0, origin, f, mc, keys=keys), want, (f, dims, "bits"))
                # float32: below the level solid; at the level, above it, NaN and +inf not; -inf solid
                field = np.where(s, level - rng.random(s.shape) - 1e-3, level + rng.random(s.shape) + 1e-3).astype(np.float32)
                pick = rng.random(s.shape)
                field[~s & (pick < 0.2)] = level
                field[~s & (pick >= 0.2) & (pick < 0.4)] = np.nan
                field[~s & (pick >= 0.4) & (pick < 0.6)] = np.inf
                field[s & (pick < 0.3)] = -np.inf
                field[s & (pick >= 0.3) & (pick < 0.5)] = np.nextafter(np.float32(level), np.float32(-1))
                assert np.array_equal(D.solid_of(field, D.F32_BELOW, level), s)
                ft = dev(field)
                same(call(dv, ft.data_ptr(), F32, st(ft), dims, level, origin, f, mc, keys=keys), want, (f, dims, "f32"))
                n += 1
    # bits through dense: 32 voxels per word
    s = rng.random((5, 6, 96)) < 0.3
    solid, corigin = dense.downsample(dv, dev(D.pack_bits(s)), 3, origin=(4, 0, 2))
    want = D.downsample(s, 3, (4, 0, 2))
    assert np.array_equal(host(solid), want["solid"] != 0) and corigin == want["corigin"]
    solid, corigin = dense.downsample(dv, dev(np.where(s, -1.0, 1.0).astype(np.float32)), 3, level=0.0, origin=(4, 0, 2))
    assert np.array_equal(host(solid), want["solid"] != 0)
    print("formats: compared", n, "grids as uint8, bool, bits and float32")


# ---- strided ------------------------------------------------------------------------------------------------------------------

def case_strided():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(172)
    dims = nx, ny, nz = (70, 20, 33)
    shape = dims[::-1]
    n = 0
    for f in (2, 3, 5, 8):
        origin = (1, f + 1, 2)
        batch_np = np.stack([labels_grid(rng, dims, d) for d in (0.05, 0.6)])
        colors_np = random_colors(rng, shape)
        batch = dev(batch_np)
        ccolors = dev(colors_np)
        _, cdims = D.box(origin, dims, f)
        cshape = cdims[::-1]
        for i in range(2):
            g = batch_np[i]
            want = D.downsample(g != 0, f, origin, 2, g, D.MIN, colors_np)
            # a slice of a batch; outputs: a slice of a batch, [x][z][y] inside a larger buffer, every second element along x
            out = torch.full((2,) + cshape, 7, dtype=torch.uint8, device=DEV)
            cbuf = torch.full((cshape[2] + 2, cshape[0], cshape[1]), -3, dtype=torch.int16, device=DEV)
            cnt = cbuf[1:-1].permute(1, 2, 0)
            vbuf = torch.full(cshape[:2] + (2 * cshape[2],), 9, dtype=torch.uint8, device=DEV)
            val = vbuf[:, :, ::2]
            abuf = torch.full((cshape[1], cshape[0], cshape[2]), -5, dtype=torch.int32, device=DEV)
            argb = abuf.permute(1, 0, 2)
            got = dense.downsample(dv, batch[i], f, origin=origin, reduce=2, values="min", colors=ccolors, out=out[1 - i], out_count=cnt,
                                   out_values=val, out_colors=argb)
            assert [t.data_ptr() for t in got[:4]] == [out[1 - i].data_ptr(), cnt.data_ptr(), val.data_ptr(), argb.data_ptr()]
            assert got[4] == want["corigin"]
            same(dict(solid=host(out[1 - i]), count=host(cnt), values=host(val), argb=host(argb)), want, (f, i, "strided outputs"))
            assert bool((out[i] == 7).all()) and bool((cbuf[0] == -3).all()) and bool((cbuf[-1] == -3).all()), "a write outside the views"
            assert bool((vbuf[:, :, 1::2] == 9).all()), "a write between the values"
            # the grid stored [y][x][z], the colours [x][y][z]
            g_p = batch[i].permute(1, 2, 0).contiguous().permute(2, 0, 1)
            c_p = ccolors.permute(2, 1, 0).contiguous().permute(2, 1, 0)
            assert g_p.stride() == (1, nx * nz, nz) and c_p.stride() == (1, nz, nz * ny)
            same(call(dv, g_p.data_ptr(), U8, st(g_p), dims, 0.0, origin, f, 2, D.MIN, c_p), want, (f, i, "permuted"))
            n += 2
        # a row broadcast over y and z (strides of 0), colours broadcast over z
        row = labels_grid(rng, (nx, 1, 1), 0.5)
        crow = random_colors(rng, (1, ny, nx))
        g_b, c_b = dev(row).expand(nz, ny, nx), dev(crow).expand(nz, ny, nx)
        assert g_b.stride() == (0, 0, 1) and c_b.stride()[0] == 0
        gb, cb = np.broadcast_to(row, shape), np.broadcast_to(crow, shape)
        same(call(dv, g_b.data_ptr(), U8, st(g_b), dims, 0.0, origin, f, 1, D.MAX, c_b), D.downsample(gb != 0, f, origin, 1, gb, D.MAX, cb),
             (f, "broadcast"))
        # 1 byte off 16-byte alignment (the scalar path) against the aligned copy (the 16-byte loads); nx a multiple of 16 here
        wide = labels_grid(rng, (96, 7, 5), 0.4)
        wcol = random_colors(rng, wide.shape)
        flat = torch.zeros(wide.size + 16, dtype=torch.uint8, device=DEV)
        assert flat.data_ptr() % 16 == 0
        flat[1:1 + wide.size] = dev(wide).reshape(-1)
        aligned, wc = dev(wide), dev(wcol)
        assert aligned.data_ptr() % 16 == 0
        a = call(dv, aligned.data_ptr(), U8, (1, 96, 96 * 7), (96, 7, 5), 0.0, origin, f, 3, D.MIN, wc)
        b = call(dv, flat.data_ptr() + 1, U8, (1, 96, 96 * 7), (96, 7, 5), 0.0, origin, f, 3, D.MIN, wc)
        want = D.downsample(wide != 0, f, origin, 3, wide, D.MIN, wcol)
        same(a, want, (f, "aligned"))
        same(b, want, (f, "1 byte off"))
        fw = np.where(wide != 0, -1.0, 1.0).astype(np.float32)
        fl = torch.zeros(fw.size + 4, dtype=torch.float32, device=DEV)
        fl[1:1 + fw.size] = dev(fw).reshape(-1)
        fa = dev(fw)
        for ptr, what in ((fa.data_ptr(), "f32 aligned"), (fl.data_ptr() + 4, "f32 4 bytes off")):
            same(call(dv, ptr, F32, (1, 96, 96 * 7), (96, 7, 5), 0.0, origin, f, 3, keys=("count", "solid")), want, (f, what))
        n += 5
    print("strided: compared", n, "calls")


# ---- thresholds, values, colours ---------------------------------------------------------------------------------------------------

def case_thresholds_values_colours():
    dv = hip.DeviceVoxelizer(0)
    rng = np.random.default_rng(173)
    n = 0
    for f in FACTORS:
        # whole blocks (origin and extent multiples of f) and clipped blocks
        for dims, origin in (((4 * f, 2 * f, 3 * f), (f, 0, 2 * f)), ((4 * f + 1, 2 * f - 1, 3 * f + 2), (f - 1, 1, 2 * f + 1))):
            g = labels_grid(rng, dims, 0.55)
            g[:, :, :f] = np.where(g[:, :, :f] == 0, 1, g[:, :, :f])            # full blocks at the low x end: "all" holds somewhere
            c = random_colors(rng, g.shape)
            gt, ct = dev(g), dev(c)
            for mc in (1, D.majority(f), f ** 3):
                for mode in (D.MIN, D.MAX):
                    want = D.downsample(g != 0, f, origin, mc, g, mode, c)
                    same(call(dv, gt.data_ptr(), U8, st(gt), dims, 0.0, origin, f, mc, mode, ct), want, (f, dims, mc, mode))
                    n += 1
            if origin[0] % f == 0:
                assert D.downsample(g != 0, f, origin, f ** 3)["solid"].any(), (f, "no full block")
            # through dense: the names of the thresholds
            for name, mc in (("any", 1), ("majority", D.majority(f)), ("all", f ** 3)):
                solid, _ = dense.downsample(dv, gt, f, origin=origin, reduce=name)
                assert np.array_equal(host(solid), D.downsample(g != 0, f, origin, mc)["solid"] != 0), (f, name)
    # the rounding halves: one channel, blocks of two, three and 512 voxels
    for f, vals, want_mean in ((2, [0, 1], 1), (2, [0, 0, 1], 0), (2, [1, 2, 2], 2), (2, [255, 254], 255), (8, [255] * 512, 255), (8, [0] * 511 + [1], 0),
                               (8, [1] * 256 + [0] * 256, 1), (8, [1] * 255 + [0] * 257, 0)):
        g = np.zeros((f, f, f), np.uint8)
        c = np.zeros((f, f, f), np.uint32)
        g.reshape(-1)[:len(vals)] = 1
        for shift in (0, 8, 16, 24):
            c.reshape(-1)[:len(vals)] |= np.array(vals, np.uint32) << np.uint32(shift)
        c.reshape(-1)[len(vals):] = 0xdeadbeef
        gt, ct = dev(g), dev(c.view(np.int32))   # (kept alive over the call: the library gets their addresses)
        got = call(dv, gt.data_ptr(), U8, (1, f, f * f), (f, f, f), 0.0, (0, 0, 0), f, 1, colors=ct, keys=("argb", "count"))
        assert got["count"].item() == len(vals) and got["argb"].view(np.uint32).item() == want_mean * 0x01010101, (f, vals[:4], hex(got["argb"].item()))
        n += 1
    # colours with alpha, garbage where the grid is empty
    dims = (37, 11, 9)
    g = labels_grid(rng, dims, 0.4)
    c = random_colors(rng, g.shape)
    garbage = np.where(g != 0, c, random_colors(rng, g.shape))
    assert (garbage != c).any()
    gt = dev(g)
    for f in FACTORS:
        want = D.downsample(g != 0, f, (2, 3, 4), 1, colors=c)
        assert len(np.unique(want["argb"] >> 24)) > 4
        a = call(dv, gt.data_ptr(), U8, st(gt), dims, 0.0, (2, 3, 4), f, 1, colors=dev(c), keys=("argb",))
        b = call(dv, gt.data_ptr(), U8, st(gt), dims, 0.0, (2, 3, 4), f, 1, colors=dev(garbage), keys=("argb",))
        same(a, want, (f, "colours"))
        same(b, want, (f, "garbage where empty"))
        n += 2
    print("thresholds_values_colours: compared", n, "calls")


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def expect_code(code, fn, what):
    try:
        fn()
    except hip.DeviceError as e:
        assert f"code {code}" in str(e) and "o2v_hip_downsample" in str(e), (what, str(e))
        return what + ": " + str(e)
    raise AssertionError(what + " was accepted")


def case_refusals():
    dv = hip.DeviceVoxelizer(0)
    n, f = 48, 2     # (48^3 and 24^3 bytes: a tensor of half the extent is short by more than any allocation granule)
    m = n // f
    shape, dims, s = (n, n, n), (n, n, n), (1, n, n * n)
    cs = (1, m, m * m)
    rng = np.random.default_rng(174)
    g_np = labels_grid(rng, dims, 0.3)
    c_np = random_colors(rng, shape)
    want = D.downsample(g_np != 0, f, (0, 0, 0), 1, g_np, D.MIN, c_np)
    lab, col = dev(g_np), dev(c_np)
    f32 = dev(np.where(g_np != 0, -1.0, 1.0).astype(np.float32))
    bits = dev(D.pack_bits(g_np != 0))
    outs = {k: torch.full((m, m, m), FILL[k], dtype=DTYPES[k], device=DEV) for k in KEYS}
    short = torch.full((m // 2, m, m), 7, dtype=torch.uint8, device=DEV)
    short_colors = torch.full((n // 2, n, n), 7, dtype=torch.int32, device=DEV)
    line = torch.full((4 * m,), 7, dtype=torch.uint8, device=DEV)
    shared = torch.full((8 * n ** 3,), 7, dtype=torch.uint8, device=DEV)      # several grids in one allocation
    host_u8 = np.zeros((m, m, m), np.uint8)
    host_grid = g_np.copy()
    torch.cuda.synchronize()
    L, C_, S = lab.data_ptr(), col.data_ptr(), shared.data_ptr()
    K, O, V, A = (outs[k].data_ptr() for k in KEYS)
    MIN = hip.DOWN_VALUE_MIN

    def good():
        """After a refusal the context still works, and the refusal wrote nothing."""
        assert all(bool((outs[k] == FILL[k]).all()) for k in KEYS)
        assert bool((short == 7).all()) and bool((line == 7).all()) and bool((shared == 7).all()) and bool((short_colors == 7).all())
        assert np.array_equal(host(lab), g_np) and np.array_equal(host(col), c_np)
        same(call(dv, L, U8, s, dims, 0.0, (0, 0, 0), f, 1, MIN, col), want, "after a refusal")

    def c(grid=L, fmt=U8, strides=s, dm=dims, level=0.0, origin=(0, 0, 0), factor=f, mc=1, mode=MIN, **kw):
        return lambda: dv.downsample(grid, fmt, strides, dm, level, origin, factor, mc, mode, **kw)

    so = dict(solid_ptr=O, solid_strides=cs)
    big = 2 ** 32 - 10
    refusals = [
        (3, c(grid=None, **so), "null grid"),
        (3, c(strides=None, **so), "null strides"),
        (3, c(solid_ptr=O), "solid without strides"),
        (3, c(count_ptr=K), "count without strides"),
        (3, c(values_ptr=V), "values without strides"),
        (3, c(argb_ptr=A, colors_ptr=C_, color_strides=s), "argb without strides"),
        (3, c(argb_ptr=A, argb_strides=cs, colors_ptr=C_), "colors without strides"),
        (3, c(), "no output at all"),
        (3, c(dm=(n, 0, n), **so), "zero dims"),
        (3, c(fmt=3, **so), "unknown format"),
        (3, c(grid=f32.data_ptr(), fmt=F32, level=float("nan"), **so), "level nan"),
        (3, c(grid=f32.data_ptr(), fmt=F32, level=float("inf"), **so), "level inf"),
        (3, c(grid=bits.data_ptr(), fmt=BITS, strides=(2, 2, 2 * n), **so), "bits with an x stride of 2"),
        (3, c(factor=1, **so), "factor 1"),
        (3, c(factor=0, **so), "factor 0"),
        (3, c(factor=9, **so), "factor 9"),
        (3, c(mc=0, **so), "min_count 0"),
        (3, c(mc=f ** 3 + 1, **so), "min_count above factor^3"),
        (3, c(grid=f32.data_ptr(), fmt=F32, values_ptr=V, value_strides=cs), "values on float32"),
        (3, c(grid=bits.data_ptr(), fmt=BITS, strides=(1, 2, 2 * n), values_ptr=V, value_strides=cs), "values on bits"),
        (3, c(mode=2, values_ptr=V, value_strides=cs), "unknown value mode"),
        (3, c(argb_ptr=A, argb_strides=cs), "argb without colors"),
        (3, c(solid_ptr=line.data_ptr(), solid_strides=(1, 0, 0)), "solid with strides of 0"),
        (3, c(solid_ptr=O, solid_strides=(1, m // 2, m * m)), "solid with y inside x"),
        (3, c(count_ptr=K, count_strides=(0, 1, m)), "count with strides of 0"),
        (3, c(values_ptr=line.data_ptr(), value_strides=(1, 0, 0)), "values with strides of 0"),
        (3, c(argb_ptr=A, argb_strides=(1, 1, m), colors_ptr=C_, color_strides=s), "argb with x on y"),
        (3, c(solid_ptr=short.data_ptr(), solid_strides=cs), "short solid"),
        (3, c(values_ptr=short.data_ptr(), value_strides=cs), "short values"),
        (3, c(argb_ptr=A, argb_strides=cs, colors_ptr=short_colors.data_ptr(), color_strides=s), "short colors"),
        (3, c(grid=short.data_ptr(), **so), "short grid"),
        (3, c(solid_ptr=host_u8.ctypes.data, solid_strides=cs), "host solid"),
        (3, c(grid=host_grid.ctypes.data, **so), "host grid"),
        (3, c(argb_ptr=A, argb_strides=cs, colors_ptr=c_np.ctypes.data, color_strides=s), "host colors"),
        # overlaps: the last element of one range is the first of the next
        (3, c(grid=S, solid_ptr=S + n ** 3 - 1, solid_strides=cs), "grid and solid overlap"),
        (3, c(grid=S, count_ptr=S + n ** 3 - 2, count_strides=cs), "grid and count overlap"),
        (3, c(solid_ptr=S, solid_strides=cs, values_ptr=S + m ** 3 - 1, value_strides=cs), "solid and values overlap"),
        (3, c(solid_ptr=S + 2 * m ** 3 - 2, solid_strides=cs, count_ptr=S, count_strides=cs), "count and solid overlap"),
        (3, c(solid_ptr=O, solid_strides=cs, values_ptr=O, value_strides=cs), "solid is values"),
        (3, c(argb_ptr=S + 4 * n ** 3 - 4, argb_strides=cs, colors_ptr=S, color_strides=s, grid=L), "colors and argb overlap"),
        (3, c(argb_ptr=S, argb_strides=cs, colors_ptr=C_, color_strides=s, solid_ptr=S + 4 * m ** 3 - 1, solid_strides=cs),
         "argb and solid overlap"),
        (5, c(dm=(65537, 1, 1), strides=(1, 65537, 65537), **so), "65 537 voxels along x"),
        (5, c(dm=(1, 1, 65537), strides=(1, 1, 1), **so), "65 537 voxels along z"),
        (5, c(origin=(big, 0, 0), **so), "origin + dims above 2^32 along x"),
        (5, c(origin=(0, 0, big), **so), "origin + dims above 2^32 along z"),
    ]
    msgs = []
    for code, fn, what in refusals:
        msgs.append(expect_code(code, fn, what))
        good()
    assert all("one element" in t for t in msgs if "strides of 0" in t.split(":")[0] or "inside x" in t.split(":")[0] or "x on y" in t.split(":")[0]), msgs
    assert all("overlap" in t.split(": ", 1)[1] for t in msgs if "overlap" in t.split(":")[0] or "solid is values" in t), msgs
    # through dense: an expand()ed out
    try:
        dense.downsample(dv, lab, f, out=line[:m].view(1, 1, m).expand(m, m, m))
        raise AssertionError("an expanded out was accepted")
    except hip.DeviceError as e:
        assert "code 3" in str(e), str(e)
    good()
    # at the limits: origin + dims == 2^32, and next to each other in one allocation: accepted
    edge = (2 ** 32 - n, 2 ** 32 - n, 2 ** 32 - n)
    same(call(dv, L, U8, s, dims, 0.0, edge, 7, 3, D.MAX, col), D.downsample(g_np != 0, 7, edge, 3, g_np, D.MAX, c_np), "origin + dims == 2^32")
    shared.zero_()
    shared[:n ** 3] = lab.reshape(-1)
    torch.cuda.synchronize()
    dv.downsample(S, U8, s, dims, 0.0, (0, 0, 0), f, 1, MIN, solid_ptr=S + n ** 3, solid_strides=cs, values_ptr=S + n ** 3 + m ** 3, value_strides=cs)
    got = host(shared)
    assert np.array_equal(got[n ** 3:n ** 3 + m ** 3].reshape(m, m, m), want["solid"])
    assert np.array_equal(got[n ** 3 + m ** 3:n ** 3 + 2 * m ** 3].reshape(m, m, m), want["values"])
    print("\n".join(msgs))
    print("refused", len(msgs) + 1)


# ---- the flow of the README ------------------------------------------------------------------------------------------------------

def case_mesh():
    dv = hip.DeviceVoxelizer(0)
    verts = meshes.uv_sphere(12)
    T = len(verts)
    types = np.full(T, hip.TRI_UNTEXTURED, np.uint32)
    dense.set_mesh(dv, dev(verts), types=dev(types.view(np.int32)), colors=dev(meshes.triangle_colors(T)))
    for R, want_voxels, want_fine in ((16, 1160, 4664), (21, 1994, 8024)):
        ss, o_ss = dense.voxelize_dense(dv, R, supersampling=2, box="tight")
        fine, o_fine = dense.voxelize_dense(dv, 2 * R, box="tight")
        half, o_half = dense.downsample(dv, fine, 2, origin=o_fine)
        a = D.place(host(ss), o_ss, (R, R, R), False)
        b = D.place(host(half), o_half, (R, R, R), False)
        assert int(a.sum()) == want_voxels and int(host(fine).sum()) == want_fine, (R, int(a.sum()), int(host(fine).sum()))
        assert np.array_equal(a, b), (R, int((a != b).sum()), "supersampling 2 differs from the downsampled grid at 2R")
        ref = D.downsample(host(fine), 2, o_fine)
        assert np.array_equal(host(half), ref["solid"] != 0) and o_half == ref["corigin"]
        print("mesh: sphere at", R, "supersampling 2:", int(a.sum()), "voxels; at", 2 * R, ":", int(host(fine).sum()))
    # labels and colours of a filled model at 64 to 32, 16 (f = 2, 4) and 22 (f = 3)
    labels, origin = dense.voxelize_dense(dv, 64, fmt="labels", fill=True, box="tight")
    argb, _ = dense.voxelize_dense(dv, 64, fmt="argb", fill=True, origin=origin, out=torch.zeros(tuple(labels.shape), dtype=torch.int32, device=DEV))
    lab, col = host(labels), host(argb)
    assert (lab == 1).sum() > 1000 and (lab == 2).sum() > 1000
    for f in (2, 3, 4):
        solid, cnt, val, mean, corigin = dense.downsample(dv, labels, f, origin=origin, count=True, values="min", colors=argb)
        want = D.downsample(lab != 0, f, origin, 1, lab, D.MIN, col)
        same(dict(solid=host(solid).astype(np.uint8), count=host(cnt), values=host(val), argb=host(mean)), want, ("mesh", f))
        assert corigin == want["corigin"] and set(np.unique(want["values"])) == {0, 1, 2}
        coverage = cnt.float() / f ** 3
        assert 0.0 < float(coverage.max()) <= 1.0
    print("mesh: labels and mean colours at 64 by 2, 3 and 4")


# ---- one call per case and its wall time ------------------------------------------------------------------------------------------

CASES = {"factors": case_factors, "formats": case_formats, "strided": case_strided,
         "thresholds_values_colours": case_thresholds_values_colours, "refusals": case_refusals, "mesh": case_mesh}

if __name__ == "__main__":
    t0 = time.time()
    CASES[sys.argv[1]]()
    print("case", sys.argv[1], "took %.1f s" % (time.time() - t0))
    print("ok")
