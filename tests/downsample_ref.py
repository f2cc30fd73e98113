"""numpy references of o2v_hip_downsample (include/o2v_hip.h): a grid merged in blocks of f^3 voxels
aligned to the global lattice into coverage counts, occupancy by a threshold, the smallest / largest non-zero byte and the mean
colour of the solid voxels.

downsample() is vectorised - pad to the global lattice, reshape, reduce -; downsample_loop() is the definition read aloud, a
scalar loop over coarse and fine voxels, for small boxes.  Arrays are indexed [z, y, x]; origins and dims are (x, y, z)."""
import numpy as np

U8, BITS, F32_BELOW = 0, 1, 2
MIN, MAX = 0, 1


def solid_of(grid, fmt=U8, level=None, nx=None):
    """bool [z, y, x]: the solid voxels of a grid of the format (BITS: int32 / uint32 words along x, nx voxels)."""
    grid = np.asarray(grid)
    if fmt == BITS:
        w = grid.view(np.uint32)
        bits = (w[..., None] >> np.arange(32, dtype=np.uint32)) & 1
        bits = bits.reshape(w.shape[0], w.shape[1], -1).astype(bool)
        return bits[:, :, :bits.shape[2] if nx is None else nx]
    if fmt == F32_BELOW:
        with np.errstate(invalid="ignore"):
            return grid < np.float32(level)
    return grid != 0


def box(origin, dims, f):
    """(corigin, cdims), each (x, y, z)."""
    corigin = tuple(int(o) // f for o in origin)
    cdims = tuple(-(-(int(o) + int(n)) // f) - c for o, n, c in zip(origin, dims, corigin))
    return corigin, cdims


def majority(f):
    return (f ** 3 + 1) // 2


def _blocks(a, origin, f, fill=0):
    """a [z, y, x] padded to the global lattice and cut into blocks: [cz, cy, cx, f, f, f] (the last three: dz, dy, dx)."""
    nz, ny, nx = a.shape
    corigin, cdims = box(origin, (nx, ny, nz), f)
    pad = []
    for o, n, c, cn in zip(origin[::-1], a.shape, corigin[::-1], cdims[::-1]):
        before = o - c * f
        pad.append((before, cn * f - before - n))
    p = np.pad(a, pad, constant_values=fill)
    cz, cy, cx = cdims[::-1]
    return p.reshape(cz, f, cy, f, cx, f).transpose(0, 2, 4, 1, 3, 5)


def downsample(solid, f, origin=(0, 0, 0), min_count=1, grid_u8=None, value_mode=None, colors=None):
    """dict(count int16, solid uint8, values uint8 (with grid_u8 and value_mode), argb uint32 (with colors), corigin) over the
    coarse box.  solid: bool [z, y, x]; grid_u8: the bytes of a U8 grid (solid == (grid_u8 != 0)); colors: 32 bits per voxel."""
    solid = np.asarray(solid, bool)
    assert 2 <= f <= 8 and 1 <= min_count <= f ** 3
    nz, ny, nx = solid.shape
    corigin, _ = box(origin, (nx, ny, nz), f)
    sb = _blocks(solid, origin, f, False)
    count = sb.sum(axis=(3, 4, 5), dtype=np.int64)
    is_solid = count >= min_count
    out = dict(count=count.astype(np.int16), solid=is_solid.astype(np.uint8), corigin=corigin)
    if value_mode is not None:
        g = np.asarray(grid_u8).astype(np.uint8)
        assert np.array_equal(g != 0, solid)
        gb = _blocks(g, origin, f, 0).astype(np.int64)
        if value_mode == MIN:
            v = np.where(gb == 0, 256, gb).min(axis=(3, 4, 5))
        else:
            v = gb.max(axis=(3, 4, 5))
        out["values"] = np.where(is_solid, v, 0).astype(np.uint8)
    if colors is not None:
        c = np.ascontiguousarray(colors).view(np.uint32)
        cb = _blocks(c, origin, f, 0)
        argb = np.zeros(count.shape, np.uint32)
        safe = np.maximum(count, 1)
        for shift in (0, 8, 16, 24):
            ch = ((cb >> np.uint32(shift)) & np.uint32(0xff)).astype(np.int64)
            s = np.where(sb, ch, 0).sum(axis=(3, 4, 5))
            argb |= ((2 * s + safe) // (2 * safe)).astype(np.uint32) << np.uint32(shift)
        out["argb"] = np.where(is_solid, argb, np.uint32(0)).astype(np.uint32)
    return out


def mean_half_up(values):
    """The rounded mean of a non-empty list of integers: (2 sum + c) / (2 c)."""
    c, s = len(values), int(sum(values))
    return (2 * s + c) // (2 * c)


def downsample_loop(solid, f, origin=(0, 0, 0), min_count=1, grid_u8=None, value_mode=None, colors=None):
    """The same, voxel by voxel."""
    solid = np.asarray(solid, bool)
    nz, ny, nx = solid.shape
    corigin, cdims = box(origin, (nx, ny, nz), f)
    shape = cdims[::-1]
    count, sol = np.zeros(shape, np.int16), np.zeros(shape, np.uint8)
    values, argb = np.zeros(shape, np.uint8), np.zeros(shape, np.uint32)
    cu = None if colors is None else np.ascontiguousarray(colors).view(np.uint32)
    for Z in range(shape[0]):
        for Y in range(shape[1]):
            for X in range(shape[2]):
                bytes_, cols = [], []
                n = 0
                for gz in range((corigin[2] + Z) * f, (corigin[2] + Z + 1) * f):
                    for gy in range((corigin[1] + Y) * f, (corigin[1] + Y + 1) * f):
                        for gx in range((corigin[0] + X) * f, (corigin[0] + X + 1) * f):
                            x, y, z = gx - origin[0], gy - origin[1], gz - origin[2]
                            if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz) or not solid[z, y, x]:
                                continue
                            n += 1
                            if grid_u8 is not None:
                                bytes_.append(int(grid_u8[z, y, x]))
                            if cu is not None:
                                cols.append(int(cu[z, y, x]))
                count[Z, Y, X] = n
                if n < min_count:
                    continue
                sol[Z, Y, X] = 1
                if value_mode is not None:
                    values[Z, Y, X] = min(bytes_) if value_mode == MIN else max(bytes_)
                if cu is not None:
                    argb[Z, Y, X] = sum(mean_half_up([(c >> s) & 0xff for c in cols]) << s for s in (0, 8, 16, 24))
    out = dict(count=count, solid=sol, corigin=corigin)
    if value_mode is not None:
        out["values"] = values
    if cu is not None:
        out["argb"] = argb
    return out


def place(a, origin, shape, fill=0):
    """a [z, y, x] with its origin (x, y, z) put into an array of `shape`, `fill` elsewhere."""
    full = np.full(shape, fill, a.dtype)
    full[origin[2]:origin[2] + a.shape[0], origin[1]:origin[1] + a.shape[1], origin[0]:origin[0] + a.shape[2]] = a
    return full


def pack_bits(solid):
    """int32 [z, y, ceil(nx / 32)]: bit x % 32 of word x / 32."""
    nz, ny, nx = solid.shape
    words = (nx + 31) // 32
    padded = np.zeros((nz, ny, words * 32), np.uint64)
    padded[:, :, :nx] = solid
    w = (padded.reshape(nz, ny, words, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32).view(np.int32)
