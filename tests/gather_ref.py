"""The numpy restatement of o2v_hip_gather_count / _write / _save (include/o2v_hip.h): which voxels of a
grid are solid, their (x, y, z, argb) records in ascending linear index, and parsers of the list formats the records are saved in.

Grids are numpy arrays indexed [z, y, x], as the tensors are.  Nothing here imports the code under test."""
import numpy as np

from tests import raycast_ref

F = np.float32
U8, BITS, F32_BELOW = 0, 1, 2                 # O2V_HIP_GRID_*
CONSTANT, GRID, PALETTE = 0, 1, 2             # O2V_HIP_GATHER_COLOR_*


def solid(grid, fmt, level=None):
    """bool [z, y, x]: the solid voxels.  U8: element != 0; BITS: bit x % 32 of word x / 32 (32 voxels per word along x);
    F32_BELOW: grid < level, a NaN is not below it."""
    if fmt == U8:
        return raycast_ref.solid_u8(grid)
    if fmt == BITS:
        return raycast_ref.solid_bits(grid)
    assert fmt == F32_BELOW and level is not None and np.isfinite(F(level))
    return raycast_ref.solid_f32(grid, level)


def records(grid, fmt, level=None, origin=(0, 0, 0), argb=0xFFFFFFFF, colors=None, palette=None):
    """uint32 [n, 4]: (origin + (x, y, z), argb) of the solid voxels in ascending (z * ny + y) * nx + x - the order of np.nonzero
    on a [z, y, x] array.  The colour: `argb`, or colors[z, y, x] (an array of the voxel shape), or palette[grid[z, y, x]]
    (256 entries, U8 grids)."""
    assert colors is None or palette is None
    S = solid(grid, fmt, level)
    z, y, x = np.nonzero(S)
    out = np.empty((len(x), 4), np.uint32)
    for k, (o, v) in enumerate(zip(origin, (x, y, z))):
        out[:, k] = (v.astype(np.uint64) + np.uint64(o)).astype(np.uint32)
    if colors is not None:
        assert np.asarray(colors).shape == S.shape
        out[:, 3] = (np.asarray(colors).astype(np.int64)[z, y, x] & 0xFFFFFFFF).astype(np.uint32)
    elif palette is not None:
        assert fmt == U8 and len(palette) == 256
        out[:, 3] = (np.asarray(palette, np.int64) & 0xFFFFFFFF).astype(np.uint32)[np.asarray(grid).astype(np.uint8)[z, y, x]]
    else:
        out[:, 3] = np.uint32(argb & 0xFFFFFFFF)
    return out


def records_scalar(grid, fmt, level=None, origin=(0, 0, 0), argb=0xFFFFFFFF, colors=None, palette=None):
    """The same by a triple loop that restates the header word for word (the check of `records`)."""
    g = np.asarray(grid)
    nz, ny = g.shape[:2]
    nx = g.shape[2] * 32 if fmt == BITS else g.shape[2]
    out = []
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                if fmt == U8:
                    is_solid = int(g[z, y, x]) != 0
                elif fmt == BITS:
                    is_solid = (int(g[z, y, x // 32]) & 0xFFFFFFFF) >> (x % 32) & 1 == 1
                else:
                    v = F(g[z, y, x])
                    is_solid = bool(v < F(level)) if not np.isnan(v) else False
                if not is_solid:
                    continue
                if colors is not None:
                    c = int(colors[z, y, x]) & 0xFFFFFFFF
                elif palette is not None:
                    c = int(palette[int(g[z, y, x])]) & 0xFFFFFFFF
                else:
                    c = argb & 0xFFFFFFFF
                out.append((origin[0] + x, origin[1] + y, origin[2] + z, c))
    return np.array(out, np.uint32).reshape(-1, 4)


def closed_form_expanded_row(i, nx, ny):
    """Records i (an int64 array) of a full grid of nx x ny x anything: voxel (i % nx, (i / nx) % ny, i / (nx * ny)), white."""
    i = np.asarray(i, np.uint64)
    out = np.empty((len(i), 4), np.uint32)
    out[:, 0] = i % np.uint64(nx)
    out[:, 1] = (i // np.uint64(nx)) % np.uint64(ny)
    out[:, 2] = i // np.uint64(nx * ny)
    out[:, 3] = 0xFFFFFFFF
    return out


# ---- the list formats (reference README.adoc:210-264) ----------------------------------------------------------------------------

def parse_vl32(data):
    """uint32 [n, 4] in file order: big-endian (x, y, z, argb) records."""
    assert len(data) % 16 == 0
    return np.frombuffer(data, dtype=">u4").astype(np.uint32).reshape(-1, 4)


def parse_ply(data):
    """uint32 [n, 4] in file order: a 300-byte header that names the vertex count, then VL32 records."""
    header = data[:300].decode()
    assert header.startswith("ply\nformat binary_big_endian 1.0\nelement vertex ") and header.endswith("end_header\n")
    n = int(header.split("element vertex ")[1].split("\n")[0])
    assert len(data) == 300 + 16 * n
    return parse_vl32(data[300:])


def parse_xyzrgb(data):
    """uint32 [n, 4] in file order: text lines "x y z r g b"; alpha is not stored and comes back as 255."""
    rows = np.array(data.decode().split(), dtype=np.int64).reshape(-1, 6).astype(np.uint32)
    argb = np.uint32(0xFF000000) | (rows[:, 3] << 16) | (rows[:, 4] << 8) | rows[:, 5]
    return np.concatenate([rows[:, :3], argb[:, None]], axis=1).astype(np.uint32)


def parse_qef(data):
    """(size [3], uint32 [n, 4] records): the Qubicle text format; colours 0 .. 1 per channel in a table, alpha 255."""
    head, n_col = data[:200].decode().split("\n")[:5], None
    assert head[:3] == ["Qubicle Exchange Format", "Version 0.2", "www.minddesk.com"]
    size, n_col = [int(t) for t in head[3].split()], int(head[4])
    body = data[sum(len(h) + 1 for h in head):].decode().split("\n", n_col)
    colors = np.array([[float(t) for t in ln.split()] for ln in body[:n_col]]).reshape(-1, 3)
    rows = np.array(body[n_col].split(), dtype=np.int64).reshape(-1, 5)
    rgb = np.rint(colors[rows[:, 3]] * 255).astype(np.uint32).reshape(-1, 3)
    argb = np.uint32(0xFF000000) | (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]
    return size, np.concatenate([rows[:, :3].astype(np.uint32), argb[:, None]], axis=1).astype(np.uint32)


def vox_records(models, trans, palette):
    """uint32 [n, 4] of a parsed MagicaVoxel file (tests/test_gpu_io.py: _parse_vox): the models put back at their places."""
    parts = []
    for k, (size, xyzi) in enumerate(models):
        origin = np.zeros(3, np.int64) if not trans else np.array(trans[("model", k)]) - np.array(size) // 2
        rgba = palette[xyzi[:, 3].astype(int) - 1].astype(np.uint32)
        argb = (rgba[:, 3] << 24) | (rgba[:, 0] << 16) | (rgba[:, 1] << 8) | rgba[:, 2]
        parts.append(np.concatenate([xyzi[:, :3].astype(np.uint32) + origin.astype(np.uint32), argb[:, None]], axis=1))
    return np.concatenate(parts).astype(np.uint32) if parts else np.zeros((0, 4), np.uint32)


def as_set(rec):
    """The records sorted by (z, y, x, argb): equal arrays for equal sets (no voxel appears twice)."""
    rec = np.asarray(rec, np.uint32).reshape(-1, 4)
    return rec[np.lexsort((rec[:, 3], rec[:, 0], rec[:, 1], rec[:, 2]))]


# ---- the slot -> word -> bit mapping the kernels use, restated ---------------------------------------------------------------------

def words64(S):
    """The set's bits as the kernels keep them: uint64 [nz * ny * ceil(nx / 64)], padding bits 0."""
    nz, ny, nx = S.shape
    W = -(-nx // 64)
    pad = np.zeros((nz, ny, W * 64), bool)
    pad[:, :, :nx] = S
    return np.ascontiguousarray((pad.reshape(nz, ny, W, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=3, dtype=np.uint64)).reshape(-1)


def slots_of_words(words):
    """(word, bit) int64 [n, 2] of every set bit of uint64 words, in ascending (word, bit): slot i is row i."""
    bits = (np.asarray(words, np.uint64)[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    w, b = np.nonzero(bits)
    return np.stack([w, b], axis=1).astype(np.int64)
