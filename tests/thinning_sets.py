"""Large sets for the thinning tests whose reference is computed object by object (tests/test_host_thinning.py proves the rule,
tests/thinning_cases.py uses it on the device), and the host's choice of tiles per workgroup restated in Python.  numpy only.

The locality lemma.  If the objects of a set are pairwise separated by at least two empty voxels (their voxels differ by three or
more along some axis) and each is thinned alone in a crop whose origin is even on every axis and which pads it by at least two
voxels, then the thinned union is the union of the thinned crops, the iterations are the most any crop takes and the removed
voxels are the sum over the crops: whether a voxel goes depends on its 26 neighbours, on their six neighbours (the border) and on
the parities of its coordinates (the subfield), and on nothing else.

An object is ((x, y, z), A, keep): A a bool array [z, y, x] placed with its first voxel at (x, y, z); keep None or an array of
A's shape.  Objects that share an array share a reference: what a crop gives is computed once per (array, parities, keep, mode)."""
import numpy as np

from tests import thinning_ref as TR

MAX_CHUNK, MAX_GRID, WGS_PER_CU = 32, 1 << 20, 16   # kThinChunk, kCcMaxGrid, the workgroups per CU the host leaves


# ---- the host's choice (o2v_hip_thin_dense): tiles per workgroup, chunks, the grid ---------------------------------------------------

def tiles_of(dims):
    """(W, tiles_y, tiles_z) of a box (nx, ny, nz): tiles of 64 x 8 x 8 voxels."""
    return -(-dims[0] // 64), -(-dims[1] // 8), -(-dims[2] // 8)


def tile_count(dims):
    W, ty, tz = tiles_of(dims)
    return W * ty * tz


def plan(tiles, cus):
    """(chunk, chunks, grid): the tiles a workgroup of k_thin_substep lists at a time, the chunks, the workgroups launched."""
    chunk = min(max(tiles // (WGS_PER_CU * cus), 1), MAX_CHUNK)
    chunks = -(-tiles // chunk)
    return chunk, chunks, min(chunks, MAX_GRID)


def visits(tiles, cus):
    """(how often each tile is listed [uint8 per tile], the chunks taken in a second or later turn of the chunk loop): every
    workgroup b takes the chunks b, b + grid, ..., thread t of it the tile t * chunks + chunk."""
    chunk, chunks, grid = plan(tiles, cus)
    seen = np.zeros(tiles, np.uint8)
    later = []
    b = np.arange(0, grid, dtype=np.int64)                      # all workgroups at once
    for turn, first in enumerate(range(0, chunks, grid)):       # turn k: the chunks b + k * grid
        c = b + first
        c = c[c < chunks]
        if turn:
            later.append(c)
        for t in range(chunk):
            ids = t * chunks + c
            seen[ids[ids < tiles]] += 1
    return seen, np.concatenate(later) if later else np.zeros(0, np.int64)


def dims_for_chunk(cus, want, nx):
    """The smallest box (nx, ny, nz), near square in y and z, for which the host picks `want` tiles per workgroup with a tile count
    that is no multiple of it; ny and nz are no multiples of a tile (5 and 7 rows in the last tiles)."""
    W = -(-nx // 64)
    need = want * WGS_PER_CU * cus
    ty = max(int(np.sqrt(need / W)), 2)
    while True:
        for tz in (ty, ty + 1):
            tiles = W * ty * tz
            if plan(tiles, cus)[0] == want and tiles % want:
                return nx, 8 * ty - 3, 8 * tz - 1
        ty += 1


GRID_TURNS_DIMS = (1, 46340, 46340)


# ---- objects, their crops and the lemma ----------------------------------------------------------------------------------------

_memo = {}


def thin_alone(origin, A, keep, mode):
    """(K, iterations, removed) of the object thinned alone: in a crop that pads it by two voxels, three where the origin's
    coordinate is odd - the crop's origin is even, so a voxel's subfield in the crop is its subfield in the box."""
    lo = tuple(2 + (o & 1) for o in origin)                   # (x, y, z)
    key = (id(A), lo, None if keep is None else id(keep), mode)
    if key not in _memo:
        pad = [(lo[2], 2), (lo[1], 2), (lo[0], 2)]
        K, iterations, removed = TR.thin(np.pad(A, pad), mode, None if keep is None else np.pad(keep, pad))
        _memo[key] = (np.ascontiguousarray(K[lo[2]:lo[2] + A.shape[0], lo[1]:lo[1] + A.shape[1], lo[0]:lo[0] + A.shape[2]]), iterations, removed, A, keep)
    return _memo[key][:3]


def coords(placed):
    """(z, y, x) of the set voxels of [(origin, array), ...]: int64 arrays.  Placements that share an array are taken together."""
    groups = {}
    for origin, A in placed:
        groups.setdefault(id(A), (A, []))[1].append(origin)
    zs, ys, xs = [], [], []
    for A, origins in groups.values():
        dz, dy, dx = (v.astype(np.int64) for v in np.nonzero(A))
        O = np.asarray(origins, np.int64).reshape(-1, 3)
        xs.append((O[:, 0:1] + dx).ravel()), ys.append((O[:, 1:2] + dy).ravel()), zs.append((O[:, 2:3] + dz).ravel())
    if not zs:
        return (np.zeros(0, np.int64),) * 3
    return np.concatenate(zs), np.concatenate(ys), np.concatenate(xs)


def grid_of(dims, placed):
    """The bool grid [z, y, x] of a box (nx, ny, nz) with the placements' voxels set."""
    G = np.zeros((dims[2], dims[1], dims[0]), bool)
    z, y, x = coords(placed)
    G[z, y, x] = True
    return G


def set_of(objects):
    return [(o, A) for o, A, _ in objects]


def keep_of(objects):
    return [(o, k) for o, _, k in objects if k is not None]


def isolated_objects(objects, mode):
    """(placements, skeleton, iterations, removed) of a set of isolated objects by the lemma.  placements: [(origin, A, keep, K)],
    K the object's skeleton in A's frame; skeleton: [(origin, K)] - for coords() and grid_of(); iterations: the most of any
    crop; removed: the sum."""
    placements, iterations, removed = [], 1, 0
    for origin, A, keep in objects:
        K, it, n = thin_alone(origin, A, keep, mode)
        placements.append((origin, A, keep, K))
        iterations, removed = max(iterations, it), removed + n
    return placements, [(p[0], p[3]) for p in placements], iterations, removed


class Boxes:
    """Boxes (x0, y0, z0, x1, y1, z1), ends exclusive, in a hash of cells: is a box within `gap` voxels of one that is there."""
    CELL = 16

    def __init__(self):
        self.cells = {}

    def _cells(self, b, gap):
        C = self.CELL
        for cz in range((b[2] - gap) // C, (b[5] - 1 + gap) // C + 1):
            for cy in range((b[1] - gap) // C, (b[4] - 1 + gap) // C + 1):
                for cx in range((b[0] - gap) // C, (b[3] - 1 + gap) // C + 1):
                    yield cx, cy, cz

    def near(self, b, gap=2):
        """Is there a box with fewer than `gap` empty voxels between it and b along every axis."""
        for c in self._cells(b, gap):
            for o in self.cells.get(c, ()):
                if all(b[a] - gap < o[a + 3] and o[a] - gap < b[a + 3] for a in range(3)):
                    return True
        return False

    def add(self, b):
        for c in self._cells(b, 0):
            self.cells.setdefault(c, []).append(b)


def box_of(origin, A):
    return origin + (origin[0] + A.shape[2], origin[1] + A.shape[1], origin[2] + A.shape[0])


def separation_holds(dims, objects):
    """Are the objects pairwise separated by two empty voxels, on the grid itself: no voxel has a voxel of another object within
    two steps along every axis (a label grid under separable maximum and minimum filters of radius 2)."""
    L = np.zeros((dims[2], dims[1], dims[0]), np.int32)
    groups = {}
    for i, (origin, A, _) in enumerate(objects):
        groups.setdefault(id(A), (A, [], []))
        groups[id(A)][1].append(origin), groups[id(A)][2].append(i + 1)
    for A, origins, ids in groups.values():
        dz, dy, dx = (v.astype(np.int64) for v in np.nonzero(A))
        O = np.asarray(origins, np.int64)
        L[(O[:, 2:3] + dz).ravel(), (O[:, 1:2] + dy).ravel(), (O[:, 0:1] + dx).ravel()] = np.repeat(np.asarray(ids, np.int32), len(dz))
    big = np.int32(2 ** 31 - 1)
    hi, lo = L.copy(), np.where(L > 0, L, big)
    for axis in range(3):
        a, b = hi.copy(), lo.copy()
        for d in (1, 2):
            n = L.shape[axis]
            if d >= n:
                break
            fwd, back = [slice(None)] * 3, [slice(None)] * 3
            fwd[axis], back[axis] = slice(d, None), slice(None, n - d)
            fwd, back = tuple(fwd), tuple(back)
            np.maximum(a[back], hi[fwd], out=a[back]), np.maximum(a[fwd], hi[back], out=a[fwd])
            np.minimum(b[back], lo[fwd], out=b[back]), np.minimum(b[fwd], lo[back], out=b[fwd])
        hi, lo = a, b
    inside = L > 0
    return bool((hi[inside] == L[inside]).all() and (lo[inside] == L[inside]).all())


# ---- tile_chunks: a lattice object in every tile and random objects across the tiles' faces ------------------------------------------

def _palette():
    """Ten small objects [3, 3, 3], each connected and of two voxels or more - ULTIMATE takes at least one away."""
    def of(*voxels):
        A = np.zeros((3, 3, 3), bool)
        for z, y, x in voxels:
            A[z, y, x] = True
        return A
    full = np.ones((3, 3, 3), bool)
    plate_z, plate_x = np.zeros((3, 3, 3), bool), np.zeros((3, 3, 3), bool)
    plate_z[1], plate_x[:, :, 1] = True, True
    cube = np.zeros((3, 3, 3), bool)
    cube[:2, :2, :2] = True
    return [full, plate_z, plate_x, of((0, 1, 1), (1, 1, 1), (2, 1, 1)), of((1, 0, 1), (1, 1, 1), (1, 2, 1)), of((1, 1, 0), (1, 1, 1), (1, 1, 2)),
            of((0, 0, 0), (1, 1, 1), (2, 2, 2)), of((0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 1, 0), (2, 2, 1)), cube, of((0, 2, 0), (1, 1, 1))]


PALETTE = _palette()
PALETTE_KEEP = []
for _A in PALETTE:                                             # keep: the object's last voxel in [z, y, x] order
    _k = np.zeros_like(_A)
    _k[tuple(np.argwhere(_A)[-1])] = True
    PALETTE_KEEP.append(_k)


def _hash(tile):
    """32 mixed bits of a tile index (the finalizer of MurmurHash3)."""
    h = tile & 0xFFFFFFFF
    h = ((h ^ h >> 16) * 0x85EBCA6B) & 0xFFFFFFFF
    h = ((h ^ h >> 13) * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ h >> 16


def lattice_box(dims, tx, ty, tz, tile):
    """(x0, y0, z0) of the tile's lattice object: rows 2 ... 4 of the tile in y and z; in x two voxels or more from a face
    that the tile shares with another, the place by a hash of the tile index."""
    width = min(64, dims[0] - 64 * tx)
    xo = 0 if width < 5 else 2 if width < 8 else 2 + (_hash(tile) >> 4) % (width - 6)
    return 64 * tx + xo, 8 * ty + 2, 8 * tz + 2


_pools = {}


def pool_of(dx):
    """Two random objects of 13 x 11 x dx voxels at density 0.7.  Few, and the same for every grid, because each costs the
    reference 0.1 - 0.15 s per parity of its origin and mode; the placements - a few hundred, anywhere across the tiles - are what
    differs."""
    if dx not in _pools:
        rng = np.random.default_rng(1311 + dx)
        _pools[dx] = [rng.random((11, 13, dx)) < 0.7 for _ in range(2)]
    return _pools[dx]


def tile_chunks_objects(dims, cus, seed, randoms=240, lists=3, with_keep=False):
    """(objects, what): the set of a tile_chunks grid.  A lattice object from the palette in every tile, chosen by a hash of
    the tile index; random objects of 13 x 11 x min(nx, 4) voxels at density 0.7 from pool_of(), across the tiles' faces, edges
    and corners (at even x where the box is wider than the object) - first at every tile t * chunks + c of `lists` workgroups'
    lists, then anywhere.  A lattice object within two voxels of a random one gives way, and a random object is placed only where
    every tile that loses its lattice object holds one of its voxels.  what: the numbers a case prints."""
    nx, ny, nz = dims
    assert nx >= 3
    W, TY, TZ = tiles_of(dims)
    tiles = W * TY * TZ
    chunk, chunks, grid = plan(tiles, cus)
    rng = np.random.default_rng(seed)
    dx = min(nx, 4)
    shapes = pool_of(dx)
    pool = len(shapes)
    boxes, dropped, out = Boxes(), set(), []

    def place(A, x0, y0, z0):
        b = box_of((x0, y0, z0), A)
        if min(b[:3]) < 0 or b[3] > nx or b[4] > ny or b[5] > nz or boxes.near(b):
            return False
        gone = []
        for tz in range(max((b[2] - 2) // 8, 0), min((b[5] + 1) // 8, TZ - 1) + 1):
            for ty in range(max((b[1] - 2) // 8, 0), min((b[4] + 1) // 8, TY - 1) + 1):
                for tx in range(max((b[0] - 2) // 64, 0), min((b[3] + 1) // 64, W - 1) + 1):
                    tile = (tz * TY + ty) * W + tx
                    lx, ly, lz = lattice_box(dims, tx, ty, tz, tile)
                    lb = (lx, ly, lz, lx + min(3, nx), ly + 3, lz + 3)
                    if not all(b[a] - 2 < lb[a + 3] and lb[a] - 2 < b[a + 3] for a in range(3)):
                        continue
                    part = A[max(8 * tz - z0, 0):max(8 * tz + 8 - z0, 0), max(8 * ty - y0, 0):max(8 * ty + 8 - y0, 0), max(64 * tx - x0, 0):max(64 * tx + 64 - x0, 0)]
                    if not part.any():
                        return False
                    gone.append(tile)
        boxes.add(b)
        dropped.update(gone)
        out.append(((x0, y0, z0), A, None))
        return True

    def x_at():
        if nx <= dx:
            return 0
        if nx >= 64 + dx and rng.random() < 0.5:
            return 62                                           # across a word's end
        return 2 * int(rng.integers(0, (nx - dx) // 2 + 1))

    list_tiles = []
    for c in (0, chunks // 2, chunks - 1, 1, chunks // 3)[:lists]:
        for t in range(chunk):
            tile = t * chunks + c
            if tile >= tiles:
                continue
            list_tiles.append(tile)
            tx, rest = tile % W, tile // W
            ty, tz = rest % TY, rest // TY
            for _ in range(60):                                 # across one of the tile's corners in y and z
                y0 = min(max(8 * ty + (8 if rng.random() < 0.5 else 0) - int(rng.integers(3, 11)), 0), ny - 13)
                z0 = min(max(8 * tz + (8 if rng.random() < 0.5 else 0) - int(rng.integers(3, 9)), 0), nz - 11)
                if place(shapes[int(rng.integers(pool))], 62 if tx else x_at(), y0, z0):
                    break
    tries = 0
    while len(out) < randoms and tries < 40 * randoms:
        tries += 1
        place(shapes[int(rng.integers(pool))], x_at(), int(rng.integers(0, ny - 13 + 1)), int(rng.integers(0, nz - 11 + 1)))
    n_random = len(out)
    for tile in range(tiles):
        if tile in dropped:
            continue
        tx, rest = tile % W, tile // W
        ty, tz = rest % TY, rest // TY
        h = _hash(tile)
        i = h % len(PALETTE)
        out.append((lattice_box(dims, tx, ty, tz, tile), PALETTE[i], PALETTE_KEEP[i] if with_keep and h % 3 == 0 else None))
    hit = tiles_hit(dims, set_of(out[:n_random]))
    what = dict(tiles=tiles, chunk=chunk, chunks=chunks, grid=grid, random=n_random, lattice=len(out) - n_random, list_tiles=len(list_tiles),
                list_tiles_hit=sum(t in hit for t in list_tiles))
    return out, what


def tiles_with_candidates(dims, S):
    """bool per tile [tz, ty, tx]: does the tile hold a border voxel of S (a candidate of some sub-step of iteration 1)."""
    W, TY, TZ = tiles_of(dims)
    B = TR.border(S)
    P = np.zeros((8 * TZ, 8 * TY, 64 * W), bool)
    P[:dims[2], :dims[1], :dims[0]] = B
    return P.reshape(TZ, 8, TY, 8, W, 64).any(axis=(1, 3, 5))


# ---- grid_turns: planar objects in a box of one voxel along x ------------------------------------------------------------------------

def _planar():
    """Eight shapes [6, 6, 1] in the y-z plane: a full square, a plus, a ring with a spur, a diagonal band and random ones."""
    rng = np.random.default_rng(46340)
    full = np.ones((6, 6, 1), bool)
    plus = np.zeros((6, 6, 1), bool)
    plus[2:4, :, 0] = plus[:, 2:4, 0] = True
    ring = np.ones((6, 6, 1), bool)
    ring[2:4, 2:4, 0] = False
    band = np.zeros((6, 6, 1), bool)
    for i in range(6):
        band[i, max(i - 1, 0):i + 2, 0] = True
    some = [rng.random((6, 6, 1)) < 0.8 for _ in range(4)]
    for A in some:                                              # (every tile the shape may lie in gets a voxel: its four corners)
        A[0, 0] = A[0, 5] = A[5, 0] = A[5, 5] = True
    return [full, plus, ring, band] + some


PLANAR = _planar()


def grid_turns_objects(dims=GRID_TURNS_DIMS, cus=256, seed=5, randoms=300):
    """(objects, required tiles, what): planar objects of 6 x 6 voxels, each across the high corner of its tile in y and z (rows 5
    ... 10 from the tile's first; pulled in at the box's end): at the last row and column, in the first and the last tile, at
    every tile t * chunks + c of the chunks c taken in a second turn of the chunk loop, and at random tiles of the first turn.
    An object within two voxels of an earlier one is left out; required: the tiles that must hold a voxel all the same."""
    nx, ny, nz = dims
    assert nx == 1
    W, TY, TZ = tiles_of(dims)
    tiles = W * TY * TZ
    chunk, chunks, grid = plan(tiles, cus)
    rng = np.random.default_rng(seed)
    boxes, out = Boxes(), []

    def at(tile):
        ty, tz = tile % TY, tile // TY
        origin = (0, min(8 * ty + 5, ny - 6), min(8 * tz + 5, nz - 6))
        A = PLANAR[_hash(tile) % len(PLANAR)]
        b = box_of(origin, A)
        if boxes.near(b):
            return False
        boxes.add(b)
        out.append((origin, A, None))
        return True
    second = np.arange(grid, chunks, dtype=np.int64)
    required = [tiles - 1, 0] + [int(t * chunks + c) for c in second for t in range(chunk) if t * chunks + c < tiles]
    placed = sum(at(tile) for tile in required)
    n = 0
    while n < randoms:
        c, t = int(rng.integers(0, grid)), int(rng.integers(0, chunk))
        if t * chunks + c < tiles and at(t * chunks + c):
            n += 1
    what = dict(tiles=tiles, chunk=chunk, chunks=chunks, grid=grid, second_turn=len(second), required=len(required), placed=placed, random=n)
    return out, required, what


def tiles_hit(dims, placed):
    """The set of tiles that hold a voxel of the placements."""
    W, TY, TZ = tiles_of(dims)
    z, y, x = coords(placed)
    return set(np.unique(((z >> 3) * TY + (y >> 3)) * W + (x >> 6)).tolist())


# ---- long_axes: 65 536 voxels along an axis ----------------------------------------------------------------------------------------

LONG_AXIS = 65536
LONG_SEGMENTS = ((0, 40), (32759, 32777), (65452, 65492), (65496, 65536))


def long_axis_set(axis):
    """Four line segments along the axis ("x", "y", "z") at 1 on the other two, in a box of 65 536 x 3 x 3 turned that way: at both
    ends of the axis - coordinates that meet where 65 536 wraps to 0 - and across its middle."""
    S = np.zeros(TR.line(axis, LONG_AXIS).shape, bool)
    for lo, hi in LONG_SEGMENTS:
        S[{"x": (1, 1, slice(lo, hi)), "y": (1, slice(lo, hi), 1), "z": (slice(lo, hi), 1, 1)}[axis]] = True
    return S
