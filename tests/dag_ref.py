"""The numpy reference of the sparse voxel DAG (include/o2v_hip.h), for tests/test_host_dag.py and
tests/dag_cases.py.

The input is a tree as tests/octree_ref.py builds it (a dict).  build() merges level by level, bottom up, with np.unique(axis=0)
over the keys (valid, full, the eight children's new ids; -1 where no child is stored), the classes reordered by their first tree
index.  build_scalar() is a second construction: a walk over the nodes in index order with a dictionary per level, which numbers a
class when it first meets it.  lookup_one() is the descent as a scalar loop.  `listed` and `skip` are uint32 arithmetic, kept in
int32 arrays; grids are [z, y, x], coordinates (x, y, z)."""
import numpy as np

from tests import octree_ref as R

U32 = 0xffffffff


def _stored(valid, full, collapsed):
    return (valid & ~full) if collapsed else valid


def _bits(m):
    """[n, 8] bool: bit o of each mask"""
    return ((np.asarray(m, np.uint8)[:, None] >> np.arange(8, dtype=np.uint8)) & 1).astype(bool)


def _offsets(counts):
    return [int(v) for v in np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))])]


def _children(t, l, off):   # noqa: E741
    """Of the nodes of level l < D - 1: (bits [n, 8], child [n, 8]: the stored children's indices within level l + 1, 0 where none).
    A stored child outside level l + 1 is a ValueError: the arrays are not a tree of these level counts."""
    a, b = off[l], off[l + 1]
    m = _stored(t["valid"][a:b], t["full"][a:b], t["collapsed"])
    bits = _bits(m)
    rank = np.cumsum(bits, 1) - bits
    child = t["first_child"][a:b].astype(np.int64)[:, None] + rank
    bad = bits & ((child < off[l + 1]) | (child >= off[l + 2]))
    if bad.any():
        raise ValueError("the arrays are not a tree of these level counts: node %d" % (a + int(np.argwhere(bad)[0, 0])))
    return bits, np.where(bits, child - off[l + 1], 0)


def _take(a, c):
    """a[c], 0 where the level a speaks of has no nodes (then no child is stored and the entry is masked away)"""
    return a[c] if len(a) else np.zeros(c.shape, a.dtype)


def _assemble(t, off, ids, listed):
    """The DAG's arrays from the class (rank within its level) and the listed voxels of every tree node."""
    D, collapsed = t["depth"], t["collapsed"]
    counts = [int(i.max()) + 1 if len(i) else 0 for i in ids]
    doff = _offsets(counts)
    valid, full, first, child, skip = [], [], [], [], []
    P = 0
    for l in range(D):   # noqa: E741
        a = off[l]
        rep = a + np.unique(ids[l], return_index=True)[1]   # the first member of class 0, 1, ...
        valid.append(t["valid"][rep]), full.append(t["full"][rep])
        if l == D - 1:
            first.append(np.full(len(rep), -1, np.int64))
            continue
        bits, c = _children(t, l, off)
        bits, c = bits[rep - a], c[rep - a]
        n = bits.sum(1)
        first.append(np.where(n > 0, P + np.cumsum(n) - n, -1))
        P += int(n.sum())
        below = np.where(bits, _take(listed[l + 1], c), 0).astype(np.uint64)
        child.append((doff[l + 1] + _take(ids[l + 1], c))[bits])
        skip.append(((np.cumsum(below, 1) - below) & np.uint64(U32))[bits])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)   # noqa: E731
    return dict(valid=cat(valid, np.uint8), full=cat(full, np.uint8), first_child=cat(first, np.int32), child=cat(child, np.int32),
                skip=cat(skip, np.uint32).view(np.int32), level_counts=counts, depth=D, collapsed=bool(collapsed), voxels_listed=t["voxels_listed"],
                tree_nodes=len(t["valid"]), classes=np.concatenate([doff[l] + ids[l] for l in range(D)]).astype(np.int64))   # classes: the DAG node of every tree node


def build(t):
    """dict(valid, full uint8 [M]; first_child int32 [M]; child, skip int32 [P]; level_counts [D]; depth; collapsed; voxels_listed;
    tree_nodes) of the tree t, with np.unique per level."""
    D = t["depth"]
    off = _offsets(t["level_counts"])
    assert off[-1] == len(t["valid"]) and len(off) == D + 1
    ids, listed = [None] * D, [None] * D
    for l in range(D - 1, -1, -1):   # noqa: E741
        a, b = off[l], off[l + 1]
        v, f = t["valid"][a:b].astype(np.int64), t["full"][a:b].astype(np.int64)
        if l == D - 1:
            keys = v[:, None]
            listed[l] = R.popcount8(t["valid"][a:b]).astype(np.uint64)
        else:
            bits, c = _children(t, l, off)
            keys = np.concatenate([v[:, None], f[:, None], np.where(bits, _take(ids[l + 1], c), -1)], 1)
            listed[l] = np.where(bits, _take(listed[l + 1], c), 0).astype(np.uint64).sum(1) & np.uint64(U32)
        if b == a:
            ids[l] = np.zeros(0, np.int64)
            continue
        _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
        rank = np.empty(len(first), np.int64)
        rank[np.argsort(first)] = np.arange(len(first))   # the classes by their smallest member
        ids[l] = rank[inverse.reshape(-1)]
    return _assemble(t, off, ids, listed)


def build_scalar(t):
    """The same DAG by a walk over the nodes in index order: a class is numbered when it is first met."""
    D, collapsed = t["depth"], t["collapsed"]
    off = _offsets(t["level_counts"])
    ids, listed = [None] * D, [None] * D
    for l in range(D - 1, -1, -1):   # noqa: E741
        seen, ids[l], listed[l] = {}, np.zeros(off[l + 1] - off[l], np.int64), np.zeros(off[l + 1] - off[l], np.uint64)
        for i in range(off[l], off[l + 1]):
            v, f = int(t["valid"][i]), int(t["full"][i])
            if l == D - 1:
                key, n = (v,), bin(v).count("1")
            else:
                m = v & ~f & 255 if collapsed else v
                kids = [int(t["first_child"][i]) + bin(m & ((1 << o) - 1)).count("1") - off[l + 1] for o in range(8) if (m >> o) & 1]
                key = (v, f) + tuple(int(ids[l + 1][c]) for c in kids)
                n = sum(int(listed[l + 1][c]) for c in kids) & U32
            ids[l][i - off[l]] = seen.setdefault(key, len(seen))
            listed[l][i - off[l]] = n
    return _assemble(t, off, ids, listed)


def lookup_one(d, x, y, z, skips=True):
    """the descent: (solid, level, node, voxel_index)"""
    D, M, P = d["depth"], len(d["valid"]), len(d["child"])
    skips = skips or P == 0   # (a DAG without pointers has nothing to skip)
    if not (0 <= x < 2 ** D and 0 <= y < 2 ** D and 0 <= z < 2 ** D):
        return (0, -1, -1, -1)
    i, acc = 0, 0
    for l in range(D):   # noqa: E741
        s = D - 1 - l
        o = ((x >> s) & 1) | ((y >> s) & 1) << 1 | ((z >> s) & 1) << 2
        v, f = int(d["valid"][i]), int(d["full"][i])
        if not (v >> o) & 1:
            return (0, l, i, -1)
        if l == D - 1:
            slot = (acc + bin(v & ((1 << o) - 1)).count("1")) & U32
            return (1, l, i, slot - (1 << 32) if slot >> 31 else slot) if skips else (1, l, i, -1)
        if d["collapsed"] and (f >> o) & 1:
            return (1, l, i, -1)
        m = v & ~f & 255 if d["collapsed"] else v
        fc = int(d["first_child"][i])
        e = fc + bin(m & ((1 << o) - 1)).count("1")
        if fc < 0 or not 0 <= e < P:
            return (0, -2, -1, -1)
        if skips:
            acc = (acc + (int(d["skip"][e]) & U32)) & U32
        i = int(d["child"][e])
        if not 0 <= i < M:
            return (0, -2, -1, -1)
    raise AssertionError("unreachable")


def lookup(d, points, skips=True):
    points = np.asarray(points).reshape(-1, 3)
    return np.array([lookup_one(d, int(x), int(y), int(z), skips) for x, y, z in points], np.int32).reshape(-1, 4)


def to_dense(d, shape, origin=(0, 0, 0)):
    """bool [nz, ny, nx]: the descent's `solid` for every voxel of the box"""
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz) + origin[2], np.arange(ny) + origin[1], np.arange(nx) + origin[0], indexing="ij")
    return lookup(d, np.stack([x, y, z], -1).reshape(-1, 3), skips=False)[:, 0].reshape(shape).astype(bool)


def same(got, want, what=""):
    """every field of two DAGs bit for bit"""
    assert got["depth"] == want["depth"] and list(got["level_counts"]) == list(want["level_counts"]), (what, got["depth"], got["level_counts"], want["level_counts"])
    for k in ("valid", "full", "first_child", "child", "skip"):
        if got[k] is None:
            continue
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, a.shape, b.dtype, b.shape)
        bad = np.argwhere(a != b)
        assert not len(bad), (what, k, len(bad), "differ, the first at", bad[0].tolist(), a[tuple(bad[0])].tolist(), b[tuple(bad[0])].tolist())


def nbytes(d):
    """valid, full, first_child: 6 bytes per node; child, skip: 8 per pointer"""
    return 6 * len(d["valid"]) + 8 * len(d["child"])


def two_balls():
    return np.concatenate([R.ball(), R.ball()], axis=2)
