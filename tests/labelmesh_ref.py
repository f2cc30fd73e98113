"""The surface nets of a label grid (o2v_hip_label_surface_count / _write / _relax) in numpy, written from the contract in
include/o2v_hip.h and not from the kernels: the arbiter of tests/test_host_labelmesh.py (which checks it against closed forms) and
of tests/labelmesh_cases.py (which compares the GPU with it bit for bit, positions included).

Grids are [z, y, x] arrays as the torch layer takes them; cells, positions and origins are (x, y, z).  Two deliberate mutations of
the rules can be switched on (links="active", gauss_seidel=True); the host tests show a grid each that tells them from the rule."""
import numpy as np

INT32_MAX = 2 ** 31 - 1


def extended(labels, closed):
    """The labels of the extended lattice as int32 [Z, Y, X]: the box, and one layer of 0 around it if closed."""
    g = np.asarray(labels)
    assert g.ndim == 3 and g.dtype in (np.dtype(np.int32), np.dtype(np.uint8), np.dtype(bool)), g.dtype
    return np.pad(g.astype(np.int32), 1 if closed else 0)


def _differs(L, axes):
    """For every 2 x .. window along the array axes `axes` (1 along the others): its samples are not all equal."""
    out_shape = tuple(n - (1 if a in axes else 0) for a, n in enumerate(L.shape))
    first = L[tuple(slice(0, n) for n in out_shape)]
    out = np.zeros(out_shape, bool)
    for corner in range(1 << len(axes)):
        sl = [slice(0, n) for n in out_shape]
        for bit, a in enumerate(axes):
            if corner >> bit & 1:
                sl[a] = slice(1, out_shape[a] + 1)
        out |= L[tuple(sl)] != first
    return out


def net(labels, closed=True, links="face"):
    """(cells [V, 3], links [V, 6], faces [2 Q, 3], pairs [Q, 2]), all int32.  links="active" is the mutation "a link whenever the
    neighbouring cell is active"."""
    E = 1 if closed else 0
    L = extended(labels, closed)
    Z, Y, X = L.shape
    N = (X, Y, Z)
    active = _differs(L, (0, 1, 2))                      # [Z - 1, Y - 1, X - 1]; empty with a dim of 1
    kji = np.argwhere(active)                            # ascending (k, j, i)
    V = len(kji)
    number = np.full(active.shape, -1, np.int64)
    number[active] = np.arange(V)
    cells = (kji[:, ::-1] - E).astype(np.int32)
    lk = np.full((V, 6), -1, np.int32)
    if V:
        k, j, i = kji.T
        for ax in range(3):                              # x, y, z: array axis 2 - ax
            arr = 2 - ax
            others = tuple(a for a in range(3) if a != arr)
            face = _differs(L, others)                   # the faces across ax: index along arr is the sample's
            c = kji[:, arr]
            for side, step in ((0, -1), (1, 1)):
                there = c + step
                exists = (there >= 0) & (there <= N[ax] - 2)
                idx = [k.copy(), j.copy(), i.copy()]
                idx[arr] = np.where(exists, there, 0)
                fidx = [k, j, i]
                fidx[arr] = c + side                      # the face at the cell's lower / upper sample
                if links == "face":
                    ok = exists & face[tuple(fidx)]
                else:
                    assert links == "active"
                    ok = exists & active[tuple(idx)]
                lk[:, 2 * ax + side] = np.where(ok, number[tuple(idx)], -1)
    # quads
    zz, yy, xx = np.indices(L.shape)
    coord = (xx, yy, zz)
    keys, quads, pairs = [], [], []
    for ax in range(3):
        arr = 2 - ax
        u, v = (ax + 1) % 3, (ax + 2) % 3
        lo = tuple(slice(0, n - 1) if a == arr else slice(None) for a, n in enumerate(L.shape))
        hi = tuple(slice(1, n) if a == arr else slice(None) for a, n in enumerate(L.shape))
        d = np.zeros(L.shape, bool)
        d[lo] = L[lo] != L[hi]
        d &= (coord[u] >= 1) & (coord[u] <= N[u] - 2) & (coord[v] >= 1) & (coord[v] <= N[v] - 2)
        c = np.argwhere(d)[:, ::-1]                      # (x, y, z) of the edge's lower sample
        if not len(c):
            continue
        e = np.eye(3, dtype=np.int64)
        q = c + e[ax]
        cs = [c - e[u] - e[v], c - e[v], c, c - e[u]]
        n4 = [number[s[:, 2], s[:, 1], s[:, 0]] for s in cs]
        assert all((n >= 0).all() for n in n4)
        Lc, Lq = L[c[:, 2], c[:, 1], c[:, 0]], L[q[:, 2], q[:, 1], q[:, 0]]
        larger = Lc > Lq
        quads.append(np.stack([n4[0], np.where(larger, n4[1], n4[3]), n4[2], np.where(larger, n4[3], n4[1])], axis=1))
        pairs.append(np.stack([np.maximum(Lc, Lq), np.minimum(Lc, Lq)], axis=1))
        keys.append(((c[:, 2] * Y + c[:, 1]) * X + c[:, 0]) * 3 + ax)
    if keys:
        order = np.argsort(np.concatenate(keys), kind="stable")
        quads, pairs = np.concatenate(quads)[order], np.concatenate(pairs)[order]
        faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
    else:
        faces, pairs = np.zeros((0, 3), np.int64), np.zeros((0, 2), np.int64)
    return cells, lk, faces.astype(np.int32), pairs.astype(np.int32)


def centres(cells, origin=(0, 0, 0)):
    return (np.asarray(origin, np.int64)[None, :] + np.asarray(cells, np.int64) + 1).astype(np.float32)


def relax(cells, links, origin=(0, 0, 0), iterations=0, relaxation=0.5, reach=0.5, gauss_seidel=False):
    """positions float32 [V, 3] after `iterations` steps, op by op in float32.  gauss_seidel=True is the mutation "the update reads
    this iteration's positions"."""
    links = np.asarray(links, np.int64)
    centre = centres(cells, origin)
    V = len(centre)
    relaxation, reach = np.float32(relaxation), np.float32(reach)
    lo, hi = centre - reach, centre + reach
    p = centre.copy()
    valid = (links >= 0) & (links < V)                   # a link < 0 or >= V is no link
    m = valid.sum(axis=1)
    for _ in range(iterations):
        if gauss_seidel:
            for v in range(V):
                s = np.zeros(3, np.float32)
                for d in range(6):
                    if valid[v, d]:
                        s = s + p[links[v, d]]
                if m[v]:
                    r = p[v] + relaxation * (s / np.float32(m[v]) - p[v])
                    p[v] = np.minimum(np.maximum(r, lo[v]), hi[v])
            continue
        s = np.zeros((V, 3), np.float32)
        for d in range(6):
            ok = valid[:, d]
            s[ok] = s[ok] + p[links[ok, d]]
        some = m > 0
        avg = s[some] / m[some].astype(np.float32)[:, None]
        r = p[some] + relaxation * (avg - p[some])
        nxt = p.copy()
        nxt[some] = np.minimum(np.maximum(r, lo[some]), hi[some])
        p = nxt
    assert p.dtype == np.float32
    return p


def label_surfaces(labels, origin=(0, 0, 0), closed=True, iterations=0, relaxation=0.5, reach=0.5):
    """(positions, faces, pairs, cells, links) as dense.label_surfaces returns them in voxel space."""
    cells, links, faces, pairs = net(labels, closed)
    return relax(cells, links, origin, iterations, relaxation, reach), faces, pairs, cells, links


def part_faces(faces, pairs, label):
    """The triangles of the quads with `label` on either side, turned over where it is the smaller label; vertex numbers of the
    whole net."""
    hi, lo = pairs[:, 0] == label, pairs[:, 1] == label
    keep, turn = np.repeat(hi | lo, 2), np.repeat(lo & ~hi, 2)
    f = np.where(turn[:, None], faces[:, [0, 2, 1]], faces)
    return f[keep]


def part_mesh(positions, faces, pairs, label):
    f = part_faces(faces, pairs, label)
    used = np.unique(f)
    return positions[used], np.searchsorted(used, f).astype(np.int32)


def signed_volume(positions, faces):
    """The volume inside the triangles, by the divergence theorem, in float64."""
    p = np.asarray(positions, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def edge_uses(faces):
    """The undirected edges of the triangles and how many triangles use each: (edges [n, 2], counts [n])."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0, return_counts=True)


def quad_edges(faces):
    """The undirected edges of the quads (their diagonals left out), each once."""
    f = np.asarray(faces, np.int64)
    q = np.stack([f[0::2, 0], f[0::2, 1], f[0::2, 2], f[1::2, 2]], axis=1)
    e = np.concatenate([q[:, [0, 1]], q[:, [1, 2]], q[:, [2, 3]], q[:, [3, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0)


def link_edges(links):
    """The undirected edges the links describe, each once; every link must be answered by the opposite one."""
    links = np.asarray(links, np.int64)
    out = []
    for d in range(6):
        v = np.nonzero(links[:, d] >= 0)[0]
        assert (links[links[v, d], d ^ 1] == v).all(), "a link that is not answered"
        out.append(np.stack([v, links[v, d]], axis=1))
    e = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    return np.unique(np.sort(e, axis=1), axis=0)


def face_contacts(labels, closed=True):
    """{(hi, lo): the face-adjacent pairs of samples of the extended lattice with these labels} - with closed=True what the
    quads count per pair."""
    L = extended(labels, closed)
    out = {}
    for arr in range(3):
        lo = tuple(slice(0, n - 1) if a == arr else slice(None) for a, n in enumerate(L.shape))
        hi = tuple(slice(1, n) if a == arr else slice(None) for a, n in enumerate(L.shape))
        a, b = L[lo].reshape(-1), L[hi].reshape(-1)
        d = a != b
        pr, cnt = np.unique(np.stack([np.maximum(a, b)[d], np.minimum(a, b)[d]], axis=1), axis=0, return_counts=True)
        for (h, l), c in zip(pr.tolist(), cnt.tolist()):
            out[(h, l)] = out.get((h, l), 0) + c
    return out


def pair_counts(pairs):
    pr, cnt = np.unique(np.asarray(pairs), axis=0, return_counts=True)
    return {(int(h), int(l)): int(c) for (h, l), c in zip(pr, cnt)}


def random_labels(rng, dims, values=(0, 1, 2, 3), dtype=np.int32):
    """Random labels out of `values` on dims = (nx, ny, nz), as [z, y, x]."""
    nx, ny, nz = dims
    return np.asarray(values, np.int64)[rng.integers(0, len(values), (nz, ny, nx))].astype(dtype)
