"""The numpy reference of the label surface nets (tests/labelmesh_ref.py) against closed forms, without a GPU: what the GPU cases
of tests/test_gpu_labelmesh.py compare the kernels with must itself be right.  Two mutations of the reference's rules - links
wherever the neighbouring cell is active, an update that reads this iteration's positions - are each told from the rule by a named
grid."""
import numpy as np
import pytest

from tests import labelmesh_ref as R


def grid(nx, ny, nz, dtype=np.int32):
    return np.zeros((nz, ny, nx), dtype)


def single_voxel():
    return np.ones((1, 1, 1), np.int32)


def uniform_face():
    """3 x 2 x 2, read open: the cells i = 0 and i = 1 are both active, the four samples at x = 1 that they share are all equal."""
    g = grid(3, 2, 2)
    g[0, 0, 0] = 1
    g[1, 1, 2] = 1
    return g


def hollow_box():
    g = np.ones((10, 10, 10), np.uint8)
    g[1:9, 1:9, 1:9] = 0
    return g


def test_single_voxel():
    cells, links, faces, pairs = R.net(single_voxel())
    assert len(cells) == 8 and len(pairs) == 6 and faces.shape == (12, 3)
    assert sorted(map(tuple, cells.tolist())) == sorted((i, j, k) for k in (-1, 0) for j in (-1, 0) for i in (-1, 0))
    assert cells.tolist() == [[i, j, k] for k in (-1, 0) for j in (-1, 0) for i in (-1, 0)]      # ascending (k, j, i)
    assert (pairs == [1, 0]).all()
    edges, uses = R.edge_uses(faces)
    assert len(edges) == 18 and (uses == 2).all()                                                # 12 cube edges and 6 diagonals
    assert ((links >= 0).sum(axis=1) == 3).all()
    assert R.signed_volume(R.centres(cells), faces) == 1.0                                       # outward normals
    # open, a single voxel has no cell at all
    assert [len(a) for a in R.net(single_voxel(), closed=False)] == [0, 0, 0, 0]


def test_hollow_box_and_two_voxels():
    cells, links, faces, pairs = R.net(hollow_box())
    assert len(pairs) == 984 and R.pair_counts(pairs) == {(1, 0): 984}
    assert len(cells) == 11 ** 3 - 9 ** 3 + 9 ** 3 - 7 ** 3
    two = grid(2, 1, 1)
    two[0, 0] = [1, 2]
    cells, links, faces, pairs = R.net(two)
    assert len(cells) == 12 and len(pairs) == 11
    assert R.pair_counts(pairs) == {(1, 0): 5, (2, 0): 5, (2, 1): 1}
    # the wall: normal from label 2 (at x = 1) to label 1, that is towards -x
    n = int(np.nonzero((pairs == [2, 1]).all(axis=1))[0][0])
    p = R.centres(cells)[faces[2 * n]]
    assert np.cross(p[1] - p[0], p[2] - p[0]).tolist() == [-1.0, 0.0, 0.0]


def test_three_labels_share_an_edge():
    g = grid(2, 2, 1)
    g[0] = [[1, 2], [3, 3]]
    cells, links, faces, pairs = R.net(g)
    f = faces.astype(np.int64)
    q = np.stack([f[0::2, 0], f[0::2, 1], f[0::2, 2], f[1::2, 2]], axis=1)
    e = np.sort(np.concatenate([q[:, [0, 1]], q[:, [1, 2]], q[:, [2, 3]], q[:, [3, 0]]]), axis=1)
    edges, uses = np.unique(e, axis=0, return_counts=True)
    assert uses.max() == 3                                                                       # (also where a wall meets the outer skin)
    v = {tuple(c): n for n, c in enumerate(cells.tolist())}
    a, b = v[(0, 0, -1)], v[(0, 0, 0)]                                                           # the line the three parts meet in
    assert uses[(edges == [a, b]).all(axis=1)].tolist() == [3]
    around = [tuple(pr) for pr, quad in zip(pairs.tolist(), q.tolist()) if a in quad and b in quad]
    assert sorted(around) == [(2, 1), (3, 1), (3, 2)]
    # per label every edge is still used an even number of times
    for label in (1, 2, 3):
        assert (R.edge_uses(R.part_faces(faces, pairs, label))[1] % 2 == 0).all()


@pytest.mark.parametrize("closed", [True, False])
def test_random_grids(closed):
    rng = np.random.default_rng(2901)
    for values in ((0, 1, 2, 3), (0, 7, R.INT32_MAX, -5)):
        g = R.random_labels(rng, (5, 6, 7), values)
        cells, links, faces, pairs = R.net(g, closed)
        assert np.array_equal(R.link_edges(links), R.quad_edges(faces)) or not closed            # (open: a border vertex may have links and no quad)
        assert set(map(tuple, R.quad_edges(faces).tolist())) <= set(map(tuple, R.link_edges(links).tolist()))
        assert (pairs[:, 0] > pairs[:, 1]).all()
        if not closed:
            continue
        assert R.pair_counts(pairs) == R.face_contacts(g)
        pos = R.centres(cells, (3, 0, 9))
        for label in values:
            f = R.part_faces(faces, pairs, label)
            assert (R.edge_uses(f)[1] % 2 == 0).all(), label
            if label:
                assert R.signed_volume(pos, f) == float((g == label).sum()), label
            p, pf = R.part_mesh(pos, faces, pairs, label)
            assert len(p) == len(np.unique(f)) and np.array_equal(p[pf], pos[f])


def test_dtypes_agree():
    rng = np.random.default_rng(2902)
    g = R.random_labels(rng, (4, 3, 5), (0, 1))
    want = R.net(g)
    for other in (g.astype(np.uint8), g.astype(bool)):
        assert all(np.array_equal(a, b) for a, b in zip(R.net(other), want))
    big = g.astype(np.uint8) * 200                                                               # (200 as uint8 is 200, not -56)
    assert R.pair_counts(R.net(big)[3]) == {(200, 0): R.pair_counts(want[3])[(1, 0)]}


def test_links_need_a_face_that_differs():
    g = uniform_face()
    cells, links, faces, pairs = R.net(g, closed=False)
    assert cells.tolist() == [[0, 0, 0], [1, 0, 0]] and (links == -1).all() and len(pairs) == 0
    mutant = R.net(g, closed=False, links="active")[1]
    assert mutant[0, 1] == 1 and mutant[1, 0] == 0                                               # the mutation links them
    # closed, the same two cells are still not linked, though each has other links
    cells, links, faces, pairs = R.net(g)
    v = {tuple(c): n for n, c in enumerate(cells.tolist())}
    assert links[v[(0, 0, 0)], 1] == -1 and links[v[(1, 0, 0)], 0] == -1
    assert not np.array_equal(links, R.net(g, links="active")[1])


def test_relaxation_of_the_single_voxel():
    cells, links, faces, pairs = R.net(single_voxel())
    o = (4, 0, 2)
    c = R.centres(cells, o)
    assert c.dtype == np.float32 and c[0].tolist() == [4.0, 0.0, 2.0] and c[7].tolist() == [5.0, 1.0, 3.0]
    assert np.array_equal(R.relax(cells, links, o, 0), c)
    third = np.float32(1) / np.float32(3)
    one = R.relax(cells, links, o, 1, relaxation=1.0)
    inward = np.where(cells == -1, 1.0, -1.0).astype(np.float32)
    assert np.allclose(one, c + inward * third, atol=1e-6, rtol=0)                               # a corner sits 1/3 inside on every axis
    assert R.relax(cells, links, (0, 0, 0), 1, relaxation=1.0)[0].tolist() == [float(third)] * 3  # ... to the bit where the centre is 0
    two = R.relax(cells, links, o, 2, relaxation=1.0)
    assert np.allclose(two, c + inward * np.float32(4 / 9), atol=1e-6, rtol=0)
    # reach 0.25: the clamp binds in the first step, and the voxel stays at half its size
    for n in (1, 50):
        assert np.array_equal(R.relax(cells, links, o, n, relaxation=1.0, reach=0.25), c + inward * np.float32(0.25))
    # reach 0.5: the eight vertices meet in the voxel's centre, never past it
    many = R.relax(cells, links, o, 200, relaxation=0.5)
    assert (np.abs(many - c) <= 0.5).all() and np.allclose(many, np.array(o, np.float32) + 0.5, atol=1e-5, rtol=0)
    # ... and the clamp binds at 0.5 where a vertex has a single link: the open 2 x 2 x 3 column of two labels
    g = grid(2, 2, 3)
    g[1:, 0, 0] = 1
    g[2, 1, 1] = 2
    cells, links, faces, pairs = R.net(g, closed=False)
    assert cells.tolist() == [[0, 0, 0], [0, 0, 1]] and links.tolist() == [[-1, -1, -1, -1, -1, 1], [-1, -1, -1, -1, 0, -1]]
    got = R.relax(cells, links, (0, 0, 0), 3, relaxation=1.0)
    assert got.tolist() == [[1.0, 1.0, 1.5], [1.0, 1.0, 1.5]]


def test_the_update_is_jacobi():
    cells, links, faces, pairs = R.net(single_voxel())
    jacobi = R.relax(cells, links, (0, 0, 0), 1, relaxation=1.0)
    seidel = R.relax(cells, links, (0, 0, 0), 1, relaxation=1.0, gauss_seidel=True)
    assert np.array_equal(jacobi[0], seidel[0]) and not np.array_equal(jacobi, seidel)           # the first vertex agrees, later ones saw moved neighbours
    # Jacobi keeps the voxel's symmetry, the mutation does not
    assert np.array_equal(jacobi + jacobi[::-1], np.ones((8, 3), np.float32)) and not np.array_equal(seidel + seidel[::-1], np.ones((8, 3), np.float32))


def test_links_from_anywhere():
    cells = np.array([[0, 0, 0], [1, 0, 0], [5, 5, 5]], np.int32)
    links = np.array([[-2, 1, 3, 99, -1, R.INT32_MAX], [0, -1, -1, -1, -1, -1], [-1, -7, 3, 3, 3, 3]], np.int32)
    got = R.relax(cells, links, (0, 0, 0), 1, relaxation=1.0)
    assert got.tolist() == [[1.5, 1.0, 1.0], [1.5, 1.0, 1.0], [6.0, 6.0, 6.0]]                    # 3 and above: no link; vertex 2 stays


def test_the_ball_gets_rounder():
    z, y, x = np.indices((13, 13, 13))
    ball = ((x - 6) ** 2 + (y - 6) ** 2 + (z - 6) ** 2 <= 20).astype(np.uint8)
    cells, links, faces, pairs = R.net(ball)
    spread = []
    for n in (0, 4):
        p = R.relax(cells, links, (0, 0, 0), n)
        spread.append(float(np.std(np.linalg.norm(p - 6.5, axis=1))))
        assert (np.abs(p - R.centres(cells)) <= 0.5).all()
    assert spread[1] < 0.5 * spread[0], spread


def test_part_mesh_and_interface_areas_in_torch():
    """The two plain-torch functions of obj2voxel_amd.labelmesh on the reference's net, on the host."""
    import torch  # first

    from obj2voxel_amd import dense
    rng = np.random.default_rng(2903)
    g = R.random_labels(rng, (6, 5, 4), (0, 1, 2, -4))
    positions, faces, pairs, cells, links = R.label_surfaces(g, (1, 2, 3), iterations=2)
    mesh = dense.LabelMesh(*(torch.from_numpy(a) for a in (positions, faces, pairs, cells, links)), origin=(1, 2, 3))
    for label in (0, 1, 2, -4, 9):
        p, f = dense.part_mesh(mesh, label)
        want_p, want_f = R.part_mesh(positions, faces, pairs, label)
        assert p.dtype == torch.float32 and f.dtype == torch.int32 and p.is_contiguous() and f.is_contiguous()
        assert np.array_equal(p.numpy(), want_p.reshape(-1, 3)) and np.array_equal(f.numpy(), want_f.reshape(-1, 3)), label
    blocky = dense.LabelMesh(torch.from_numpy(R.centres(cells)), mesh.faces, mesh.pairs, mesh.cells, mesh.links)
    got_pairs, areas = dense.interface_areas(blocky)
    counts = R.pair_counts(pairs)
    assert got_pairs.dtype == torch.int32 and areas.dtype == torch.float64
    assert [tuple(p) for p in got_pairs.tolist()] == sorted(counts) and areas.tolist() == [float(counts[k]) for k in sorted(counts)]
    _, smooth = dense.interface_areas(mesh)
    assert float(smooth.sum()) < float(areas.sum())
    empty = dense.LabelMesh(*(torch.zeros((0, w), dtype=d) for w, d in ((3, torch.float32), (3, torch.int32), (2, torch.int32), (3, torch.int32), (6, torch.int32))))
    assert [tuple(t.shape) for t in dense.interface_areas(empty)] == [(0, 2), (0,)] and [tuple(t.shape) for t in dense.part_mesh(empty, 1)] == [(0, 3), (0, 3)]
    with pytest.raises(TypeError):
        dense.part_mesh((positions, faces), 1)
    with pytest.raises(ValueError):
        dense.part_mesh(mesh, 2 ** 31)
