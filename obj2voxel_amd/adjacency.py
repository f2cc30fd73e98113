"""Which labels of a label grid touch - the region adjacency graph - on the voxelizer's device (o2v_hip_adjacency_count / _write,
DESIGN.md section 27): the torch layer, which obj2voxel_amd.dense re-exports as dense.label_adjacency, dense.adjacency_neighbours,
dense.coordination and dense.skeleton_graph beside watershed.  It waits on the voxelizer's device (dense._sync) before the library
call, as every function of dense.py does; tests/test_host_adjacency.py holds that wait.

torch is imported first on purpose (see obj2voxel_amd/dense.py)."""
import dataclasses
import numbers

import torch  # first

from . import hip


@dataclasses.dataclass(frozen=True)
class LabelAdjacency:
    """What label_adjacency returns: row i of every tensor is for the pair pairs[i] = (a, b), a < b; the pairs are sorted by
    (a, b); on the grid's device, exact."""
    pairs: torch.Tensor       # int32 [m, 2]
    faces: torch.Tensor       # int64 [m]: contacts through a shared face - the contact area in voxel faces
    edges: torch.Tensor       # int64 [m]: contacts through a shared edge only (0 at connectivity 6)
    corners: torch.Tensor     # int64 [m]: contacts through a shared corner only (0 at connectivity 6 and 18)
    pass_high: torch.Tensor   # int32 [m]: the maximum over the contacts of min(values[u], values[v]); None without values
    pass_low: torch.Tensor    # int32 [m]: the minimum over the contacts of max(values[u], values[v]); None without values
    outside: int              # the voxels whose value is negative or above n: they touch nothing
    n: int                    # the highest label that takes part
    connectivity: int

    @property
    def contacts(self):
        """int64 [m]: faces + edges + corners."""
        return self.faces + self.edges + self.corners


def label_adjacency(dv, labels, n=None, *, connectivity=6, background=False, values=None):
    """Which labels touch, in one read of a label grid on the voxelizer's device: a LabelAdjacency with
    one row per pair of labels a < b that have a voxel each within one step of the other, and per pair the contacts by class.
    Everything is an integer and exact; one run equals another bit for bit.

        labels, n = dense.split_parts(dv, solid, min_depth=2)
        depth2 = dense.inner_distance(dv, solid)
        adj = dense.label_adjacency(dv, labels, n, connectivity=26, values=depth2)
        adj.pairs, adj.faces, adj.pass_high           # which parts touch, over what area, and the neck's squared depth

    labels:        int32, uint8 or bool, any 3-D view [z, y, x], as label_stats takes it; it is only read.
    n:             the highest label that takes part; None: 255 for uint8, 1 for bool, max(labels.max(), 0) for int32 (a device
                   reduction and a wait).  A voxel whose value is negative or above n is counted in `outside` and touches nothing.
    connectivity:  6: contacts through faces; 18: and through edges; 26: and through corners.  The three counts are exclusive:
                   a pair of voxels is counted once, by the number of axes on which it differs.
    background:    False: the value 0 touches nothing; True: it is a label like any other (pairs (0, b)).
    values:        None, or an int32 tensor of labels' shape (any strides): pass_high and pass_low are the two passes of this
                   relief between the labels - with the depth map of a solid, pass_high is the depth of the neck between two parts,
                   watershed's saddle."""
    from . import dense   # (at call time: dense imports this module)
    dense._require_shared_runtime()
    device = dense._device(dv)
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3:
        raise ValueError("labels must be a 3-D tensor [z, y, x]")
    if labels.dtype not in (torch.int32, torch.uint8, torch.bool):
        raise TypeError(f"labels must be int32, uint8 or bool, not {labels.dtype}")
    dense._check_grid(labels, "labels", labels.dtype, device)
    if 0 in labels.shape:
        raise ValueError("labels has an empty dimension")
    if isinstance(connectivity, bool) or connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity must be 6, 18 or 26, not {connectivity!r}")
    if not isinstance(background, bool):
        raise ValueError(f"background must be True or False, not {background!r}")
    nz, ny, nx = labels.shape
    dims = (nx, ny, nz)
    dense._limit_voxels(dims)
    if values is not None:
        if not isinstance(values, torch.Tensor):
            raise TypeError("values must be a torch.int32 tensor")
        dense._check_grid(values, "values", torch.int32, device, tuple(labels.shape))
    top = dense.MAX_STATS_LABELS if labels.dtype == torch.int32 else 1 if labels.dtype == torch.bool else 255
    if n is None:
        n = max(int(labels.max()), 0) if labels.dtype == torch.int32 else top
    elif isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 0 <= n <= top:
        raise ValueError(f"n must be an integer 0 ... {top} for {labels.dtype} labels, not {n!r}")
    n = int(n)
    dense._sync(device)   # (the caller's writes to labels and values have landed)
    m, outside = dv.adjacency_count(labels.data_ptr(), hip.LABELS_I32 if labels.dtype == torch.int32 else hip.LABELS_U8, dense._strides(labels), dims, n,
                                    connectivity, hip.ADJ_ZERO if background else 0, dense._ptr(values), None if values is None else dense._strides(values))
    pairs = torch.empty((m, 2), dtype=torch.int32, device=device)
    table = torch.empty((m, hip.ADJ_COLUMNS), dtype=torch.int64, device=device)
    dv.adjacency_write(pairs.data_ptr() if m else None, table.data_ptr() if m else None, m)
    with_values = values is not None
    return LabelAdjacency(pairs=pairs, faces=table[:, 0], edges=table[:, 1], corners=table[:, 2],
                          pass_high=table[:, 3].to(torch.int32) if with_values else None, pass_low=table[:, 4].to(torch.int32) if with_values else None,
                          outside=outside, n=n, connectivity=connectivity)


def _adjacency(adj):
    if not isinstance(adj, LabelAdjacency):
        raise TypeError("adj must be a LabelAdjacency, what label_adjacency returns")
    return adj


def adjacency_neighbours(adj):
    """The symmetric CSR form of a LabelAdjacency: (row_ptr int64 [n + 2], neighbour int32 [2 m], pair int64 [2 m]).  The neighbours
    of label L are neighbour[row_ptr[L]:row_ptr[L + 1]], ascending, and pair is the row of adj.pairs that each comes from.  Plain
    torch."""
    adj = _adjacency(adj)
    m, device = adj.pairs.shape[0], adj.pairs.device
    a, b = adj.pairs[:, 0].to(torch.int64), adj.pairs[:, 1].to(torch.int64)
    label, other = torch.cat([a, b]), torch.cat([b, a])
    index = torch.arange(m, dtype=torch.int64, device=device).repeat(2)
    order = torch.argsort(label * (adj.n + 1) + other)   # (keys are distinct: a pair is listed once)
    counts = torch.bincount(label, minlength=adj.n + 1)
    row_ptr = torch.zeros(adj.n + 2, dtype=torch.int64, device=device)
    row_ptr[1:] = torch.cumsum(counts, 0)
    return row_ptr, other[order].to(torch.int32), index[order]


def coordination(adj):
    """int64 [n + 1]: the number of distinct labels that each label touches.  Plain torch."""
    adj = _adjacency(adj)
    return torch.bincount(adj.pairs.reshape(-1).to(torch.int64), minlength=adj.n + 1)


@dataclasses.dataclass(frozen=True)
class SkeletonGraph:
    """What skeleton_graph returns: the nodes 1 ... n_nodes and the branches n_nodes + 1 ... n_nodes + n_branches of a skeleton."""
    labels: torch.Tensor          # int32 [z, y, x]: 0, a node's label or a branch's
    n_nodes: int
    n_branches: int
    node_voxels: torch.Tensor     # int64 [n_nodes]
    branch_voxels: torch.Tensor   # int64 [n_branches]
    incidence: torch.Tensor       # int32 [k, 2]: (node, branch - n_nodes) that touch, sorted
    node_contacts: torch.Tensor   # int32 [j, 2]: pairs of nodes that touch directly, sorted (none: nodes are 26-components, an end beside a
                                  # junction is one node with it)


def skeleton_graph(dv, degree):
    """The graph of a skeleton from skeletonize's fmt="degree" grid: a SkeletonGraph.

        degree = dense.skeletonize(dv, solid, fmt="degree")
        graph = dense.skeleton_graph(dv, degree)
        graph.incidence                               # which branch ends at which node

    Node voxels are the skeleton voxels whose degree is not 3 - isolated voxels, ends and junctions -, and their 26-components are
    the nodes 1 ... N: a cluster of junction voxels is one node.  Branch voxels are those of degree 3; their 26-components are the
    branches N + 1 ... N + B.  One int32 grid holds both; label_stats of it gives the sizes, label_adjacency(connectivity=26) the
    incidences.  A branch with no incidence is a closed loop; nothing is claimed about a branch having at most two nodes."""
    from . import dense
    device = dense._device(dv)
    if not isinstance(degree, torch.Tensor) or degree.dim() != 3 or degree.dtype != torch.uint8:
        raise ValueError("degree must be a 3-D torch.uint8 tensor [z, y, x]")
    dense._check_grid(degree, "degree", torch.uint8, device)
    if 0 in degree.shape:
        raise ValueError("degree has an empty dimension")
    nodes, n_nodes = dense.components(dv, (degree != 0) & (degree != 3), connectivity=26)
    branches, n_branches = dense.components(dv, degree == 3, connectivity=26)
    labels = torch.where(branches > 0, branches + n_nodes, nodes)
    n = n_nodes + n_branches
    count = dense.label_stats(dv, labels, n, box=False, sums=False).count
    adj = label_adjacency(dv, labels, n, connectivity=26)
    a, b = adj.pairs[:, 0], adj.pairs[:, 1]
    inc = (a <= n_nodes) & (b > n_nodes)
    incidence = torch.stack([a[inc], b[inc] - n_nodes], 1)
    return SkeletonGraph(labels=labels, n_nodes=n_nodes, n_branches=n_branches, node_voxels=count[1:n_nodes + 1], branch_voxels=count[n_nodes + 1:],
                         incidence=incidence, node_contacts=adj.pairs[b <= n_nodes])
