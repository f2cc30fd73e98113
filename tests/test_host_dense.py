"""obj2voxel_amd.dense without a GPU: the argument checks of the torch layer and its z-slab loop, with the device calls
stubbed; the wait for torch's stream in front of every function's first library call that takes a tensor; and a static check of
the K7 kernels in the gfx950 code object (hipcc cross-compiles)."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "obj2voxel_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CPU = torch.device("cpu")


class StubVoxelizer:
    """Records the device calls dense.py makes.  voxelize returns `n` records per slab with box [lo, hi)."""

    def __init__(self, n=10, layers=1 << 30, lo=(1, 2, 3), hi=(5, 6, 7), outside=0, interior=0):
        self.device, self.calls, self.n, self.layers = None, [], n, layers
        self.lo, self.hi, self.outside, self.interior = lo, hi, outside, interior
        self.count = 0

    def set_triangles_device(self, *args):
        self.calls.append(("set", args))

    def max_slab_layers(self, resolution, **kw):
        return self.layers

    def plan_slabs(self, resolution, n, **kw):
        self.calls.append(("plan", resolution))
        return [0, resolution], np.zeros(6, np.float32)

    def voxelize(self, resolution, *, zslab, read, **kw):
        self.calls.append(("voxelize", zslab, kw.get("fill")))
        self.count = self.n
        return self.n

    def voxels_box(self):
        return self.lo, self.hi

    def stats(self):
        return {"interior_voxels": self.interior}

    def write_dense(self, ptr, fmt, origin, dims, strides):
        self.calls.append(("write", fmt, tuple(origin), tuple(dims), tuple(strides)))
        return self.outside

    # the entry points of the other families: their names go to `calls`; the counts are `n`
    def distance_dense(self, *args):
        self.calls.append(("distance",))

    def mesh_distance_dense(self, *args, **kw):
        self.calls.append(("mesh_distance",))

    def surface_count(self, *args):
        self.calls.append(("surface_count",))
        return self.n, self.n

    def surface_write(self, *args):
        self.calls.append(("surface_write",))

    def raycast_build(self, *args):
        self.calls.append(("raycast_build",))
        return 7

    def raycast_generation(self):
        return 7

    def raycast(self, *args):
        self.calls.append(("raycast",))

    def components_dense(self, grid_ptr, fmt, strides, dims, level, connectivity, flags, labels_ptr, label_strides):
        self.calls.append(("components",))
        C.memset(labels_ptr, 0, 4 * dims[0] * dims[1] * dims[2])   # (a new contiguous tensor: every voxel background)
        return 0

    def flood_dense(self, *args):
        self.calls.append(("flood",))

    def gather_count(self, *args):
        self.calls.append(("gather_count",))
        return self.n

    def gather_write(self, *args):
        self.calls.append(("gather_write",))

    def gather_save(self, *args):
        self.calls.append(("gather_save",))
        return self.n

    def faces_count(self, *args):
        self.calls.append(("faces_count",))
        return self.n

    def faces_write(self, *args):
        self.calls.append(("faces_write",))

    def nearest_dense(self, *args):
        self.calls.append(("nearest",))

    def downsample(self, *args):
        self.calls.append(("downsample",))

    def crossings_dense(self, *args, **kw):
        self.calls.append(("crossings",))

    def label_stats(self, labels_ptr, fmt, strides, dims, origin, n, which, table_ptr):
        self.calls.append(("label_stats",))
        C.memset(table_ptr, 0, 8 * (n + 1) * hip.STATS_COLUMNS)   # (a new contiguous table: no voxel counted)
        return 0

    def geodesic_dense(self, *args):
        self.calls.append(("geodesic",))

    def geodesic_paths(self, *args):
        self.calls.append(("geodesic_paths",))

    def thickness_dense(self, *args):
        self.calls.append(("thickness",))


# the stub's calls that hand a tensor's pointer to the library
POINTER_CALLS = {"set", "write", "distance", "mesh_distance", "surface_count", "surface_write", "raycast_build", "raycast", "components", "flood",
                 "gather_count", "gather_write", "gather_save", "faces_count", "faces_write", "nearest", "downsample", "crossings", "label_stats",
                 "geodesic", "geodesic_paths", "thickness"}


@pytest.fixture(autouse=True)
def on_cpu(monkeypatch):
    monkeypatch.setattr(dense, "_device", lambda dv: CPU)
    monkeypatch.setattr(dense, "_sync", lambda device: None)
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: True)


def test_set_mesh_indexed_and_flat():
    dv = StubVoxelizer()
    p, f = torch.zeros((5, 3)), torch.zeros((4, 3), dtype=torch.int64)
    dense.set_mesh(dv, p, f, types=torch.zeros(4, dtype=torch.int32))
    _, args = dv.calls[-1]
    assert args[1] == 5 and args[3] == 8 and args[4] == 4 and args[6] is not None and args[5] is None
    dense.set_mesh(dv, torch.zeros((4, 9)), colors=torch.zeros((4, 3)))
    _, args = dv.calls[-1]
    assert args[2] is None and args[3] == 0 and args[4] == 4 and args[7] is not None
    # a non-contiguous view is made contiguous
    dense.set_mesh(dv, torch.zeros((3, 5)).t(), f.to(torch.int32))
    assert dv.calls[-1][1][3] == 4


@pytest.mark.parametrize("bad, exc", [
    (dict(positions=torch.zeros((5, 3), dtype=torch.float64)), TypeError),
    (dict(positions=torch.zeros((5, 4))), ValueError),
    (dict(faces=torch.zeros((4, 3), dtype=torch.int16)), TypeError),
    (dict(faces=torch.zeros((4, 2), dtype=torch.int32)), ValueError),
    (dict(uvs=torch.zeros((3, 6))), ValueError),
    (dict(types=torch.zeros(4, dtype=torch.int64)), TypeError),
    (dict(colors=torch.zeros((4, 4))), ValueError),
    (dict(texids=torch.zeros((4, 1), dtype=torch.int32)), ValueError),
    (dict(positions=np.zeros((5, 3), np.float32)), TypeError),
])
def test_set_mesh_rejects(bad, exc):
    kw = dict(positions=torch.zeros((5, 3)), faces=torch.zeros((4, 3), dtype=torch.int32))
    kw.update(bad)
    dv = StubVoxelizer()
    with pytest.raises(exc):
        dense.set_mesh(dv, kw.pop("positions"), kw.pop("faces"), **kw)
    assert not dv.calls


def test_set_mesh_refuses_a_device_mismatch(monkeypatch):
    monkeypatch.setattr(dense, "_device", lambda dv: torch.device("cuda", 1))
    with pytest.raises(ValueError, match="voxelizer"):
        dense.set_mesh(StubVoxelizer(), torch.zeros((5, 3)), torch.zeros((4, 3), dtype=torch.int32))


def test_refused_when_the_library_came_first(monkeypatch):
    monkeypatch.setattr(hip, "torch_was_loaded_first", lambda: False)
    with pytest.raises(RuntimeError, match="before torch"):
        dense.voxelize_dense(StubVoxelizer(), 8)
    with pytest.raises(RuntimeError, match="before torch"):
        dense.set_mesh(StubVoxelizer(), torch.zeros((1, 9)))


@pytest.mark.parametrize("fmt, dtype, shape", [("occupancy", torch.bool, (16, 16, 16)), ("labels", torch.uint8, (16, 16, 16)),
                                               ("argb", torch.int32, (16, 16, 16)), ("bits", torch.int32, (16, 16, 1))])
def test_default_tensors(fmt, dtype, shape):
    dv = StubVoxelizer()
    t, origin = dense.voxelize_dense(dv, 16, fmt=fmt)
    assert t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and origin == (0, 0, 0)
    w = [c for c in dv.calls if c[0] == "write"]
    assert len(w) == 1
    _, code, o, dims, strides = w[0]
    assert code == dense.FORMATS[fmt][0] and o == (0, 0, 0)
    assert dims == (16, 16, 16)
    assert strides == (1, shape[2], shape[1] * shape[2])


def test_tight_box_and_out_views():
    dv = StubVoxelizer(lo=(1, 2, 3), hi=(5, 8, 12))
    t, origin = dense.voxelize_dense(dv, 16, box="tight")
    assert origin == (1, 2, 3) and tuple(t.shape) == (9, 6, 4)
    assert [c[0] for c in dv.calls] == ["voxelize", "write"]   # (one pass: its records are written without a second run)
    batch = torch.zeros((2, 16, 16, 16), dtype=torch.uint8)
    dv = StubVoxelizer()
    out, _ = dense.voxelize_dense(dv, 16, fmt="labels", out=batch[1].permute(1, 0, 2))
    assert out.data_ptr() == batch[1].data_ptr()
    assert dv.calls[-1][4] == (1, 256, 16)


@pytest.mark.parametrize("kw, exc", [
    (dict(fmt="rgb"), ValueError), (dict(box="loose"), ValueError), (dict(strategy="min"), ValueError),
    (dict(supersampling=3), ValueError), (dict(resolution=40000, supersampling=2), ValueError),
    (dict(resolution=65536), ValueError), (dict(box="tight", origin=(0, 0, 0)), ValueError), (dict(max_layers=0), ValueError),
    (dict(out=torch.zeros((16, 16), dtype=torch.bool)), ValueError), (dict(out=torch.zeros((16, 16, 16), dtype=torch.uint8)), TypeError),
    (dict(fmt="bits", out=torch.zeros((16, 1, 16), dtype=torch.int32).permute(0, 2, 1)), ValueError),
    (dict(fmt="argb", out=torch.zeros((16, 16, 16), dtype=torch.float32)), TypeError),
])
def test_voxelize_dense_rejects(kw, exc):
    dv = StubVoxelizer()
    res = kw.pop("resolution", 16)
    with pytest.raises(exc):
        dense.voxelize_dense(dv, res, **kw)
    assert not [c for c in dv.calls if c[0] in ("voxelize", "write")]


def test_records_outside_the_tensor_raise():
    with pytest.raises(ValueError, match="outside"):
        dense.voxelize_dense(StubVoxelizer(outside=3), 16)


def test_slabs_cover_the_grid_once():
    dv = StubVoxelizer(layers=1 << 20, interior=5)
    t, _ = dense.voxelize_dense(dv, 30, max_layers=9, fill=True)
    vox = [c[1] for c in dv.calls if c[0] == "voxelize"]
    assert vox == [(0, 8), (8, 16), (16, 24), (24, 30)]
    assert len([c for c in dv.calls if c[0] == "write"]) == 4
    assert ("plan", 30) in dv.calls      # the mesh bounds once, for every slab
    dv = StubVoxelizer(layers=12)
    dense.voxelize_dense(dv, 30, box="tight")
    vox = [c[1] for c in dv.calls if c[0] == "voxelize"]
    # the boxes of all slabs, then the writes: the last slab's records are still there and go first
    assert vox == [(0, 12), (12, 24), (24, 30), (0, 12), (12, 24)]


def test_empty_result_tight():
    t, origin = dense.voxelize_dense(StubVoxelizer(n=0), 16, box="tight")
    assert tuple(t.shape) == (0, 0, 0) and origin == (0, 0, 0)


# ---- the wait in front of the library ----------------------------------------------------------------------------------------------

def _grids():
    g = torch.zeros((4, 5, 6), dtype=torch.bool)
    g[1:3, 1:4, 2:5] = True
    rays = torch.ones((3, 3))
    return dict(g=g, labels=g.to(torch.uint8), field=torch.where(g, -1.0, 1.0), colors=torch.zeros(g.shape, dtype=torch.int32), o=rays, d=rays.clone(),
                seeds=torch.tensor([[2, 1, 1]], dtype=torch.int32))


def _caster(dv, t):
    return dense.RayCaster(dv, t["g"])


# (name, what runs before the log starts or None, the call): every public function of dense.py that hands a tensor to the library
WAIT_CASES = [
    ("set_mesh", None, lambda dv, t, _: dense.set_mesh(dv, torch.zeros((4, 9)))),
    ("voxelize_dense", None, lambda dv, t, _: dense.voxelize_dense(dv, 16)),
    ("voxelize_dense out=", None, lambda dv, t, _: dense.voxelize_dense(dv, 16, fmt="argb", out=torch.zeros((16, 16, 16), dtype=torch.int32))),
    ("voxelize_dense sdf", None, lambda dv, t, _: dense.voxelize_dense(dv, 16, fmt="sdf", fill=True)),
    ("distance_transform", None, lambda dv, t, _: dense.distance_transform(dv, t["labels"])),
    ("mesh_distance", None, lambda dv, t, _: dense.mesh_distance(dv, 16, band=2.0, closest=True, max_layers=4)),
    ("extract_surface", None, lambda dv, t, _: dense.extract_surface(dv, t["field"])),
    ("RayCaster", None, lambda dv, t, _: dense.RayCaster(dv, t["g"])),
    ("RayCaster.cast", _caster, lambda dv, t, caster: caster.cast(t["o"], t["d"])),
    ("raycast", None, lambda dv, t, _: dense.raycast(dv, t["field"], t["o"], t["d"], level=0.0)),
    ("components", None, lambda dv, t, _: dense.components(dv, t["g"])),
    ("flood", None, lambda dv, t, _: dense.flood(dv, t["g"], seeds=t["seeds"])),
    ("exterior", None, lambda dv, t, _: dense.exterior(dv, t["g"])),
    ("solidify", None, lambda dv, t, _: dense.solidify(dv, t["g"])),
    ("remove_small", None, lambda dv, t, _: dense.remove_small(dv, t["g"], 2)),
    ("count_voxels", None, lambda dv, t, _: dense.count_voxels(dv, t["g"])),
    ("to_voxels", None, lambda dv, t, _: dense.to_voxels(dv, t["g"], colors=t["colors"])),
    ("save_voxels", None, lambda dv, t, _: dense.save_voxels(dv, t["g"], "never_written.vl32")),
    ("count_faces", None, lambda dv, t, _: dense.count_faces(dv, t["g"], merge="rects")),
    ("voxel_faces", None, lambda dv, t, _: dense.voxel_faces(dv, t["g"], merge="rects", colors=t["colors"])),
    ("nearest_voxel", None, lambda dv, t, _: dense.nearest_voxel(dv, t["g"], dist2=True)),
    ("spread_colors", None, lambda dv, t, _: dense.spread_colors(dv, t["g"], t["colors"])),
    ("crossing_numbers", None, lambda dv, t, _: dense.crossing_numbers(dv, 16, max_layers=5)),
    ("crossing_numbers out=", None, lambda dv, t, _: dense.crossing_numbers(dv, 16, axes="zx", out=torch.zeros((4, 5, 6), dtype=torch.int32))),
    ("winding_fill", None, lambda dv, t, _: dense.winding_fill(dv, 16)),
    ("downsample", None, lambda dv, t, _: dense.downsample(dv, t["g"], 2)),
    ("downsample values, colours, out=", None, lambda dv, t, _: dense.downsample(
        dv, t["labels"], 2, count=True, values="max", colors=t["colors"], out=torch.zeros((2, 3, 3), dtype=torch.uint8),
        out_count=torch.zeros((2, 3, 3), dtype=torch.int16), out_values=torch.zeros((2, 3, 3), dtype=torch.uint8),
        out_colors=torch.zeros((2, 3, 3), dtype=torch.int32))),
    ("label_stats", None, lambda dv, t, _: dense.label_stats(dv, t["labels"], moments=True, faces=True)),
    ("label_stats int32", None, lambda dv, t, _: dense.label_stats(dv, t["colors"])),   # (n from labels.max(): a read before the call)
    ("component_stats", None, lambda dv, t, _: dense.component_stats(dv, t["g"])),
    ("keep_largest", None, lambda dv, t, _: dense.keep_largest(dv, t["g"])),
    ("geodesic_distance", None, lambda dv, t, _: dense.geodesic_distance(dv, t["g"], t["seeds"])),
    ("geodesic_distance border, out=", None, lambda dv, t, _: dense.geodesic_distance(dv, t["g"], border=True, out=torch.zeros(t["g"].shape, dtype=torch.int32))),
    ("shortest_paths", None, lambda dv, t, _: dense.shortest_paths(dv, t["colors"], t["seeds"])),
    ("shortest_paths max_len=", None, lambda dv, t, _: dense.shortest_paths(dv, t["colors"], [(2, 1, 1), (0, 0, 0)], max_len=7)),
    ("local_thickness", None, lambda dv, t, _: dense.local_thickness(dv, t["g"], 3)),
    ("local_thickness depth2=, out=", None, lambda dv, t, _: dense.local_thickness(
        dv, t["field"], 3, level=0.0, fmt="thickness", depth2=torch.zeros(t["g"].shape, dtype=torch.int32), out=torch.zeros(t["g"].shape))),
    ("inner_distance", None, lambda dv, t, _: dense.inner_distance(dv, t["g"])),
    ("inner_distance out=", None, lambda dv, t, _: dense.inner_distance(dv, t["g"], out=torch.zeros(t["g"].shape, dtype=torch.int32))),
    ("erode", None, lambda dv, t, _: dense.erode(dv, t["g"], 1)),
    ("dilate", None, lambda dv, t, _: dense.dilate(dv, t["g"], 1)),
    ("opening", None, lambda dv, t, _: dense.opening(dv, t["g"], 1)),
    ("closing", None, lambda dv, t, _: dense.closing(dv, t["g"], 1)),
    ("thin_regions", None, lambda dv, t, _: dense.thin_regions(dv, t["g"], 3)),
]

# the public callables of dense.py that take a voxelizer and hand nothing to the library: none so far.  (One that only reads the
# context - its limits, its transform - would go here, with the reason.)
NO_TENSOR_TO_THE_LIBRARY = set()


def _check_wait(monkeypatch, before, call):
    """Runs one dense call on a stub whose log also takes the waits, and asserts that the first library call that is handed a
    tensor comes behind a wait, and that every wait before it is on the voxelizer's device: the very object dense._device gave
    for this voxelizer, not a device made from torch's current one.  Returns the names logged."""
    dv = StubVoxelizer(n=3)
    own = torch.device("cpu")
    monkeypatch.setattr(dense, "_device", lambda v: own if v is dv else None)
    monkeypatch.setattr(dense, "_sync", lambda device: dv.calls.append(("sync", device)))
    t = _grids()
    state = before(dv, t) if before else None
    del dv.calls[:]
    call(dv, t, state)
    names = [c[0] for c in dv.calls]
    first = next((i for i, name in enumerate(names) if name in POINTER_CALLS), None)
    assert first is not None, "no library call was handed a tensor"
    waits = [c for c in dv.calls[:first] if c[0] == "sync"]
    assert waits, f"{names[first]} was called before any wait: {names}"
    assert all(c[1] is own for c in waits), "a wait on another device than the voxelizer's"
    return names


@pytest.mark.parametrize("name, before, call", WAIT_CASES, ids=[c[0] for c in WAIT_CASES])
def test_a_wait_comes_before_the_first_library_call_that_takes_a_tensor(monkeypatch, name, before, call):
    """The context's stream does not wait for torch's (it is created non-blocking), so dense._sync(device) is all that keeps a
    kernel of the library from reading a tensor torch has not finished writing, or a queued torch.zeros from landing on its
    output.  Every public function that hands a tensor to the library must wait on the voxelizer's device before its first such
    call; the write of a count / write pair needs no wait of its own.  (The mutation below, a count_voxels without its wait, was
    seen to fail this check - "gather_count was called before any wait" - when the test was written.)"""
    names = _check_wait(monkeypatch, before, call)
    pairs = {"extract_surface": ("surface_count", "surface_write"), "to_voxels": ("gather_count", "gather_write"),
             "voxel_faces": ("faces_count", "faces_write")}
    if name in pairs:   # (both calls of the pair were made, behind one wait)
        count, write = pairs[name]
        assert names.index("sync") < names.index(count) < names.index(write)


def test_the_wait_table_holds_every_public_function_that_takes_a_voxelizer():
    """WAIT_CASES by introspection: every public function or class of dense.py whose first parameter is `dv` is in the table under
    its own name, or in NO_TENSOR_TO_THE_LIBRARY; and the table names nothing else."""
    takes_dv = set()
    for name, f in vars(dense).items():
        if name.startswith("_") or not (inspect.isfunction(f) or inspect.isclass(f)) or getattr(f, "__module__", None) != dense.__name__:
            continue
        try:
            params = list(inspect.signature(f).parameters)
        except (TypeError, ValueError):
            continue
        if params and params[0] == "dv":
            takes_dv.add(name)
    assert len(takes_dv) >= 34 and {"set_mesh", "RayCaster", "thin_regions", "keep_largest"} <= takes_dv, sorted(takes_dv)
    in_table = {c[0].split()[0].split(".")[0] for c in WAIT_CASES}
    assert not NO_TENSOR_TO_THE_LIBRARY & in_table
    assert takes_dv - in_table - NO_TENSOR_TO_THE_LIBRARY == set(), "public functions of dense.py without a wait case"
    assert in_table | NO_TENSOR_TO_THE_LIBRARY <= takes_dv, sorted((in_table | NO_TENSOR_TO_THE_LIBRARY) - takes_dv)


def test_the_wait_check_fails_a_count_voxels_without_its_wait(monkeypatch):
    def count_voxels(dv, grid, *, level=None):
        _, grid_args, _ = dense._gather_args(dv, grid, level, (0, 0, 0), 0, None, None)
        return dv.gather_count(*grid_args)

    _check_wait(monkeypatch, None, lambda dv, t, _: dense.count_voxels(dv, t["g"]))
    monkeypatch.setattr(dense, "count_voxels", count_voxels)
    with pytest.raises(AssertionError, match="gather_count was called before any wait"):
        _check_wait(monkeypatch, None, lambda dv, t, _: dense.count_voxels(dv, t["g"]))


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_dense") / "o2v_device.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-function",
           "--cuda-device-only", "-S", "o2v_device.hip", "-o", str(out)]
    subprocess.run(cmd, cwd=SRC, check=True, capture_output=True)
    return out.read_text()


@pytest.mark.parametrize("kernel", ["k_gather_trisIi", "k_gather_trisIl", "k_any_textured", "k_dense_scatterILj0E", "k_dense_scatterILj1E",
                                    "k_dense_scatterILj2E", "k_dense_box"])
def test_k7_kernels_in_the_code_object_without_scratch(device_asm, kernel):
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    body = m.group(2)
    scratch = re.findall(r"; ScratchSize: (\d+)", device_asm[m.end():m.end() + 4000])
    assert scratch and scratch[0] == "0", scratch[:1]
    assert "scratch_" not in body and "buffer_store_dword v" not in body.replace("buffer_store_dwordx", "")
    if "scatter" in kernel or "box" in kernel:
        # one vector load per record (x, y, z, argb; the compiler leaves out argb where it is unused: 12 bytes of the 16)
        assert re.search(r"global_load_dwordx[34]", body) and not re.search(r"global_load_dword\s", body)
