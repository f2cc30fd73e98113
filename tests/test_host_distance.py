"""The distance transform without a GPU: the separable numpy reference against brute force (and scipy when it is there), the
argument checks and call sequence of obj2voxel_amd.dense's distance paths with the device calls stubbed, and a static check of
the K8 kernels in the gfx950 code object."""
import numpy as np
import pytest

from tests import distance_ref as R

torch = pytest.importorskip("torch")

from obj2voxel_amd import dense, hip  # noqa: E402
from tests.test_host_dense import StubVoxelizer, device_asm, on_cpu  # noqa: E402,F401


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 4), (1, 1, 70), (70, 1, 1), (5, 9, 13), (12, 11, 10)])
@pytest.mark.parametrize("density", [0.0, 0.02, 0.2, 1.0])
def test_separable_reference_equals_brute_force(shape, density):
    lab = R.random_labels(np.random.default_rng(hash((shape, density)) & 0xFFFF), shape, density)
    assert np.array_equal(R.separable_d2(lab), R.brute_d2(lab))


def test_separable_reference_adversarial():
    lab = np.zeros((6, 40, 45), np.uint8)
    lab[:, 0, 0] = 1             # seeds on one edge only
    lab[5, 39, 44] = 1
    assert np.array_equal(R.separable_d2(lab), R.brute_d2(lab))
    lab = np.zeros((3, 30, 31), np.uint8)
    lab[1, ::7, 30] = 1          # rows without seeds, seeds only at the far end of others
    assert np.array_equal(R.separable_d2(lab), R.brute_d2(lab))
    assert (R.separable_d2(np.zeros((2, 3, 4), np.uint8)) == R.INF).all()


def test_sdf_reference():
    lab = np.array([[[1, 0, 2, 2]]], np.uint8)
    d2 = R.separable_d2(lab)
    assert d2.tolist() == [[[0, 1, 4, 9]]]
    assert R.sdf(lab, d2).tolist() == [[[0.0, 1.0, -2.0, -3.0]]]
    s = R.sdf(np.full((1, 1, 2), 2, np.uint8), np.full((1, 1, 2), R.INF, np.int32))
    assert np.isneginf(s).all()


def test_separable_reference_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    lab = R.random_labels(np.random.default_rng(7), (40, 50, 60), 0.003)
    edt = ndimage.distance_transform_edt(lab != 1)
    assert np.array_equal(R.separable_d2(lab), np.rint(edt ** 2).astype(np.int32))


# ---- the reference at the shapes of the device's limit cases (tests/distance_cases.py) -----------------------------------

def _sampled(lab, want, seed, n=300):
    """`want` against an int64 brute force over every seed at n voxels: a third near seeds, the corners, the rest anywhere."""
    rng = np.random.default_rng(seed)
    shape = np.array(lab.shape)
    seeds = np.argwhere(lab == 1)
    assert len(seeds)
    pts = rng.integers(0, shape, (n, 3))
    near = seeds[rng.integers(0, len(seeds), n // 3)] + rng.integers(-3, 4, (n // 3, 3))
    pts[:n // 3] = np.clip(near, 0, shape - 1)
    pts[-8:] = [[z, y, x] for z in (0, shape[0] - 1) for y in (0, shape[1] - 1) for x in (0, shape[2] - 1)]
    got = want[pts[:, 0], pts[:, 1], pts[:, 2]].astype(np.int64)
    assert np.array_equal(got, R.sampled_brute_d2(lab, pts)), lab.shape
    return int(got.max())


@pytest.mark.parametrize("shape, density, empty_plane", [(R.LANE_CAP_SHAPES[0], 0.01, None), (R.LANE_CAP_SHAPES[0], 3e-6, 2),
                                                         (R.LANE_CAP_SHAPES[1], 0.01, None), (R.LANE_CAP_SHAPES[1], 3e-6, 2)])
def test_separable_reference_above_the_lane_cap(shape, density, empty_plane):
    assert min(R.pass_lines(shape)) > R.LANE_CAP
    lab = R.lane_cap_labels(shape, density, seed=17, empty_plane=empty_plane)
    _sampled(lab, R.separable_d2(lab), 1)


@pytest.mark.parametrize("shape", R.LONG_SHAPES)
def test_separable_reference_on_the_longest_lines(shape):
    lab = R.long_line_labels(shape, seed=29)
    v = np.moveaxis(lab, int(np.argmax(shape)), 0)
    assert v.shape[0] == R.LONG and v[0, 0, 0] == 1 and v[-1, 0, 0] == 1
    assert sum((n - 1) ** 2 for n in shape) <= R.D2_LIMIT
    _sampled(lab, R.separable_d2(lab), 2)
    if shape[2] == R.LONG:
        return
    # one seed at the far end of a long envelope line: the largest value of the box, by the closed form
    lab[lab == 1] = 0
    v[-1, -1, -1] = 1
    want = R.separable_d2(lab)
    assert int(want[0, 0, 0]) == sum((n - 1) ** 2 for n in shape) and _sampled(lab, want, 3) == want[0, 0, 0]


@pytest.mark.parametrize("along_z, interior", [(False, None), (True, 43)])
def test_separable_reference_on_deep_stacks(along_z, interior):
    lab = R.deep_stack_labels(along_z, interior)
    _sampled(lab, R.separable_d2(lab), 4)


def test_envelope_stats_counts_depth_and_pops():
    # 10, 10, 10, 0: three pushes, then the 0 pops all of them at one position (of 5, 5, 5, 0 the first stays: 5 < 9 at t = 0);
    # a line without values; a line of one value; a line that only pushes
    f = np.array([[10, 10, 10, 0], [5, 5, 5, 0], [R.INF] * 4, [R.INF, 7, R.INF, R.INF], [0, 0, 0, 0]], np.int64)
    depth, pops, stacks = R.envelope_stats(f)
    assert depth.tolist() == [3, 3, 0, 1, 4] and pops.tolist() == [3, 2, 0, 0, 0]
    assert [R.final_stack(*stacks, line) for line in range(5)] == [[(3, 0)], [(0, 0), (3, 1)], [], [(1, 0)], [(0, 0), (1, 1), (2, 2), (3, 3)]]
    assert R.envelope(f).tolist() == [[9, 4, 1, 0], [5, 4, 1, 0], [R.INF] * 4, [8, 7, 8, 11], [0, 0, 0, 0]]


def test_deep_stack_grid_reaches_its_depth_and_pop_runs():
    fy, fz = R.pass_inputs(R.deep_stack_labels())
    assert fy.shape == (2100, 1024) and fz.shape == (2100 * 1024, 1)
    depth, pops, _ = R.envelope_stats(fy)
    assert int(depth.min()) == 1023 and int(depth.max()) == 1024
    assert int((pops >= 1000).sum()) == 1099 and int(((pops >= 1) & (pops <= 100)).sum()) == 100 and int(pops.max()) == 1023
    fy, fz = R.pass_inputs(R.deep_stack_labels(along_z=True))
    assert fz.shape == (2100, 1024) and np.array_equal(R.envelope_stats(fz)[0], depth)


class DistStub(StubVoxelizer):
    def distance_dense(self, labels_ptr, label_strides, dst_ptr, fmt, dst_strides, dims):
        self.calls.append(("distance", fmt, tuple(label_strides), tuple(dst_strides), tuple(dims)))


def test_distance_transform_strides_and_formats():
    dv = DistStub()
    lab = torch.zeros((2, 5, 6, 7), dtype=torch.uint8)
    out = dense.distance_transform(dv, lab[1], "dist2")
    assert out.dtype == torch.int32 and tuple(out.shape) == (5, 6, 7) and out.is_contiguous()
    assert dv.calls[-1] == ("distance", hip.DIST_SQ_I32, (1, 7, 42), (1, 7, 42), (7, 6, 5))
    buf = torch.zeros((6, 7, 5), dtype=torch.float32)
    got = dense.distance_transform(dv, lab[0].permute(0, 2, 1).contiguous().permute(0, 2, 1), out=buf.permute(2, 0, 1))
    assert got.data_ptr() == buf.data_ptr()
    assert dv.calls[-1] == ("distance", hip.DIST_SDF_F32, (6, 1, 42), (5, 35, 1), (7, 6, 5))


@pytest.mark.parametrize("args, kw, exc", [
    ((torch.zeros((4, 4, 4), dtype=torch.uint8), "udf"), {}, ValueError),
    ((torch.zeros((4, 4, 4), dtype=torch.int32),), {}, TypeError),
    ((torch.zeros((4, 4), dtype=torch.uint8),), {}, ValueError),
    ((torch.zeros((4, 0, 4), dtype=torch.uint8),), {}, ValueError),
    ((torch.zeros((4, 4, 4), dtype=torch.uint8), "dist2"), dict(out=torch.zeros((4, 4, 4), dtype=torch.float32)), TypeError),
    ((torch.zeros((4, 4, 4), dtype=torch.uint8), "sdf"), dict(out=torch.zeros((4, 4, 5), dtype=torch.float32)), ValueError),
])
def test_distance_transform_rejects(args, kw, exc):
    dv = DistStub()
    with pytest.raises(exc):
        dense.distance_transform(dv, *args, **kw)
    assert not dv.calls


def test_voxelize_dense_distance_formats():
    dv = DistStub(layers=12, interior=3)
    t, origin = dense.voxelize_dense(dv, 30, fmt="sdf", fill=True)
    assert t.dtype == torch.float32 and tuple(t.shape) == (30, 30, 30) and origin == (0, 0, 0)
    kinds = [c[0] for c in dv.calls]
    # the labels slab by slab (as fmt="labels"), then one transform over the whole box
    assert kinds.count("voxelize") == 3 and kinds.count("write") == 3 and kinds[-1] == "distance"
    assert all(c[1] == hip.DENSE_U8 for c in dv.calls if c[0] == "write")
    assert dv.calls[-1] == ("distance", hip.DIST_SDF_F32, (1, 30, 900), (1, 30, 900), (30, 30, 30))
    dv = DistStub(lo=(1, 2, 3), hi=(5, 8, 12))
    t, origin = dense.voxelize_dense(dv, 16, fmt="dist2", box="tight")
    assert t.dtype == torch.int32 and tuple(t.shape) == (9, 6, 4) and origin == (1, 2, 3)
    assert dv.calls[-1][1] == hip.DIST_SQ_I32 and dv.calls[-1][4] == (4, 6, 9)
    out = torch.zeros((2, 16, 16, 16), dtype=torch.int32)
    got, _ = dense.voxelize_dense(DistStub(), 16, fmt="dist2", out=out[1])
    assert got.data_ptr() == out[1].data_ptr()


@pytest.mark.parametrize("kw, exc", [
    (dict(fmt="sdf"), ValueError), (dict(fmt="sdf", fill=False), ValueError),
    (dict(fmt="dist2", out=torch.zeros((16, 16, 16), dtype=torch.float32)), TypeError),
    (dict(fmt="sdf", fill=True, out=torch.zeros((16, 16), dtype=torch.float32)), ValueError),
])
def test_voxelize_dense_distance_rejects(kw, exc):
    dv = DistStub()
    with pytest.raises(exc):
        dense.voxelize_dense(dv, 16, **kw)
    assert not dv.calls


def test_existing_formats_do_not_run_the_transform():
    dv = DistStub()
    dense.voxelize_dense(dv, 16, fmt="labels", fill=True)
    assert "distance" not in [c[0] for c in dv.calls]


@pytest.mark.parametrize("kernel", ["k_dist_x", "k_dist_envelopeILj0E", "k_dist_envelopeILj1E", "k_dist_envelopeILj2E", "k_near_x", "k_near_envelope",
                                    "k_thick_depth_x", "k_thick_core_x"])
def test_k8_kernels_in_the_code_object_without_scratch(device_asm, kernel):  # noqa: F811
    import re
    m = re.search(r"^(_ZN\S*" + kernel + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", device_asm, re.M | re.S)
    assert m, kernel + " is not in the gfx950 code object"
    body = m.group(2)
    scratch = re.findall(r"; ScratchSize: (\d+)", device_asm[m.end():m.end() + 4000])
    assert scratch and scratch[0] == "0", scratch[:1]
    assert "scratch_" not in body and "buffer_store_dword v" not in body.replace("buffer_store_dwordx", "")
    # no private segment: neither spills nor a stack array in scratch
    assert re.search(r"^\s*\.set " + re.escape(m.group(1)) + r"\.private_seg_size, 0$", device_asm, re.M)


def test_scratch_is_sized_per_pass():
    """8 bytes x the larger of the two envelope passes' lanes (at most 2^17) x their line length."""
    def bytes_(dims):
        return hip._bind().o2v_hip_distance_scratch_bytes((hip.C.c_uint32 * 3)(*dims), hip.DIST_SQ_I32)
    try:
        hip._bind()
    except (ImportError, OSError) as e:
        pytest.skip(f"library not loadable: {e}")
    assert bytes_((1024, 1024, 1024)) == 8 * (1 << 17) * 1024
    assert bytes_((4096, 4096, 1)) == 8 * 4096 * 4096          # the y pass: 4096 lines of 4096
    assert bytes_((1, 1, 46341)) == 8 * 46341                   # one line along z
    assert bytes_((300, 7, 129)) == 8 * max(300 * 129 * 7, 300 * 7 * 129)
    assert bytes_((5, 0, 5)) == 0
