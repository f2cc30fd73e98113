"""Solid fill (O2V_HIP_FLAG_FILL_INTERIOR) without a GPU: the parity restatement against analytic lattice sets, and the
feature's public surface (C entry point, Python bindings, command line)."""
import os
import subprocess

import numpy as np

from obj2voxel_amd import meshes
from tests import fill_ref


def _box(lo, hi):
    """closed axis-aligned box [lo, hi] (3-vectors) as 12 triangles of the unit cube's layout"""
    v = meshes.unit_cube().reshape(-1, 3).astype(np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return (lo + v * (hi - lo)).astype(np.float32).reshape(-1, 3, 3)


def _lattice(G, ss, lo, hi, x_rule, z_rule):
    c = np.arange(G) * ss + 0.5 * ss
    inx = x_rule(c, lo[0], hi[0])
    iny = x_rule(c, lo[1], hi[1])
    inz = z_rule(c, lo[2], hi[2])
    x, y, z = np.meshgrid(np.nonzero(inx)[0], np.nonzero(iny)[0], np.nonzero(inz)[0], indexing="ij")
    return np.sort(((x * G + y) * G + z).ravel().astype(np.int64))


def test_unit_cube_is_closed_and_uv_sphere_closes_when_welded():
    assert fill_ref.odd_edges(meshes.unit_cube().reshape(-1, 3, 3)) == []
    sv = meshes.uv_sphere(12).reshape(-1, 3, 3)
    assert fill_ref.odd_edges(fill_ref.weld(sv).reshape(-1, 3, 3)) == []


def test_parity_of_an_axis_aligned_box_is_its_lattice_set():
    for ss in (1, 2):
        G = 24
        lo, hi = (3.3 * ss, 2.71 * ss, 5.05 * ss), (17.9 * ss, 20.2 * ss, 11.49 * ss)
        sv = _box(lo, hi)
        assert fill_ref.odd_edges(sv) == []
        want = _lattice(G, ss, np.float32(lo), np.float32(hi), lambda c, a, b: (c > a) & (c < b), lambda c, a, b: (c > a) & (c < b))
        assert np.array_equal(fill_ref.parity_keys(sv, G, ss), want)


def test_parity_of_a_box_with_faces_on_column_centres():
    """Faces exactly through column centres: the perturbation P + (eps, eps^2) puts the columns of the low x / y faces
    inside and those of the high faces outside; a horizontal face exactly at a layer centre toggles the layers above it."""
    for ss in (1, 2):
        G = 20
        h = 0.5 * ss
        lo = (3 * ss + h, 2 * ss + h, 4 * ss + h)
        hi = (15 * ss + h, 9 * ss + h, 13 * ss + h)
        sv = _box(lo, hi)
        want = _lattice(G, ss, lo, hi, lambda c, a, b: (c >= a) & (c < b), lambda c, a, b: (c > a) & (c <= b))
        got = fill_ref.parity_keys(sv, G, ss)
        assert np.array_equal(got, want), (len(got), len(want))


def test_parity_of_nested_boxes_is_the_shell():
    G = 32
    outer, inner = _box((2.2, 2.2, 2.2), (29.6, 29.6, 29.6)), _box((9.3, 9.3, 9.3), (20.7, 20.7, 20.7))
    got = fill_ref.parity_keys(np.concatenate([outer, inner]), G, 1)
    rule = lambda c, a, b: (c > a) & (c < b)  # noqa: E731
    a = _lattice(G, 1, (2.2, 2.2, 2.2), (29.6, 29.6, 29.6), rule, rule)
    b = _lattice(G, 1, (9.3, 9.3, 9.3), (20.7, 20.7, 20.7), rule, rule)
    assert np.array_equal(got, np.setdiff1d(a, b))


def test_exact_sign_decides_what_float64_cannot():
    # an edge through a column centre up to a rounding of float64: only the exact value has the sign
    u = np.array([[0.1, 0.3]], np.float32)
    v = np.array([[np.float32(0.1) + np.float32(2.0 ** -20), 1e7]], np.float32)
    s = fill_ref._signs(u, v, np.array([0.5]), np.array([7.5]))
    want = fill_ref._exact_sign(float(u[0, 0]), float(u[0, 1]), float(v[0, 0]), float(v[0, 1]), 0.5, 7.5)
    assert s[0] == want != 0


def test_o2v_set_fill_is_exported_and_bound():
    from obj2voxel_amd import capi, _lib
    lib = _lib.lib()
    assert hasattr(lib, "o2v_set_fill")
    assert "o2v_set_fill" in capi.EXTENSIONS
    assert capi.api().o2v_set_fill.argtypes is not None


def test_python_structures_mirror_the_appended_fields():
    from obj2voxel_amd import hip
    assert [n for n, _ in hip._Params._fields_][-1] == "fill_argb"
    assert [n for n, _ in hip.Stats._fields_][-1] == "interior_voxels"
    assert [n for n, _ in hip.Timings._fields_][-1] == "fill_ms"
    assert hip.FLAG_FILL_INTERIOR == 8


def test_cli_help_lists_fill_flags():
    import obj2voxel_amd
    cli = os.path.join(os.path.dirname(obj2voxel_amd.LIB_PATH), "obj2voxel-amd")
    r = subprocess.run([cli, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--fill " in r.stdout and "--fill-color" in r.stdout
    bad = subprocess.run([cli, "a.stl", "b.vl32", "-r", "8", "--fill-color", "xyz"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--fill-color" in bad.stderr
