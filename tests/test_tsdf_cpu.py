"""No GPU: the numpy restatement of the TSDF fusion and the surface-nets extraction (tests/tsdf_ref.py) against
its float64 twin, the mesh conditions on the analytic sphere scenes, the random frames' coverage of every branch, the PLY
bytes parsed back, and the declarations of the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

import tsdf_ref as tr

f32 = np.float32


def _twin_figures(v32, v64, tag):
    agree = tr.agreement(v32, v64)
    sel = agree & (v64.weight > 0)
    err = np.abs(v32.tsdf.astype(np.float64) - v64.tsdf)
    bound = tr.tsdf_bound(v64)
    print(f"{tag}: {int((~agree).sum())} of {agree.size} samples disagree, {int(sel.sum())} compared, "
          f"worst err / bound {(err[sel] / bound[sel]).max() if sel.any() else 0.0:.3f}")
    return agree, sel, err, bound


@pytest.mark.parametrize("case", ["A", "B"])
def test_fp32_against_float64_on_the_sphere(case):
    """|Δtsdf| <= max_v e_s + 3·2^-24·w (tsdf_ref.tsdf_bound) wherever the decisions and the pixels agree in every view; at most
    1 % of the samples may disagree — the cap the GPU test relies on, checked here on the restatement alone."""
    v32, v64 = tr.sphere_fused(case, True), tr.sphere_fused(case, True, np.float64)
    agree, sel, err, bound = _twin_figures(v32, v64, case)
    assert (~agree).mean() <= 0.01 and sel.sum() > 1000
    assert (err[sel] <= bound[sel]).all()
    assert np.array_equal(v32.weight[agree], v64.weight[agree].astype(f32))
    assert np.abs(v32.color.astype(np.float64) - v64.color)[agree].max() <= 14 * 4 * tr.EPS    # 3 roundings + q's per view


@pytest.mark.parametrize("dims", tr.RANDOM_DIMS)
def test_fp32_against_float64_on_random_views(dims):
    v32, views = tr.random_views(dims, True)
    v64 = tr.Volume(dims, v32.origin, v32.h, v32.trunc, True, np.float64)
    for frame, cam in views:
        tr.integrate(v32, frame, cam)
        tr.integrate(v64, frame, cam)
    agree, sel, err, bound = _twin_figures(v32, v64, dims)
    assert (~agree).mean() <= 0.01
    assert (err[sel] <= bound[sel]).all()


def test_random_views_reach_every_branch():
    """(41, 13, 11): samples behind the camera, outside the frame, on alpha = 0, below min_alpha, on NaN alpha and depth, on
    negative depth, behind the truncation, fused once and more than once, clamped and unclamped; projections exactly on the
    frame's edges on the axis-aligned camera, for (65, 3, 2) on the high edge as well."""
    vol, views = tr.random_views((41, 13, 11), True)
    for frame, cam in views:
        tr.integrate(vol, frame, cam)
    assert vol.weight.max() >= 2 and (vol.weight == 0).any() and (vol.weight == 1).any()
    assert ((vol.tsdf < 1) & (vol.weight > 0)).sum() > 50 and (vol.tsdf < 0).sum() > 10
    assert np.isfinite(vol.tsdf).all() and np.isfinite(vol.color).all()
    (frame, cam), (frame_o, cam_o) = views[0], views[1]
    R, t = np.asarray(cam_o.R, np.float64), np.asarray(cam_o.t, np.float64)
    nx, ny, nz = vol.dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = vol.origin.astype(np.float64) + float(vol.h) * np.stack([i, j, k], -1)
    z = p @ R[2] + t[2]
    assert (z <= tr.NEAR).sum() > 100 and (z > tr.NEAR).sum() > 100, "samples on both sides of the oblique camera"
    ok, iu, iv = vol.views[0]
    # the axis-aligned camera, plane k = 1: u = i - 0.5 and v = j - 0.5 exactly
    assert (iu[1][ok[1]] == i[1][ok[1]]).all() and (iv[1][ok[1]] == j[1][ok[1]]).all()
    a = frame[..., 4]
    d = frame[..., 3] / np.where(a > 0, a, 1)
    assert (a == 0).any() and ((a > 0) & (a < tr.MIN_ALPHA)).any() and np.isnan(a).any() and np.isnan(frame[..., 3]).any() and (d < 0).any()
    assert ok[1][:, 0].any() and ok[1][0, :].any(), "the low edges are inside"
    v65, views65 = tr.random_views((65, 3, 2))
    full = np.zeros((tr.EDGE_H, tr.EDGE_W, 5), f32)
    full[..., 3:] = (3.0, 1.0)                       # every pixel covered, depth 3: only the range decides
    ok65 = tr.integrate(v65, full, views65[0][1])
    assert not ok65[1, :, 64].any() and ok65[1, :, :64].all(), "u + 0.5 = W exactly is outside"


@pytest.mark.parametrize("case", ["A", "B"])
def test_sphere_mesh_conditions(case):
    """Every undirected edge in exactly two triangles, once per direction; V - E + F = 2; every face normal away from the centre;
    max | |v| - 1 | <= 0.5·h.  (fp32: 728 / 1452 at 0.19·h and 1506 / 3008 at 0.39·h.)"""
    vol = tr.sphere_fused(case, True)
    mesh = tr.extract_volume(vol)
    rep = tr.mesh_report(mesh.vertices, mesh.faces, vol.h)
    print(case, mesh.n_vertices, len(mesh.faces), rep)
    assert (mesh.n_vertices, len(mesh.faces)) == {"A": (728, 1452), "B": (1506, 3008)}[case]
    assert rep["closed"] and rep["euler"] == 2 and rep["outward"] and rep["used"]
    assert rep["radius_h"] <= 0.5
    assert mesh.colors.min() >= 0 and mesh.colors.max() <= 1
    # the colour of a vertex is the normal's picture: 0.5 + 0.5·n, n = v / |v| on the unit sphere, to within the voxel
    n = mesh.vertices / np.linalg.norm(mesh.vertices, axis=1, keepdims=True)
    assert np.abs(mesh.colors - (0.5 + 0.5 * n)).max() < 1.5 * float(vol.h)


def test_extraction_fp32_against_float64_and_small_volumes():
    sparse = tr.extract_volume(tr.random_volume((9, 8, 7), 3))
    assert sparse.n_vertices > 5 and sparse.n_quads >= 1
    vol = tr.random_volume((9, 8, 7), 3, p_zero=0.05)
    a, b = tr.extract_volume(vol), tr.extract_volume(vol, np.float64)
    assert a.n_vertices == b.n_vertices > 100 and a.n_quads == b.n_quads > 50 and np.array_equal(a.faces, b.faces)
    assert a.faces.min() >= 0 and a.faces.max() < a.n_vertices
    # a mean of at most 12 crossings s in [0, 1], the position 2 more roundings of values of at most |o| + h·n
    assert np.abs(a.vertices - b.vertices).max() <= 16 * tr.EPS * (np.abs(vol.origin).max() + float(vol.h) * 10)
    assert np.abs(a.colors - b.colors).max() <= 8 * tr.EPS
    one = tr.extract_volume(tr.one_cell_volume())
    assert one.n_vertices == 1 and one.n_quads == 0 and one.faces.shape == (0, 3)
    # the three crossings of the inside corner's edges, s = 0.25: their mean is (0.25, 0.25, 0.25)/3 of a cell
    assert np.allclose(one.vertices, 0.5 * 0.25 / 3.0, rtol=1e-6)
    for dims in ((1, 4, 4), (2, 2, 1)):
        e = tr.extract_volume(tr.random_volume(dims, 4))
        assert e.n_vertices == 0 and e.n_quads == 0 and e.vertices.shape == (0, 3)


@pytest.mark.parametrize("colors", [True, False])
def test_ply_bytes_parse_back(pkg, colors):
    SM = pkg.surface_mesh
    ref = tr.extract_volume(tr.sphere_fused("A", True))
    col = ref.colors.copy()
    col[0], col[1] = (-0.5, 0.5, 1.5), (0.001, 0.002, 127.5 / 255.0)
    mesh = SM.Mesh(torch.from_numpy(ref.vertices), torch.from_numpy(ref.faces), torch.from_numpy(col) if colors else None)
    data = SM.mesh_ply_bytes(mesh)
    assert isinstance(data, bytes) and data.startswith(b"ply\nformat binary_little_endian 1.0\n")
    v, c, f = tr.parse_ply(data)
    assert np.array_equal(v.view(np.int32), ref.vertices.view(np.int32)) and np.array_equal(f, ref.faces)
    if colors:
        assert np.array_equal(c, tr.quantize8(col)) and tuple(c[0]) == (0, 128, 255) and tuple(c[1]) == (0, 1, 128)
    else:
        assert c is None
    empty = SM.Mesh(torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32), None)
    v, c, f = tr.parse_ply(SM.mesh_ply_bytes(empty))
    assert v.shape == (0, 3) and f.shape == (0, 3)
    with pytest.raises(ValueError):
        SM.mesh_ply_bytes(SM.Mesh(torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int64), None))


def test_entry_points_are_declared(pkg):
    """The four entry points in the public header, the ctypes list and the build's object list; the ABI version unchanged."""
    L = pkg._lib
    header = open(L.HEADER_PATH).read()
    for name in ("gsr_tsdf_integrate", "gsr_mesh_scratch_bytes", "gsr_mesh_count", "gsr_mesh_emit"):
        assert re.search(rf"GSR_API \w+ {name}\(", header) and name in L.EXPORTS
    assert "#define GSR_ABI_VERSION 6" in header
    makefile = open(os.path.join(os.path.dirname(L.__file__), "csrc", "Makefile")).read()
    exact = re.search(r"^EXACT_OBJS = (.*)$", makefile, re.M).group(1).split()
    assert "build/tsdf.o" in exact and re.search(r"^build/tsdf\.o: .*block_reduce\.h", makefile, re.M)
    assert callable(pkg.surface_mesh.extract_mesh) and callable(pkg.surface_mesh.fuse_views)
    with pytest.raises(ValueError, match="no CPU path"):
        pkg.surface_mesh.TSDFVolume((4, 4, 4), (0, 0, 0), 0.1, 0.2, device="cpu")
