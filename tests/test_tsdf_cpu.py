"""No GPU: the numpy restatement of the TSDF fusion and the surface-nets extraction (tests/tsdf_ref.py) against
its float64 twin, the mesh conditions on the analytic sphere scenes, the random frames' coverage of every branch, the PLY
bytes parsed back, the declarations of the new entry points, and the conditions on the inputs that take the GPU tests past one
run per slab, one workgroup, one round of the scan (MULTI_RUN_CASES) and one 256-block of x (wide_views)."""
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


# ---- the inputs that take the kernels past one run, one workgroup, one scan round, one 256-block of x ----
# dims -> (vertices, quads, triangles with vertices in two runs of ONE slab, active cells in the last run of a slab)
MULTI_RUN_FIGURES = {(64, 5, 3): (311, 150, 0, 311), (65, 5, 3): (327, 138, 0, 327), (127, 4, 3): (484, 238, 0, 484),
                     (130, 40, 5): (12839, 9075, 362, 3116), (513, 12, 4): (11111, 7237, 1246, 3045),
                     (1025, 7, 3): (8051, 4260, 1556, 2643), (1026, 10, 3): (12204, 6792, 6588, 1372),
                     (2050, 4, 3): (8111, 3687, 3276, 2717), (1026, 42, 26): (60044, 2480, 1626, 1494)}


def test_mesh_plan_is_the_formula():
    """rows = max(1, 2048 // (nx - 1)), nruns = ceil((ny - 1) / rows), nblk = nruns·(nz - 1); every volume of the earlier
    extraction tests has ONE run per slab and at most 25 runs — what MULTI_RUN_CASES is there to leave."""
    for dims, want in (((9, 8, 7), (256, 1, 6, 336)), ((41, 13, 11), (51, 1, 10, 4800)), ((300, 4, 3), (6, 1, 2, 1794)),
                       ((17, 18, 19), (128, 1, 18, 4896)), ((24, 25, 26), (89, 1, 25, 13800)), ((2, 2, 2), (2048, 1, 1, 1)),
                       ((1025, 7, 3), (2, 3, 6, 12288)), ((1026, 7, 3), (1, 6, 12, 12300)), ((2049, 3, 2), (1, 2, 2, 4096)),
                       ((2050, 3, 2), (1, 2, 2, 4098)), ((256, 256, 256), (8, 32, 8160, 255 ** 3))):
        assert tr.mesh_plan(dims) == want, dims
        assert tr.mesh_scratch_bytes(dims) == 4 * want[3] + 8 * (want[2] + 1)
    for dims in ((1, 4, 4), (2, 2, 1), (5, 1, 5)):
        assert tr.mesh_plan(dims)[1:] == (0, 0, 0) and tr.mesh_scratch_bytes(dims) == 0
    assert tr.run_of((130, 40, 5), 14, 0) == 0 and tr.run_of((130, 40, 5), 15, 0) == 1 and tr.run_of((130, 40, 5), 38, 3) == 2 + 3 * 3
    assert any(not c.color and c.plan[1] >= 2 for c in tr.MULTI_RUN_CASES), "one multi-run case without colour"


@pytest.mark.parametrize("case", tr.MULTI_RUN_CASES, ids=tr.multi_run_name)
def test_multi_run_volumes_reach_what_they_are_for(case):
    """The plan of the case; its counts; fp32 against float64 as for the small volumes; and, where a slab has two runs or
    more: at least 100 triangles take vertices from two runs of ONE slab (mesh_vertex_id's j / rows and the run stride), an
    active cell lies in the last run of a slab — the shorter one where the rows do not divide — and for the 1025-run case a
    cell has run id 1024, the one entry of the scan's second round, with triangles joining it to earlier runs."""
    rows, nruns, nblk, ncells = tr.mesh_plan(case.dims)
    assert (rows, nruns, nblk) == case.plan
    nx, ny, nz = case.dims
    vol, a = tr.multi_run(case)
    assert (vol.color is not None) == case.color
    b = tr.extract_volume(vol, np.float64)
    assert a.n_vertices == b.n_vertices and a.n_quads == b.n_quads and np.array_equal(a.faces, b.faces)
    assert a.faces.min() >= 0 and a.faces.max() < a.n_vertices
    assert np.abs(a.vertices - b.vertices).max() <= 16 * tr.EPS * (np.abs(vol.origin).max() + float(vol.h) * max(case.dims))
    if case.color:
        assert np.abs(a.colors - b.colors).max() <= 8 * tr.EPS
    else:
        assert a.colors is None and b.colors is None
    run, K, J = tr.vertex_runs(vol)
    assert len(run) == a.n_vertices and (np.diff(run) >= 0).all(), "the runs ascend with the vertex order"
    f_run, f_k = run[a.faces], K[a.faces]
    cross = int(((f_k.max(1) == f_k.min(1)) & (f_run.max(1) != f_run.min(1))).sum())
    in_last = int((J // rows == nruns - 1).sum())
    print(f"{case.dims}: plan {case.plan}, {a.n_vertices} vertices, {a.n_quads} quads, {cross} triangles across runs of one slab, "
          f"{in_last} active cells in the last run of a slab")
    assert (a.n_vertices, a.n_quads, cross, in_last) == MULTI_RUN_FIGURES[case.dims]
    if nruns >= 2:
        assert cross >= 100 and in_last > 0
        assert run.max() == nblk - 1 and len(np.unique(run)) == nblk, "every run has a vertex"
    if case.dims in ((130, 40, 5), (513, 12, 4)):
        assert 0 < (ny - 1) - (nruns - 1) * rows < rows, "the last run is shorter"
    if nblk > tr.SCAN_ROUND:
        assert nblk == tr.SCAN_ROUND + 1 and (run == 1024).sum() > 0
        joins = (f_run.max(1) == 1024) & (f_run.min(1) < 1024)
        assert joins.sum() >= 2 and (f_run[-1] == 1024).any() and run[-1] == 1024, "the last vertex and the last face come from run 1024"


# dims -> samples whose weight changes in some view, per 256-block of x
WIDE_FIGURES = {(257, 3, 2): [1510, 6], (300, 4, 3): [3041, 521], (513, 5, 3): [3806, 3779, 15], (770, 3, 2): [1507, 1516, 1516, 12]}


@pytest.mark.parametrize("dims", tr.WIDE_DIMS)
def test_wide_views_reach_every_block_and_every_branch(dims):
    """Every 256-block of x, the partly filled last one included, holds at least 30 samples whose weight changes in some view —
    all of its samples where the block has fewer than 30 ((257, 3, 2): 6, (513, 5, 3): 15, (770, 3, 2): 12) — and the views
    reach what test_random_views_reach_every_branch lists.  random_views' cameras update no sample past i = 255 of such a box:
    they see 3.25 deep at most."""
    nx, ny, nz = dims
    old, old_views = tr.random_views(dims)
    for frame, cam in old_views:
        tr.integrate(old, frame, cam)
    if dims in ((257, 3, 2), (300, 4, 3)):
        assert not old.weight[..., 256:].any(), "the cameras of random_views stop short of the second block"
    vol, views = tr.wide_views(dims, True)
    assert len(views) >= 3 and vol.dims == dims and float(vol.h) == 1.0 / 16.0
    changed = np.zeros(vol.weight.shape, bool)
    for frame, cam in views:
        changed |= tr.integrate(vol, frame, cam)
    assert np.array_equal(changed, vol.weight > 0)
    blocks = [changed[..., b:b + 256] for b in range(0, nx, 256)]
    print(dims, [(int(b.sum()), b.size) for b in blocks])
    assert len(blocks) == (nx + 255) // 256 >= 2
    for b in blocks:
        assert b.sum() >= min(30, b.size)
    assert [int(b.sum()) for b in blocks] == WIDE_FIGURES[dims]
    # the branches
    assert vol.weight.max() >= 2 and (vol.weight == 0).any() and (vol.weight == 1).any()
    assert ((vol.tsdf < 1) & (vol.weight > 0)).sum() > 50 and (vol.tsdf < 0).sum() > 10
    assert np.isfinite(vol.tsdf).all() and np.isfinite(vol.color).all()
    (frame, cam), (frame_o, cam_o) = views[0], views[1]
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = vol.origin.astype(np.float64) + float(vol.h) * np.stack([i, j, k], -1)
    z = p @ np.asarray(cam_o.R, np.float64)[2] + float(cam_o.t[2])
    assert (z <= tr.NEAR).sum() > 100 and (z > tr.NEAR).sum() > 100, "samples on both sides of the oblique camera"
    ok, iu, iv = vol.views[0]
    assert ok[1].any() and (iu[1][ok[1]] == i[1][ok[1]]).all() and (iv[1][ok[1]] == j[1][ok[1]]).all()   # u = i - 0.5, v = j - 0.5 exactly
    for fr_ in (frame, views[2][0]):
        a = fr_[..., 4]
        d = fr_[..., 3] / np.where(a > 0, a, 1)
        assert (a == 0).any() and ((a > 0) & (a < tr.MIN_ALPHA)).any() and np.isnan(a).any() and np.isnan(fr_[..., 3]).any() and (d < 0).any()
    assert ok[1][:, 0].any() and ok[1][0, :].any(), "the low edges are inside"
    fresh, _ = tr.wide_views(dims)
    full = np.zeros((tr.EDGE_H, tr.EDGE_W, 5), f32)
    full[..., 3:] = (3.0, 1.0)
    ok_full = tr.integrate(fresh, full, cam)
    assert not ok_full[1, :, 64:].any() and ok_full[1, :, :64].all(), "u + 0.5 = W exactly is outside"
    # every kind of skip happens in the far blocks too: outside the frame, an unusable pixel, behind the truncation
    far = [v[0][..., 256:] for v in vol.views[2:]]
    assert any((~o).any() for o in far) and all(o.any() for o in far)


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
