"""-m gpu: TSDF fusion and surface-nets extraction on the MI355X (csrc/tsdf.hip through surface_mesh).
  1. `integrate` against the fp32 restatement of tests/tsdf_ref.py, bit for bit — tsdf, weight and colour as integers, after the
     first and after all 14 views of the sphere cases, on random frames over the four odd volumes, two runs; over volumes of two
     to four 256-blocks of x under cameras that see their whole length;
  2. against the float64 twin;
  3. the extraction against the restatement: counts, vertices and colours as bits, faces as integers; one read-back; the volumes
     of tsdf_ref.MULTI_RUN_CASES among them (several runs per slab, several workgroups, a second round of the scan);
  4. the mesh conditions on the device's meshes of the sphere cases;
  5. gsr_mesh_emit with capacities below the counts, on guarded buffers;
  6. through the rasterizer: fuse_views on a small :rgbd scene;
  7. every entry point on guarded arenas, and the error codes.
Every test fails on a build without the feature: the package has no surface_mesh, the library no gsr_tsdf_* / gsr_mesh_*."""
import ctypes as C

import numpy as np
import pytest
import torch

import tsdf_ref as tr
from guarded import Arena, placements
from hip_helpers import dev
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu
f32 = np.float32
U8, I32 = torch.uint8, torch.int32


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, f32).view(np.int32)


def pkg_cam(pkg, cam):
    return pkg.Camera(cam.width, cam.height, tuple(float(x) for x in cam.focal), tuple(float(x) for x in cam.principal),
                      np.asarray(cam.R, f32), np.asarray(cam.t, f32))


def device_volume(pkg, ref, load=False):
    """A fresh TSDFVolume with the geometry of the restatement's `ref`; load=True: with its state as well."""
    vol = pkg.surface_mesh.TSDFVolume(ref.dims, ref.origin, ref.h, ref.trunc, color=ref.color is not None)
    if load:
        vol.volume.copy_(torch.from_numpy(ref.packed().astype(f32)))
        if ref.color is not None:
            vol.color.copy_(torch.from_numpy(ref.color.astype(f32)))
    return vol


def assert_same_volume(vol, ref, tag):
    got, want = bits(vol.volume), bits(ref.packed())
    bad = np.argwhere(got != want)
    assert bad.size == 0, (tag, len(bad), bad[:4], vol.volume.cpu().numpy()[tuple(bad[0][:3])], ref.packed()[tuple(bad[0][:3])])
    if ref.color is not None:
        bad = np.argwhere(bits(vol.color) != bits(ref.color))
        assert bad.size == 0, (tag, "colour", len(bad), bad[:4])


def assert_same_mesh(mesh, want, tag):
    assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32
    assert (mesh.vertices.shape[0], mesh.faces.shape[0]) == (want.n_vertices, 2 * want.n_quads), (tag, mesh.vertices.shape, mesh.faces.shape)
    assert tuple(mesh.vertices.shape) == (want.n_vertices, 3) and tuple(mesh.faces.shape) == (2 * want.n_quads, 3)
    assert np.array_equal(bits(mesh.vertices), bits(want.vertices)), tag
    assert np.array_equal(mesh.faces.cpu().numpy(), want.faces), tag
    if want.colors is None:
        assert mesh.colors is None
    else:
        assert np.array_equal(bits(mesh.colors), bits(want.colors)), tag


_fused = {}


def fused_on_device(pkg, case):
    """The device's volume of a sphere case after all 14 views, with colour; fused once."""
    if case not in _fused:
        vol = device_volume(pkg, tr.sphere_volume(case, True))
        for cam in tr.sphere_cameras():
            vol.integrate(dev(tr.sphere_frame(cam)), pkg_cam(pkg, cam))
        _fused[case] = vol
    return _fused[case]


# ---- 1. integrate, bit for bit ----
@pytest.mark.parametrize("case", ["A", "B"])
def test_integrate_sphere_is_the_fp32_restatement_bit_for_bit(pkg, case):
    cams = tr.sphere_cameras()
    first = tr.sphere_fused(case, True, f32, 1)
    vol = device_volume(pkg, first)
    vol.integrate(dev(tr.sphere_frame(cams[0])), pkg_cam(pkg, cams[0]))
    assert_same_volume(vol, first, (case, "first view"))
    assert int((vol.volume[..., 1] > 0).sum()) > 300
    full = fused_on_device(pkg, case)
    assert_same_volume(full, tr.sphere_fused(case, True), (case, "14 views"))
    # a second run, and a volume without colour: the same {tsdf, weight} bits
    again = device_volume(pkg, tr.sphere_volume(case, False))
    assert again.color is None
    for cam in cams:
        again.integrate(dev(tr.sphere_frame(cam)), pkg_cam(pkg, cam))
    assert torch.equal(again.volume.view(I32), full.volume.view(I32))
    # reset gives the fresh volume back
    again.reset()
    assert bool((again.volume[..., 0] == 1).all()) and not bool(again.volume[..., 1].any())


@pytest.mark.parametrize("dims", tr.RANDOM_DIMS)
def test_integrate_random_frames_bit_for_bit(pkg, dims):
    """Frames carrying alpha < min_alpha, alpha = 0, NaN and negative depths, samples behind the camera, projections exactly on
    the frame's edges (tests/test_tsdf_cpu.py shows that they do); volumes below one wave, across a wave boundary, no multiple
    of any block."""
    ref, views = tr.random_views(dims, True)
    runs = [device_volume(pkg, ref), device_volume(pkg, ref)]
    for n, (frame, cam) in enumerate(views):
        tr.integrate(ref, frame, cam)
        for vol in runs:
            vol.integrate(dev(frame), pkg_cam(pkg, cam))
        assert_same_volume(runs[0], ref, (dims, n))
    assert torch.equal(runs[0].volume.view(I32), runs[1].volume.view(I32)) and torch.equal(runs[0].color.view(I32), runs[1].color.view(I32))
    assert int((runs[0].volume[..., 1] > 0).sum()) > 0


@pytest.mark.parametrize("dims", tr.WIDE_DIMS)
def test_integrate_past_the_first_256_samples_of_x(pkg, dims):
    """Volumes of two, three and four workgroups in x (blockIdx.x·256 beyond 0), the last with 1, 44, 1 and 2 live lanes, under
    cameras that see the whole length of the box (tests/test_tsdf_cpu.py: every 256-block holds fused samples in the
    restatement; random_views' cameras reach none past i = 255): compared after every view, two runs, and the device's own
    weights are non-zero in every block."""
    ref, views = tr.wide_views(dims, True)
    runs = [device_volume(pkg, ref), device_volume(pkg, ref)]
    for n, (frame, cam) in enumerate(views):
        tr.integrate(ref, frame, cam)
        for vol in runs:
            vol.integrate(dev(frame), pkg_cam(pkg, cam))
        assert_same_volume(runs[0], ref, (dims, n))
    assert torch.equal(runs[0].volume.view(I32), runs[1].volume.view(I32)) and torch.equal(runs[0].color.view(I32), runs[1].color.view(I32))
    weight = runs[0].volume[..., 1]
    blocks = [int((weight[..., b:b + 256] > 0).sum()) for b in range(0, dims[0], 256)]
    sizes = [weight[..., b:b + 256].numel() for b in range(0, dims[0], 256)]
    print(dims, list(zip(blocks, sizes)))
    assert len(blocks) == (dims[0] + 255) // 256 >= 2 and all(n >= min(30, size) for n, size in zip(blocks, sizes)), (blocks, sizes)
    # without colour: the same {tsdf, weight} bits
    plain = device_volume(pkg, tr.Volume(dims, ref.origin, ref.h, ref.trunc, False))
    for frame, cam in views:
        plain.integrate(dev(frame), pkg_cam(pkg, cam))
    assert plain.color is None and torch.equal(plain.volume.view(I32), runs[0].volume.view(I32))


def test_min_alpha_and_near_reach_the_kernel(pkg):
    ref, views = tr.random_views((41, 13, 11), True)
    vol = device_volume(pkg, ref)
    for (frame, cam), (ma, near) in zip(views, ((0.5, 0.2), (1e-3, 1.0), (1e-4, -1.0))):
        tr.integrate(ref, frame, cam, ma, near)
        vol.integrate(dev(frame), pkg_cam(pkg, cam), min_alpha=ma, near=near)
    assert_same_volume(vol, ref, "min_alpha / near")
    frame, cam = dev(views[0][0]), pkg_cam(pkg, views[0][1])
    with pytest.raises(ValueError, match="min_alpha"):
        vol.integrate(frame, cam, min_alpha=0.0)
    with pytest.raises(ValueError, match="C >= 5"):
        vol.integrate(frame[..., :4].contiguous(), cam)
    with pytest.raises(ValueError, match="resolution"):
        vol.integrate(frame[:, :32].contiguous(), cam)
    with pytest.raises(ValueError):
        vol.integrate(frame.cpu(), cam)
    SM = pkg.surface_mesh
    for bad in (dict(dims=(0, 4, 4)), dict(dims=(4, 4)), dict(voxel_size=0.0), dict(trunc=-1.0), dict(origin=(0, 0, float("nan")))):
        kw = dict(dims=(4, 4, 4), origin=(0, 0, 0), voxel_size=0.1, trunc=0.2)
        kw.update(bad)
        with pytest.raises(ValueError):
            SM.TSDFVolume(**kw)


def test_around_is_the_box_of_the_points(pkg, monkeypatch):
    SM = pkg.surface_mesh
    pts = dev(np.array([[0, 0, 0], [2, 1, 0.5], [1, -1, 0.25]], f32))
    calls = []
    real = SM._read_back
    monkeypatch.setattr(SM, "_read_back", lambda t: (calls.append(t.numel()), real(t))[1])
    vol = SM.TSDFVolume.around(pts, 21, margin=0.5, color=True)
    assert calls == [6], "one small read-back: the minimum and the maximum"
    assert vol.dims == (21, 21, 11) and np.allclose(vol.origin, (-0.5, -1.5, -0.5)) and abs(vol.voxel_size - 0.15) < 1e-6
    assert abs(vol.trunc - 0.6) < 1e-6 and vol.color is not None and vol.volume.shape == (11, 21, 21, 2)
    with pytest.raises(ValueError):
        SM.TSDFVolume.around(pts[:1], 8)


# ---- 2. against the float64 twin ----
@pytest.mark.parametrize("case", ["A", "B"])
def test_integrate_against_the_float64_twin(pkg, case):
    """|Δtsdf| <= max_v e_s + 3·u·w, u = 2^-24, wherever the device's decisions and pixels — the fp32 restatement's, by test 1 —
    agree with the twin's in every view; at most 1 % of the samples may disagree (tests/test_tsdf_cpu.py: none does on the
    restatement).  e_s = u·((8·zmag + 2·|d| + |z|)/trunc + 1) is what fp32 may lose on s = min(1, (D/α - z)/trunc) in one view:
    8 roundings on the way to z, each of a value of at most zmag = Σ_c |R[2,c]|·(|o_c| + h·idx_c) + |t_2| (2 per coordinate, 3
    products, 3 sums: 6 first-order, 8 with room for the second order), one on d = D/α, one on the difference (a value of at
    most |d| + |z|), one on the quotient (|s| <= 1).  The running mean (tsdf·w + s)/(w + 1) passes the error of s on damped by
    1/(w + 1) and the old error by w/(w + 1) — never more than the largest e_s — and adds three roundings of values of at most
    1 after the division, per view.  Observed: worst err / bound 0.05 on both cases."""
    v32, v64 = tr.sphere_fused(case, True), tr.sphere_fused(case, True, np.float64)
    vol = fused_on_device(pkg, case)
    assert np.array_equal(bits(vol.volume), bits(v32.packed()))
    agree = tr.agreement(v32, v64)
    sel = agree & (v64.weight > 0)
    err = np.abs(vol.volume[..., 0].cpu().numpy().astype(np.float64) - v64.tsdf)
    bound = tr.tsdf_bound(v64)
    print(f"{case}: {int((~agree).sum())} of {agree.size} samples disagree, {int(sel.sum())} compared, worst err / bound {(err[sel] / bound[sel]).max():.3f}")
    assert (~agree).mean() <= 0.01 and sel.sum() > 1000
    assert (err[sel] <= bound[sel]).all()


# ---- 3. extraction against the restatement ----
def _extraction_cases():
    cases = {"sphere A": lambda: tr.sphere_fused("A", True), "sphere B": lambda: tr.sphere_fused("B", True)}
    for dims in ((9, 8, 7), (41, 13, 11)):
        cases[f"random {dims}"] = lambda dims=dims: tr.random_volume(dims, 11)
        cases[f"dense random {dims}"] = lambda dims=dims: tr.random_volume(dims, 12, p_zero=0.05)
    cases["random (41, 13, 11), no colour"] = lambda: tr.random_volume((41, 13, 11), 13, color=False, p_zero=0.05)
    cases["a long row (300, 4, 3)"] = lambda: tr.random_volume((300, 4, 3), 14, p_zero=0.02)   # more than one chunk of cells per row
    cases["one active cell"] = tr.one_cell_volume
    cases["no cell (1, 4, 4)"] = lambda: tr.random_volume((1, 4, 4), 15)
    cases["no cell (2, 2, 1)"] = lambda: tr.random_volume((2, 2, 1), 16)
    for case in tr.MULTI_RUN_CASES:   # past one step of 63 cells, one run per slab, one workgroup, one round of the scan
        cases[tr.multi_run_name(case)] = lambda case=case: tr.multi_run(case)[0]
    return cases


_MULTI_RUN = {tr.multi_run_name(case): case for case in tr.MULTI_RUN_CASES}


@pytest.mark.parametrize("name", list(_extraction_cases()))
def test_extraction_is_the_restatement(pkg, name, monkeypatch):
    SM = pkg.surface_mesh
    ref = _extraction_cases()[name]()
    want = tr.multi_run(_MULTI_RUN[name])[1] if name in _MULTI_RUN else tr.extract_volume(ref)
    assert SM.mesh_scratch_bytes(ref.dims) == tr.mesh_scratch_bytes(ref.dims), "the plan of the library is the restated one"
    vol = device_volume(pkg, ref, load=True)
    calls = []
    real = SM._read_back
    monkeypatch.setattr(SM, "_read_back", lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    mesh = SM.extract_mesh(vol)
    assert calls == [(2,)], "exactly one read-back: the two counts"
    assert_same_mesh(mesh, want, name)
    again = SM.extract_mesh(vol)
    assert torch.equal(again.vertices.view(I32), mesh.vertices.view(I32)) and torch.equal(again.faces, mesh.faces), "two runs"
    if name.startswith("dense"):
        assert want.n_vertices > 100 and want.n_quads > 50
    if name == "one active cell":
        assert (want.n_vertices, want.n_quads) == (1, 0)
    if name.startswith("no cell"):
        assert (want.n_vertices, want.n_quads) == (0, 0) and SM.mesh_scratch_bytes(ref.dims) == 0
    if name in _MULTI_RUN:
        rows, nruns, nblk, ncells = tr.mesh_plan(ref.dims)
        assert (rows, nruns, nblk) == _MULTI_RUN[name].plan and SM.mesh_scratch_bytes(ref.dims) == 4 * ncells + 8 * (nblk + 1)
        assert want.n_vertices > 300 and want.n_quads > 100
    assert_same_volume(vol, ref, "the volume is an input")


# ---- 4. the conditions of the CPU file, on the device's meshes ----
@pytest.mark.parametrize("case", ["A", "B"])
def test_sphere_mesh_conditions_on_the_device(pkg, case):
    """Every undirected edge in exactly two triangles, once per direction; V - E + F = 2; every face normal away from the centre;
    max | |v| - 1 | <= 0.5·h — on the mesh extracted on the device from the volume fused on the device."""
    SM = pkg.surface_mesh
    vol = fused_on_device(pkg, case)
    mesh = SM.extract_mesh(vol)
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    rep = tr.mesh_report(v, f, vol.voxel_size)
    print(case, len(v), len(f), rep)
    assert (len(v), len(f)) == {"A": (728, 1452), "B": (1506, 3008)}[case]
    assert rep["closed"] and rep["euler"] == 2 and rep["outward"] and rep["used"]
    assert rep["radius_h"] <= 0.5
    pv, pc, pf = tr.parse_ply(SM.mesh_ply_bytes(mesh))
    assert np.array_equal(pv.view(np.int32), v.view(np.int32)) and np.array_equal(pf, f)
    assert np.array_equal(pc, tr.quantize8(mesh.colors.cpu().numpy()))


# ---- 5. capacities below the counts ----
def _ptr(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def _origin(ref):
    return (C.c_float * 3)(*[float(x) for x in ref.origin])


def _arena_bytes(*nbytes):
    """Room for placements of these sizes: each with its guards and the skew of its start."""
    return sum(int(n) for n in nbytes) + len(nbytes) * (2 * 1024 + 64)


def _emit_below_capacity(pkg, skew, ref, want, capacities):
    """gsr_mesh_count + gsr_mesh_emit per (max_vertices, max_faces) of `capacities`, on an arena sized from the case."""
    lib = pkg._lib.load()
    M, Q = want.n_vertices, want.n_quads
    nx, ny, nz = ref.dims
    nb = int(lib.gsr_mesh_scratch_bytes(nx, ny, nz))
    assert nb == tr.mesh_scratch_bytes(ref.dims)
    st = _stream()
    for caps in capacities:
        P = Arena(max(1 << 20, _arena_bytes(ref.packed().nbytes, ref.color.nbytes, nb, 8, 12 * caps[0], 12 * caps[0], 12 * caps[1])), "cuda", skew, 1)
        volume, color = P.place("volume", ref.packed(), align=8), P.place("color", ref.color)
        scratch = P.place("scratch", (nb,), U8, align=8, role="scratch")
        counts = P.place("counts", (2,), I32)
        vertices, vcolors = P.place("vertices", (caps[0], 3)), P.place("vertex colours", (caps[0], 3))
        faces = P.place("faces", (caps[1], 3), I32)
        for t in (scratch, counts, vertices, vcolors, faces):
            if t.numel():
                t.view(-1).view(U8).fill_(0xFF)
        rc = lib.gsr_mesh_count(nx, ny, nz, _ptr(volume), _ptr(counts), _ptr(scratch), nb, st)
        rc2 = lib.gsr_mesh_emit(nx, ny, nz, _origin(ref), float(ref.h), _ptr(volume), _ptr(color), _ptr(scratch), nb, caps[0], caps[1],
                                _ptr(vertices), _ptr(vcolors), _ptr(faces), st)
        assert (rc, rc2) == (0, 0), lib.gsr_last_error_string().decode()
        torch.cuda.synchronize()
        assert P.check() == [], (caps, P.check())
        P.assert_inputs_unchanged()
        assert counts.tolist() == [M, Q], caps
        assert np.array_equal(bits(vertices), bits(want.vertices[:caps[0]])) and np.array_equal(bits(vcolors), bits(want.colors[:caps[0]]))
        assert np.array_equal(faces.cpu().numpy(), want.faces[:caps[1]]), caps


@pytest.mark.parametrize("skew", ["aligned", "worst"])
def test_emit_below_capacity_on_guarded_buffers(pkg, skew):
    """max_vertices = M // 2 and an odd max_faces (the last quad written as ONE triangle): the first rows are the full mesh's,
    the output arrays end where the capacities do and their guards are intact, the counts are the true ones."""
    ref = tr.random_volume((41, 13, 11), 12, p_zero=0.05)
    want = tr.extract_volume(ref)
    M, Q = want.n_vertices, want.n_quads
    cap_v, cap_f = M // 2, (2 * Q) // 2 | 1
    assert 0 < cap_v < M and 0 < cap_f < 2 * Q
    _emit_below_capacity(pkg, skew, ref, want, ((cap_v, cap_f), (M, 0), (0, 2 * Q), (1, 1)))


@pytest.mark.parametrize("skew", ["aligned", "worst"])
def test_emit_below_capacity_inside_a_second_run(pkg, skew):
    """(130, 40, 5), three runs per slab.  The capacities M // 2 and Q | 1 of the test above end inside the short last run of
    slab 1 and inside run 0 of slab 2; a second pair ends in the MIDDLE of run 1 of slab 1, the last quad as one triangle — a
    wave of a workgroup stops writing while its neighbours write all or nothing; a third with the last vertex and the last
    whole quad of run 0 of slab 2 (all of a run is written, nothing of its successor); and (M, 0), (0, 2Q), (1, 1)."""
    case = next(c for c in tr.MULTI_RUN_CASES if c.dims == (130, 40, 5))
    ref, want = tr.multi_run(case)
    M, Q = want.n_vertices, want.n_quads
    nruns = case.plan[1]
    run, _, _ = tr.vertex_runs(ref)
    quad_run = run[want.faces[0::2]].max(1)          # the run that emits a quad is the run of its cell p, the last of its four
    assert (np.diff(quad_run) >= 0).all()
    first_v, first_q = (lambda r: int(np.searchsorted(run, r))), (lambda r: int(np.searchsorted(quad_run, r)))
    cap_v, cap_f = M // 2, (2 * Q) // 2 | 1
    assert run[cap_v] == run[cap_v - 1] == nruns + 2 and quad_run[cap_f // 2] == 2 * nruns
    mid_v = (first_v(nruns + 1) + first_v(nruns + 2)) // 2
    mid_f = (first_q(nruns + 1) + first_q(nruns + 2)) | 1
    assert run[mid_v] == run[mid_v - 1] == nruns + 1 and quad_run[mid_f // 2] == quad_run[mid_f // 2 - 1] == quad_run[mid_f // 2 + 1] == nruns + 1
    edge_v, edge_q = first_v(2 * nruns + 1), first_q(2 * nruns + 1)
    assert 0 < edge_v < M and 0 < edge_q < Q and run[edge_v - 1] == 2 * nruns == quad_run[edge_q - 1]
    _emit_below_capacity(pkg, skew, ref, want, ((cap_v, cap_f), (mid_v, mid_f), (M, 0), (0, 2 * Q), (1, 1), (edge_v, 2 * edge_q)))


# ---- 6. through the rasterizer ----
def test_fuse_views_through_the_rasterizer(pkg):
    """A :rgbd scene at 64 x 48 under three poses of synthetic.view_pose: the fused volume is, bit for bit, the restatement fed
    the frames read back from the device (the very tensors fuse_views rendered); nothing else is read back."""
    R, SM = pkg.rasterizer, pkg.surface_mesh
    W, H, n, deg = 64, 48, 1500, 1
    s = pkg.synthetic.make_scene(n, W, H, deg, 2121, sigma_px=5.0)
    cams = [pkg.Camera(W, H, tuple(float(x) for x in s.focal), (0.5, 0.5), *pkg.synthetic.view_pose(j)) for j in (1, 4, 6)]
    d = dict(means=dev(s.means), opac=dev(s.opacities_raw.reshape(-1, 1)), scales=dev(s.scales_raw), rots=dev(s.rotations),
             dc=dev(s.shs[:, :1]), rest=dev(s.shs[:, 1:]))
    acts = R.prologue_forward(d["dc"], d["rest"], d["opac"], d["scales"])
    rast = R.GaussianRasterizer(W, H, mode="rgbd")
    ref = tr.Volume((30, 21, 26), (-3.1, -2.05, 1.5), 0.21, 0.9, True)
    vol = device_volume(pkg, ref)
    frames, render = [], rast.forward_raw

    def recording(*a, **k):
        assert k.get("forward_only") is True and tuple(a[7]) == (0.0, 0.0, 0.0)
        frames.append(render(*a, **k).clone())
        return frames[-1]

    rast.forward_raw = recording
    out = SM.fuse_views(rast, d["means"], acts, d["rots"], cams, deg, vol)
    assert out is vol and len(frames) == 3 and frames[0].shape == (H, W, 5)
    for frame, cam in zip(frames, cams):
        tr.integrate(ref, frame.cpu().numpy(), tr.Cam(W, H, cam.focal, cam.principal, cam.R, cam.t))
    assert_same_volume(vol, ref, "fuse_views")
    assert (ref.weight > 0).sum() > 500 and ref.weight.max() == 3 and ((ref.tsdf < 1) & (ref.weight > 0)).sum() > 100
    with pytest.raises(ValueError, match="rgbd"):
        SM.fuse_views(R.GaussianRasterizer(W, H, mode="rgb"), d["means"], acts, d["rots"], cams, deg, vol)


# ---- 7. guarded arenas and error codes ----
G_DIMS, G_W, G_H = (41, 13, 11), 64, 48


def _guarded_inputs(pkg, dims=G_DIMS, wide=False):
    ref = tr.Volume(dims, (-2.0, -1.0, -1.0625), 1.0 / 16.0, 0.25, True)
    cam = tr.wide_camera(ref, +1, 1.0, 0.5, G_W, G_H) if wide else tr.oblique_camera(77, G_W, G_H, ref)
    frame = tr.random_frame(78, G_W, G_H, 8)
    start = tr.random_volume(dims, 12, p_zero=0.05)          # a volume in mid-fusion: weights 0..8, colours
    ref.tsdf, ref.weight, ref.color = start.tsdf.copy(), start.weight.copy(), start.color.copy()
    before = ref.packed().copy(), ref.color.copy()
    tr.integrate(ref, frame, cam)
    want = tr.extract_volume(ref)
    return ref, cam, frame, before, want, pkg.geometry_frames.camera_struct(pkg_cam(pkg, cam), G_W, G_H)


def _guarded_calls(lib, P, inputs, tag):
    ref, cam, frame_h, before, want, cs = inputs
    nx, ny, nz = ref.dims
    nb = int(lib.gsr_mesh_scratch_bytes(nx, ny, nz))
    if ref.dims == G_DIMS:
        assert nb == 4 * 40 * 12 * 10 + 8 * (10 + 1)      # 4 bytes per cell; one run of 12 rows of 40 cells per slab, 10 slabs; the total
    rows, nruns, nblk, ncells = tr.mesh_plan(ref.dims)
    assert nb == 4 * ncells + 8 * (nblk + 1)
    M, Q = want.n_vertices, want.n_quads
    frame = P.place("frame", frame_h)
    volume, color = P.place("volume", before[0], align=8, role="inout"), P.place("color", before[1], role="inout")
    volume2 = P.place("volume, no colour", before[0], align=8, role="inout")
    scratch, counts = P.place("scratch", (nb,), U8, align=8, role="scratch"), P.place("counts", (2,), I32)
    vertices, vcolors, faces = P.place("vertices", (M, 3)), P.place("vertex colours", (M, 3)), P.place("faces", (2 * Q, 3), I32)
    scratch2, counts2 = P.place("scratch2", (nb,), U8, align=8, role="scratch"), P.place("counts2", (2,), I32)
    vertices2, faces2 = P.place("vertices2", (M, 3)), P.place("faces2", (2 * Q, 3), I32)
    if P.skew == "worst":
        assert frame.data_ptr() % 16 == 4 and color.data_ptr() % 16 == 4 and volume.data_ptr() % 16 == 8 and scratch.data_ptr() % 16 == 8
    for t in (scratch, counts, vertices, vcolors, faces, scratch2, counts2, vertices2, faces2):
        t.view(-1).view(U8).fill_(0xFF)
    st, o, h = _stream(), _origin(ref), float(ref.h)
    integ = lambda v, c: lib.gsr_tsdf_integrate(nx, ny, nz, o, h, float(ref.trunc), G_W, G_H, 8, _ptr(frame), C.byref(cs),  # noqa: E731
                                                tr.MIN_ALPHA, tr.NEAR, _ptr(v), _ptr(c), st)
    rcs = [integ(volume, color), integ(volume2, None),
           lib.gsr_mesh_count(nx, ny, nz, _ptr(volume), _ptr(counts), _ptr(scratch), nb, st),
           lib.gsr_mesh_emit(nx, ny, nz, o, h, _ptr(volume), _ptr(color), _ptr(scratch), nb, M, 2 * Q, _ptr(vertices), _ptr(vcolors), _ptr(faces), st),
           lib.gsr_mesh_count(nx, ny, nz, _ptr(volume2), _ptr(counts2), _ptr(scratch2), nb, st),
           lib.gsr_mesh_emit(nx, ny, nz, o, h, _ptr(volume2), None, _ptr(scratch2), nb, M, 2 * Q, _ptr(vertices2), None, _ptr(faces2), st)]
    assert rcs == [0] * 6, (tag, rcs, lib.gsr_last_error_string().decode())
    torch.cuda.synchronize()
    assert P.check() == [], (tag, P.check())
    P.assert_inputs_unchanged()
    assert np.array_equal(bits(volume), bits(ref.packed())) and np.array_equal(bits(color), bits(ref.color)), tag
    assert torch.equal(volume2.view(I32), volume.view(I32)), tag
    assert counts.tolist() == [M, Q] and counts2.tolist() == [M, Q], tag
    assert np.array_equal(bits(vertices), bits(want.vertices)) and np.array_equal(bits(vcolors), bits(want.colors)), tag
    assert np.array_equal(faces.cpu().numpy(), want.faces), tag
    assert torch.equal(vertices2.view(I32), vertices.view(I32)) and torch.equal(faces2, faces), tag
    return {k: v.clone() for k, v in dict(volume=volume, color=color, vertices=vertices, vcolors=vcolors, faces=faces).items()}


def test_entry_points_on_guarded_buffers(pkg):
    """(41, 13, 11) with a 64 x 48 :rgbdn frame on the five placements: no guard word changes, the frame is unchanged, poisoned
    outputs and scratch do not reach a result, the same bits everywhere.  Under skew "worst" the frame and the colours start at
    4 mod 16, the volume and the scratch at 8 mod 16: the entry points may not ask for more."""
    lib = pkg._lib.load()
    inputs = _guarded_inputs(pkg)
    assert inputs[4].n_vertices > 100 and inputs[4].n_quads > 50
    assert (inputs[0].packed() != inputs[3][0]).any(), "the view fuses something"
    ref = None
    for P in placements(1 << 20, "cuda"):
        tag = f"{P.skew}/{P.fill}"
        got = _guarded_calls(lib, P, inputs, tag)
        if ref is None:
            ref = got
            continue
        for k in got:
            assert torch.equal(got[k].contiguous().view(-1).view(U8), ref[k].contiguous().view(-1).view(U8)), (tag, k)


W_DIMS = (513, 12, 4)


def test_entry_points_on_guarded_buffers_across_runs_and_blocks(pkg):
    """(513, 12, 4) on the five placements: three workgroups of the integration in x (the last with one live lane), three runs
    per slab in one workgroup of the extraction, the last run with 3 rows of 4.  The volume starts in mid-fusion and the camera
    sees its whole length; the scratch is 4 bytes per cell and 8 per run and for the total."""
    lib = pkg._lib.load()
    inputs = _guarded_inputs(pkg, W_DIMS, wide=True)
    ref, want, before = inputs[0], inputs[4], inputs[3]
    assert tr.mesh_plan(W_DIMS)[:3] == (4, 3, 9) and int(lib.gsr_mesh_scratch_bytes(*W_DIMS)) == 4 * 512 * 11 * 3 + 8 * (9 + 1)
    assert want.n_vertices > 1000 and want.n_quads > 500
    fused = ref.packed()[..., 1] != before[0][..., 1]
    assert all(fused[..., b:b + 256].sum() >= min(30, fused[..., b:b + 256].size) for b in (0, 256, 512)), "the view fuses samples of every block of x"
    run, K, _ = tr.vertex_runs(ref)
    f_run, f_k = run[want.faces], K[want.faces]
    assert ((f_k.max(1) == f_k.min(1)) & (f_run.max(1) != f_run.min(1))).sum() >= 100 and len(np.unique(run)) == 9
    volume_b, scratch_b = before[0].nbytes, tr.mesh_scratch_bytes(W_DIMS)
    mesh_b = 12 * want.n_vertices, 24 * want.n_quads
    need = _arena_bytes(inputs[2].nbytes, volume_b, before[1].nbytes, volume_b, scratch_b, 8, mesh_b[0], mesh_b[0], mesh_b[1], scratch_b, 8,
                        mesh_b[0], mesh_b[1])
    first = None
    for P in placements(need, "cuda"):
        tag = f"{P.skew}/{P.fill}"
        got = _guarded_calls(lib, P, inputs, tag)
        if first is None:
            first = got
            continue
        for k in got:
            assert torch.equal(got[k].contiguous().view(-1).view(U8), first[k].contiguous().view(-1).view(U8)), (tag, k)


def test_second_round_of_the_scan(pkg):
    """(1026, 42, 26): 1025 runs, one past a round of the 1024-thread scan — the last run's offset is the carry that crossed the
    rounds through LDS plus nothing, and the totals are the packed {vertices, quads << 32} word after that carry.  Through the
    entry points, on poisoned outputs: the counts read back, the LAST vertex and the LAST face (both of run 1024, by
    tests/test_tsdf_cpu.py: their ids and position come from that offset), then every row."""
    lib = pkg._lib.load()
    case = tr.MULTI_RUN_CASES[-1]
    ref, want = tr.multi_run(case)
    nx, ny, nz = ref.dims
    M, Q = want.n_vertices, want.n_quads
    rows, nruns, nblk, ncells = tr.mesh_plan(ref.dims)
    assert nblk == 1025 and (nx, ny, nz) == (1026, 42, 26)
    nb = int(lib.gsr_mesh_scratch_bytes(nx, ny, nz))
    assert nb == 4 * ncells + 8 * (nblk + 1)
    volume, color = dev(ref.packed()), dev(ref.color)
    scratch, counts = torch.empty(nb, dtype=U8, device="cuda"), torch.empty(2, dtype=I32, device="cuda")
    vertices, vcolors = torch.empty(M, 3, device="cuda"), torch.empty(M, 3, device="cuda")
    faces = torch.empty(2 * Q, 3, dtype=I32, device="cuda")
    for t in (scratch, counts, vertices, vcolors, faces):
        t.view(-1).view(U8).fill_(0xFF)
    st = _stream()
    rc = lib.gsr_mesh_count(nx, ny, nz, _ptr(volume), _ptr(counts), _ptr(scratch), nb, st)
    rc2 = lib.gsr_mesh_emit(nx, ny, nz, _origin(ref), float(ref.h), _ptr(volume), _ptr(color), _ptr(scratch), nb, M, 2 * Q,
                            _ptr(vertices), _ptr(vcolors), _ptr(faces), st)
    assert (rc, rc2) == (0, 0), lib.gsr_last_error_string().decode()
    torch.cuda.synchronize()
    assert counts.tolist() == [M, Q]
    run, _, _ = tr.vertex_runs(ref)
    assert run[-1] == 1024 and run[want.faces[-1]].max() == 1024 and run[want.faces[-1]].min() < 1024
    assert np.array_equal(bits(vertices[-1]), bits(want.vertices[-1])), (vertices[-1].tolist(), want.vertices[-1])
    assert faces[-1].tolist() == want.faces[-1].tolist()
    first_v = int(np.searchsorted(run, 1024))
    assert np.array_equal(bits(vertices[first_v:]), bits(want.vertices[first_v:])), "the vertices of run 1024"
    assert np.array_equal(bits(vertices), bits(want.vertices)) and np.array_equal(bits(vcolors), bits(want.colors))
    bad = np.flatnonzero((faces.cpu().numpy() != want.faces).any(1))
    assert bad.size == 0, (len(bad), bad[:4], faces[int(bad[0])].tolist(), want.faces[bad[0]])
    assert np.array_equal(bits(volume), bits(ref.packed()))


def test_error_codes(pkg):
    L = pkg._lib
    lib = L.load()
    bad = L.GSR_E_INVALID_ARG
    ref, cam, frame_h, before, want, cs = _guarded_inputs(pkg)
    nx, ny, nz = ref.dims
    nb = int(lib.gsr_mesh_scratch_bytes(nx, ny, nz))
    assert lib.gsr_mesh_scratch_bytes(1, 4, 4) == 0 and lib.gsr_mesh_scratch_bytes(0, 4, 4) == 0 and lib.gsr_mesh_scratch_bytes(-3, 4, 4) == 0
    assert lib.gsr_mesh_scratch_bytes(2, 2, 2) == 4 + 8 + 8 and lib.gsr_mesh_scratch_bytes(70000, 2, 2) == 0
    P = Arena(1 << 20, "cuda", "aligned", 0)
    frame = P.place("frame", frame_h)
    volume, color = P.place("volume", before[0], align=8, role="inout"), P.place("color", before[1], role="inout")
    scratch, counts = P.place("scratch", (nb,), U8, align=8, role="scratch"), P.place("counts", (2,), I32)
    vertices, vcolors, faces = P.place("vertices", (16, 3)), P.place("vertex colours", (16, 3)), P.place("faces", (16, 3), I32)
    st, o, h, trunc = _stream(), _origin(ref), float(ref.h), float(ref.trunc)
    state = [t.clone() for t in (volume, color, scratch, counts, vertices, vcolors, faces)]

    def integ(n=(nx, ny, nz), o=o, h=h, trunc=trunc, W=G_W, H=G_H, Cn=8, frame=frame, cam=C.byref(cs), ma=tr.MIN_ALPHA, near=tr.NEAR,
              volume=volume, color=color):
        return lib.gsr_tsdf_integrate(*n, o, h, trunc, W, H, Cn, _ptr(frame), cam, ma, near, _ptr(volume), _ptr(color), st)

    nan = float("nan")
    for kw, word in ((dict(o=None), b"null"), (dict(cam=None), b"null"), (dict(frame=None), b"null"), (dict(volume=None), b"null"),
                     (dict(n=(0, ny, nz)), b"side"), (dict(n=(nx, -1, nz)), b"side"), (dict(n=(nx, ny, 0)), b"side"),
                     (dict(n=(nx, 70000, nz)), b"exceed"), (dict(h=0.0), b"voxel_size"), (dict(h=-1.0), b"voxel_size"), (dict(h=nan), b"voxel_size"),
                     (dict(trunc=0.0), b"trunc"), (dict(trunc=nan), b"trunc"), (dict(ma=0.0), b"min_alpha"), (dict(ma=-1.0), b"min_alpha"),
                     (dict(ma=nan), b"min_alpha"), (dict(Cn=4), b"C = 4"), (dict(W=0), b"image size"), (dict(H=-2), b"image size"),
                     (dict(near=nan), b"near_plane"), (dict(volume=volume.view(-1)[1:]), b"8-byte")):
        assert integ(**kw) == bad and word in lib.gsr_last_error_string(), (kw, lib.gsr_last_error_string())

    def count(n=(nx, ny, nz), volume=volume, counts=counts, scratch=scratch, nb=nb):
        return lib.gsr_mesh_count(*n, _ptr(volume), _ptr(counts), _ptr(scratch), nb, st)

    def emit(n=(nx, ny, nz), o=o, h=h, volume=volume, color=color, scratch=scratch, nb=nb, mv=16, mf=16, vertices=vertices, vcolors=vcolors,
             faces=faces):
        return lib.gsr_mesh_emit(*n, o, h, _ptr(volume), _ptr(color), _ptr(scratch), nb, mv, mf, _ptr(vertices), _ptr(vcolors), _ptr(faces), st)

    for kw, word in ((dict(volume=None), b"null"), (dict(counts=None), b"null"), (dict(scratch=None), b"null"), (dict(n=(nx, 0, nz)), b"side"),
                     (dict(nb=nb - 1), b"scratch"), (dict(scratch=scratch[4:], nb=nb), b"aligned"), (dict(volume=volume.view(-1)[1:]), b"8-byte"),
                     (dict(n=(1 << 14, 1 << 14, 8)), b"2^30")):
        assert count(**kw) == bad and word in lib.gsr_last_error_string(), (kw, lib.gsr_last_error_string())
    for kw, word in ((dict(volume=None), b"null"), (dict(o=None), b"null"), (dict(scratch=None), b"null"), (dict(vertices=None), b"null"),
                     (dict(faces=None), b"null"), (dict(vcolors=None), b"together"), (dict(color=None), b"together"), (dict(n=(-1, ny, nz)), b"side"),
                     (dict(h=0.0), b"voxel_size"), (dict(mv=-1), b"capacity"), (dict(mf=-1), b"capacity"), (dict(nb=nb - 1), b"scratch"),
                     (dict(scratch=scratch[4:], nb=nb), b"aligned")):
        assert emit(**kw) == bad and word in lib.gsr_last_error_string(), (kw, lib.gsr_last_error_string())
    torch.cuda.synchronize()
    assert P.check() == []
    for t, was in zip((volume, color, scratch, counts, vertices, vcolors, faces), state):
        assert torch.equal(t.view(-1).view(U8), was.view(-1).view(U8)), "a refused call touches nothing"
    # empty calls: a volume without a cell is an empty mesh, without a scratch; zero capacities write nothing
    counts.fill_(-1)
    assert count(n=(1, 4, 4), scratch=None, nb=0) == 0 and emit(n=(1, 4, 4), scratch=None, nb=0) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0]
    assert count() == 0 and emit(mv=0, mf=0, vertices=None, vcolors=None, faces=None) == 0
    torch.cuda.synchronize()
    assert P.check() == [] and torch.equal(vertices, state[4]) and torch.equal(faces, state[6])
