"""The geometry frames on the MI355X: gsr_depth_scale, gsr_frame_depth16, gsr_frame_normal8 and gsr_pick_point
(csrc/frames.hip) against the restatement (frames_ref.py), bit for bit: n, the two order statistics and the white level; every
depth word and normal byte; and `render_views` on a small scene.

Sizes, by the kernels' own extents: the encoders run one pixel per thread in workgroups of 256; the selection's passes run
workgroups of 256 threads that take 4 pixels per thread and trip, one workgroup per 2048 pixels up to 1024 workgroups.
  (1,1), (64,1), (1,64) : one pixel, one row, one column: one workgroup, most of it idle;
  (55,23)   : odd, 1265 pixels: one workgroup of the selection, two trips, the second ragged;
  (130,67)  : 8710 pixels: five workgroups with ragged tails in every pass;
  (640,368) : 235 520 pixels, 115 workgroups: histogram flushes from many workgroups meet in every bin that is hit.
The selection has no size threshold between two code paths: its three levels always run."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_ref as fr
import scenes
from hip_helpers import dev
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu

f32 = np.float32
U8 = torch.uint8
SHAPES = [(1, 1), (64, 1), (1, 64), (55, 23), (130, 67), (640, 368)]
PERCENTILES = [99.0, 100.0, 50.0, 1e-4]     # 100: j = n - 1, gamma = 1;  1e-4: j = 1 for every n below a million
ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], f32)   # a rotation with no zero in its first row


@pytest.fixture(scope="module")
def GF(pkg):
    return pkg.geometry_frames


def _poisoned(shape, dtype):
    item = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full((int(np.prod(shape)) * item,), 0xFF, dtype=U8, device="cuda")
    return raw.view(dtype).view(*shape)


def _bytes(t):
    return t.contiguous().view(-1).view(U8).cpu().numpy()


def _stats(GF, ti, pct):
    """one gsr_depth_scale into poisoned statistics and scratch -> (device tensor, its four uint32 words)"""
    H, W, _ = ti.shape
    st = GF.depth_scale(ti, pct, stats=_poisoned((4,), torch.int32), scratch=_poisoned((GF.frames_scratch_bytes(W, H),), U8))
    return st, st.cpu().numpy().view(np.uint32)


_CASES = {}


def _case(W, H, Cn, kind="random", pct=50.0):
    key = (W, H, Cn, kind, pct if kind == "clusters" else None)
    if key not in _CASES:
        _CASES[key] = fr.make_case(W, H, Cn, seed=W * 1000 + H + Cn, kind=kind, percentile=pct)
    return _CASES[key]


@pytest.mark.parametrize("Cn", [5, 8])
@pytest.mark.parametrize("W,H", SHAPES)
def test_depth_scale_and_depth16_by_shape(GF, pkg, W, H, Cn):
    lib = pkg._lib.load()
    frame = _case(W, H, Cn)
    ti = dev(frame)
    assert GF.frames_scratch_bytes(W, H) == (32832 + 4 * W * H + 7) // 8 * 8
    want = fr.depth_stats(frame, 99.0)
    st, got = _stats(GF, ti, 99.0)
    print(f"[{W}x{H} C={Cn}] n={got[1]} a={got[2]:#x} b={got[3]:#x} scale={got[:1].view(f32)[0]!r}; want {want}")
    assert np.array_equal(got, fr.stats_words(want)), (got, want)
    assert torch.equal(_stats(GF, ti, 99.0)[0], st)                                     # a second run: the same bits
    scale = want["scale"]
    for flip in (False, True):
        # expected depth, white level from the device
        pic, st2 = GF.frame_depth16(ti, 0.0, 99.0, flip_rows=flip, out=_poisoned((H, W), torch.uint16), stats=_poisoned((4,), torch.int32))
        assert torch.equal(st2, st)
        ref = fr.depth16(frame, scale, True, flip_rows=flip)
        assert np.array_equal(pic.cpu().numpy(), ref), (W, H, Cn, flip)
        again, _ = GF.frame_depth16(ti, 0.0, 99.0, flip_rows=flip, out=_poisoned((H, W), torch.uint16))
        assert np.array_equal(_bytes(again), _bytes(pic))
        # expected depth, fixed white level
        pic, none = GF.frame_depth16(ti, 3.5, flip_rows=flip, out=_poisoned((H, W), torch.uint16))
        assert none is None and np.array_equal(pic.cpu().numpy(), fr.depth16(frame, f32(3.5), True, flip_rows=flip))
        # the raw channel: the viewer's picture, and with the device's white level
        pic = GF.viewer_depth16(ti, flip, out=_poisoned((H, W), torch.uint16))
        assert np.array_equal(pic.cpu().numpy(), fr.depth16(frame, f32(50), False, flip_rows=flip))
        pic = _poisoned((H, W), torch.uint16)
        assert lib.gsr_frame_depth16(W, H, Cn, ti.data_ptr(), 0, 1e-3, 0.0, st.data_ptr(), int(flip), pic.data_ptr(), _stream()) == 0
        assert np.array_equal(pic.cpu().numpy(), fr.depth16(frame, scale, False, flip_rows=flip))
    if W * H >= 8:      # alpha == min_alpha is covered (e = depth / min_alpha); just below it and 0 are black
        cov = fr.covered_mask(frame).reshape(-1)
        assert cov[0] and not cov[1] and not cov[2]
        got = GF.frame_depth16(ti, 1e4)[0].cpu().numpy().reshape(-1)
        assert got[1] == 0 and got[2] == 0 and got[0] == fr.depth16(frame, f32(1e4)).reshape(-1)[0]


@pytest.mark.parametrize("kind", [k for k in fr.KINDS if k != "random"])
@pytest.mark.parametrize("W,H", [(55, 23), (130, 67)])
def test_selection_on_adversarial_sets(GF, W, H, kind):
    for pct in PERCENTILES:
        frame = _case(W, H, 5, kind, pct)
        ti = dev(frame)
        want = fr.depth_stats(frame, pct)
        st, got = _stats(GF, ti, pct)
        print(f"[{W}x{H} {kind} p={pct}] n={got[1]} j={want['j']} gamma={want['gamma']:.6f} a={got[2]:#x} b={got[3]:#x} scale={got[:1].view(f32)[0]!r}")
        assert np.array_equal(got, fr.stats_words(want)), (kind, pct, got, want)
        assert torch.equal(_stats(GF, ti, pct)[0], st)
        if kind == "none":
            assert got[1] == 0 and got[:1].view(f32)[0] == 1.0
        pic, _ = GF.frame_depth16(ti, 0.0, pct, out=_poisoned((H, W), torch.uint16))
        assert np.array_equal(pic.cpu().numpy(), fr.depth16(frame, want["scale"], True)), (kind, pct)


def test_random_frames_at_every_percentile(GF):
    frame = _case(130, 67, 8)
    ti = dev(frame)
    for pct in PERCENTILES + [1.0, 37.5]:
        assert np.array_equal(_stats(GF, ti, pct)[1], fr.stats_words(fr.depth_stats(frame, pct))), pct
    # another min_alpha moves the covered set and the divisor
    want = fr.depth_stats(frame, 80.0, f32(0.25))
    H, W, _ = ti.shape
    got = GF.depth_scale(ti, 80.0, 0.25).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, fr.stats_words(want)) and want["n"] < fr.depth_stats(frame, 80.0)["n"]


@pytest.mark.parametrize("W,H", SHAPES)
def test_normal8(GF, W, H):
    frame = _case(W, H, 8)
    ti = dev(frame)
    for R in (None, ROT):
        pic = GF.frame_normal8(ti, R, out=_poisoned((H, W, 3), U8))
        ref = fr.normal8(frame, R)
        assert np.array_equal(pic.cpu().numpy(), ref), (W, H, R is None, int((pic.cpu().numpy() != ref).sum()))
        assert torch.equal(GF.frame_normal8(ti, R, out=_poisoned((H, W, 3), U8)), pic)
    if W * H >= 8:      # alpha == min_alpha is covered; just below it and 0 are not; a sum of length just under 1e-6 is degenerate
        got = GF.frame_normal8(ti).cpu().numpy().reshape(-1, 3)
        assert tuple(got[1]) == tuple(got[2]) == tuple(got[3]) == (128, 128, 128) and tuple(got[4]) == (128, 255, 128)
        assert fr.covered_mask(frame).reshape(-1)[0]
    cam_space, world = fr.normal8(frame), fr.normal8(frame, ROT)
    if W * H > 64:
        assert (cam_space != world).any()
    another = GF.frame_normal8(ti, None, 0.25).cpu().numpy()
    assert np.array_equal(another, fr.normal8(frame, None, f32(0.25)))


def _pick_camera(pkg, W, H):
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], f32) @ np.array([[1, 0, 0], [0, 0.8, -0.6], [0, 0.6, 0.8]], f32)
    return pkg.Camera(W, H, (70.0, 65.0), (0.48, 0.53), R.astype(f32), np.array([0.2, -0.1, 0.4], f32))


@pytest.mark.parametrize("W,H,Cn", [(55, 23, 8), (130, 67, 5), (1, 1, 4), (9, 40, 4)])
def test_pick_point(GF, pkg, W, H, Cn):
    r = np.random.default_rng(W + H)
    frame = r.uniform(0.0, 1.0, (H, W, Cn)).astype(f32)
    depth = r.uniform(0.5, 9.0, (H, W)).astype(f32)
    depth[r.integers(0, 3, (H, W)) == 0] = 0.0                 # background
    depth[r.integers(0, 9, (H, W)) == 0] = f32(1e-2)           # exactly the threshold: not > 1e-2
    if W > 20:
        depth[:10, :10] = 0.0                                  # an all-background window
    frame[..., 3] = depth
    cam = _pick_camera(pkg, W, H)
    bare = pkg.Camera(W, H, cam.focal, cam.principal)          # identity pose: the third coordinate IS the mean depth z
    ti = dev(frame)
    spots = [(1, 1), (W, 1), (1, H), (W, H), ((W + 1) // 2, 1), ((W + 1) // 2, H), (1, (H + 1) // 2), (W, (H + 1) // 2),
             ((W + 1) // 2, (H + 1) // 2), (min(W, 5), min(H, 5)),
             (0, 1), (W + 1, 1), (1, 0), (1, H + 1), (-7, -7), (2 ** 31 - 1, 1), (-2 ** 31, 1)]
    for hw in (0, 1, 4, 16):
        for px, py in spots:
            out = GF.pick_point(ti, cam, px, py, hw, out=_poisoned((4,), torch.float32))
            got = out.cpu().numpy()
            plain = GF.pick_point(ti, bare, px, py, hw, out=_poisoned((4,), torch.float32)).cpu().numpy()
            win = fr.pick_window(frame, px, py, hw)
            tag = (W, H, px, py, hw)
            if win is None or win.size == 0:
                assert np.array_equal(got.view(np.uint32), np.zeros(4, np.uint32)), tag
                assert np.array_equal(plain.view(np.uint32), np.zeros(4, np.uint32)), tag
                continue
            assert got[3] == win.size and plain[3] == win.size, tag                      # the count is exact
            z = plain[2]
            mean = float(np.mean(win.astype(np.float64)))
            assert abs(float(z) - mean) <= (win.size + 1) * 2.0 ** -24 * mean, (tag, z, mean)
            for o, c in ((got, cam), (plain, bare)):       # given the device's z: the coordinates bit for bit
                want = fr.pick_from_z(z, W, H, c, px, py)
                assert np.array_equal(o[:3].view(np.uint32), want.view(np.uint32)), (tag, o, want)
            assert torch.equal(GF.pick_point(ti, cam, px, py, hw), out), tag
    if W > 20:
        assert fr.pick_window(frame, 5, 5, 4).size == 0        # the all-background window was among the spots


def test_pick_point_is_the_unprojection(GF, pkg):
    """A plane at depth 4 seen by a posed camera: the picked point projects back onto the pixel's centre."""
    W, H = 40, 30
    frame = np.zeros((H, W, 5), f32)
    frame[..., 3] = 4.0
    cam = _pick_camera(pkg, W, H)
    got = GF.pick_point(dev(frame), cam, 13, 7).cpu().numpy()
    assert got[3] == 81
    p = np.asarray(cam.R, np.float64) @ got[:3].astype(np.float64) + np.asarray(cam.t, np.float64)    # world -> camera
    u = p[0] / p[2] * cam.focal[0] + cam.principal[0] * W
    v = p[1] / p[2] * cam.focal[1] + cam.principal[1] * H
    assert abs(p[2] - 4.0) < 1e-5 and abs(u - 12.5) < 1e-4 and abs(v - 6.5) < 1e-4


def test_rejected_calls_change_nothing(GF, pkg):
    L, lib = pkg._lib, pkg._lib.load()
    buf = torch.full((8192,), 0xA5, dtype=U8, device="cuda")
    cam = C.byref(GF.camera_struct(pkg.Camera(8, 8, (10.0, 10.0)), 8, 8))
    table = fr.rejected_calls(lib, cam, buf.data_ptr())
    assert len(table) > 50
    for what, rc, msg in table:
        assert rc == L.GSR_E_INVALID_ARG and msg, what
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    img = torch.zeros((4, 6, 8), device="cuda")
    with pytest.raises(ValueError, match="image must be"):
        GF.depth_scale(torch.zeros((4, 6, 4), device="cuda"))
    with pytest.raises(ValueError, match="image must be"):
        GF.frame_normal8(torch.zeros((4, 6, 5), device="cuda"))
    with pytest.raises(ValueError, match="image must be"):
        GF.frame_depth16(torch.zeros((4, 6, 4), device="cuda"))                 # a per-view white level needs alpha
    assert GF.viewer_depth16(torch.zeros((4, 6, 4), device="cuda")).shape == (4, 6)
    with pytest.raises(ValueError, match="out must be"):
        GF.frame_depth16(img, out=torch.zeros((4, 6), dtype=torch.int16, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        GF.frame_normal8(img, out=torch.zeros((6, 4, 3), dtype=U8, device="cuda"))
    with pytest.raises(ValueError, match="stats must be"):
        GF.depth_scale(img, stats=torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError, match="scratch must be"):
        GF.depth_scale(img, scratch=torch.zeros(64, dtype=U8, device="cuda"))
    with pytest.raises(ValueError, match="resolution"):
        GF.pick_point(img, pkg.Camera(8, 8, (10.0, 10.0)), 1, 1)


def test_render_views_on_a_small_scene(GF, pkg, monkeypatch):
    """tests/scenes.py::grid_scene_rgbdn through `render_views` for two cameras: the rgb bytes equal frame_rgb8, the depth
    words, normal bytes and white levels equal the restatement applied to the frame read back; ONE device -> host copy."""
    sc, cam0 = scenes.grid_scene_rgbdn()
    W, H = cam0.width, cam0.height
    c, s = np.cos(0.4), np.sin(0.4)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], f32)
    cams = [pkg.Camera(W, H, tuple(cam0.focal)),
            pkg.Camera(W, H, tuple(cam0.focal), (0.5, 0.5), R, np.array([-3 * s, 0, 3 - 3 * c], f32))]
    t = [dev(sc["means"]), dev(sc["shs"]), dev(sc["opac"].reshape(-1, 1)), dev(sc["scales"]), dev(sc["rots"])]
    rast = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgbdn")
    try:
        reads = []
        real = GF._read_back
        monkeypatch.setattr(GF, "_read_back", lambda x: (reads.append(tuple(x.shape)), real(x))[1])
        for world in (False, True):
            for depth_max in (0.0, 4.0):
                reads.clear()
                rgb, depth, normal, scales = GF.render_views(rast, t[0], (t[1], t[2], t[3]), t[4], cams, 0, depth_max, 97.0, world)
                assert reads == ([(2, 4)] if depth_max == 0.0 else []), reads
                assert len(rgb) == len(depth) == len(normal) == len(scales) == 2
                for v, cam in enumerate(cams):
                    img = rast.forward_raw(*t, cam, 0, (0.0, 0.0, 0.0), forward_only=True).clone()
                    frame = img.cpu().numpy()
                    assert fr.covered_mask(frame).any()
                    assert torch.equal(rgb[v], pkg.evaluation.frame_rgb8(img))
                    want = fr.depth_stats(frame, 97.0)["scale"] if depth_max == 0.0 else f32(depth_max)
                    print(f"[view {v} world={world} depth_max={depth_max}] white level {scales[v]!r}, restated {want!r}")
                    assert f32(scales[v]).view(np.uint32) == f32(want).view(np.uint32)
                    assert np.array_equal(depth[v].cpu().numpy(), fr.depth16(frame, want, True))
                    M = np.asarray(cam.R, f32).T if world else None
                    assert np.array_equal(normal[v].cpu().numpy(), fr.normal8(frame, M))
                assert (normal[1] != normal[0]).any()
        # a picked point of the first view lies on the grid's plane z = 3
        img = rast.forward_raw(*t, cams[0], 0, (0.0, 0.0, 0.0), forward_only=True)
        p = GF.pick_point(img, cams[0], W // 2, H // 2).cpu().numpy()
        assert p[3] > 0 and abs(p[2] - 3.0) < 0.05
        assert GF.render_views(rast, t[0], (t[1], t[2], t[3]), t[4], [], 0) == ([], [], [], [])
    finally:
        rast.close()
