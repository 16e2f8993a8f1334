"""gsr_depth_scale, gsr_frame_depth16, gsr_frame_normal8 and gsr_pick_point (with gsr_frames_scratch_bytes) on guarded arenas
(tests/guarded.py) at both skews and both guard fills: nothing outside stats_out / scratch / the pictures / out4 is written,
the inputs are unchanged, poisoned outputs and scratch do not reach a result, and the results are the same bits in every
placement.  Under skew "worst" the byte picture starts at an odd address, the 16-bit picture at 2 mod 4 and every float array
(the statistics and out4 among them) at 4 mod 16; the scratch at 8 mod 16: no entry point may ask for more."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_ref as fr
from guarded import placements
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu

f32 = np.float32
U8 = torch.uint8
ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], f32)


@pytest.mark.parametrize("W,H,Cn", [(55, 23, 8), (1, 1, 8)])
def test_entry_points_on_guarded_buffers(pkg, W, H, Cn):
    GF, lib = pkg.geometry_frames, pkg._lib.load()
    frame = fr.make_case(W, H, Cn, seed=W + H + Cn)
    if W * H == 1:                    # the one pixel: covered, with a depth the pick accepts
        frame = frame.copy()
        frame[0, 0, 3:] = (2.5, 0.5, 0.1, -0.2, 0.3)
    cam = pkg.Camera(W, H, (40.0, 45.0), (0.5, 0.5), ROT, np.array([0.1, 0.2, 0.3], f32))
    bare = pkg.Camera(W, H, cam.focal, cam.principal)     # identity pose: its third coordinate is the mean depth z
    cs, cs_bare = GF.camera_struct(cam, W, H), GF.camera_struct(bare, W, H)
    rot9 = GF._rotation9(ROT)
    nb = int(lib.gsr_frames_scratch_bytes(W, H))
    assert nb == (32832 + 4 * W * H + 7) // 8 * 8
    px, py = (W + 1) // 2, (H + 1) // 2
    ptr = lambda t: t.data_ptr()  # noqa: E731
    ref = None
    for P in placements(1 << 20, "cuda"):
        tag = f"{P.skew}/{P.fill}"
        im = P.place("image", frame)
        stats, scr = P.place("stats_out", (4,), torch.int32), P.place("scratch", (nb,), U8, align=8, role="scratch")
        d_dev, d_max, d_raw = (P.place(n, (H, W), torch.uint16) for n in ("depth16_scale_dev", "depth16_depth_max", "depth16_raw_flipped"))
        n_cam, n_world = P.place("normal8_out", (H, W, 3), U8), P.place("normal8_world", (H, W, 3), U8)
        out4, out4_bare = P.place("out4", (4,)), P.place("out4_identity_pose", (4,))
        if P.skew == "worst":
            assert n_cam.data_ptr() % 2 == 1 and d_dev.data_ptr() % 4 == 2 and im.data_ptr() % 16 == 4
            assert stats.data_ptr() % 16 == 4 and out4.data_ptr() % 16 == 4 and scr.data_ptr() % 16 == 8
        for t in (stats, scr, d_dev, d_max, d_raw, n_cam, n_world, out4, out4_bare):
            t.view(-1).view(U8).fill_(0xFF)
        calls = [
            lib.gsr_depth_scale(W, H, Cn, ptr(im), 1e-3, 90.0, ptr(stats), ptr(scr), _stream()),
            lib.gsr_frame_depth16(W, H, Cn, ptr(im), 1, 1e-3, 0.0, ptr(stats), 0, ptr(d_dev), _stream()),
            lib.gsr_frame_depth16(W, H, Cn, ptr(im), 1, 1e-3, 4.0, None, 0, ptr(d_max), _stream()),
            lib.gsr_frame_depth16(W, H, Cn, ptr(im), 0, 1e-3, 50.0, None, 1, ptr(d_raw), _stream()),
            lib.gsr_frame_normal8(W, H, Cn, ptr(im), 1e-3, None, ptr(n_cam), _stream()),
            lib.gsr_frame_normal8(W, H, Cn, ptr(im), 1e-3, rot9, ptr(n_world), _stream()),
            lib.gsr_pick_point(W, H, Cn, ptr(im), C.byref(cs), px, py, 4, ptr(out4), _stream()),
            lib.gsr_pick_point(W, H, Cn, ptr(im), C.byref(cs_bare), px, py, 4, ptr(out4_bare), _stream()),
        ]
        assert calls == [0] * len(calls), (tag, calls, lib.gsr_last_error_string().decode())
        torch.cuda.synchronize()
        assert P.check() == [], (tag, P.check())
        P.assert_inputs_unchanged()
        got = {k: v.clone().contiguous().view(-1).view(U8) for k, v in
               dict(stats=stats, d_dev=d_dev, d_max=d_max, d_raw=d_raw, n_cam=n_cam, n_world=n_world, out4=out4, out4_bare=out4_bare).items()}
        if ref is None:
            ref = got
            want = fr.depth_stats(frame, 90.0)
            assert np.array_equal(stats.cpu().numpy().view(np.uint32), fr.stats_words(want)), tag
            assert np.array_equal(d_dev.cpu().numpy(), fr.depth16(frame, want["scale"]))
            assert np.array_equal(d_max.cpu().numpy(), fr.depth16(frame, f32(4.0)))
            assert np.array_equal(d_raw.cpu().numpy(), fr.depth16(frame, f32(50.0), False, flip_rows=True))
            assert np.array_equal(n_cam.cpu().numpy(), fr.normal8(frame))
            assert np.array_equal(n_world.cpu().numpy(), fr.normal8(frame, ROT))
            o, ob = out4.cpu().numpy(), out4_bare.cpu().numpy()
            win = fr.pick_window(frame, px, py, 4)
            assert win.size > 0 and o[3] == win.size == ob[3]
            mean = float(np.mean(win.astype(np.float64)))
            assert abs(float(ob[2]) - mean) <= (win.size + 1) * 2.0 ** -24 * mean
            assert np.array_equal(o[:3].view(np.uint32), fr.pick_from_z(ob[2], W, H, cam, px, py).view(np.uint32))
            continue
        for k in got:
            assert torch.equal(got[k], ref[k]), (tag, k)
