"""gsr_eval_scratch_bytes, gsr_eval_metrics and gsr_frame_rgb8 on guarded arenas (tests/guarded.py) at both skews and both
guard fills: nothing outside out / ssim_map / scratch / rgb8_out is written, the inputs are unchanged, poisoned outputs do
not reach a result, and the results are the same bits in every placement.  Under skew "worst" the byte target and the
exported picture start at odd addresses and every float array at 4 mod 16: neither entry point may ask for more."""
import numpy as np
import pytest
import torch

import eval_ref as er
from guarded import placements
from hip_helpers import stream as _stream

pytestmark = pytest.mark.gpu

U8 = torch.uint8


@pytest.mark.parametrize("W,H,Cn", [(55, 23, 5), (55, 23, 8), (1, 1, 5), (1, 1, 3)])
def test_entry_points_on_guarded_buffers(pkg, orc, W, H, Cn):
    L, lib = pkg._lib, pkg._lib.load()
    frame, sky, target = er.make_case(W, H, Cn, seed=W + H + Cn)
    has_sky = Cn >= 5
    nb = int(lib.gsr_eval_scratch_bytes(W, H))
    assert nb == 72 * ((W + 53) // 54) * ((H + 31) // 32)
    tfloat = er.target_float(target)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    ref = None
    for P in placements(1 << 20, "cuda"):
        tag = f"{P.skew}/{P.fill}"
        im, sk = P.place("image", frame), P.place("sky_rgb", sky)
        t8, tf = P.place("target_u8", target, guard=(0, 255)), P.place("target_f32", tfloat)
        out, smap = P.place("out", (4,)), P.place("ssim_map", (3, H, W))
        scr = P.place("scratch", (nb,), U8, align=8, role="scratch")
        out2, scr2 = P.place("out_f32_target", (4,)), P.place("scratch_f32_target", (nb,), U8, align=8, role="scratch")
        pic, pic2 = P.place("rgb8_out", (H, W, 3), U8), P.place("rgb8_out_flipped", (H, W, 3), U8)
        if P.skew == "worst":
            assert t8.data_ptr() % 2 == 1 and pic.data_ptr() % 2 == 1 and im.data_ptr() % 16 == 4
        for t in (out, smap, scr, out2, scr2, pic, pic2):
            t.view(-1).view(U8).fill_(0xFF)
        s = ptr(sk) if has_sky else None
        calls = [
            lib.gsr_eval_metrics(W, H, Cn, ptr(im), s, None, ptr(t8), 1, ptr(smap), ptr(out), ptr(scr), _stream()),
            lib.gsr_eval_metrics(W, H, Cn, ptr(im), None, ptr(tf), None, 0, None, ptr(out2), ptr(scr2), _stream()),
            lib.gsr_frame_rgb8(W, H, Cn, ptr(im), s, 0, ptr(pic), _stream()),
            lib.gsr_frame_rgb8(W, H, Cn, ptr(im), None, 1, ptr(pic2), _stream()),
        ]
        assert calls == [0] * 4, (tag, calls, lib.gsr_last_error_string().decode())
        torch.cuda.synchronize()
        assert P.check() == [], (tag, P.check())
        P.assert_inputs_unchanged()
        got = {k: v.clone() for k, v in dict(out=out, smap=smap, out2=out2, pic=pic, pic2=pic2).items()}
        if ref is None:
            ref = got
            hs = sky if has_sky else None
            x = er.scored(frame, hs, True)
            m = er.ssim_map(orc, x, tfloat)
            assert np.array_equal(got["smap"].cpu().numpy().view(np.uint32), m.view(np.uint32)), tag
            x2 = er.scored(frame, None, False)
            for o, want in ((got["out"], er.metrics64(x, tfloat, m)), (got["out2"], er.metrics64(x2, tfloat, er.ssim_map(orc, x2, tfloat)))):
                for a, b in zip(o.cpu().numpy(), want):
                    assert abs(float(a) - b) <= float(np.spacing(np.float32(abs(b)))), (tag, a, b)
            assert np.array_equal(got["pic"].cpu().numpy(), er.rgb8(frame, hs))
            assert np.array_equal(got["pic2"].cpu().numpy(), er.rgb8(frame, None, True))
            continue
        for k in got:
            assert torch.equal(got[k].contiguous().view(-1).view(U8), ref[k].contiguous().view(-1).view(U8)), (tag, k)
