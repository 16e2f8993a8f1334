"""The evaluation head without a GPU: the restatement's known answers (runtests.jl:496-520, utils.jl:107-109), the
quantiser on its rounding boundaries against a committed table, `validate`'s averaging, the new exports and the calls the
C ABI refuses before it touches a device."""
import os

import numpy as np
import pytest

import eval_ref as er

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantize8_ties.npz")


@pytest.fixture(scope="module")
def EV(pkg):
    return pkg.evaluation


# "SSIM" — runtests.jl:496-510 — and mse / psnr — utils.jl:107-109
def test_known_answers(orc):
    ones, zeros = np.ones((3, 16, 16), f32), np.zeros((3, 16, 16), f32)
    s, mse, psnr, l1 = er.metrics64(ones, ones, er.ssim_map(orc, ones, ones))
    assert s == 1.0 and mse == 0.0 and psnr == np.inf and l1 == 0.0
    s, mse, psnr, l1 = er.metrics64(ones, zeros, er.ssim_map(orc, ones, zeros))
    assert abs(s) <= 1e-4 and mse == 1.0 and psnr == 0.0 and l1 == 1.0
    x = np.zeros((3, 16, 16), f32)          # the reference's (W, H) blocks, as (H, W) here
    x[:, 0:4, 0:4], x[:, 0:4, 4:8], x[:, 12:16, 8:12], x[:, 12:16, 12:16] = 0.25, 0.5, 0.75, 1.0
    assert abs(er.metrics64(x, ones, er.ssim_map(orc, x, ones))[0] - 0.1035) <= 1e-3 + 1e-3 * 0.1035
    # a constant offset of 0.1 is 20 dB, to the rounding of the fp32 difference
    y = np.full((3, 7, 5), 0.25, f32)
    _, mse, psnr, l1 = er.metrics64(y + f32(0.1), y, np.ones_like(y))
    assert abs(psnr - 20.0) <= 20.0 * 2.0 ** -22 and abs(l1 - 0.1) <= 2.0 ** -24 and abs(mse - 0.01) <= 0.01 * 2.0 ** -22
    # ... and agrees with the reference's host expression 20·log10(1 / sqrt(mse)) in Float32 to fp32 rounding
    ref = f32(20) * np.log10(f32(1) / np.sqrt(f32(mse)), dtype=f32)
    assert abs(float(ref) - psnr) <= 4 * np.spacing(f32(20))


def test_scored_colours_and_layouts():
    frame, sky, target = er.make_case(9, 4, 8, seed=3)
    rgb, alpha = frame[..., :3], frame[..., 4]
    assert (rgb < 0).any() and (rgb > 1).any() and (rgb == 0).any() and (rgb == 1).any()
    assert ((alpha > 0) & (alpha < 1)).any() and (alpha < 0).any() and (alpha > 1).any() and (alpha == 0).any() and (alpha == 1).any()
    x = er.scored(frame, sky, False)
    assert x.shape == (3, 4, 9) and x.dtype == f32
    assert x[1, 2, 3] == frame[2, 3, 1] + (f32(1) - frame[2, 3, 4]) * sky[2, 3, 1]
    q = er.scored(frame, sky, True)
    assert q.min() == 0.0 and q.max() == 1.0 and np.array_equal(q, er.levels(x) * er.INV255) and np.unique(q).size <= 256
    pic = er.rgb8(frame, sky)
    assert pic.shape == (4, 9, 3) and pic.dtype == np.uint8
    # scoring the quantised render == scoring the picture that would be written
    assert np.array_equal(er.target_float(pic), q)
    assert np.array_equal(er.rgb8(frame, sky, flip_rows=True), pic[::-1])
    assert np.array_equal(er.levels(np.array([-np.inf, np.inf, -0.0, 0.5], f32)), [0, 255, 0, 128])
    assert er.target_float(target).shape == (3, 4, 9) and er.target_float(target)[2, 0, 0] == f32(target[0, 0, 2]) * er.INV255


def test_quantiser_on_the_tie_set():
    """255 · 33 inputs around the rounding boundaries (k + 0.5) / 255.  The as-written fp32 expression differs there from
    round-to-nearest of the exact product at 128 inputs: rintf, a float -> uint8 conversion or double arithmetic fail it."""
    g = np.load(GOLDEN)
    t = er.tie_set()
    assert t.size == 8415 and t.dtype == f32 and np.array_equal(t.view(np.uint32), g["inputs"].view(np.uint32))
    lv = er.levels(t)
    assert g["levels"].dtype == np.uint8 and np.array_equal(lv, g["levels"].astype(f32))
    exact = np.floor(t.astype(np.float64) * 255.0 + 0.5)            # the product is exact in float64
    assert int((exact != lv).sum()) == 128
    assert int((np.rint(t.astype(np.float64) * 255.0) != lv).sum()) == 128
    assert (np.rint(t * f32(255)) != lv).any() and ((t * f32(255)).astype(np.uint8) != lv).any()
    assert np.array_equal(er.tie_frame().reshape(-1), t)


def test_validate_averaging(EV):
    r = np.random.default_rng(4)
    rows = r.uniform(0.0, 40.0, (7, 4)).astype(f32)
    rows[3, 2] = 35.123
    got = EV.average_views(rows)
    assert tuple(got) == ("eval_ssim", "eval_mse", "eval_psnr", "eval_l1") == EV.METRICS
    for j, k in enumerate(EV.METRICS):
        acc = f32(0)
        for v in rows[:, j]:
            acc = f32(acc + v)
        assert f32(got[k]).tobytes() == f32(acc / f32(7)).tobytes(), k
    # one view scored exactly: +Inf travels through the mean, as it does in the reference
    rows[2, 2] = np.inf
    assert EV.average_views(rows)["eval_psnr"] == np.inf
    # no test views: zeros, and nothing else is touched (training.jl:495-496)
    assert EV.average_views(np.zeros((0, 4), f32)) == dict(eval_ssim=0.0, eval_mse=0.0, eval_psnr=0.0, eval_l1=0.0)
    assert EV.validate(None, None, None, None, [], [], 0) == dict(eval_ssim=0.0, eval_mse=0.0, eval_psnr=0.0, eval_l1=0.0)
    with pytest.raises(ValueError, match="2 cameras, 1 targets"):
        EV.validate(None, None, None, None, [None, None], [None], 0)


def test_exports_and_refused_calls(pkg):
    L, lib = pkg._lib, pkg._lib.load()
    for name in ("gsr_eval_scratch_bytes", "gsr_eval_metrics", "gsr_frame_rgb8"):
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert lib.gsr_abi_version() == 6                       # new functions, no struct change
    for what, rc, msg in er.rejected_calls(lib):
        assert rc == L.GSR_E_INVALID_ARG and msg, what
    # one row of three doubles per wave: three waves per 54 x 32 strip
    assert lib.gsr_eval_scratch_bytes(0, 5) == 0 and lib.gsr_eval_scratch_bytes(5, -1) == 0
    assert lib.gsr_eval_scratch_bytes(54, 32) == 72 and lib.gsr_eval_scratch_bytes(55, 33) == 4 * 72
    assert pkg.evaluation.eval_scratch_bytes(1920, 1080) == 36 * 34 * 72


def test_host_mirror_rejects_cpu_tensors(EV):
    import torch
    with pytest.raises(ValueError, match="image must be"):
        EV.eval_metrics(torch.zeros(4, 4, 3), torch.zeros(3, 4, 4))
    with pytest.raises(ValueError, match="image must be"):
        EV.frame_rgb8(torch.zeros(4, 4, 3))
