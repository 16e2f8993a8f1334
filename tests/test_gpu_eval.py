"""The evaluation head on the MI355X: gsr_eval_metrics and gsr_frame_rgb8 (csrc/eval.hip) against the restatement
(eval_ref.py) — the SSIM map and the 8-bit picture bit for bit, the four scalars within one fp32 ulp of the float64 means —,
the identities that tie scoring to export, the loss head's numbers, and `validate` on a small scene.

Sizes, by the kernel's own extents: a wave owns 54 output columns with a halo of 5 and walks a strip of 32 rows (fixed:
eval.hip STRIP_H); a workgroup is the three channel waves of one strip; the final pass is one workgroup of 256 threads over
one partial row per wave.
  columns : 1, 4 / 5 / 6 (below, at, above the halo), 11 (the filter), 53 / 54 / 55 (below, at, above one strip), 109 (three
            strips), 130;
  rows    : 1, 3, 6, 8, 11, 12, 23, 35, and 31 / 32 / 33 (below, at, above the strip height), 37 / 38 (the second strip holds
            the halo exactly / one row more), 65 (three strips);
  partials: 4591 x 1 is the smallest frame whose launch leaves more partial rows (86 strips x 3 = 258) than one round of the
            final pass has threads; 487 x 257 (10 x 9 strips: 270 rows) is the same in two dimensions.

Tolerance of the scalars: the device sums the same fp32 per-pixel values in double in another order than numpy; the two
sums differ by less than n · 2^-53 relative, far below half an fp32 ulp, so after the one rounding to fp32 they can only
disagree across one rounding boundary: 1 ulp."""
import numpy as np
import pytest
import torch

import eval_ref as er
import scenes
from hip_helpers import dev

pytestmark = pytest.mark.gpu

f32 = np.float32
U8 = torch.uint8
SIZES = [(1, 1), (4, 3), (5, 6), (11, 11), (53, 8), (54, 8), (55, 23), (109, 12), (130, 35),
         (7, 31), (7, 32), (7, 33), (6, 37), (6, 38), (3, 65), (4591, 1), (487, 257)]
COMBOS = [(False, False), (False, True), (True, False), (True, True)]     # (sky, quantize)


@pytest.fixture(scope="module")
def EV(pkg):
    return pkg.evaluation


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=f32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _within_one_ulp(got, want):
    """|got - want| <= one fp32 ulp at want (want: float64)"""
    if np.isinf(want):
        return got == want
    return abs(float(got) - want) <= float(np.spacing(f32(abs(want))))


def _poisoned(shape, dtype=torch.float32):
    n = int(np.prod(shape)) * (4 if dtype == torch.float32 else 1)
    raw = torch.full((n,), 0xFF, dtype=U8, device="cuda")
    return raw.view(*shape) if dtype == U8 else raw.view(torch.float32).view(*shape)


_CASES = {}


def _case(orc, W, H, C):
    """inputs and, per (sky, quantize), the restatement (scored colours, map, float64 scalars): computed once, shared"""
    key = (W, H, C)
    if key not in _CASES:
        frame, sky, target = er.make_case(W, H, C, seed=W * 1000 + H + C)
        y = er.target_float(target)
        per = {}
        for use_sky, quant in COMBOS:
            if use_sky and C < 5:
                continue
            x = er.scored(frame, sky if use_sky else None, quant)
            m = er.ssim_map(orc, x, y)
            per[(use_sky, quant)] = (x, m, er.metrics64(x, y, m))
        _CASES[key] = (frame, sky, target, per)
    return _CASES[key]


def _score(EV, image, target, sky=None, quantize=False, with_map=True):
    """one call into poisoned out / map / scratch -> (out, map or None)"""
    H, W, _ = image.shape
    out = _poisoned((4,))
    smap = _poisoned((3, H, W)) if with_map else None
    scratch = _poisoned((EV.eval_scratch_bytes(W, H),), U8)
    EV.eval_metrics(image, target, sky, quantize, ssim_map=smap, out=out, scratch=scratch)
    torch.cuda.synchronize()
    return out, smap


@pytest.mark.parametrize("C", [3, 5, 8])
@pytest.mark.parametrize("W,H", SIZES)
def test_metrics_vs_restatement(EV, orc, W, H, C):
    frame, sky, target, per = _case(orc, W, H, C)
    if W * H >= 100:    # on the inputs alone: the frame holds what the quantiser and the composite have to survive
        rgb = frame[..., :3]
        assert (rgb < 0).any() and (rgb > 1).any() and (rgb == 0).any() and (rgb == 1).any()
        if C >= 5:
            a = frame[..., 4]
            assert ((a > 0) & (a < 1)).any() and (a < 0).any() and (a > 1).any()
    ti, ts, t8 = dev(frame), dev(sky), dev(target, U8)
    tf = dev(er.target_float(target))
    for (use_sky, quant), (x, m, want) in per.items():
        tag = (W, H, C, use_sky, quant)
        s = ts if use_sky else None
        out, smap = _score(EV, ti, t8, s, quant)
        # 1. the map, bit for bit
        assert _same_bits(smap.cpu().numpy(), m), tag
        # 2. the scalars within one fp32 ulp of the float64 means
        got = out.cpu().numpy()
        print(f"[{W}x{H} C={C} sky={use_sky} q={quant}] gpu {got} f64 {want}")
        for j, name in enumerate(("ssim", "mse", "psnr", "l1")):
            assert _within_one_ulp(got[j], want[j]), (tag, name, got[j], want[j])
        # 3. a second run into freshly poisoned buffers, without a map, and with the float form of the same target: same bits
        out2, smap2 = _score(EV, ti, t8, s, quant)
        out3, _ = _score(EV, ti, t8, s, quant, with_map=False)
        out4, smap4 = _score(EV, ti, tf, s, quant)
        for o in (out2, out3, out4):
            assert torch.equal(_bits(o), _bits(out)), tag
        assert torch.equal(_bits(smap2), _bits(smap)) and torch.equal(_bits(smap4), _bits(smap)), tag


@pytest.mark.parametrize("W,H", [(1, 1), (55, 23), (130, 35)])
def test_identical_inputs_score_exactly(EV, orc, W, H):
    frame, _, _, per = _case(orc, W, H, 3)
    x = per[(False, False)][0]
    out, smap = _score(EV, dev(frame), dev(x))
    got = out.cpu().numpy()
    assert got[0] == 1.0 and got[1] == 0.0 and got[2] == np.inf and got[3] == 0.0
    assert (smap == 1.0).all().item()


@pytest.mark.parametrize("C", [5, 8])
@pytest.mark.parametrize("W,H", [(1, 1), (55, 23), (130, 35), (7, 33)])
def test_sky_in_the_loads_equals_scoring_the_composite(EV, pkg, orc, W, H, C):
    frame, sky, target, _ = _case(orc, W, H, C)
    ti, ts, t8 = dev(frame), dev(sky), dev(target, U8)
    comp = pkg.sky_dome.composite_sky(ti, ts)
    for quant in (False, True):
        a, ma = _score(EV, ti, t8, ts, quant)
        b, mb = _score(EV, comp, t8, None, quant)
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(ma), _bits(mb)), (W, H, C, quant)
    assert torch.equal(EV.frame_rgb8(ti, ts), EV.frame_rgb8(comp))


@pytest.mark.parametrize("C", [3, 5, 8])
@pytest.mark.parametrize("W,H", [(1, 1), (4, 3), (55, 23), (130, 35), (7, 33)])
def test_export_and_scoring_share_the_quantiser(EV, orc, W, H, C):
    """frame_rgb8 against the restatement, with and without the sky frame and flip_rows, into poisoned bytes; and
    quantize=True on a frame == quantize=False on its exported picture fed back as floats u · (1/255)."""
    frame, sky, target, _ = _case(orc, W, H, C)
    ti, ts, t8 = dev(frame), dev(sky), dev(target, U8)
    inv = torch.tensor(er.INV255, device="cuda")
    for use_sky in ((False, True) if C >= 5 else (False,)):
        s, s_host = (ts, sky) if use_sky else (None, None)
        for flip in (False, True):
            pic = EV.frame_rgb8(ti, s, flip, out=_poisoned((H, W, 3), U8))
            assert np.array_equal(pic.cpu().numpy(), er.rgb8(frame, s_host, flip)), (W, H, C, use_sky, flip)
        pic = EV.frame_rgb8(ti, s)
        back = (pic.to(torch.float32) * inv).contiguous()              # an (H, W, 3) frame of the levels as floats
        assert _same_bits(back.cpu().numpy(), er.target_float(pic.cpu().numpy()).transpose(1, 2, 0))
        a, ma = _score(EV, ti, t8, s, True)
        b, mb = _score(EV, back, t8, None, False)
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(ma), _bits(mb)), (W, H, C, use_sky)
        # ... and the exported picture is a valid byte target: scoring the quantised frame against it is exact
        c, _ = _score(EV, ti, pic, s, True)
        assert c[1].item() == 0.0 and c[2].item() == np.inf and c[3].item() == 0.0


def test_quantiser_on_the_tie_set_as_a_frame(EV):
    """The 8 415 inputs around the rounding boundaries (k + 0.5) / 255, laid out as a 55 x 51 frame: the device's levels are
    the as-written fp32 expression's at every one of them (rintf, a float -> uint8 conversion and double arithmetic differ
    at 128 or more)."""
    frame = er.tie_frame()
    H, W, _ = frame.shape
    ti = dev(frame)
    for flip in (False, True):
        assert np.array_equal(EV.frame_rgb8(ti, None, flip).cpu().numpy(), er.rgb8(frame, None, flip))
    lv = er.levels(frame)
    assert int((np.floor(frame.astype(np.float64) * 255.0 + 0.5) != lv).sum()) == 128
    # the same levels through the scoring path: against a zero target MSE is the mean of the squared levels
    zero = torch.zeros((H, W, 3), dtype=U8, device="cuda")
    out, _ = _score(EV, ti, zero, None, True)
    q = (lv * er.INV255).astype(f32)
    assert _within_one_ulp(out[1].item(), float(np.mean(q.astype(np.float64) ** 2)))
    assert _within_one_ulp(out[3].item(), float(np.mean(q.astype(np.float64))))


@pytest.mark.parametrize("W,H", [(55, 23), (130, 35), (64, 48), (1, 1), (54, 32), (55, 33), (109, 65)])
def test_cross_check_with_the_loss_head(EV, pkg, W, H):
    """At gsr_ssim_precision(1), no sky, no quantiser: the map is gsr_ssim_forward's exact map bit for bit, and out[0] and
    out[3] reproduce gsr_loss_l1_ssim's loss (1 - λ) · L1 + λ · (1 - mean SSIM) to its stated 1e-6 absolute.  Both kernels walk
    the strips of csrc/ssim_strip.h and cut them differently (eval.hip: 32 rows; ssim.hip: 8..64 per launch): 54 / 55 columns
    are one / two strip columns, 32 / 33 and 65 rows one / two and three of eval.hip's strip rows."""
    FS = pkg.fused_ssim
    r = np.random.default_rng(W + H)
    frame = r.uniform(0.0, 1.0, (H, W, 3)).astype(f32)
    tgt = pkg.synthetic.make_target(W, H, 5)
    ti, tt = dev(frame), dev(tgt)
    out, smap = _score(EV, ti, tt)
    rast = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgb")
    try:
        with FS.exact_arithmetic():
            x = ti.permute(2, 0, 1).contiguous()[None]
            m = FS._fused_ssim(x, tt[None].contiguous(), float(f32(0.01) ** 2), float(f32(0.03) ** 2), train=False)[0]
            lam = 0.2
            loss, _ = FS.l1_ssim_loss(rast, ti, tt, lam)
            torch.cuda.synchronize()
        assert torch.equal(_bits(m[0]), _bits(smap))
        mine = (1.0 - lam) * float(out[3].item()) + lam * (1.0 - float(out[0].item()))
        print(f"[{W}x{H}] loss head {loss.item():.9g} from eval {mine:.9g}")
        assert abs(mine - float(loss.item())) <= 1e-6
    finally:
        rast.close()


def test_validate_on_a_small_scene(EV, pkg, orc, monkeypatch):
    """64 x 48, 3 views, :rgbd with a small dome: `validate` equals the fp32 mean of per-view eval_metrics calls bit for bit,
    and the restatement on the frames within the scalars' tolerance — on the oracle's frames where the HIP frames equal them
    bit for bit, else on the HIP frames copied to the host.  One device -> host copy of results."""
    SD = pkg.sky_dome
    W, H, deg, V = 64, 48, 1, 3
    gt = pkg.synthetic.make_scene(400, W, H, deg, 77, sigma_px=4.0)
    cams = [pkg.Camera(W, H, tuple(gt.focal), (0.5, 0.5), *pkg.synthetic.view_pose(j + 2)) for j in range(V)]
    rast = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgbd")
    t = [dev(gt.means), dev(gt.shs), dev(gt.opacities.reshape(-1, 1)), dev(gt.scales), dev(gt.rotations)]
    sky = SD.SkyDome(cams[0], 1024, "sphere", radius=50.0, color=(0.3, 0.5, 0.8))
    r = np.random.default_rng(9)
    targets = [r.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(V)]
    tdev = [dev(x, U8) for x in targets]
    try:
        reads = []
        real = EV._read_back
        monkeypatch.setattr(EV, "_read_back", lambda x: (reads.append(tuple(x.shape)), real(x))[1])
        for quant in (False, True):
            reads.clear()
            got = EV.validate(rast, t[0], (t[1], t[2], t[3]), t[4], cams, tdev, deg, (0.0, 0.0, 0.0), sky=sky, quantize=quant)
            assert reads == [(V, 4)], reads
            rows, want_rows = [], []
            for v, cam in enumerate(cams):
                img = rast.forward_raw(*t, cam, deg, (0.0, 0.0, 0.0), forward_only=True).clone()
                sky_rgb = SD.render_sky(sky, cam, forward_only=True).clone()
                rows.append(EV.eval_metrics(img, tdev[v], sky_rgb, quant).cpu().numpy())
                frame, sframe = img.cpu().numpy(), sky_rgb.cpu().numpy()
                ocam = orc.Camera(W, H, tuple(gt.focal), R=np.asarray(cam.R, f32), t=np.asarray(cam.t, f32))
                oframe = orc.forward(gt.means, gt.shs, gt.opacities, gt.scales, gt.rotations, ocam, deg, background=(0, 0, 0), mode="rgbd").image
                if _same_bits(frame, oframe):
                    frame = oframe
                print(f"[view {v}] HIP frame == oracle frame bit for bit: {frame is oframe}")
                x, y = er.scored(frame, sframe, quant), er.target_float(targets[v])
                want_rows.append(er.metrics64(x, y, er.ssim_map(orc, x, y)))
                for j in range(4):
                    assert _within_one_ulp(rows[-1][j], want_rows[-1][j]), (quant, v, j)
            mean = EV.average_views(np.stack(rows))
            assert got == mean and set(got) == {"eval_ssim", "eval_mse", "eval_psnr", "eval_l1"}
            assert 0.0 < got["eval_mse"] < 1.0 and np.isfinite(got["eval_psnr"]) and -1.0 <= got["eval_ssim"] <= 1.0
        # without a dome the same call scores the bare render; no views: zeros, and nothing is rendered or read back
        reads.clear()
        bare = EV.validate(rast, t[0], (t[1], t[2], t[3]), t[4], cams, tdev, deg)
        assert reads == [(V, 4)] and bare != got
        assert EV.validate(rast, t[0], (t[1], t[2], t[3]), t[4], [], [], deg) == dict(eval_ssim=0.0, eval_mse=0.0, eval_psnr=0.0, eval_l1=0.0)
        assert reads == [(V, 4)]
    finally:
        sky.close()
        rast.close()


def test_error_codes_and_host_refusals(EV, pkg):
    L, lib = pkg._lib, pkg._lib.load()
    for what, rc, msg in er.rejected_calls(lib):
        assert rc == L.GSR_E_INVALID_ARG and msg, what
    img = torch.zeros((4, 6, 5), device="cuda")
    with pytest.raises(ValueError, match="image must be"):
        EV.eval_metrics(torch.zeros((4, 6, 2), device="cuda"), torch.zeros((3, 4, 6), device="cuda"))
    with pytest.raises(ValueError, match="alpha row"):
        EV.eval_metrics(torch.zeros((4, 6, 3), device="cuda"), torch.zeros((3, 4, 6), device="cuda"), torch.zeros((4, 6, 3), device="cuda"))
    with pytest.raises(ValueError, match="target must be"):
        EV.eval_metrics(img, torch.zeros((4, 6, 3), device="cuda"))              # a float target is (3, H, W)
    with pytest.raises(ValueError, match="target must be"):
        EV.eval_metrics(img, torch.zeros((3, 4, 6), dtype=U8, device="cuda"))    # a byte target is (H, W, 3)
    with pytest.raises(ValueError, match="target must be"):
        EV.eval_metrics(img, torch.zeros((3, 4, 6), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="ssim_map must be"):
        EV.eval_metrics(img, torch.zeros((3, 4, 6), device="cuda"), ssim_map=torch.zeros((4, 6, 3), device="cuda"))
    with pytest.raises(ValueError, match="scratch must be"):
        EV.eval_metrics(img, torch.zeros((3, 4, 6), device="cuda"), scratch=torch.zeros(8, dtype=U8, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        EV.frame_rgb8(img, out=torch.zeros((4, 6, 3), device="cuda"))
