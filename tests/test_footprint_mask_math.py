"""The arithmetic of the per-instance footprint masks (csrc/tile_mask.h instance_row_mask), without a GPU: the numpy fp32
restatement of the mask word (tests/footprint_ref.py mask_words) against the restatement of the kernels' own blend test,
bits(sigma) < X on the tile's 256 pixel centres, on seeded hostile instances — axis ratios to 100 : 1, axes of 0.3 .. 300 px,
a fifth of the opacities within 0.02 of 1/255, centres up to three standard deviations outside the tile.

  * conservative: no active pixel outside a flagged row or a flagged quadrant;
  * tight: flagged rows <= 1.25 x active rows + 16, the bound tests/test_gpu_parity.py test_footprint_masks_are_conservative
    holds the library to.

The restatement is part of the mask's specification: the derivation (the clamped vertex of a convex parabola per row and half,
one slack ts = S + 2e-3 + 4e-6·M per instance, sign bits instead of compares) is written out in csrc/tile_mask.h."""
import numpy as np

import footprint_ref as fr

N, SEED, CHUNK = 120_000, 20240611, 20_000


def test_threshold_bits_is_the_last_sigma_that_passes():
    o = np.array([1.0, 0.99, 0.5, 0.02, 1.0 / 255.0 + 1e-6, 1.0 / 255.0, 0.00392, 0.0039, 1e-4, 0.0, np.nan], np.float32)
    X = fr.threshold_bits(o)
    amin = np.float32(1.0) / np.float32(255.0)

    def passes(bits):
        g = np.exp(-bits.astype(np.uint32).view(np.float32).astype(np.float64)).astype(np.float32)
        with np.errstate(invalid="ignore"):
            return np.minimum(np.float32(0.99), o * g) >= amin

    some = X > 0
    assert some[:5].all() and not some[7:].any()
    assert passes(np.where(some, X - 1, 0))[some].all() and not passes(X)[some].any() and not passes(np.zeros_like(X))[~some].any()
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = np.log(255.0 * o[some].astype(np.float64))
    assert np.abs((X[some] - 1).view(np.float32) - np.maximum(tau, 0.0)).max() <= 1e-5


def test_restated_masks_are_conservative_and_tight_on_hostile_instances():
    miss_rows = miss_quads = act_rows = flag_rows = act_quads = flag_quads = partial = 0
    for k in range(0, N, CHUNK):
        mx, my, a, b, c, o, X0, Y0 = fr.hostile_instances(CHUNK, [SEED, k])
        X = fr.threshold_bits(o)
        act = fr.active_pixels(mx, my, a, b, c, X, X0, Y0)
        words = fr.mask_words(mx, my, a, b, c, X, X0, Y0)
        r = fr.check_masks(words, act)
        miss_rows += r[0]; miss_quads += r[1]; act_rows += r[2]; flag_rows += r[3]; act_quads += r[4]; flag_quads += r[5]
        nrows = np.array([bin(int(w) & 0xFFFF).count("1") for w in words])
        partial += int(((nrows >= 1) & (nrows <= 15)).sum())
        assert not words[X == 0].any(), "an opacity below 1/255 is never flagged"
    print(f"instances {N}: rows active {act_rows} flagged {flag_rows} ({flag_rows / act_rows:.4f}), quadrants active {act_quads} "
          f"flagged {flag_quads}, partly flagged instances {partial}")
    assert miss_rows == 0 and miss_quads == 0
    assert partial >= N // 10 and act_rows >= N, "the inputs exercise partial masks"
    assert flag_rows <= 1.25 * act_rows + 16
    assert flag_quads <= 1.25 * act_quads + 16


def test_degenerate_conic_and_subthreshold_opacity():
    f = lambda *v: np.array(v, np.float32)
    z = np.zeros(3, np.int64)
    X = fr.threshold_bits(f(0.5, 0.5, 0.001))
    w = fr.mask_words(f(8, 8, 8), f(8, 8, 8), f(0.0, np.nan, 0.1), f(0, 0, 0), f(0.1, 0.1, 0.1), X, z, z)
    assert list(w) == [0xFFFFF, 0xFFFFF, 0]
