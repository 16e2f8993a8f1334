"""The geometry frames without a GPU: the restatement (frames_ref.py) against independent implementations — numpy's own sort
order and `np.quantile` —, the 16-bit quantiser on its tie set, the adversarial depth sets, and the refusals of the Python
wrappers (geometry_frames.py) before any library call."""
import numpy as np
import pytest

import frames_ref as fr

f32 = np.float32


@pytest.fixture(scope="module")
def GF(pkg):
    return pkg.geometry_frames


def test_key_order_is_the_sort_order():
    """Unsigned order of the keys == numpy's ascending order of the floats, with -0.0 in front of +0.0; the map is a bijection."""
    r = np.random.default_rng(11)
    special = np.array([-0.0, 0.0, 1e-45, -1e-45, 3e-39, -3e-39, 1.17549435e-38, -1.17549435e-38, 1.0, -1.0, 3.4028235e38,
                        -3.4028235e38, np.inf, -np.inf], f32)
    x = np.concatenate([special, r.normal(0, 10, 4000).astype(f32), r.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32).view(f32)])
    x = x[~np.isnan(x)]
    k = fr.keys(x)
    assert np.array_equal(fr.values(k).view(np.uint32), x.view(np.uint32))
    by_key = x[np.argsort(k, kind="stable")]
    assert np.array_equal(by_key, np.sort(x))                       # as values (np.sort does not order the zeros)
    zeros = by_key[by_key == 0]
    signs = np.signbit(zeros)
    assert signs.any() and not signs.all() and np.array_equal(signs, np.sort(signs)[::-1])   # every -0.0 in front of every +0.0
    assert fr.keys(f32(-0.0)) + 1 == fr.keys(f32(0.0))
    # equal keys <=> equal bits; strictly larger value => strictly larger key
    s = np.sort(x)
    assert (np.diff(fr.keys(s).astype(np.int64))[np.diff(s) > 0] > 0).all()


def test_scale_against_numpy_quantile():
    """The restated rank and interpolation against np.quantile(float64 values, p, method="linear") — Hyndman-Fan 7, the same
    definition from an independent implementation — to one fp32 ulp, over a few hundred random (n, p)."""
    r = np.random.default_rng(5)
    worst = 0.0
    for it in range(300):
        n = int(r.integers(2, 3000)) if it % 3 else int(r.integers(2, 12))
        pct = float(r.uniform(0.0, 100.0)) if it % 5 else (100.0, 50.0, 99.0, 1e-4, 1.0)[(it // 5) % 5]
        if pct == 0.0:
            continue
        v = np.sort(r.uniform(0.25, 80.0, n).astype(f32))
        j, gamma = fr.rank(n, pct)
        assert 1 <= j <= n - 1 and 0.0 <= gamma <= 1.0
        got = fr.scale_from(v[j - 1], v[j], gamma)
        want = np.quantile(v.astype(np.float64), pct / 100.0, method="linear")
        err = abs(float(got) - want) / float(np.spacing(f32(want)))
        worst = max(worst, err)
        assert err <= 1.0, (n, pct, got, want)
    print(f"worst distance to np.quantile: {worst:.3f} ulp")
    assert fr.rank(1000, 100.0) == (999, 1.0) and fr.rank(1000, 1e-4)[0] == 1 and fr.rank(2, 50.0) == (1, 0.5)


def test_depth_stats_of_the_adversarial_sets():
    """What make_case promises of each kind, from the restatement alone."""
    for W, H in ((55, 23), (130, 67)):
        st = fr.depth_stats(fr.make_case(W, H, 5, 1, "none"), 99.0)
        assert st["n"] == 0 and st["scale"] == 1 and st["a_bits"] == st["b_bits"] == 0
        st = fr.depth_stats(fr.make_case(W, H, 5, 2, "one"), 99.0)
        assert st["n"] == 1 and st["a_bits"] == st["b_bits"]
        assert fr.depth_stats(fr.make_case(W, H, 5, 3, "two"), 50.0)["n"] == 2
        st = fr.depth_stats(fr.make_case(W, H, 8, 4, "equal"), 50.0)
        assert st["n"] > 2 and st["a_bits"] == st["b_bits"] == int(np.array([2.5], f32).view(np.uint32)[0]) and st["scale"] == 2.5
        st = fr.depth_stats(fr.make_case(W, H, 5, 5, "lowbits"), 50.0)
        assert st["a_bits"] >> 14 == st["b_bits"] >> 14 == 0x40490000 >> 14 and st["a_bits"] <= st["b_bits"]
        for pct in (99.0, 100.0, 50.0, 1e-4):
            st = fr.depth_stats(fr.make_case(W, H, 5, 6, "clusters", pct), pct)
            ka, kb = fr.keys(np.array([st["a_bits"]], np.uint32).view(f32)), fr.keys(np.array([st["b_bits"]], np.uint32).view(f32))
            assert ka[0] >> 21 != kb[0] >> 21, pct                  # different top-level bins of an 11-bit first level
        frame = fr.make_case(W, H, 5, 7, "signed")
        e = fr.expected_depth(frame)[fr.covered_mask(frame)]
        assert (e < 0).any() and np.signbit(e[e == 0]).any() and (~np.signbit(e[e == 0])).any()
        assert ((np.abs(e) < f32(1.17549435e-38)) & (e != 0)).any()
        frame = fr.make_case(W, H, 8, 8, "random")
        a = frame[..., 4].reshape(-1)
        assert a[0] == fr.MIN_ALPHA and a[1] < fr.MIN_ALPHA and a[1] > 0 and a[2] == 0 and np.isnan(a).any()
        cov = fr.covered_mask(frame).reshape(-1)
        assert cov[0] and not cov[1] and not cov[2]
        n8 = fr.normal8(frame).reshape(-1, 3)
        assert tuple(n8[3]) == (128, 128, 128) and tuple(n8[4]) == (128, 255, 128)   # length just under 1e-6: zero; at 1e-6: unit
        assert (n8[~cov] == 128).all()


def test_word_quantiser_on_the_tie_set():
    """Inputs around the rounding boundaries (k + 0.5) / 65535: the as-written fp32 expression equals its closed form (the
    exact product and the exact sum, each rounded once to fp32), lands on k or k + 1, and is monotone."""
    t, k = fr.word_tie_set()
    assert t.size == 9 * 256 and t.dtype == f32
    w = fr.words(t)
    assert np.array_equal(w, fr.words_closed_form(t))
    assert ((w == k) | (w == k + 1)).all() and (w == k).any() and (w == k + 1).any()
    assert (np.diff(w.astype(np.int64)) >= 0).all()
    assert list(fr.words(np.array([0.0, 1.0, 0.5], f32))) == [0, 65535, 32768]
    # round-trip: the value a word stands for quantises to that word
    allw = np.arange(65536, dtype=np.int64)
    assert np.array_equal(fr.words((allw.astype(np.float64) / 65535.0).astype(f32)), allw.astype(np.uint16))
    # through the encoder: clamping, a NaN depth, and the white level
    frame = np.zeros((1, 6, 5), f32)
    frame[0, :, 4] = 1.0
    frame[0, :, 3] = (-1.0, 0.0, 2.5, 5.0, 7.0, np.nan)
    assert list(fr.depth16(frame, f32(5.0))[0]) == [0, 0, 32768, 65535, 65535, 0]
    assert list(fr.depth16(frame, f32(5.0), flip_rows=True)[0]) == [0, 0, 32768, 65535, 65535, 0]


def test_pick_restatement():
    frame = np.zeros((5, 7, 4), f32)
    frame[..., 3] = np.arange(35, dtype=f32).reshape(5, 7) * f32(0.01)     # 0.00, 0.01, ...: the first two are not > 1e-2
    assert fr.pick_window(frame, 0, 1, 4) is None and fr.pick_window(frame, 8, 1, 4) is None and fr.pick_window(frame, 1, 6, 0) is None
    assert fr.pick_window(frame, 1, 1, 0).size == 0 and fr.pick_window(frame, 3, 1, 0).size == 1
    assert fr.pick_window(frame, 1, 1, 1).size == 2 and fr.pick_window(frame, 4, 3, 16).size == 33
    from types import SimpleNamespace
    cam = SimpleNamespace(focal=(10.0, 12.0), principal=(0.5, 0.5), R=np.eye(3, dtype=f32), camera_center=np.array([1.0, 2.0, 3.0], f32))
    got = fr.pick_from_z(2.0, 7, 5, cam, 4, 3)            # the centre pixel: on the axis
    assert np.array_equal(got, np.array([1.0, 2.0, 5.0], f32))


def test_wrappers_refuse_before_any_library_call(GF, pkg, monkeypatch):
    import torch

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(pkg._lib, "load", no_library)
    cam = pkg.Camera(6, 4, (10.0, 10.0))
    host = torch.zeros((4, 6, 8))                                      # the wrong device
    for pct in (0.0, -1.0, 100.5, float("nan")):
        with pytest.raises(ValueError, match="percentile"):
            GF.depth_scale(host, percentile=pct)
        with pytest.raises(ValueError, match="percentile"):
            GF.frame_depth16(host, percentile=pct)
    with pytest.raises(ValueError, match="min_alpha"):
        GF.depth_scale(host, min_alpha=0.0)
    with pytest.raises(ValueError, match="min_alpha"):
        GF.frame_normal8(host, min_alpha=float("nan"))
    for dm in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="depth_max"):
            GF.frame_depth16(host, depth_max=dm)
    with pytest.raises(ValueError, match="half_window"):
        GF.pick_point(host, cam, 1, 1, half_window=17)
    with pytest.raises(ValueError, match="half_window"):
        GF.pick_point(host, cam, 1, 1, half_window=-1)
    bad = [host, torch.zeros((4, 6, 8), dtype=torch.float64), torch.zeros((4, 6)), torch.zeros((2, 4, 6, 8)), np.zeros((4, 6, 8), f32), None]
    for image in bad:
        for call in (lambda: GF.depth_scale(image), lambda: GF.frame_depth16(image), lambda: GF.frame_depth16(image, depth_max=5.0),
                     lambda: GF.viewer_depth16(image), lambda: GF.frame_normal8(image), lambda: GF.pick_point(image, cam, 1, 1)):
            with pytest.raises(ValueError, match="image must be"):
                call()
    with pytest.raises(ValueError, match="R_c2w"):
        GF._rotation9(np.eye(4))
    assert list(GF._rotation9(np.arange(9).reshape(3, 3))) == [0, 3, 6, 1, 4, 7, 2, 5, 8]    # column-major
    with pytest.raises(ValueError, match="rgbdn"):
        GF.render_views(type("R", (), dict(mode="rgbd", width=6, height=4))(), host, (host, host, host), host, [cam], 0)


def test_every_rejected_call(GF, pkg):
    """The invalid-argument table of the five entry points: refused on the arguments alone, with a message, GPU or not."""
    import ctypes as C
    L, lib = pkg._lib, pkg._lib.load()
    cam = C.byref(GF.camera_struct(pkg.Camera(8, 8, (10.0, 10.0)), 8, 8))
    table = fr.rejected_calls(lib, cam)
    assert len(table) > 50
    for what, rc, msg in table:
        assert rc == L.GSR_E_INVALID_ARG and msg, what
    assert lib.gsr_frames_scratch_bytes(0, 5) == 0 and lib.gsr_frames_scratch_bytes(5, -1) == 0
    assert lib.gsr_frames_scratch_bytes(1, 1) == 32840 and lib.gsr_frames_scratch_bytes(1920, 1080) == 32832 + 4 * 1920 * 1080
