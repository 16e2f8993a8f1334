"""-m gpu: the exact number of bytes a handle holds (gsr_memory_usage) after each step of create -> reserve -> reserve again ->
forward + backward -> release_scene_buffers, per render mode and image size.  The sizes of the handle's buffers are written in
one place (csrc/gsr_sizes.h) and used by gsr_reserve, the forward, the backward and gsr_buffer; this file holds them to numbers
that were NOT computed by that code:

  * EXPECT: what the library printed at commit 06352cf — before the size table existed, when every call site still carried its
    own expressions — for each (mode, image size): bytes after gsr_create, after gsr_reserve(257, 1031), after one forward +
    backward of a 257-Gaussian scene on a fresh handle, and after gsr_release_scene_buffers.
  * the closed forms below for the steps whose sizes do not depend on the scene (create, reserve, release), written out here
    from include/gsr.h's description of the buffers; every capacity is rounded up to 256 bytes.

Every call is a valid one: nothing is provoked."""
import numpy as np
import pytest
import torch

from hip_helpers import dev

pytestmark = pytest.mark.gpu

N, D, DEG, BG = 257, 1031, 1, (0.1, 0.2, 0.3)
SIZES = ((1, 1), (33, 17), (130, 70))
MODES = ("rgb", "rgbd", "rgbdn")

# (mode, W, H) -> bytes after (create, reserve(257, 1031), forward + backward on a fresh handle, release_scene_buffers),
# as printed by this test's body on the library of commit 06352cf
EXPECT = {
    ("rgb", 1, 1): (2048, 176640, 96768, 2048),
    ("rgb", 33, 17): (6144, 180736, 189440, 6144),
    ("rgb", 130, 70): (75520, 250112, 334336, 75520),
    ("rgbd", 1, 1): (2048, 193280, 102144, 2048),
    ("rgbd", 33, 17): (6144, 197376, 201984, 6144),
    ("rgbd", 130, 70): (75520, 266752, 363520, 75520),
    ("rgbdn", 1, 1): (2048, 197632, 107520, 2048),
    ("rgbdn", 33, 17): (6144, 201728, 212224, 6144),
    ("rgbdn", 130, 70): (75520, 271104, 369152, 75520),
}


def up(b):
    return (b + 255) // 256 * 256


def create_bytes(W, H):
    T, P = ((W + 15) // 16) * ((H + 15) // 16), W * H
    #      ranges       n_contrib, final_T   tile_count        tile_start        tile_order        totals   big_list
    return up(2 * T * 4) + 2 * up(P * 4) + up((T + 2) * 4) + up((T + 1) * 4) + up((T + 8) * 4) + up(8 * 4) + up((3 * T + 1) * 4)


def reserve_bytes(n, d, C):
    nb = (n + 255) // 256
    #         geo          radii       bsum, bpre, bvis       vmean2d     pose_part (12 floats per 256 Gaussians)
    per_n = up(n * 64) + up(n * 4) + 3 * up((nb + 1) * 4) + up(n * 8) + up(nb * 12 * 4) + (up(n * 16) if C > 5 else 0)  # gnormal
    #         values_sorted  s0, s1, s2        s3                                rows: 1.5 slots of 64 bytes per instance
    per_d = up(d * 4) + 3 * up(d * 16) + (up(d * 16) if C > 3 else 0) + up(d * 96)
    return per_n + per_d


@pytest.mark.parametrize("W,H", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("mode", MODES)
def test_handle_bytes_at_every_step(pkg, mode, W, H):
    L = pkg._lib
    C = L.MODES[mode]
    usage = lambda r: int(L.load().gsr_memory_usage(r._h))  # noqa: E731
    got = []
    a = pkg.rasterizer.GaussianRasterizer(W, H, mode=mode)
    b = pkg.rasterizer.GaussianRasterizer(W, H, mode=mode)
    try:
        got.append(usage(a))                                  # 1: after gsr_create
        a.reserve(N, D)
        got.append(usage(a))                                  # 2: after gsr_reserve(257, 1031)
        live = a._forward_live()
        a.reserve(N, D)
        again, live_again = usage(a), a._forward_live()       # 3: an identical reserve allocates nothing, ends nothing
        seed = 7 + C + W
        s = pkg.synthetic.make_scene(N, W, H, DEG, seed, sigma_px=4.0)
        t = [dev(s.means), dev(s.shs), dev(s.opacities.reshape(-1, 1)), dev(s.scales), dev(s.rotations)]
        cam = pkg.Camera(W, H, tuple(s.focal))
        vp = dev(np.random.default_rng(seed).standard_normal((H, W, C)).astype(np.float32))
        for r in (a, b):
            r.forward_raw(*t, cam, DEG, BG)
            r.backward_raw(vp, *t, cam, DEG, BG)
        torch.cuda.synchronize()
        # (3, where a forward is live: the reserved handle holds at least reserve(257, 1031) of everything, so the same reserve
        # once more reallocates nothing and the forward stays live)
        held = usage(a)
        a.reserve(N, D)
        assert usage(a) == held and a._forward_live()
        got.append(usage(b))                                  # 4: after one forward + backward on a fresh handle
        b.release_scene_buffers()
        got.append(usage(b))                                  # 5: after gsr_release_scene_buffers
    finally:
        a.close()
        b.close()
    print(f"HANDLE_BYTES ({mode!r}, {W}, {H}): {tuple(got)}, again={again} live={live} D={int(b.stats.n_rendered)}")
    assert again == got[1] and live_again == live
    assert got[0] == create_bytes(W, H)
    assert got[1] == create_bytes(W, H) + reserve_bytes(N, D, C)
    assert got[3] == create_bytes(W, H)                       # (no loss head, no long list: only gsr_create's buffers are left)
    assert tuple(got) == EXPECT[(mode, W, H)]

