"""The evaluation head (src/training.jl:487-532 `validate`; utils.jl:107-109,118) restated for the tests: no product code.
Plain numpy, every fp32 operation as the kernels write it (csrc/eval.hip); the SSIM map is the CPU oracle's
(`oracle.ssim_forward(train=False)`).

- `scored`   : the colours a view is scored on — composite over the sky frame, then `quantize8`, planar (3, H, W).
- `metrics64`: float64 means of the oracle's fp32 per-pixel values, PSNR = -10·log10(MSE) in float64: what the device's
               double sums are held to.
- `rgb8`     : the 8-bit picture of the same colours.
- `tie_set`  : fp32 inputs around every rounding boundary (k + 0.5) / 255 of the quantiser.
- `make_case`: frames that hold values below 0, above 1, exact 0 and 1, and alpha inside (0, 1) and outside it.

Layouts: a frame is (H, W, C), the sky frame (H, W, 3), a float target and the map (3, H, W), a byte target and the picture
(H, W, 3) uint8."""
import numpy as np

f32 = np.float32
INV255 = f32(1.0) / f32(255.0)


def levels(x):
    """floor(clamp(x, 0, 1) · 255 + 0.5) as fp32, each operation rounded to fp32 in that order (utils.jl:118)."""
    x = np.asarray(x, f32)
    return np.floor(np.minimum(np.maximum(x, f32(0)), f32(1)) * f32(255) + f32(0.5))


def quantize8(x):
    return levels(x) * INV255


def scored(image, sky=None, quantize=False):
    """(3, H, W) fp32: image[c] (+ (1 - image[4]) · sky[c]: a product, then a sum — sky_dome.jl:246-250), then quantize8."""
    image = np.asarray(image, f32)
    x = image[..., :3]
    if sky is not None:
        t = f32(1) - image[..., 4]
        x = x + t[..., None] * np.asarray(sky, f32)
    x = np.ascontiguousarray(np.transpose(x, (2, 0, 1))).astype(f32)
    return quantize8(x) if quantize else x


def target_float(target):
    """A target as the kernel scores it, (3, H, W) fp32: a uint8 (H, W, 3) image is Float32(u) · (1/255) (dataset.jl:253-260)."""
    target = np.asarray(target)
    if target.dtype == np.uint8:
        return np.transpose(target.astype(f32) * INV255, (2, 0, 1)).copy()   # (a copy: canonical strides for 1 x 1 too)
    return np.ascontiguousarray(target, dtype=f32)


def ssim_map(orc, x, y):
    """fused_ssim.jl:34-238 with train = false on (3, H, W) planes: the oracle's map."""
    return orc.ssim_forward(x[None], y[None], train=False)[0][0]


def metrics64(x, y, smap):
    """(mean SSIM, MSE, PSNR, mean |x - y|) in float64 of the fp32 per-pixel values: the map, d = x - y, |d|; d² exactly."""
    d = (np.asarray(x, f32) - np.asarray(y, f32)).astype(f32)
    mse = float(np.mean(d.astype(np.float64) ** 2))
    with np.errstate(divide="ignore"):
        psnr = float(-10.0 * np.log10(np.float64(mse)))
    return float(np.mean(np.asarray(smap, f32).astype(np.float64))), mse, psnr, float(np.mean(np.abs(d).astype(np.float64)))


def rgb8(image, sky=None, flip_rows=False):
    """(H, W, 3) uint8: the level of every scored colour; flip_rows reverses the rows (`gl_texture`, rasterizer.jl:155-182)."""
    pic = np.ascontiguousarray(np.transpose(levels(scored(image, sky, False)), (1, 2, 0))).astype(np.uint8)
    return np.ascontiguousarray(pic[::-1]) if flip_rows else pic


def tie_set():
    """For k = 0..254 the fp32 nearest to (k + 0.5) / 255 and its 16 fp32 neighbours on each side: 255 · 33 = 8 415 inputs."""
    out = []
    for k in range(255):
        c = f32((k + 0.5) / 255.0)
        lo = c
        for _ in range(16):
            lo = np.nextafter(lo, f32(-1))
        v = [lo]
        for _ in range(32):
            v.append(np.nextafter(v[-1], f32(2)))
        out.extend(v)
    return np.asarray(out, f32)


def tie_frame():
    """The tie set as a (51, 55, 3) frame (8 415 = 3 · 55 · 51)."""
    return tie_set().reshape(51, 55, 3)


def make_case(W, H, C, seed=0):
    """(frame (H, W, C), sky (H, W, 3), target_u8 (H, W, 3)).  A quarter of the colours lie below 0, a quarter above 1, and
    the first flat positions of the colour block are -0.25, 1.5, exact 0, exact 1 (a 1 x 1 frame has room for three of
    them); alpha (C >= 5) is drawn from {inside (0, 1), exact 0, exact 1, below 0, above 1} with the first pixels forced to
    0.5, 1.25 and -0.125.  The target has exact 0 and 255."""
    r = np.random.default_rng(seed)
    frame = r.uniform(0.0, 1.0, (H, W, C)).astype(f32)
    rgb = r.uniform(-0.5, 1.5, (H, W, 3)).astype(f32)
    pick = r.integers(0, 8, (H, W, 3))
    rgb[pick == 0] = 0.0
    rgb[pick == 1] = 1.0
    flat = rgb.reshape(-1)
    forced = np.array([-0.25, 1.5, 0.0, 1.0], f32)[:flat.size]
    flat[:forced.size] = forced
    frame[..., :3] = rgb
    if C > 3:
        frame[..., 3] = r.uniform(0.5, 6.0, (H, W))
    if C >= 5:
        alpha = r.uniform(0.0, 1.0, (H, W)).astype(f32)
        pa = r.integers(0, 8, (H, W))
        alpha[pa == 0] = 0.0
        alpha[pa == 1] = 1.0
        alpha[pa == 2] = -0.0625
        alpha[pa == 3] = 1.125
        fa = alpha.reshape(-1)
        forced = np.array([0.5, 1.25, -0.125], f32)[:fa.size]
        fa[:forced.size] = forced
        frame[..., 4] = alpha
    sky = r.uniform(-0.1, 1.1, (H, W, 3)).astype(f32)
    target = r.integers(0, 256, (H, W, 3)).astype(np.uint8)
    tf = target.reshape(-1)
    tf[0] = 255
    if tf.size > 1:
        tf[-1] = 0
    for a in (frame, sky, target):
        a.setflags(write=False)
    return frame, sky, target


def rejected_calls(lib):
    """Every call gsr_eval_metrics / gsr_frame_rgb8 must refuse on its arguments alone (the pointers are never
    dereferenced) -> [(what, return code, message)]."""
    import ctypes as C
    one, two = C.c_void_p(64), C.c_void_p(4096)
    out = []

    def metrics(what, W=8, H=8, Cn=5, image=one, sky=None, t32=one, t8=None, smap=None, res=one, scratch=one):
        rc = lib.gsr_eval_metrics(W, H, Cn, image, sky, t32, t8, 0, smap, res, scratch, None)
        out.append(("metrics: " + what, rc, lib.gsr_last_error_string().decode()))

    def rgb8_(what, W=8, H=8, Cn=5, image=one, sky=None, dst=one):
        rc = lib.gsr_frame_rgb8(W, H, Cn, image, sky, 0, dst, None)
        out.append(("rgb8: " + what, rc, lib.gsr_last_error_string().decode()))

    for call in (metrics, rgb8_):
        call("W = 0", W=0)
        call("H < 0", H=-3)
        call("C < 3", Cn=2)
        call("sky with C = 3", Cn=3, sky=two)
        call("sky with C = 4", Cn=4, sky=two)
        call("null image", image=None)
        call("2^32 elements", W=65536, H=16384, Cn=4)
        call("2^32 elements and more", W=1 << 20, H=1 << 20, Cn=8)
    metrics("null out", res=None)
    metrics("null scratch", scratch=None)
    metrics("both targets", t32=one, t8=two)
    metrics("neither target", t32=None, t8=None)
    metrics("map aliases the image", smap=one)
    metrics("scratch not 8-byte aligned", scratch=C.c_void_p(68))
    rgb8_("null output", dst=None)
    return out
