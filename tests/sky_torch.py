"""The sky-dome composite and the sky-mask loss (src/sky_dome.jl:246-250, :315-320) restated for the tests: no product code.

- `evaluate`: the formulation in torch with autograd — float64 is the truth, float32 on the CPU the yardstick.
- `restate`: plain numpy fp32 in the ORDER the kernels state (csrc/sky.hip), the double sums included: what the bit tests
  compare against.
- `make_case`: frames whose alpha holds exact 0, exact 1 and the interior, and the three masks (fractional, zero, Σw < 1).

Frames are (H, W, C), C = 5 or 8, channel 4 alpha; the sky frame is (H, W, 3); a mask is (H, W)."""
import numpy as np
import torch

f32 = np.float32
MASKS = ("fractional", "zero", "small")


def make_case(W, H, C, seed=0):
    """(frame, sky, masks: dict, g) — g (H, W, C) is a cotangent whose channels >= 3 already hold other terms' values."""
    r = np.random.default_rng(seed)
    frame = r.uniform(0.0, 1.0, (H, W, C)).astype(f32)
    frame[..., 3] = r.uniform(0.5, 6.0, (H, W))
    alpha = r.uniform(0.0, 1.0, (H, W)).astype(f32)
    pick = r.integers(0, 4, (H, W))
    alpha[pick == 0] = 0.0
    alpha[pick == 1] = 1.0
    if W * H >= 2:
        alpha.reshape(-1)[0], alpha.reshape(-1)[-1] = 1.0, 0.0
    frame[..., 4] = alpha
    sky = r.uniform(0.0, 1.0, (H, W, 3)).astype(f32)
    frac = r.uniform(0.0, 1.0, (H, W)).astype(f32)
    frac[r.random((H, W)) < 0.4] = 0.0
    frac.reshape(-1)[0] = 0.75            # the saturated pixel is on the mask
    small = np.zeros((H, W), f32)
    small.reshape(-1)[0] = 0.375          # Σw < 1: the divisor is 1
    masks = dict(fractional=frac, zero=np.zeros((H, W), f32), small=small)
    g = (r.standard_normal((H, W, C)) * 1e-3).astype(f32)
    for a in (frame, sky, g, *masks.values()):
        a.setflags(write=False)
    return frame, sky, masks, g


def composite_and_loss(image, sky, mask, loss_weight):
    """The formulation on torch tensors of any dtype and device: (image[..., :3] + (1 - α) · sky, loss_weight · Σ w·α² /
    max(Σw, 1) or None, 1 / max(Σw, 1) or None); Σw is detached (sky_dome.jl:318)."""
    alpha = image[..., 4]
    comp = image[..., :3] + (1 - alpha)[..., None] * sky
    if mask is None:
        return comp, None, None
    d = torch.clamp(mask.sum(), min=1.0).detach()
    return comp, loss_weight * ((mask * alpha ** 2).sum() / d), 1.0 / d


def evaluate(frame, sky, mask, loss_weight, g, dtype=torch.float64):
    """The cotangent of Σ comp · g[..., :3] + term, by autograd -> dict(comp, loss, inv, valpha, vsky)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)  # noqa: E731
    image, s = t(frame).requires_grad_(True), t(sky).requires_grad_(True)
    comp, loss, inv = composite_and_loss(image, s, None if mask is None else t(mask), torch.tensor(loss_weight, dtype=dtype))
    total = (comp * t(g[..., :3])).sum()
    if loss is not None:
        total = total + loss
    total.backward()
    return dict(comp=comp.detach().numpy(), loss=None if loss is None else float(loss.detach()),
                inv=None if inv is None else float(inv), valpha=image.grad[..., 4].numpy(), vsky=s.grad.numpy())


def _block_sums(v):
    """The forward's partials over the double values v (zero past the end), one per workgroup of 1024 pixels: thread t adds
    its pixels t, t + 256, t + 512, t + 768 ascending; then gsr::block_sum of the 256 thread sums: per wave the xor butterfly
    v += v[lane ^ off], off = 32..1 (lane 0's value), then ((w0 + w1) + w2) + w3."""
    n = v.size
    nb = (n + 1023) // 1024
    x = np.zeros(nb * 1024, np.float64)
    x[:n] = v
    x = x.reshape(nb, 4, 256)
    x = (((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]).reshape(nb, 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ off]
    w = x[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _sum_partials(p):
    """gsr::sum_partials: thread t adds rows t, t + 256, ... ascending from 0.0; thread 0 adds the 256 thread sums ascending."""
    rounds = (p.size + 255) // 256
    x = np.zeros(rounds * 256, np.float64)
    x[:p.size] = p
    acc = np.zeros(256, np.float64)
    for row in x.reshape(rounds, 256):
        acc = acc + row
    s = 0.0
    for v in acc:
        s = s + float(v)
    return s


def restate(frame, sky, mask, loss_weight, vpixels):
    """The kernels' arithmetic in numpy fp32, in their stated order -> dict(out, loss, inv, vsky, v4): `out` the composite
    frame, `v4` what channel 4 of `vpixels` holds after the backward."""
    frame, sky, vpixels = (np.asarray(a, f32) for a in (frame, sky, vpixels))
    alpha = frame[..., 4]
    t = f32(1) - alpha
    out = frame.copy()
    for c in range(3):
        out[..., c] = frame[..., c] + t * sky[..., c]
    g = vpixels[..., :3]
    vsky = (t[..., None] * g).astype(f32)
    dot = (g[..., 0] * sky[..., 0] + g[..., 1] * sky[..., 1]) + g[..., 2] * sky[..., 2]
    add = -dot
    loss = inv = None
    if mask is not None:
        w = np.asarray(mask, f32)
        wd, ad = w.astype(np.float64).reshape(-1), alpha.astype(np.float64).reshape(-1)
        s_w, s_wa = _sum_partials(_block_sums(wd)), _sum_partials(_block_sums(wd * (ad * ad)))
        d = s_w if s_w > 1.0 else 1.0
        inv = f32(1.0 / d)
        loss = f32(loss_weight) * f32(s_wa / d)
        add = add + ((f32(2) * w) * alpha) * (f32(loss_weight) * inv)
    return dict(out=out, loss=loss, inv=inv, vsky=vsky, v4=(vpixels[..., 4] + add).astype(f32))
