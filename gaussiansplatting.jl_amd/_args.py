"""Argument plumbing shared by the host mirrors of the device entry points: ONE tensor check, ONE scratch policy and ONE
autograd form of a "term whose pullback ADDS onto a cotangent".  torch is imported on first use: the modules whose host
side is numpy stay importable without it."""
from __future__ import annotations


def _torch():
    import torch
    return torch


def check(t, message: str, *, dtype=None, shape=None, last=None, device=None):
    """`t` is a contiguous `dtype` (default float32) HIP tensor — and, where given, of `shape` (None: any extent), with its
    last dimension in `last`, on `device` — or ValueError(message): the wording is the caller's.  Returns `t`."""
    torch = _torch()
    if (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == (torch.float32 if dtype is None else dtype) and t.is_contiguous()
            and (device is None or t.device == device) and (shape is None or _fits(t.shape, shape))
            and (last is None or (t.dim() and t.shape[-1] in last))):
        return t
    raise ValueError(message)


def _fits(have, want) -> bool:
    """(a plain loop: this runs on every call of every entry point, in front of launches of a few microseconds)"""
    if len(have) != len(want):
        return False
    for n, w in zip(have, want):
        if w is not None and n != w:
            return False
    return True


def frame_check(channels, wording: str):
    """-> check_frame(image, name="image"): a contiguous float32 (H, W, C) HIP tensor with C in `channels`, or
    ValueError(wording.format(name))."""
    def check_frame(image, name="image"):
        return check(image, wording.format(name), shape=(None, None, None), last=channels)
    return check_frame


def check_like(t, name, shape, device, dtype=None):
    """`t` is a contiguous `dtype` tensor of exactly `shape` on the image's device."""
    kind = "float32" if dtype is None else str(dtype).split(".")[-1]
    return check(t, f"{name} must be a contiguous {kind} HIP tensor of shape {tuple(shape)} on the image's device",
                 dtype=dtype, shape=shape, device=device)


def check_same(t, name, image, what="image"):
    """`t` (already known to be a HIP tensor of the right kind) has the shape and the device of `image`."""
    if t.shape != image.shape or t.device != image.device:
        raise ValueError(f"{name} must have the {what}'s shape and device")
    return t


def check_vpixels(check_frame, vpixels, image):
    """The cotangent a pullback adds onto: a frame like `image` (already checked by `check_frame`), and another buffer."""
    check_same(check_frame(vpixels, "vpixels"), "vpixels", image)
    if vpixels.data_ptr() == image.data_ptr():
        raise ValueError("vpixels must not be the image")
    return vpixels


def check_scratch(scratch, nbytes: int, device, align: int = 1):
    """A caller-owned scratch buffer: >= nbytes, contiguous, on `device`, at the alignment the C entry point demands."""
    torch = _torch()
    if not (isinstance(scratch, torch.Tensor) and scratch.is_cuda and scratch.is_contiguous() and scratch.device == device
            and scratch.numel() * scratch.element_size() >= nbytes and scratch.data_ptr() % align == 0):
        aligned = f", {align}-byte aligned" if align > 1 else ""
        raise ValueError(f"scratch must be a contiguous{aligned} HIP tensor of at least {nbytes} bytes on the image's device")
    return scratch


def grow_scratch(cache: dict, key, nbytes: int, device, min_bytes: int = 1):
    """The dict-keyed form: cache[key], reallocated when it is missing, too small or on another device (grow-only)."""
    buf = cache.get(key)
    if buf is None or buf.numel() < nbytes or buf.device != device:
        buf = cache[key] = _torch().empty(max(nbytes, min_bytes), dtype=_torch().uint8, device=device)
    return buf


class FrameScratch:
    """The scratch of a forward / backward pair over one frame: what the forward leaves on the device for the backward of
    the same image.  `scratch_bytes(W, H)` is the library's gsr_*_scratch_bytes query, `align` what the C entry point
    demands of the pointer, `min_bytes` the smallest allocation.  Each module keeps one."""

    def __init__(self, scratch_bytes, align: int = 1, min_bytes: int = 0):
        self.scratch_bytes, self.align, self.min_bytes = scratch_bytes, align, min_bytes
        self.cache: dict = {}   # grow-only, per (W, H, device)

    def get(self, scratch, W: int, H: int, device, create: bool = True):
        """scratch=None: the module's own buffer for (W, H, device) — None with create=False when no forward made one;
        otherwise the caller's buffer, validated and returned as it is."""
        nb = int(self.scratch_bytes(W, H))
        if scratch is not None:
            return check_scratch(scratch, nb, device, self.align)
        if not create:
            return self.cache.get((W, H, device))
        return grow_scratch(self.cache, (W, H, device), nb, device, self.min_bytes)


def cotangent_term(image, forward_fn, backward_fn, scratch_bytes):
    """A loss term under autograd whose device pullback ADDS onto a cotangent: `forward_fn(image, scratch)` -> the 0-d
    value, `backward_fn(image, v, scratch)` adds ∂term/∂image onto the zeroed `v`, `scratch_bytes(W, H)` sizes the buffer
    the pair shares (owned by the graph node, so that two terms in flight never meet).  Differentiable w.r.t. `image`."""
    torch = _torch()

    class _Term(torch.autograd.Function):
        @staticmethod
        def forward(ctx, image):
            image = image.detach().contiguous()
            ctx.scratch = torch.empty(scratch_bytes(image.shape[1], image.shape[0]), dtype=torch.uint8, device=image.device)
            ctx.save_for_backward(image)
            return forward_fn(image, ctx.scratch)

        @staticmethod
        def backward(ctx, delta):
            (image,) = ctx.saved_tensors
            v = torch.zeros_like(image)
            backward_fn(image, v, ctx.scratch)
            return v * delta

    return _Term.apply(image)
