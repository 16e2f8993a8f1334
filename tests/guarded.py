"""Guarded buffers for the tests: arrays placed inside ONE allocation with known words right before their first and right
after their last byte, so that a kernel that reads or writes outside an array shows up — a write as a changed guard, a read
as a result that follows the guard's contents.  Plain torch: no product code, no oracle, runs on CPU tensors as well.

    a = Arena(nbytes, device, skew="worst", fill=0)
    x = a.place("x", host_array)                      # a const input: x is a contiguous view into the arena
    y = a.place("y", (771,), torch.float32, role="out")
    ... the library reads x.data_ptr() and writes y.data_ptr() ...
    assert a.check() == []                            # no guard word changed
    a.assert_inputs_unchanged()                       # x still holds host_array, bit for bit

Layout of one placement:  | guard, >= 1 KiB | data, numel * itemsize bytes, end NOT rounded | guard, >= 1 KiB |  and the arena
ends with 4 KiB that belong to no buffer, so an overrun of less than a guard never leaves the allocation.

Address of the first data byte:
  skew "aligned": a multiple of 16 (the library's vector paths run);
  skew "worst"  : the weakest the ABI allows.  `align` = the alignment the interface documents for the argument (16 or 8):
                  exactly that and no more (16 mod 32, 8 mod 16); no documented requirement: the element size and no more
                  (4-byte elements 4 mod 16, 8-byte elements 8 mod 16, 2-byte 2 mod 16, bytes at an odd address).

Guard contents (fill = 0 or 1; a case must give the same results under both):
  float buffers   : the words 0xFFFFFFFF (a NaN) / 0x7F7F7F7F (3.4e38; NaN hides behind comparisons);
  integer buffers : `guard=(v0, v1)`, two different values that are IN RANGE for what the kernel does with an element
                    (an index, a row number, a count, a mask byte) — a poison word there would turn an over-read into a wild
                    address instead of a changed result.  Default (0, 1).
The guard elements are laid out in phase with the data: the element "one past the end" reads exactly the guard value."""
import numpy as np
import torch

GUARD = 1024      # bytes, at least, on each side of every placement
TAIL = 4096       # bytes at the end of the arena that belong to no buffer
FLOAT_WORDS = (0xFFFFFFFF, 0x7F7F7F7F)
SKEWS = ("aligned", "worst")
FILLS = (0, 1)


def worst_residue(itemsize, align=None):
    """(modulus, residue) of the data address under skew "worst"."""
    if align is not None:
        if align not in (8, 16) or align < itemsize:
            raise ValueError(f"align = {align}")
        return 2 * align, align
    if itemsize >= 16:
        return 32, 16
    return 16, itemsize % 16 if itemsize > 1 else 1


def _pattern(dtype, value, nbytes, phase=0):
    """nbytes bytes of `value` (dtype elements) repeated, starting `phase` bytes into an element."""
    item = np.array([value]).astype(dtype).view(np.uint8)
    reps = (nbytes + phase) // len(item) + 2
    return np.tile(item, reps)[phase:phase + nbytes].copy()


class Arena:
    def __init__(self, nbytes, device="cpu", skew="aligned", fill=0):
        if skew not in SKEWS or fill not in FILLS:
            raise ValueError((skew, fill))
        self.skew, self.fill = skew, fill
        self.nbytes = int(nbytes) + TAIL
        self.mem = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)   # THE allocation
        self.base = self.mem.data_ptr()
        if self.base % 32:
            raise RuntimeError("arena base is not 32-byte aligned")
        self.host = np.zeros(self.nbytes, np.uint8)     # what every byte outside the data regions must hold
        self.is_guard = np.ones(self.nbytes, bool)
        self.cursor = 0                                 # end of the last placement's trailing guard
        self.records = []                               # dict(name, start, end, lo, hi, role, host)
        self._expected = None
        # until something is placed the whole arena is "tail": the float word of this fill
        self.host[:] = _pattern(np.uint32, FLOAT_WORDS[fill], self.nbytes)
        self.mem.copy_(torch.from_numpy(self.host))

    # ---- placement -------------------------------------------------------------------------------------------------
    def place(self, name, array_or_shape, dtype=None, align=None, skew=None, role=None, guard=None):
        """A contiguous tensor view of the arena.  An array (numpy / torch) is copied in and registered as a const input
        (role "in") unless role says "inout"; a shape + dtype is an output (role "out", zero-filled) or "scratch"."""
        skew = self.skew if skew is None else skew
        if isinstance(array_or_shape, (tuple, list, int)):
            shape = (array_or_shape,) if isinstance(array_or_shape, int) else tuple(array_or_shape)
            tdtype = dtype or torch.float32
            src = None
            role = role or "out"
        else:
            src = array_or_shape.detach().cpu() if isinstance(array_or_shape, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array_or_shape))
            if dtype is not None:
                src = src.to(dtype)
            src = src.contiguous()
            shape, tdtype = tuple(src.shape), src.dtype
            role = role or "in"
        item = torch.empty(0, dtype=tdtype).element_size()
        ndtype = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[item]
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        mod, res = (16, 0) if skew == "aligned" else worst_residue(item, align)
        start = self.cursor + GUARD
        start += (res - (self.base + start)) % mod
        end = start + nbytes
        hi = end + GUARD                                 # the next placement's own guard begins where this one ends
        if hi + TAIL > self.nbytes:
            raise RuntimeError(f"arena too small for {name}: needs {hi + TAIL} of {self.nbytes} bytes")
        if tdtype.is_floating_point:
            w = FLOAT_WORDS[self.fill]
            g = {2: w & 0xFFFF, 4: w, 8: w | (w << 32)}[item]
        else:
            g = int((guard or (0, 1))[self.fill]) % (1 << (8 * item))
        lo = self.cursor
        pre = start - lo
        self.host[lo:start] = _pattern(ndtype, g, pre, phase=(-pre) % item)
        self.host[end:hi] = _pattern(ndtype, g, hi - end)
        self.is_guard[start:end] = False
        self.mem[lo:start].copy_(torch.from_numpy(self.host[lo:start]))
        self.mem[end:hi].copy_(torch.from_numpy(self.host[end:hi]))
        view = self.mem[start:end].view(tdtype).view(shape) if nbytes else torch.empty(shape, dtype=tdtype, device=self.mem.device)
        if src is not None:
            view.copy_(src)
        else:
            view.zero_()
        self.records.append(dict(name=name, start=start, end=end, lo=lo, hi=hi, role=role,
                                 host=src.clone() if (src is not None and role == "in") else None, view=view))
        self.cursor = hi
        self._expected = None
        return view

    def address_of(self, name):
        r = next(r for r in self.records if r["name"] == name)
        return self.base + r["start"]

    # ---- checks ----------------------------------------------------------------------------------------------------
    def check(self):
        """Every guard (and the tail) against what was written, compared on the device.  Returns one dict per damaged guard:
        name, side ("before" / "after"), offset = first changed byte relative to the buffer's first byte (negative: before it;
        >= its size: after it), words = number of changed 4-byte words, counted in phase with the buffer's first byte."""
        if self._expected is None:
            self._expected = torch.from_numpy(self.host).to(self.mem.device)
            self._mask = torch.from_numpy(self.is_guard).to(self.mem.device)
        bad = (self.mem != self._expected) & self._mask
        if not bool(bad.any()):
            return []
        bad = bad.cpu().numpy()
        out = []
        for r in self.records:
            for side, a, b in (("before", r["lo"], r["start"]), ("after", r["end"], r["hi"])):
                idx = np.flatnonzero(bad[a:b]) + a
                if idx.size:
                    words = np.unique((idx - r["start"]) // 4).size
                    out.append(dict(name=r["name"], side=side, offset=int(idx[0] - r["start"]), words=int(words)))
        last = self.records[-1]["hi"] if self.records else 0
        idx = np.flatnonzero(bad[last:]) + last
        if idx.size:
            out.append(dict(name="<arena tail>", side="after", offset=int(idx[0] - last), words=int(np.unique(idx // 4).size)))
        return out

    def assert_inputs_unchanged(self):
        for r in self.records:
            if r["host"] is not None:
                now = r["view"].detach().cpu()
                a = now.contiguous().view(torch.uint8) if now.numel() else now
                b = r["host"].view(torch.uint8) if now.numel() else r["host"]
                if not torch.equal(a, b):
                    d = (a.reshape(-1) != b.reshape(-1)).nonzero()
                    raise AssertionError(f"const input {r['name']} was written: {d.numel()} bytes differ, first at byte {int(d[0])}")


class Plain:
    """The same interface with every buffer its own torch allocation (the runs the suite has always made)."""
    skew, fill = "plain", None

    def __init__(self, device="cpu"):
        self.device = device
        self.records = []

    def place(self, name, array_or_shape, dtype=None, align=None, skew=None, role=None, guard=None):
        if isinstance(array_or_shape, (tuple, list, int)):
            shape = (array_or_shape,) if isinstance(array_or_shape, int) else tuple(array_or_shape)
            t = torch.zeros(shape, dtype=dtype or torch.float32, device=self.device)
            host = None
        else:
            src = array_or_shape.detach().cpu() if isinstance(array_or_shape, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array_or_shape))
            if dtype is not None:
                src = src.to(dtype)
            t = src.contiguous().to(self.device).clone()
            host = src.contiguous().clone() if (role or "in") == "in" else None
        self.records.append(dict(name=name, view=t, host=host))
        return t

    def check(self):
        return []

    def assert_inputs_unchanged(self):
        for r in self.records:
            if r["host"] is not None and r["host"].numel():
                if not torch.equal(r["view"].detach().cpu().contiguous().view(torch.uint8), r["host"].view(torch.uint8)):
                    raise AssertionError(f"const input {r['name']} was written")


def placements(nbytes, device):
    """The five runs of a case: plain, then the two placements times the two guard fills."""
    yield Plain(device)
    for skew in SKEWS:
        for fill in FILLS:
            yield Arena(nbytes, device, skew, fill)
