"""Guarded, poisoned buffers for the output-contract tests (tests/test_gpu_contracts.py).

An :class:`Arena` is one ``torch.uint8`` allocation laid out as ``[guard | payload | guard]``
and filled with a poison byte. The payload is what a kernel is handed as an output or as
scratch of exactly the documented size; anything the kernel writes before it, after it, or
into the gaps between the rows of a row-strided payload lands inside the same allocation and
:meth:`Arena.check` finds it. Plain Python on plain tensors: it works on CPU tensors too
(tests/test_arena.py plants each kind of defect there).

Each guard is 4096 B: more than any vector store (16 B) and more than any output row
(256 x 4 B), so an overrun of one row still lands in a guard. The payload starts 4096 B into
the allocation, so it keeps the allocation's alignment; the trailing guard starts at the
payload's last byte + 1, with no rounding.

Poison patterns: 0xFF reads as f32 NaN, u8 255, i32 -1 and the largest u32 (which wins a
max-reduction over bit patterns); 0x5A reads as f32 ~ 1.5e16, finite, so a NaN-ignoring min/max
or a "+= dirty" that cancels cannot hide behind NaN propagation.
"""
import torch

GUARD = 4096
POISONS = (0xFF, 0x5A)


class Arena:
    """``Arena(spec, device, poison)``; ``spec`` is a byte count (payload: u8 ``[nbytes]``) or
    ``(rows, cols, dtype)`` / ``(rows, cols, dtype, row_stride)`` with the stride in elements
    (payload: ``[rows, cols]`` of ``dtype``, unit column stride; the last row has no gap behind
    it). ``payload`` is the typed view, ``ptr`` its address (valid also when it is empty)."""

    def __init__(self, spec, device, poison):
        assert 0 <= poison <= 0xFF
        self.poison = poison
        if isinstance(spec, int):
            rows, cols, dtype, stride = 1, spec, torch.uint8, spec
        else:
            rows, cols, dtype = spec[:3]
            stride = spec[3] if len(spec) > 3 and spec[3] else cols
        assert rows >= 0 and cols >= 0 and stride >= cols
        self.rows, self.cols, self.dtype, self.stride = rows, cols, dtype, stride
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        elems = (rows - 1) * stride + cols if rows > 0 and cols > 0 else 0
        self.nbytes = elems * self.itemsize
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), poison, dtype=torch.uint8,
                              device=device)
        self.ptr = self.buf.data_ptr() + GUARD
        flat = self.buf[GUARD:GUARD + self.nbytes].view(dtype)
        if isinstance(spec, int):
            self.payload = flat
        else:
            self.payload = torch.as_strided(flat, (rows, cols), (stride, 1)) if elems else \
                flat.new_empty((rows, cols))

    # ------------------------------------------------------------------ layout
    def _payload_mask(self):
        """bool [total bytes]: True where the byte belongs to a payload element."""
        m = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        if self.nbytes:
            body = m[GUARD:GUARD + self.nbytes]
            if self.stride == self.cols:
                body.fill_(True)
            else:
                rb, cb = self.stride * self.itemsize, self.cols * self.itemsize
                torch.as_strided(body, (self.rows, cb), (rb, 1)).fill_(True)
        return m

    def _where(self, pos):
        """Names a byte of the allocation: (region, byte offset from the payload's start)."""
        off = pos - GUARD
        if off < 0:
            return ("leading guard", off)
        if off >= self.nbytes:
            return ("trailing guard", off)
        rb = self.stride * self.itemsize
        return (f"gap after row {off // rb}", off)

    # ------------------------------------------------------------------ checks
    def check(self):
        """``None`` when both guards and every stride gap still hold the poison, else
        ``(region, byte offset from the payload's start, value found)`` of the first changed
        byte (the byte one before the payload is offset -1, the one after it offset nbytes)."""
        changed = (self.buf != self.poison) & ~self._payload_mask()
        hit = changed.nonzero()
        if hit.numel() == 0:
            return None
        pos = int(hit[0, 0])
        return self._where(pos) + (int(self.buf[pos]),)

    def first_poisoned(self):
        """Index (a tuple; ``None`` if there is none) of the first payload element whose every
        byte still holds the poison: an element the kernel never wrote. Only meaningful where
        the poison is no legal value (not for u8 selectors: 255 and 0x5A are features)."""
        if self.nbytes == 0:
            return None
        by = self.payload.contiguous().view(torch.uint8).reshape(-1, self.itemsize)
        hit = (by == self.poison).all(dim=1).nonzero()
        if hit.numel() == 0:
            return None
        flat = int(hit[0, 0])
        return (flat,) if self.payload.dim() == 1 else (flat // self.cols, flat % self.cols)

    def fill(self, value):
        """Overwrites the payload (a prior for accumulating kernels): ``value`` broadcasts."""
        self.payload.copy_(torch.as_tensor(value, dtype=self.dtype))
        return self


def arena(spec, device, poison):
    """The :class:`Arena` for ``spec``; ``arena(...).payload`` is the typed payload view."""
    return Arena(spec, device, poison)
