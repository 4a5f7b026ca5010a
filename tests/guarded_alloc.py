"""Guard-band, poisoned allocations for the buffers an op makes with torch.empty / torch.empty_like.

``GuardedAlloc(poison, device)`` is a context manager.  While it is active ``torch.empty`` and
``torch.empty_like`` are wrappers: a contiguous, non-empty tensor on ``device`` is carved out of the
middle of one uint8 buffer of ``guard + nbytes + guard`` bytes that is filled, payload included, with
the poison byte; anything else (another device, no elements, non-contiguous, ``out=``, pinned or
gradient-requiring) is handed through unchanged and counted.  After the op, ``violations()`` reports
every buffer whose front or back guard no longer holds the poison: a store before the start or past
the end of an output or workspace.  A value read before it is written shows as a result that differs
between the two poisons (``POISONS``): 0xFF is NaN as fp32 / fp64 and −1 as an integer, 0x7F is
≈3.4e38 / ≈1.4e306 and a huge positive integer — a NaN is swallowed by ``>`` comparisons, a huge
finite value is not.

Guards are ordinary allocated bytes: nothing here reads or writes outside an allocation.
"""
import os
import sys
from unittest import mock

import torch

_REAL_EMPTY = torch.empty            # saved at import: the wrappers' own allocations do not recurse
_REAL_EMPTY_LIKE = torch.empty_like

POISONS = (0xFF, 0x7F)
GUARD = 1024                         # bytes on each side; a multiple of 256 keeps the payload's alignment

_SKIP_FILES = (os.path.abspath(__file__).rstrip("c"), os.path.abspath(mock.__file__).rstrip("c"))


def _call_site():
    """file:line (function) of the first frame outside this module and unittest.mock."""
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename).rstrip("c") in _SKIP_FILES:
        f = f.f_back
    if f is None:
        return "?"
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} ({f.f_code.co_name})"


class Record:
    """One guarded allocation: the backing buffer (kept alive), its payload's bytes, shape, dtype and
    the line that asked for it."""

    def __init__(self, index, buf, nbytes, shape, dtype, site):
        self.index, self.buf, self.nbytes, self.shape, self.dtype, self.site = index, buf, nbytes, shape, dtype, site


class GuardedAlloc:
    def __init__(self, poison, device, op="", guard=GUARD, caches=()):
        """``caches``: (module, attribute) pairs of dict caches that hold device workspaces or kernel
        outputs; each is an empty dict while the context is active, so their contents are allocated
        (guarded) inside it."""
        if guard <= 0 or guard % 256:
            raise ValueError("guard must be a positive multiple of 256 bytes")
        if not 0 <= poison <= 255:
            raise ValueError("poison is one byte")
        self.poison, self.guard, self.op = int(poison), int(guard), op
        self.device = torch.device(device)
        self.caches = tuple(caches)
        self.records = []
        self.passed = []        # (reason, shape, dtype, device, call site) of every pass-through
        self._stack = None

    # ------------------------------------------------------------------ the context
    def __enter__(self):
        self._stack = []
        try:
            for obj, name, new in ([(torch, "empty", self._empty), (torch, "empty_like", self._empty_like)]
                                   + [(m, a, {}) for m, a in self.caches]):
                p = mock.patch.object(obj, name, new)
                p.start()
                self._stack.append(p)
        except BaseException:
            self._restore()
            raise
        return self

    def __exit__(self, *exc):
        self._restore()
        return False

    def _restore(self):
        while self._stack:
            self._stack.pop().stop()

    # ------------------------------------------------------------------ the wrappers
    def _same_device(self, dev):
        if dev.type != self.device.type:
            return False
        return self.device.index is None or dev.index is None or dev.index == self.device.index

    def _wrap(self, t, kwargs, site):
        reason = None
        if kwargs.get("out") is not None:
            reason = "out="
        elif not self._same_device(t.device):
            reason = "other device"
        elif t.numel() == 0:
            reason = "empty"
        elif not t.is_contiguous():
            reason = "non-contiguous"
        elif t.layout != torch.strided or t.requires_grad or kwargs.get("pin_memory"):
            reason = "layout / requires_grad / pinned"
        if reason is not None:
            self.passed.append((reason, tuple(t.shape), t.dtype, str(t.device), site))
            return t
        return self._carve(tuple(t.shape), t.dtype, t.device, site)

    def _carve(self, shape, dtype, device, site):
        n = 1
        for s in shape:
            n *= int(s)
        nbytes = n * _REAL_EMPTY((), dtype=dtype).element_size()
        buf = _REAL_EMPTY(self.guard + nbytes + self.guard, dtype=torch.uint8, device=device)
        buf.fill_(self.poison)
        self.records.append(Record(len(self.records), buf, nbytes, shape, dtype, site))
        return buf[self.guard:self.guard + nbytes].view(dtype).view(shape)

    def _empty(self, *args, **kwargs):
        return self._wrap(_REAL_EMPTY(*args, **kwargs), kwargs, _call_site())

    def _empty_like(self, *args, **kwargs):
        return self._wrap(_REAL_EMPTY_LIKE(*args, **kwargs), kwargs, _call_site())

    def guarded(self, shape, dtype, device=None):
        """A guarded, poisoned buffer for a tensor the CALLER hands to an op (``bgemm(out=...)``)."""
        if isinstance(shape, int):
            shape = (shape,)
        return self._carve(tuple(int(s) for s in shape), dtype, torch.device(device or self.device), _call_site())

    # ------------------------------------------------------------------ the check
    def violations(self):
        """One line per guard that no longer holds the poison (after a device synchronize): op,
        allocation index, shape, dtype, call site, side and the first offending byte's offset — from
        the payload's end for the back guard, (negative) from its start for the front guard."""
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        out = []
        for r in self.records:
            g = self.guard
            for side, region in (("front", r.buf[:g]), ("back", r.buf[g + r.nbytes:])):
                bad = (region != self.poison).nonzero()
                if bad.numel():
                    first = int(bad[0, 0])
                    off = first - g if side == "front" else first
                    out.append(f"{self.op or 'op'}: allocation {r.index} shape={r.shape} dtype={r.dtype} at {r.site}: "
                               f"{side} guard, first bad byte at offset {off:+d} from the payload's "
                               f"{'start' if side == 'front' else 'end'} ({int(bad.shape[0])} bytes changed)")
        return out

    def report(self):
        """Counts and the pass-throughs, for a failure message."""
        lines = [f"{self.op or 'op'} under poison 0x{self.poison:02X}: {len(self.records)} guarded, "
                 f"{len(self.passed)} passed through"]
        lines += [f"  passed ({why}): shape={shape} dtype={dtype} device={dev} at {site}"
                  for why, shape, dtype, dev, site in self.passed]
        return "\n".join(lines)

    def passed_on(self, device_type):
        """The pass-throughs that live on ``device_type`` and are not empty tensors."""
        return [p for p in self.passed if p[3].startswith(device_type) and p[0] != "empty"]


def bits(t):
    """An integer view of ``t``'s bytes (a NaN compares equal to the same NaN), on the CPU."""
    return t.detach().contiguous().cpu().reshape(-1).view(torch.uint8)


def bit_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))
