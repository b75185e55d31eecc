"""Guard-banded buffers for testing what an entry point does to the memory it is handed.

`guarded(shape, dtype, offset_elems)` lays one flat buffer out as [guard | pad | payload | guard], fills all of it with
a sentinel and returns a `Guarded` whose `.payload` is the view a kernel gets.  With `offset_elems = 1` the payload
starts one element past a 16-byte boundary: the smallest alignment a contiguous slice of a tensor can have.

Everything is compared as integers (NaN != NaN): an output checker demands untouched guards, a documented written
region in which no element still holds the sentinel and a documented untouched region in which every element does; an
input checker demands that the whole buffer is bit-identical to what was uploaded.  tests/test_buffer_contract_host.py
keeps the checkers honest with torch CPU "kernels" that commit each fault."""

import numpy as np
import torch

GUARD_BYTES = 64 * 1024
# quiet NaNs with a fixed payload (a kernel that produces NaN by arithmetic gives the canonical 0x7ff8000000000000 /
# 0x7fc00000, never these), and a negative int64 no index or count can be
SENTINEL_BITS = {torch.float64: 0x7FF8_0000_DEAD_BEEF, torch.float32: 0x7FC0_BEEF, torch.int64: -0x5A5A_5A5A_5A5A_5A5B}
_INT_VIEW = {torch.float64: torch.int64, torch.float32: torch.int32, torch.int64: torch.int64}


class ContractViolation(AssertionError):
    pass


def _bits(t):
    """integer view of a contiguous tensor (same shape)"""
    return t.view(_INT_VIEW[t.dtype])


class Guarded:
    def __init__(self, shape, dtype, offset_elems, device):
        if offset_elems not in (0, 1):
            raise ValueError("offset_elems is 0 or 1")
        self.shape = tuple(int(s) for s in shape)
        self.dtype = dtype
        esize = torch.empty((), dtype=dtype).element_size()
        self.guard = GUARD_BYTES // esize
        self.numel = int(np.prod(self.shape)) if len(self.shape) else 1
        self.start = self.guard + offset_elems
        self.flat = torch.empty((self.start + self.numel + self.guard,), dtype=dtype, device=device)
        if self.flat.data_ptr() % 16 != 0:
            raise RuntimeError("allocator returned a base that is not 16-byte aligned")
        _bits(self.flat).fill_(SENTINEL_BITS[dtype])
        self.payload = self.flat[self.start:self.start + self.numel].view(self.shape)
        # the address a kernel gets (data_ptr() of an empty view is not defined to be this)
        self.ptr = self.flat.data_ptr() + self.start * esize
        assert self.ptr % 16 == offset_elems * esize % 16 and (self.numel == 0 or self.payload.data_ptr() == self.ptr)
        self.uploaded = None

    # ---- inputs
    def upload(self, values):
        """copy `values` (same shape and dtype) into the payload and remember the whole buffer, guards included"""
        values = torch.as_tensor(values)
        if tuple(values.shape) != self.shape or values.dtype != self.dtype:
            raise ValueError(f"upload of {tuple(values.shape)} {values.dtype} into {self.shape} {self.dtype}")
        self.payload.copy_(values.to(self.flat.device))
        self.uploaded = _bits(self.flat).clone()
        return self

    def expect(self, values):
        """as `upload` for a buffer that is filled later (by a copy enqueued on a stream): what it must hold at the end"""
        snap = _bits(self.flat).clone()
        snap[self.start:self.start + self.numel] = _bits(torch.as_tensor(values).to(self.flat.device).contiguous()
                                                         ).reshape(-1)
        self.uploaded = snap
        return self

    def check_input(self, name="input"):
        if self.uploaded is None:
            raise RuntimeError("check_input without upload")
        now = _bits(self.flat)
        if not torch.equal(now, self.uploaded):
            bad = int((now != self.uploaded).nonzero()[0]) - self.start
            raise ContractViolation(f"{name}: the call changed its input (first difference at payload element {bad}; "
                                    f"negative or >= {self.numel} is a guard band)")

    # ---- outputs
    def check_output(self, written=None, name="output"):
        """`written`: boolean mask of the payload's shape (numpy or torch), True where the call must have written and
        False where it must not have; None = everything written.  Guards must hold the sentinel."""
        s = SENTINEL_BITS[self.dtype]
        b = _bits(self.flat)
        lo, hi = b[:self.start], b[self.start + self.numel:]
        if not bool((lo == s).all()):
            at = int((lo != s).nonzero()[-1]) - self.start
            raise ContractViolation(f"{name}: write before the start (payload element {at})")
        if not bool((hi == s).all()):
            at = int((hi != s).nonzero()[0]) + self.numel
            raise ContractViolation(f"{name}: write past the end (payload element {at} of {self.numel})")
        still = (b[self.start:self.start + self.numel] == s).view(self.shape)
        if written is None:
            mask = torch.ones(self.shape, dtype=torch.bool, device=still.device)
        else:
            mask = torch.as_tensor(np.asarray(written) if not isinstance(written, torch.Tensor) else written,
                                   dtype=torch.bool).to(still.device)
            mask = mask.expand(self.shape) if mask.dim() == len(self.shape) else mask.reshape(self.shape)
        unwritten = still & mask
        if bool(unwritten.any()):
            raise ContractViolation(f"{name}: element {tuple(int(i) for i in unwritten.nonzero()[0])} of the documented "
                                    "written region was left unwritten")
        touched = ~still & ~mask
        if bool(touched.any()):
            raise ContractViolation(f"{name}: element {tuple(int(i) for i in touched.nonzero()[0])} lies in a region "
                                    "documented as untouched and was written")


def guarded(shape, dtype, offset_elems=0, device="cpu"):
    """(payload view, the Guarded that checks it)"""
    g = Guarded(shape, dtype, offset_elems, device)
    return g.payload, g
