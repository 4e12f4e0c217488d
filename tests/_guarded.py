"""Guarded argument buffers for memory-contract tests of the C ABI (include/fpsg_hip.h).

An Arena is ONE uint8 allocation from which every argument buffer of one call is carved:
  - every region starts at exactly the alignment the header documents for it and at no stricter one: a region of
    alignment a starts at an address that is a mod 2a (4 mod 8, 8 mod 16, 16 mod 32);
  - every region has exactly its documented size, a workspace what its size function returned and not a byte more;
  - at least GUARD bytes of guard zone lie in front of and behind every region;
  - the whole allocation, payload included, is filled with a pattern (0xFF bytes, zeros, seeded random bytes) before
    the inputs are copied in.
After the call, check() compares the allocation with its saved image in one masked comparison on the arena's device:
every guard byte and every byte of a pure input must be unchanged; a failure names the region and the byte offset.

Roomy is the forgiving counterpart: one torch.zeros allocation per buffer (256-byte aligned by the allocator, sizes
rounded up to 256 bytes), workspaces twice the required size.

Both work on CPU tensors, so the helper itself is tested without a GPU (tests/test_memory_contract_cpu.py).
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import torch

GUARD = 64 * 1024
PATTERNS = ("ff", "zero", "random")

IN, OUT, INOUT, WS = "in", "out", "inout", "ws"


@dataclasses.dataclass
class Buf:
    """One argument buffer of a call.  role: IN (never written), OUT (fully written unless `unspecified` masks a
    part), INOUT (initialised from `data`, compared like an output), WS (caller scratch, contents unspecified)."""
    name: str
    role: str
    dtype: torch.dtype
    shape: tuple
    align: int = 4                                  # bytes, as include/fpsg_hip.h documents it for this argument
    data: Optional[torch.Tensor] = None             # CPU tensor of dtype / shape for IN and INOUT
    unspecified: Optional[torch.Tensor] = None      # CPU bool tensor of `shape`: elements the header leaves open
    why: str = ""                                   # the header line behind `unspecified` or INOUT

    @property
    def nbytes(self) -> int:
        n = 1
        for s in self.shape:
            n *= int(s)
        return n * torch.empty((), dtype=self.dtype).element_size()


def inp(name, data, align=4):
    data = data.contiguous()
    return Buf(name, IN, data.dtype, tuple(data.shape), align, data)


def out(name, dtype, shape, align=4, unspecified=None, why=""):
    return Buf(name, OUT, dtype, tuple(shape), align, None, unspecified, why)


def inout(name, data, align=4, why=""):
    data = data.contiguous()
    return Buf(name, INOUT, data.dtype, tuple(data.shape), align, data, None, why)


def ws(name, nbytes, align=4):
    return Buf(name, WS, torch.uint8, (int(nbytes),), align)


def _fill(t: torch.Tensor, pattern: str, seed: int) -> None:
    if pattern == "ff":
        t.fill_(0xFF)
    elif pattern == "zero":
        t.zero_()
    elif pattern == "random":
        g = torch.Generator().manual_seed(seed)
        t.copy_(torch.randint(0, 256, (t.numel(),), dtype=torch.uint8, generator=g))
    else:
        raise ValueError(f"unknown fill pattern {pattern!r}")


class Arena:
    def __init__(self, bufs: Sequence[Buf], pattern: str, device="cpu", seed: int = 0, guard: int = GUARD):
        assert guard >= GUARD
        self.bufs = list(bufs)
        self.pattern = pattern
        # relative offsets first (against a base that is a multiple of 256), then shifted by the real base's residue
        slack = 256
        off, rel = 0, {}
        for b in self.bufs:
            assert b.align in (1, 2, 4, 8, 16, 32, 64, 128) and b.align * 2 <= slack, b
            off += guard
            two = 2 * b.align
            off += (b.align - off) % two                      # off = align (mod 2 align): that alignment, no stricter one
            rel[b.name] = off
            off += b.nbytes
        total = off + guard + slack
        self.mem = torch.empty(total, dtype=torch.uint8, device=device)
        shift = (-self.mem.data_ptr()) % slack                # first byte at a multiple of 256
        self.off = {k: v + shift for k, v in rel.items()}
        _fill(self.mem, pattern, seed)
        for b in self.bufs:
            if b.role in (IN, INOUT):
                assert b.data is not None and tuple(b.data.shape) == b.shape and b.data.dtype == b.dtype, b.name
                self.region(b).copy_(b.data.to(device))
        # what every byte outside an output, in/out buffer or workspace must still hold after the call
        self.expected = self.mem.clone()
        self.watch = torch.ones(total, dtype=torch.bool, device=device)
        for b in self.bufs:
            if b.role != IN and b.nbytes:
                self.watch[self.off[b.name]: self.off[b.name] + b.nbytes] = False
        for b in self.bufs:
            assert self.ptr(b) is None or (self.ptr(b) % (2 * b.align) == b.align % (2 * b.align)), b.name

    def raw(self, b: Buf) -> torch.Tensor:
        o = self.off[b.name]
        return self.mem[o: o + b.nbytes]

    def region(self, b: Buf) -> torch.Tensor:
        return self.raw(b).view(b.dtype).view(b.shape)

    def ptr(self, b: Buf) -> Optional[int]:
        """The address to pass, or None (a NULL pointer) for a buffer of no bytes."""
        return self.mem.data_ptr() + self.off[b.name] if b.nbytes else None

    def ptrs(self) -> dict:
        return {b.name: self.ptr(b) for b in self.bufs}

    def poke(self, name: str, data: torch.Tensor) -> None:
        """Late input bytes (a table of addresses of other regions): written into the region and into its image."""
        b = next(x for x in self.bufs if x.name == name)
        assert b.role == IN and data.dtype == b.dtype and tuple(data.shape) == b.shape
        self.region(b).copy_(data.to(self.mem.device))
        o = self.off[name]
        self.expected[o: o + b.nbytes] = self.mem[o: o + b.nbytes]

    def violation(self) -> Optional[str]:
        """None when every guard byte and every pure-input byte still holds its image, else a message that names
        the region and the byte offset of the first change.  One masked comparison, on the arena's device."""
        bad = (self.mem != self.expected) & self.watch
        if not bool(bad.any()):
            return None
        at = int(torch.nonzero(bad)[0])
        n = int(bad.sum())
        best = None
        for b in self.bufs:
            o, e = self.off[b.name], self.off[b.name] + b.nbytes
            if o <= at < e:
                return f"input '{b.name}' was written at byte {at - o} of {b.nbytes} ({n} bytes changed in all)"
            d, where = (o - at, f"{o - at} bytes in front of") if at < o else (at - e + 1, f"{at - e} bytes behind")
            if best is None or d < best[0]:
                best = (d, f"guard zone written {where} '{b.name}' ({b.role}, {b.nbytes} bytes; {n} bytes changed in all)")
        return best[1]

    def check(self) -> None:
        msg = self.violation()
        assert msg is None, f"[{self.pattern}] {msg}"

    def outputs(self) -> dict:
        """CPU copies of the bytes of every OUT / INOUT buffer, the unspecified parts zeroed."""
        return {b.name: _masked_bytes(b, self.region(b)) for b in self.bufs if b.role in (OUT, INOUT)}


class Roomy:
    """The same call with one zeroed, 256-byte aligned allocation per buffer and twice the workspace."""

    def __init__(self, bufs: Sequence[Buf], device="cpu"):
        self.bufs = list(bufs)
        self.pattern = "roomy"
        self.t = {}
        for b in self.bufs:
            n = b.nbytes * (2 if b.role == WS else 1)
            padded = (n + 255) // 256 * 256 + 256
            mem = torch.zeros(padded, dtype=torch.uint8, device=device)
            shift = (-mem.data_ptr()) % 256
            self.t[b.name] = (mem, shift)
            if b.role in (IN, INOUT):
                self.region(b).copy_(b.data.to(device))

    def region(self, b: Buf) -> torch.Tensor:
        mem, shift = self.t[b.name]
        return mem[shift: shift + b.nbytes].view(b.dtype).view(b.shape)

    def ptr(self, b: Buf) -> Optional[int]:
        mem, shift = self.t[b.name]
        return mem.data_ptr() + shift if b.nbytes else None

    def ptrs(self) -> dict:
        return {b.name: self.ptr(b) for b in self.bufs}

    def poke(self, name: str, data: torch.Tensor) -> None:
        b = next(x for x in self.bufs if x.name == name)
        self.region(b).copy_(data.to(self.t[name][0].device))

    def check(self) -> None:
        pass

    def outputs(self) -> dict:
        return {b.name: _masked_bytes(b, self.region(b)) for b in self.bufs if b.role in (OUT, INOUT)}


def _masked_bytes(b: Buf, region: torch.Tensor) -> torch.Tensor:
    t = region.detach().cpu().clone()
    if b.unspecified is not None:
        assert b.why, f"{b.name}: a masked part needs the header line that leaves it open"
        assert tuple(b.unspecified.shape) == b.shape and b.unspecified.dtype == torch.bool
        t[b.unspecified] = 0
    return t.contiguous().view(-1).view(torch.uint8)


def first_difference(a: torch.Tensor, b: torch.Tensor, elem: int) -> Optional[int]:
    """Index of the first element (of `elem` bytes) at which two byte images differ, or None."""
    d = torch.nonzero(a != b)
    return None if d.numel() == 0 else int(d[0]) // elem
