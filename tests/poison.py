"""Poisoned-buffer harness for the C ABI (include/b2h.h), called through ctypes.

Every device operand of a launch gets a buffer of its own: a guard band, the operand, a second guard band.
  - input guards hold a quiet NaN (a load from outside the operand that is then multiplied by a zero mask
    still shows as NaN);
  - output guards and the output itself hold POISON, a NaN bit pattern no kernel computes (compared as raw
    int32 bits: the metric kernels legitimately write NaN for an empty sequence).
The same launch is then repeated on zero-filled buffers.  `launch` asserts that every guard is unchanged,
that inputs were not written, that no output word is left at POISON, and that the poisoned and the zeroed
launch agree bit for bit: an unwritten row, a store past the end or a read of stale memory cannot pass.
An operand starts on the 16-byte grid unless the caller shifts it (`Guarded(..., shift)`, `launch(..., shifts=)`): 4, 8
or 12 bytes past it, for the pointers include/b2h.h promises less than 16 bytes for (tests/test_alignment_gpu.py).

A helper module, not a conftest.py: the tests import it by name.
"""
import ctypes

import torch

GUARD = 64 * 1024               # bytes per guard band
QNAN = 0x7FC00000               # fp32 quiet NaN: input guards
POISON = 0x7FA5A5A5             # NaN payload no kernel writes: output guards and output regions
_vp = ctypes.c_void_p


def _i32(bits):
    return bits - (1 << 32) if bits >= 1 << 31 else bits


class Guarded:
    """One device operand of `nbytes` (a multiple of 4) between two guard bands.  The operand starts
    GUARD + `shift` bytes into a fresh 256-byte-aligned allocation: on the 16-byte grid with shift 0, `shift`
    bytes (a multiple of 4, 0..12) past it otherwise.  The lower band is everything before the operand; the
    upper band (GUARD bytes) starts right after its last word, so a store one word past the end lands in it."""

    def __init__(self, nbytes, fill, body_fill, device, shift=0):
        assert nbytes % 4 == 0
        assert shift in (0, 4, 8, 12)
        self.nbytes = nbytes
        self.shift = shift
        self.fill = _i32(fill)
        self.lo = (GUARD + shift) // 4
        self.hi = self.lo + nbytes // 4
        self.words = torch.full((self.hi + GUARD // 4,), self.fill, dtype=torch.int32, device=device)
        assert self.words.data_ptr() % 256 == 0
        if body_fill is not None:
            self.words[self.lo:self.hi] = _i32(body_fill)

    @property
    def ptr(self):
        return _vp(self.words.data_ptr() + GUARD + self.shift)

    @property
    def body(self):
        """The operand's words (int32 view)."""
        return self.words[self.lo:self.hi]

    def view(self, dtype, shape):
        return self.body.view(dtype).view(shape)

    def guards_intact(self):
        return bool((self.words[:self.lo] == self.fill).all()) and bool((self.words[self.hi:] == self.fill).all())


def guarded_input(t, poisoned, device, shift=0):
    """Device copy of tensor `t` (any dtype) between quiet-NaN guards (zero guards when not poisoned)."""
    t = t.detach().contiguous()
    nbytes = t.numel() * t.element_size()
    g = Guarded(nbytes, QNAN if poisoned else 0, None, device, shift)
    if nbytes:
        g.body.copy_(t.to(device).reshape(-1).view(torch.int32))
    return g


def guarded_output(nbytes, poisoned, device, shift=0):
    return Guarded(nbytes, POISON if poisoned else 0, POISON if poisoned else 0, device, shift)


def launch(call, inputs, outputs, device, scratch=None, check_written=True, shifts=None):
    """Run `call(ptrs) -> b2h_status` once on poisoned and once on zeroed buffers and check both (module doc).

    inputs:  name -> tensor (copied into guarded device buffers; must come back unchanged)
    outputs: name -> shape of a float32 output (every word must be written)
    scratch: name -> byte count, or a Guarded the caller keeps (e.g. a dirty workspace from an earlier call):
             guards are checked, contents are not (the zeroed run gets a fresh zero-filled buffer of the same size)
    shifts:  name -> bytes (a multiple of 4, 0..12) by which that input or output starts past the 16-byte grid;
             names left out start on it.  The tensors of a pointer array are operands of their own (one name
             each), so the array the caller builds from `ptrs` has its entries shifted one by one.
    Returns name -> float32 tensor of the poisoned run's outputs."""
    scratch = scratch or {}
    shifts = shifts or {}
    unknown = set(shifts) - set(inputs) - set(outputs)
    assert not unknown, f"shifts for unknown operands: {sorted(unknown)}"
    runs = []
    for poisoned in (True, False):
        ins = {k: guarded_input(v, poisoned, device, shifts.get(k, 0)) for k, v in inputs.items()}
        outs = {k: guarded_output(4 * _numel(s), poisoned, device, shifts.get(k, 0)) for k, s in outputs.items()}
        scr = {}
        for k, v in scratch.items():
            if isinstance(v, Guarded) and poisoned:
                scr[k] = v
            else:
                n = v.nbytes if isinstance(v, Guarded) else v
                scr[k] = Guarded(n, POISON if poisoned else 0, POISON if poisoned else 0, device)
        ptrs = {k: b.ptr for d in (ins, outs, scr) for k, b in d.items()}
        rc = call(ptrs)
        torch.cuda.synchronize(device)
        assert rc == 0, f"status {rc}"
        for k, b in list(ins.items()) + list(outs.items()) + list(scr.items()):
            assert b.guards_intact(), f"{k}: guard band overwritten (poisoned={poisoned})"
        for k, v in inputs.items():
            want = v.detach().contiguous().reshape(-1).to(device)
            if want.numel():
                assert torch.equal(ins[k].body, want.view(torch.int32)), f"{k}: input modified"
        runs.append(outs)
    result = {}
    for k, s in outputs.items():
        got, zero = runs[0][k].body, runs[1][k].body
        if check_written:
            left = int((got == _i32(POISON)).sum())
            assert left == 0, f"{k}: {left} of {got.numel()} words never written"
        assert torch.equal(got, zero), f"{k}: poisoned and zero-filled launches differ"
        result[k] = got.view(torch.float32).view(tuple(s)).clone()
    return result


def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n
