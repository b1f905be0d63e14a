"""A guarded, poisoning stand-in for `latentaugment_amd._lib.workspace`, and the same for outputs that a test allocates itself.

    g = Guarded('ones')
    monkeypatch.setattr(_lib, 'workspace', g.alloc)
    ... calls into the package ...
    g.check()

Every allocation is GUARD + nbytes + GUARD bytes of one fresh uint8 tensor.  The payload starts GUARD = 4096 bytes into it (so it keeps
the alignment torch gives an allocation, up to 4096) and the rear band starts exactly at byte `nbytes`, not at a rounded size: a write
one byte past the reported size lands in it.  Both bands hold 0xA5; the payload holds the pattern:

    zeros   0x00 bytes
    ones    0xFF bytes: NaN as f16 / f32 / f64, -1 as a signed integer, the maximum as an unsigned one
    bytes   seeded torch.randint uint8, the same bytes on every run

A buffer that starts at zero hides a missing atomicMax reset and one that starts at 0xFF a missing atomicMin reset, hence more than one.
`check()` synchronises and asserts that every band of every allocation made so far is still 0xA5 to the byte; a failure names the
allocation (index, size, the caller's file and line) and the first damaged offset relative to the payload (negative: in front of it,
>= nbytes: behind it).  Nothing here touches a GPU at import time, and everything works on CPU tensors too."""
import os
import traceback

import torch

GUARD = 4096
BAND = 0xA5
PATTERNS = ('zeros', 'ones', 'bytes')
_HERE = os.path.abspath(__file__)
_BLOCK = (1 << 20) + 13          # the seeded bytes repeat with an odd period: no power-of-two stride sees the same byte twice


def _caller():
    """file:line of the innermost frame that is neither this module nor _lib.py (the package's call site of _lib.workspace)."""
    for fr in reversed(traceback.extract_stack()[:-2]):
        if os.path.abspath(fr.filename) != _HERE and os.path.basename(fr.filename) != '_lib.py':
            return f'{fr.filename}:{fr.lineno}'
    return '?'


class GuardError(AssertionError):
    pass


class Guarded:
    def __init__(self, pattern, seed=20240229):
        if not (pattern in PATTERNS or isinstance(pattern, int) and 0 <= pattern <= 255):
            raise ValueError(f'pattern: one of {PATTERNS} or a byte value, got {pattern!r}')
        self.pattern, self.seed = pattern, seed
        self.records = []          # (parent uint8 tensor, payload bytes, caller)
        self._block = None

    def _fill(self, payload):
        n = payload.numel()
        if n == 0:
            return
        if self.pattern == 'bytes':
            if self._block is None:
                self._block = torch.randint(0, 256, [_BLOCK], dtype=torch.uint8, generator=torch.Generator().manual_seed(self.seed))
            block = self._block.to(payload.device)
            for lo in range(0, n, _BLOCK):
                payload[lo:lo + _BLOCK] = block[:min(_BLOCK, n - lo)]
        else:
            payload.fill_({'zeros': 0, 'ones': 0xFF}.get(self.pattern, self.pattern))

    def _new(self, nbytes, device, caller):
        parent = torch.empty([GUARD + nbytes + GUARD], dtype=torch.uint8, device=device)
        parent[:GUARD] = BAND
        parent[GUARD + nbytes:] = BAND
        payload = parent[GUARD:GUARD + nbytes]
        self._fill(payload)
        self.records.append((parent, nbytes, caller))
        return payload

    def alloc(self, nbytes, device, dtype=None):
        """Signature and result of `_lib.workspace`: nbytes // itemsize elements of `dtype` (uint8 unless given) on `device`."""
        dtype = torch.uint8 if dtype is None else dtype
        item = torch.empty([], dtype=dtype).element_size()
        count = int(nbytes) // item
        return self._new(count * item, device, _caller()).view(dtype)

    def tensor(self, shape, dtype, device, fill):
        """A contiguous tensor of `shape` between two bands, every element `fill` (choose a value that a correct run never leaves)."""
        shape = [int(s) for s in shape]
        count = 1
        for s in shape:
            count *= s
        item = torch.empty([], dtype=dtype).element_size()
        caller = _caller()
        t = self._new(count * item, device, caller).view(dtype).reshape(shape)
        t.fill_(fill)
        return t

    def damage(self):
        """[(index, nbytes, caller, first damaged offset relative to the payload)] of every allocation with a changed band."""
        bad = []
        synced = set()
        for i, (parent, n, caller) in enumerate(self.records):
            if parent.is_cuda and parent.device not in synced:
                torch.cuda.synchronize(parent.device)
                synced.add(parent.device)
            front, rear = parent[:GUARD], parent[GUARD + n:]
            off = None
            if not bool((front == BAND).all()):
                off = int((front != BAND).nonzero()[0]) - GUARD
            elif not bool((rear == BAND).all()):
                off = n + int((rear != BAND).nonzero()[0])
            if off is not None:
                bad.append((i, n, caller, off))
        return bad

    def check(self):
        bad = self.damage()
        if bad:
            raise GuardError('; '.join(f'allocation #{i} ({n} bytes, from {c}): guard band written, first at payload offset {o}'
                                       + (f' ({-o} before the payload)' if o < 0 else f' ({o - n} past its end)')
                                       for i, n, c, o in bad))


def guarded_tensor(shape, dtype, device, fill, guard=None):
    """An output that a test allocates itself and passes through ctypes, kept between bands that `guard.check()` covers.  Without a
    `guard` it gets one of its own, reachable as the tensor's `.guard` (`t.guard.check()`)."""
    own = Guarded('zeros') if guard is None else guard
    t = own.tensor(shape, dtype, device, fill)
    t.guard = own
    return t
