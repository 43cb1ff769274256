"""
Caller memory with known contents, for the tests that ask what a call WROTE rather than what it computed
(test_footprint_gpu.py; the helper's own checks, on a CPU arena, are test_footprint_host.py).

An Arena is ONE torch.uint8 allocation filled with a poison byte.  `take` hands out views of it, each with a guard band
of `guard` bytes on either side: the view's first byte follows the last byte of its front guard, the byte after its last
element is the first of its back guard, and the padding that aligns the view lies BEFORE the front guard, never between
the array and a guard.  A store one element before or after the array therefore lands in a guard, and `guards_intact`
finds it.

The guard is a condition, not a measurement: 64 KiB is more than a whole stray workgroup of 1024 lanes storing 16 bytes
(one double2) each, so a workgroup that runs past an array's end, or starts before its beginning, by up to its own length
stays inside memory the arena owns and is seen.  A store farther away than that is outside this method.

Poison 0xFF gives three recognisable values: the float64 0xFFFFFFFFFFFFFFFF, a NaN no arithmetic produces (computed NaNs
are 0x7FF8... / 0xFFF8...), the uint8 255, which is neither 0 nor 1, and the int64 / int32 -1.  `fully_written` looks for
the poison WORD of the view's dtype, so it is meaningful on a 0xFF arena only; the constructor takes the fill byte, and a
second arena of 0x00 shows that a result does not depend on what the memory held.

All comparisons are bitwise (on the integer view of the data): a NaN equals itself, +0 differs from -0.
The helpers raise AssertionError with what was hit and where, and return True, so that `assert guards_intact(a)` reads well.
"""
import numpy as np
import torch

GUARD = 65536
_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t):
    """The integer view of a tensor's data (any strides), for bitwise comparisons."""
    if t.dtype in (torch.uint8, torch.int16, torch.int32, torch.int64):
        return t
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    return t.view(_INT_OF[t.element_size()])


def poison_word(dtype, fill=0xFF):
    """The value an untouched element of `dtype` reads as, as an integer of the element's width."""
    size = torch.empty(0, dtype=dtype).element_size()
    return int.from_bytes(bytes([fill]) * size, 'little', signed=size > 1)


class Arena:
    """One uint8 allocation of `capacity` bytes on `device`, filled with `fill`; see the module docstring."""

    def __init__(self, device, guard=GUARD, fill=0xFF, capacity=16 << 20):
        if guard < 16 or not 0 <= fill <= 255:
            raise ValueError('guard >= 16 bytes, fill one byte')
        self.device, self.guard, self.fill = torch.device(device), int(guard), int(fill)
        self.buf = torch.full((int(capacity),), self.fill, dtype=torch.uint8, device=self.device)
        self.base = self.buf.data_ptr()
        self.cursor = 0
        self.views = []                                  # (name, offset of the first byte, bytes)

    def view_at(self, offset, shape, dtype, align=16, name=None):
        """The view of `shape` and `dtype` whose first byte is byte `offset` of the arena, with its two guards registered.
        Refused (ValueError): an address that is no multiple of `align`, an `align` the element does not divide, a view
        whose guards overlap an earlier view's or leave the arena."""
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(v) for v in shape)
        size = torch.empty(0, dtype=dtype).element_size()
        if align < size or align % size or align & (align - 1):
            raise ValueError(f'align {align} must be a power of two and a multiple of the element size {size}')
        if (self.base + offset) % align:
            raise ValueError(f'offset {offset}: address {self.base + offset:#x} is no multiple of the alignment {align}')
        nbytes = int(np.prod(shape, dtype=np.int64)) * size
        if offset - self.guard < self.cursor or offset + nbytes + self.guard > self.buf.numel():
            raise ValueError(f'view [{offset}, {offset + nbytes}) with guards of {self.guard} bytes does not fit: the arena is '
                             f'used up to {self.cursor} of {self.buf.numel()} bytes')
        self.views.append((name or f'#{len(self.views)}', offset, nbytes))
        self.cursor = offset + nbytes + self.guard
        return self.buf[offset:offset + nbytes].view(dtype).view(shape)

    def take(self, shape, dtype=torch.float64, align=16, name=None):
        """A fresh view, C-contiguous, at the lowest address that is a multiple of `align` and leaves room for the front guard."""
        offset = self.cursor + self.guard
        offset += -(self.base + offset) % align
        return self.view_at(offset, shape, dtype, align, name)

    def put(self, array, dtype=None, align=16, name=None):
        """`take` of the array's shape, filled with the array's bits (an input of a call; NumPy or torch) -> (view, snapshot)."""
        src = array.contiguous() if isinstance(array, torch.Tensor) else torch.from_numpy(np.array(array, order='C'))
        if dtype is not None:
            src = src.to(dtype)
        v = self.take(src.shape, src.dtype, align, name)
        v.copy_(src)
        return v, v.clone()


def guards_intact(arena):
    """Every byte of the arena outside the views is still the fill byte: the guards and the alignment padding."""
    bad = arena.buf != arena.fill
    for _, off, nb in arena.views:
        bad[off:off + nb] = False
    if not bool(bad.any()):
        return True
    hits = torch.nonzero(bad).ravel().cpu().numpy()
    msgs = []
    for name, off, nb in arena.views:
        front = hits[(hits >= off - arena.guard) & (hits < off)]
        back = hits[(hits >= off + nb) & (hits < off + nb + arena.guard)]
        if front.size:
            msgs.append(f'{name}: {front.size} byte(s) of the FRONT guard, the nearest {off - int(front.max())} byte(s) before '
                        f'the first element, the farthest {off - int(front.min())}')
        if back.size:
            msgs.append(f'{name}: {back.size} byte(s) of the BACK guard, the nearest at byte {int(back.min()) - off - nb} past '
                        f'the last element, the farthest at {int(back.max()) - off - nb}')
    if not msgs:
        msgs.append(f'{hits.size} byte(s) of alignment padding, the first at arena offset {int(hits.min())}')
    raise AssertionError('guard hit: ' + '; '.join(msgs))


def fully_written(view, leave=None, fill=0xFF, name='output'):
    """No element of `view` still holds the poison word.  `leave`: a boolean mask (the view's shape, or broadcastable to
    it) of the entries the contract leaves alone; they are not looked at (`untouched` is the check for them)."""
    left = _bits(view) == poison_word(view.dtype, fill)
    if leave is not None:
        left = left & ~torch.as_tensor(leave, dtype=torch.bool, device=view.device).broadcast_to(view.shape)
    if bool(left.any()):
        idx = torch.nonzero(left)
        raise AssertionError(f'{name}: {idx.shape[0]} of {view.numel()} element(s) not written (still poison), the first at '
                             f'{idx[0].tolist()}, the last at {idx[-1].tolist()}')
    return True


def untouched(view, where=None, fill=0xFF, name='array'):
    """Every element of `view` (those of the boolean mask `where`, if given) still holds the poison word."""
    hit = _bits(view) != poison_word(view.dtype, fill)
    if where is not None:
        hit = hit & torch.as_tensor(where, dtype=torch.bool, device=view.device).broadcast_to(view.shape)
    if bool(hit.any()):
        idx = torch.nonzero(hit)
        raise AssertionError(f'{name}: {idx.shape[0]} element(s) the call must leave alone were written, the first at '
                             f'{idx[0].tolist()}, the last at {idx[-1].tolist()}')
    return True


def same_bits(a, b, name='array'):
    """`a` and `b` (same shape and dtype, any strides) hold the same bits."""
    if a.shape != b.shape or a.dtype != b.dtype:
        raise AssertionError(f'{name}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}')
    diff = _bits(a) != _bits(b).to(a.device)
    if bool(diff.any()):
        idx = torch.nonzero(diff)
        raise AssertionError(f'{name}: {idx.shape[0]} of {a.numel()} element(s) differ bitwise, the first at {idx[0].tolist()}, '
                             f'the last at {idx[-1].tolist()}')
    return True


def unchanged(view, snapshot, name='input'):
    """`view` still holds the bits of `snapshot` (a clone taken before the call)."""
    return same_bits(view, snapshot, name + ' (must be unchanged)')


def scrub(ctx, U, Ep, mats_kw=None):
    """Leaves nothing of an earlier call in the context's persistent device buffers (fep_api.hip: fep_ctx::hbuf), so that a
    following K,F-only / K-only / F-only / accepting step or assemble() cannot pass a bitwise pin with what the call before
    it left there: one full-output host step on another state (-1.7 U, another plastic strain; `mats_kw`: the step's e0 /
    e0_field / e0_scale keywords), then assemble() of all-NaN ds and s.  Afterwards the K and F buffers hold NaN and the
    point buffers NaN or the other state's values.  The library promises that non-finite data leaves no trace
    (include/fep.h, rule 4)."""
    kw = dict(mats_kw or {})
    n = ctx.n_int
    ep2 = None if Ep is None else np.ascontiguousarray(0.5 * np.asarray(Ep, dtype=float)[:, ::-1])
    ctx.step(-1.7 * np.asarray(U, dtype=float), ep2, want=('E', 's', 'ds', 'ind_p', 'K', 'F'), **kw)
    ctx.assemble(np.full((9, n), np.nan), np.full((4, n), np.nan))
