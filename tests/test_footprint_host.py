"""
The checks of tests/footprint.py on a CPU arena, where the writes are torch's own and their place is known: a helper that
cannot see a store one element outside a view, or an element nobody wrote, would make every test of test_footprint_gpu.py
pass for nothing.  No GPU.
"""
import numpy as np
import pytest
import torch

from footprint import Arena, _bits, fully_written, guards_intact, poison_word, same_bits, unchanged, untouched

DTYPES = [(torch.float64, 8), (torch.int64, 8), (torch.int32, 4), (torch.uint8, 1)]


def _arena(fill=0xFF):
    return Arena('cpu', guard=4096, fill=fill, capacity=1 << 18)


def test_views_touch_their_guards_and_padding_lies_before_the_front_guard():
    a = _arena()
    v1 = a.take(5, torch.uint8, align=1, name='bytes')                  # ends at an odd address
    v2 = a.take((3, 7), torch.float64, name='doubles')
    v3 = a.take(3, torch.int32, align=4, name='ints')
    for v, (name, off, nb) in zip((v1, v2, v3), a.views):
        assert v.data_ptr() == a.base + off and nb == v.numel() * v.element_size() and v.is_contiguous()
    assert v2.data_ptr() % 16 == 0 and v3.data_ptr() % 4 == 0
    (_, o1, n1), (_, o2, n2), (_, o3, n3) = a.views
    assert o1 == a.guard                                                # no slack in front of the first view
    # back guard of one view, then padding, then the front guard of the next: the padding is what is left over
    pad = o2 - a.guard - (o1 + n1 + a.guard)
    assert 0 <= pad < 16 and (a.base + o1 + n1 + a.guard + pad + a.guard) % 16 == 0
    assert o3 - a.guard - (o2 + n2 + a.guard) == 0                      # already aligned: none
    assert guards_intact(a)
    assert float(v2.view(torch.int64)[0, 0]) == -1 and int(v1[0]) == 255 and int(v3[0]) == -1
    assert torch.isnan(v2).all()


@pytest.mark.parametrize('dtype,size', DTYPES)
@pytest.mark.parametrize('side', ['front', 'back'])
def test_a_write_one_element_outside_a_view_is_flagged(dtype, size, side):
    a = _arena()
    a.take(9, torch.float64, name='first')
    v = a.take((4, 6), dtype, name='victim')
    a.take(2, torch.float64, name='last')
    _, off, nb = a.views[1]
    assert guards_intact(a)
    # torch's own write through a view of the arena that is one element longer on that side
    start = off - size if side == 'front' else off
    longer = a.buf[start:start + nb + size].view(dtype)
    longer[0 if side == 'front' else -1] = 3
    with pytest.raises(AssertionError, match=rf'victim: {size} byte\(s\) of the {side.upper()} guard, the nearest '
                       + (rf'1 byte\(s\) before the first element, the farthest {size}$' if side == 'front' else r'at byte 0 past')):
        guards_intact(a)
    assert fully_written(v.fill_(1))                                    # the view itself is whole


def test_a_write_into_the_padding_is_flagged():
    a = _arena()
    a.take(5, torch.uint8, align=1)
    a.take(4, torch.float64)
    (_, o1, n1), (_, o2, _) = a.views
    assert o2 - a.guard > o1 + n1 + a.guard
    a.buf[o1 + n1 + a.guard] = 0
    with pytest.raises(AssertionError, match='alignment padding'):
        guards_intact(a)


@pytest.mark.parametrize('dtype,size', DTYPES)
def test_an_unwritten_element_is_flagged(dtype, size):
    a = _arena()
    v = a.take((3, 5), dtype, name='out')
    with pytest.raises(AssertionError, match=r'15 of 15 element\(s\) not written'):
        fully_written(v)
    v.fill_(1)
    assert fully_written(v)
    _bits(v).view(-1)[7] = poison_word(dtype)                           # one hole
    with pytest.raises(AssertionError, match=r'1 of 15 element\(s\) not written \(still poison\), the first at \[1, 2\]'):
        fully_written(v, name='out')
    leave = np.zeros((3, 5), dtype=bool)
    leave[1, 2] = True
    assert fully_written(v, leave=leave) and untouched(v, where=leave)
    with pytest.raises(AssertionError, match='must leave alone'):
        untouched(v, where=~leave)


def test_a_computed_nan_is_written_and_the_poison_nan_is_not():
    a = _arena()
    v = a.take(4, torch.float64)
    v[:] = torch.tensor([float('nan'), -float('nan'), float('inf'), 0.0], dtype=torch.float64)
    assert fully_written(v)
    v[1] = torch.tensor([-1], dtype=torch.int64).view(torch.float64)[0]
    with pytest.raises(AssertionError, match=r'the first at \[1\]'):
        fully_written(v)


def test_strided_views_unused_columns_stay_poison():
    a = _arena()
    full = a.take((10, 5), torch.float64)
    used = full[:, :3]
    used.copy_(torch.arange(30, dtype=torch.float64).reshape(10, 3))
    cols = np.arange(5) >= 3
    assert fully_written(used) and fully_written(full, leave=cols) and untouched(full, where=cols) and untouched(full[:, 3:])
    full[4, 3] = 0.0
    with pytest.raises(AssertionError, match=r'the first at \[4, 3\]'):
        untouched(full, where=cols)
    f = a.take((3, 10), torch.float64).t()                              # F order
    assert not f.is_contiguous()
    with pytest.raises(AssertionError):
        fully_written(f)
    f.fill_(2.0)
    assert fully_written(f)


def test_unchanged_is_bitwise():
    a = _arena(fill=0x00)
    v, snap = a.put(np.array([0.0, 1.0, np.nan]))
    assert unchanged(v, snap) and guards_intact(a)                      # a NaN equals itself
    v[0] = -0.0
    with pytest.raises(AssertionError, match=r'1 of 3 element\(s\) differ bitwise, the first at \[0\]'):
        unchanged(v, snap)
    with pytest.raises(AssertionError):
        same_bits(v, snap[:2])


def test_a_second_poison_of_zero():
    a = _arena(fill=0x00)
    v = a.take(6, torch.float64)
    assert (v == 0).all() and guards_intact(a)
    a.buf[a.views[0][1] + 48] = 1
    with pytest.raises(AssertionError, match='BACK guard'):
        guards_intact(a)


def test_a_misaligned_view_is_refused():
    a = _arena()
    aligned = a.guard + (-(a.base + a.guard) % 16)
    with pytest.raises(ValueError, match='no multiple of the alignment 16'):
        a.view_at(aligned + 8, 4, torch.float64, align=16)
    with pytest.raises(ValueError, match='no multiple of the alignment 8'):
        a.view_at(aligned + 4, 4, torch.float64, align=8)
    with pytest.raises(ValueError, match='multiple of the element size'):
        a.view_at(aligned, 4, torch.float64, align=4)
    assert a.views == []                                                # a refused view registers nothing
    v = a.view_at(aligned + 8, 4, torch.float64, align=8)               # the same address at the alignment it has
    assert v.data_ptr() % 16 == 8
    with pytest.raises(ValueError, match='does not fit'):               # its guard would overlap the view before
        a.view_at(aligned + 8 + 32, 4, torch.float64, align=8)
    with pytest.raises(ValueError, match='does not fit'):
        a.take(1 << 18, torch.uint8, align=1)
