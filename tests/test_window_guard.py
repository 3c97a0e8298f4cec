"""window_guard on the host (no device): the layouts the operator tests use are in their classes, a planted byte is found
and named, an untouched parent reports intact.  This is the evidence that the guard of test_gpu_operator_guard.py can fail."""
import re

import numpy as np
import pytest

from resize_guard import GUARD_BYTES, GUARD_ROWS
from test_gpu_exit_guard import layouts_used as exit_layouts_used
from test_gpu_operator_guard import layouts_used
from window_guard import KINDS, WindowLayout, describe, guard_compare, layout_for, locate, make_parent


def _frames(lay, n):
    rng = np.random.Generator(np.random.PCG64(7))
    return [rng.integers(0, 256, size=(lay.rows, lay.row_bytes), dtype=np.uint8) for _ in range(n)]


def test_every_layout_of_the_operator_tests_is_in_its_class():
    n = exits = 0
    for used in (layouts_used, exit_layouts_used):
        for lay in used():
            where = (lay.cls, lay.row_bytes, lay.rows, lay.count, lay.offset, lay.step, lay.stride)
            assert lay.in_class(), where
            guard = max(GUARD_ROWS * lay.step, GUARD_BYTES)
            assert lay.step >= lay.row_bytes and lay.offset >= guard and lay.total - lay.last >= guard, where
            assert lay.stride >= (lay.rows + GUARD_ROWS) * lay.step, where            # guard rows between frames
            if used is exit_layouts_used:
                # the exits' windows: a padded pitch, and a JPEG block's 15 columns past a row's end (60 bytes of BGRA) or a
                # download's step * rows bytes from the last window's start are still the parent's
                assert lay.step > lay.row_bytes and lay.total - lay.last >= 60 + lay.step, where
                exits += 1
            else:
                n += 1
    assert n > 100
    assert exits > 100


def test_the_kinds_differ_where_the_kernels_look():
    w, h = 36, 32
    for c in (3, 4):
        rb = w * c
        lay = {k: layout_for(k, w, h, c, 3) for k in KINDS}
        for k in ("a16", "a4", "a1"):
            assert lay[k].step > rb
        assert all(v % 16 == 0 for v in (lay["a16"].offset, lay["a16"].step, lay["a16"].stride))
        assert all(v % 4 == 0 and v % 16 for v in (lay["a4"].offset, lay["a4"].step, lay["a4"].stride))
        assert all(v % 2 for v in (lay["a1"].offset, lay["a1"].step, lay["a1"].stride))
        for k in ("contig", "contig-a4", "contig-s4"):
            assert lay[k].step == rb
        assert lay["contig"].offset % 16 == 0 and lay["contig"].stride % 16 == 0
        assert lay["contig-a4"].offset % 4 == 0 and lay["contig-a4"].offset % 16 != 0 and lay["contig-a4"].stride % 16 == 0
        assert lay["contig-s4"].offset % 16 == 0 and lay["contig-s4"].stride % 4 == 0 and lay["contig-s4"].stride % 16 != 0
    # a frame stride chosen freely above rows * step: the same pitch with a stride on and off the 16-byte grid
    a, b = WindowLayout(144, 32, 3, "a16", step=144, stride=144 * 32 + 16), WindowLayout(144, 32, 3, "a16", step=144, stride=144 * 32 + 4)
    assert a.in_class() and b.in_class() and a.stride % 16 == 0 and b.stride % 16 == 4
    with pytest.raises(AssertionError):
        WindowLayout(144, 32, 3, "a16", step=144, stride=144 * 32 - 1)


def test_the_parent_is_random_and_holds_the_frames():
    lay = layout_for("a4", 21, 9, 3, 5)
    frames = _frames(lay, 3)
    parent = make_parent(lay, frames, seed=1)
    assert parent.dtype == np.uint8 and parent.shape == (lay.total,)
    assert np.array_equal(parent, make_parent(lay, frames, seed=1)) and not np.array_equal(parent, make_parent(lay, frames, seed=2))
    view = lay.windows(parent)
    for i in range(5):
        assert np.array_equal(view[i], frames[i % 3])
    outside = parent.copy()
    lay.windows(outside)[...] = 0
    counts = np.bincount(outside[:lay.offset], minlength=256)                  # the guard in front: no constant
    assert (counts > 0).sum() > 100


@pytest.mark.parametrize("kind", KINDS)
def test_an_untouched_parent_reports_intact(kind):
    lay = layout_for(kind, 21, 9, 3, 3)
    frames = _frames(lay, 3)
    before = make_parent(lay, frames)
    for fresh in (False, True):
        rep = guard_compare(before, before.copy(), lay, fresh=fresh)
        assert rep.intact and rep.touched == []
        assert np.array_equal(rep.windows, np.stack(frames))
    # what an in-place operator does: every window byte changes, nothing else
    after = before.copy()
    lay.windows(after)[...] ^= 0xFF
    rep = guard_compare(before, after.copy(), lay)
    assert rep.intact and np.array_equal(rep.windows, np.stack(frames) ^ 0xFF)
    rep = guard_compare(before, after.copy(), lay, fresh=True)                  # ... which a fresh-frame operator must not
    assert not rep.intact and locate(lay, rep.touched[0][0]) == (0, 0, 0)


def _named(rep):
    """(byte, frame, row, col-byte) of every offender in describe()'s text."""
    return [tuple(int(v) for v in m) for m in re.findall(r"byte (\d+) = frame (-?\d+) row (-?\d+) col-byte (-?\d+)", describe(rep))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fresh", [False, True])
def test_a_planted_byte_is_found_and_named(kind, fresh):
    lay = layout_for(kind, 21, 9, 3, 3)
    rb, rows, padded = lay.row_bytes, lay.rows, lay.step > lay.row_bytes
    before = make_parent(lay, _frames(lay, 2))
    places = {"in the gap between frames": (lay.offset + rows * lay.step + 3, (0, rows, 3)),
              "one before frame 0": (lay.offset - 1, (-1, -1, -1)),
              "one past the last pixel": (lay.last, (2, rows - 1, rb) if padded else (2, rows, 0)),
              "the first byte of the parent": (0, (-1, -1, -lay.offset)),
              "the last byte of the parent": (lay.total - 1, None)}
    if padded:                                                                   # (a contiguous row ends where the next begins)
        places["one past a row's end"] = (lay.offset + lay.stride + 2 * lay.step + rb, (1, 2, rb))
        places["one before a row's start"] = (lay.offset + 2 * lay.stride + 4 * lay.step - 1, (2, 3, lay.step - 1))
    for name, (off, want) in places.items():
        after = before.copy()
        after[off] ^= 0x40
        rep = guard_compare(before, after, lay, fresh=fresh)
        assert not rep.intact, name
        assert rep.touched == [(off, off - lay.offset)], name
        if want is not None:
            assert locate(lay, off) == want, name
            assert _named(rep) == [(off,) + want], (name, describe(rep))
    # several at once: all compared, the first few named in order
    after = before.copy()
    offs = [0, lay.offset - 1, lay.offset + rows * lay.step, lay.last, lay.total - 1]
    after[offs] ^= 1
    rep = guard_compare(before, after, lay, fresh=fresh)
    assert [t[0] for t in rep.touched] == offs and len(_named(rep)) == len(offs)
    # inside a window: the caller's to compare in place, an offender for a fresh-frame operator
    after = before.copy()
    off = lay.offset + lay.stride + 4 * lay.step + 5
    after[off] ^= 0x01
    rep = guard_compare(before, after, lay, fresh=fresh)
    assert rep.intact == (not fresh)
    assert rep.windows[1, 4, 5] == before[off] ^ 0x01
    if fresh:
        assert _named(rep) == [(off, 1, 4, 5)]
