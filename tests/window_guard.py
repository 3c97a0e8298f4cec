"""A guard for the operators that work in place on a caller's memory, or read a caller's window and write a fresh frame:
the frames are windows inside one parent buffer of seeded RANDOM bytes (resize_guard's destination parent holds a constant:
here the parent is also what a border tap that leaves its window would read, and a random byte there gives a wrong pixel,
not a plausible one), a host copy of the parent is kept from before the call, and afterwards every byte outside the
windows -- all of them, not a sample -- must equal that copy.  For an operator that writes a fresh frame the windows must
be unchanged as well (`fresh=True`).

The layouts are resize_guard's, with two freedoms the pointwise kernels choose their form by: a contiguous pitch
(step == row_bytes, Layout(step=...) already allows it) whose start and frame stride are classed on their own, and a frame
stride chosen freely above rows * step.

    lay = layout_for("contig-s4", w, h, c, count)       # one of KINDS
    g = GuardedParent(lay, frames)                       # needs a device
    gpu.batch_filters(g.ptr(), lay.stride, w, h, c, lay.step, count, filters)
    rep = g.report(gpu)                                  # .windows, .intact, .touched; describe(rep) for the message
"""
import numpy as np

from resize_guard import CLASSES, GUARD_BYTES, GUARD_ROWS, Layout, _fit, describe  # noqa: F401  (describe: for the callers)


def _is(v, cls):
    if cls == "a16":
        return v % 16 == 0
    if cls == "a4":
        return v % 4 == 0 and v % 16 != 0
    assert cls == "a1", cls
    return v % 2 == 1


class WindowLayout(Layout):
    """resize_guard.Layout whose start, pitch and frame stride are classed one by one.  `cls` is the class of the pitch
    (unless `step` gives the pitch itself: then it belongs to no class, as a contiguous pitch is whatever the row is) and
    the default for the other two; `start` the class of the offset of frame 0; the frame stride is the smallest of
    `stride_cls` that leaves GUARD_ROWS rows between two frames, or `stride` itself, anything from rows * step on."""

    def __init__(self, row_bytes, rows, count, cls, step=None, start=None, stride_cls=None, stride=None):
        assert cls in CLASSES, cls
        Layout.__init__(self, row_bytes, rows, count, cls, step=step)
        self.step_cls = None if step is not None else cls
        self.start_cls = start or cls
        self.stride_cls = None if stride is not None else (stride_cls or cls)
        guard = max(GUARD_ROWS * self.step, GUARD_BYTES)
        self.offset = _fit(guard + 16, self.start_cls)                                  # guard in front + the left margin
        self.stride = stride if stride is not None else _fit((rows + GUARD_ROWS) * self.step, self.stride_cls)
        assert self.stride >= rows * self.step, (self.stride, rows, self.step)
        self.last = self.offset + (count - 1) * self.stride + (rows - 1) * self.step + row_bytes   # one past the last pixel
        self.total = self.last + guard + self.step

    def in_class(self):
        return (_is(self.offset, self.start_cls) and (self.step_cls is None or _is(self.step, self.step_cls))
                and (self.stride_cls is None or _is(self.stride, self.stride_cls)))


# The layouts the operator tests use.  "a16" / "a4" / "a1": everything in that class, the pitch padded to the right.  The
# contiguous ones have step == row_bytes: all on the 16-byte grid ("contig"), only the start moved to the 4-byte grid
# ("contig-a4"), only the frame stride moved to it ("contig-s4").
KINDS = ("a16", "a4", "a1", "contig", "contig-a4", "contig-s4")


def layout_for(kind, w, h, c, count=1):
    rb = w * c
    if kind in CLASSES:
        return WindowLayout(rb, h, count, kind)
    if kind == "contig":
        return WindowLayout(rb, h, count, "a16", step=rb)
    if kind == "contig-a4":
        return WindowLayout(rb, h, count, "a16", step=rb, start="a4")
    assert kind == "contig-s4", kind
    return WindowLayout(rb, h, count, "a16", step=rb, stride_cls="a4")


def make_parent(layout, frames, seed=0):
    """The parent's bytes on the host: seeded random everywhere, frames[i % len(frames)] in window i."""
    frames = [np.ascontiguousarray(f, dtype=np.uint8).reshape(layout.rows, layout.row_bytes) for f in frames]
    assert 1 <= len(frames) <= layout.count
    rng = np.random.Generator(np.random.PCG64(0x1A4D9200 + seed + layout.row_bytes * 31 + layout.rows * 7))
    parent = rng.integers(0, 256, size=layout.total, dtype=np.uint8)
    view = layout.windows(parent)
    for i in range(layout.count):
        view[i] = frames[i % len(frames)]
    return parent


class Report:
    """What a guarded call left: .windows (count, rows, row_bytes), .intact (every byte that had to stay equals the copy
    from before), .touched (the first few that do not, as describe() takes them) and .dst, the layout."""

    def __init__(self, windows, intact, touched, layout):
        self.windows, self.intact, self.touched, self.dst = windows, intact, touched, layout


def guard_compare(before, after, layout, fresh=False):
    """before / after: the parent's bytes around the call (`after` is consumed).  Every byte outside the windows must be
    unchanged; with fresh=True (the operator wrote a frame of its own) every byte inside them too."""
    assert before.shape == after.shape == (layout.total,)
    view = layout.windows(after)
    windows = view.copy()
    if not fresh:
        view[...] = layout.windows(before)                     # whatever the call left there is the caller's to compare
    bad = np.flatnonzero(after != before)
    return Report(windows, bad.size == 0, [(int(o), int(o) - layout.offset) for o in bad[:8]], layout)


def locate(layout, off):
    """Parent offset -> (frame, row, column byte), in describe()'s arithmetic (-1, -1, negative before frame 0)."""
    rel = off - layout.offset
    if rel < 0:
        return -1, -1, rel
    f, r = divmod(rel, layout.stride)
    return f, r // layout.step, r % layout.step


class GuardedParent:
    """The parent on the device (a torch uint8 tensor whose base is 16-byte aligned: the classes are relative to it) and
    its host copy from before the call."""

    def __init__(self, layout, frames, seed=0):
        import torch

        assert layout.in_class(), (layout.offset, layout.step, layout.stride)
        self.layout = layout
        self.before = make_parent(layout, frames, seed)
        self.dev = torch.from_numpy(self.before).cuda()
        assert self.dev.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def ptr(self, frame=0):
        return self.dev.data_ptr() + self.layout.offset + frame * self.layout.stride

    def wrap(self, gpu, w, h, c, frame=0):
        """impgpu_image_wrap of window `frame`; release the handle before this object goes."""
        assert w * c == self.layout.row_bytes and h == self.layout.rows
        return gpu.Image.wrap(self.ptr(frame), w, h, c, self.layout.step)

    def report(self, gpu, fresh=False):
        gpu.sync()
        return guard_compare(self.before, self.dev.cpu().numpy(), self.layout, fresh)
