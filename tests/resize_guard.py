"""A guarded batch for the resize entry points: every source frame is a window inside a larger random parent, every
destination frame a window inside one canary-filled parent, and the pitches, frame strides and start offsets follow an
alignment class -- the properties launch_cn chooses its kernels by.

The destination parent has guard rows and at least 256 guard bytes before the first frame and after the last, guard rows
between frames (dst_stride > dh * dstep), pitch padding to the right (dstep > dw * c) and a left margin (the pointer
offset).  The guards are generous on purpose: a store that leaves its window lands in memory the test owns and shows as a
touched canary -- every byte outside the count * dh windows of dw * c bytes is compared, not a sample.

Alignment classes (of dst / dstep / dst_stride, and of src / sstep / src_stride):
  a16  everything a multiple of 16
  a4   multiples of 4, none of them a multiple of 16
  a1   odd pitch, odd frame stride and odd start (gray and BGR only: BGRA is rejected)
"""
import numpy as np

CANARY = 0xA5
CLASSES = ("a16", "a4", "a1")
GUARD_ROWS = 2
GUARD_BYTES = 256


def _up(v, m):
    return (v + m - 1) // m * m


def _fit(v, cls):
    """The smallest value >= v that belongs to the class."""
    if cls == "a16":
        return _up(v, 16)
    if cls == "a4":
        v = _up(v, 4)
        return v + 4 if v % 16 == 0 else v
    assert cls == "a1", cls
    return v | 1


class Layout:
    """Where `count` frames of `rows` rows of `row_bytes` bytes sit inside one parent buffer whose base is 16-byte aligned:
    frame f, row r starts at offset + f * stride + r * step."""

    def __init__(self, row_bytes, rows, count, cls, step=None, tail=None):
        self.row_bytes, self.rows, self.count, self.cls = row_bytes, rows, count, cls
        self.step = _fit(row_bytes + 5, cls) if step is None else step               # pitch padding to the right
        assert self.step >= row_bytes
        self.stride = _fit((rows + GUARD_ROWS) * self.step, cls)                       # guard rows between frames
        self.offset = _fit(max(GUARD_ROWS * self.step, GUARD_BYTES) + 16, cls)         # guard in front + the left margin
        self.last = self.offset + (count - 1) * self.stride + (rows - 1) * self.step + row_bytes   # one past the last pixel
        self.total = self.last + (max(GUARD_ROWS * self.step, GUARD_BYTES) + self.step if tail is None else tail)

    def windows(self, flat):
        """A (count, rows, row_bytes) view of the frames inside the parent's bytes."""
        assert flat.ndim == 1 and flat.dtype == np.uint8 and flat.size == self.total
        return np.lib.stride_tricks.as_strided(flat[self.offset:], shape=(self.count, self.rows, self.row_bytes),
                                               strides=(self.stride, self.step, 1), writeable=flat.flags.writeable)

    def in_class(self):
        vals = (self.offset, self.step, self.stride)
        if self.cls == "a16":
            return all(v % 16 == 0 for v in vals)
        if self.cls == "a4":
            return all(v % 4 == 0 and v % 16 != 0 for v in vals)
        return all(v % 2 == 1 for v in vals)


class Guarded:
    """What a guarded call left: .windows (count, fh, fw, c), .intact (no byte outside them changed), and the layouts."""

    def __init__(self, windows, intact, touched, src, dst):
        self.windows, self.intact, self.touched, self.src, self.dst = windows, intact, touched, src, dst

    def __iter__(self):                                    # windows, intact = guarded_batch(...)
        return iter((self.windows, self.intact))


def guarded_batch(gpu, frames, dw, dh, c, interp, count, align="a16", src_align=None, rotate=None, config=None,
                  sstep=None, src_at_end=False):
    """Resize `count` frames to dw x dh under guard.  `frames` holds the distinct sources (sh x sw x c each); frame i of the
    batch is frames[i % len(frames)], so a large batch costs one upload of its period.  align / src_align: the class of
    the destination and (by default the same) of the source.  With `rotate` (0, 90, 180, 270) and `config` the call is
    impgpu_batch_resize_rotate_watermark and the windows are the turned frames, otherwise impgpu_batch_cv_resize.
    sstep overrides the source pitch; src_at_end makes the last source row's last pixel the last byte of its parent.
    Returns a Guarded: `windows, intact = guarded_batch(...)`."""
    import torch

    frames = [np.ascontiguousarray(f).reshape(f.shape[0], f.shape[1], c) for f in frames]
    sh, sw = frames[0].shape[:2]
    assert all(f.shape == (sh, sw, c) for f in frames) and 1 <= len(frames) <= count
    period = len(frames)
    # ---- the sources: one period of frames on the host, repeated on the device
    sl = Layout(sw * c, sh, count, src_align or align, step=sstep, tail=0 if src_at_end else None)
    rng = np.random.Generator(np.random.PCG64(0x1A4D9100 + sw * 31 + sh * 7 + c))
    block = rng.integers(0, 256, size=period * sl.stride, dtype=np.uint8)           # bytes around the windows differ from them
    # the parent is this block repeated, so byte k of it is block[k % size]: frame i's window holds frames[i % period]
    at = sl.offset + (np.arange(period)[:, None, None] * sl.stride + np.arange(sh)[None, :, None] * sl.step
                      + np.arange(sw * c)[None, None, :])
    block[at % block.size] = np.stack(frames).reshape(period, sh, sw * c)
    one = torch.from_numpy(block).cuda()
    src = one.repeat((sl.total + block.size - 1) // block.size)[:sl.total]
    # ---- the destination: the final frames are fw x fh
    fw, fh = (dh, dw) if rotate in (90, 270) else (dw, dh)
    dl = Layout(fw * c, fh, count, align)
    assert sl.in_class() or sstep is not None, (sl.offset, sl.step, sl.stride)
    assert dl.in_class(), (dl.offset, dl.step, dl.stride)
    dst = torch.full((dl.total,), CANARY, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0                     # the classes are relative to the base
    torch.cuda.synchronize()
    if rotate is None:
        gpu.batch_cv_resize(src.data_ptr() + sl.offset, sl.stride, sw, sh, sl.step, dst.data_ptr() + dl.offset, dl.stride,
                            dw, dh, dl.step, c, count, interp)
    else:
        gpu.batch_resize_rotate_watermark(src.data_ptr() + sl.offset, sl.stride, sw, sh, sl.step, dst.data_ptr() + dl.offset,
                                          dl.stride, dl.step, dw, dh, rotate, config, c, count)
    gpu.sync()
    windows, intact, touched = guard_report(dst.cpu().numpy(), dl)
    del src, one, dst
    return Guarded(windows.reshape(count, fh, fw, c), intact, touched, sl, dl)


def guard_report(out, layout):
    """The parent's bytes after the call -> (the windows, whether every byte outside them is still the canary, the first
    few that are not as (parent offset, offset from frame 0's first pixel)).  `out` is consumed."""
    view = layout.windows(out)
    windows = view.copy()
    view[...] = CANARY
    bad = np.flatnonzero(out != CANARY)
    return windows, bad.size == 0, [(int(o), int(o) - layout.offset) for o in bad[:8]]


def describe(g):
    """For an assertion message: where the first touched guard bytes are."""
    d = g.dst
    out = []
    for off, rel in g.touched:
        f, r = divmod(rel, d.stride) if rel >= 0 else (-1, rel)
        out.append("byte %d = frame %d row %d col-byte %d" % (off, f, r // d.step if rel >= 0 else -1, r % d.step if rel >= 0 else r))
    return "dstep %d dst_stride %d row bytes %d: %s" % (d.step, d.stride, d.row_bytes, "; ".join(out))
