"""Contents and streams shared by tests/test_inflate_lanes.py (CPU) and tests/test_gpu_png_inflate.py (GPU): what the wave's
inflate (csrc/imp_inflate_lanes.h) has to get through -- zlib's own output over every strategy, and hand-made token lists
(tests/deflate_writer.py).  Every content here is a run of PNG scanlines: the first byte of each row is a filter type."""
import zlib

import numpy as np

import deflate_writer as D


def rows_of(data, stride):
    """`data` with a valid filter byte (0) at the start of every `stride` bytes"""
    b = bytearray(data)
    for at in range(0, len(b), stride):
        b[at] = 0
    return bytes(b)


def steep(n, seed=5):
    """a steep geometric histogram over about 40 symbols: P(k) ~ 2^-(k+1), which forces the longest codes"""
    rng = np.random.default_rng(seed)
    return np.minimum(rng.geometric(0.5, size=n) - 1, 39).astype(np.uint8).tobytes()


def photo(n, seed=1):
    from ngx_http_imgproc_amd.workloads import photo_like

    side = int(np.ceil(np.sqrt(n / 3.0))) + 1
    a = photo_like(side, side, seed).astype(np.int16)
    sub = (a - np.roll(a, 1, axis=1)) & 255                 # roughly what the Sub filter leaves
    return sub.astype(np.uint8).tobytes()[:n]


def content(kind, n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "photo":
        return photo(n, seed + 1)
    if kind == "solid":
        return bytes([7]) * n
    if kind == "random":
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    if kind == "skewed":
        return (rng.integers(0, 256, size=n) * rng.integers(0, 2, size=n) // 37).astype(np.uint8).tobytes()
    if kind == "steep":
        return steep(n, seed + 5)
    raise ValueError(kind)


def compress(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, sync_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    if not sync_every:
        return c.compress(data) + c.flush()
    out = b""
    for at in range(0, len(data), sync_every):
        out += c.compress(data[at:at + sync_every]) + c.flush(zlib.Z_SYNC_FLUSH)
    return out + c.flush()


def far_stream(n=40000, length=258, stride=None):
    """stored blocks of n bytes (n >= 32768), then ONE match of distance 32 768 exactly -- from a position past 32 KB when
    n > 32768 (the window ring has wrapped) -> (zlib stream, the bytes it means).  `stride`: rows of that many bytes (their
    filter bytes are valid in the stored part; choose it so that no row starts inside the match)"""
    rng = np.random.default_rng(n)
    head = rows_of(rng.integers(0, 256, size=n, dtype=np.uint8).tobytes(), stride or n + length)
    blocks = [D.stored(head[at:at + 30000]) for at in range(0, n, 30000)] + [D.fixed([(length, 32768)], final=True)]
    data = D.expand(blocks)
    return D.zlib_wrap(D.deflate(blocks), data), data


def shape_for(n):
    """(w, h) of the 8-bit gray PNG whose scanlines are n bytes: (w + 1) * h == n, w <= 4096; None where there is none"""
    for h in range(1, n + 1):
        if n % h == 0 and 2 <= n // h <= 4097 and h <= 16384:
            return n // h - 1, h
        if n // h < 2:
            break
    return None
