"""A small PNG encoder for the palette, 1/2/4-bit gray and Adam7 tests (PNG specification 7.2 bit packing, 8.2 Adam7, 9.2
filters with a chosen type per row).  Pillow cannot write Adam7 and picks its own row filters; this file never DECODES: the
expected pixels come from Pillow (libpng's rules), or from `model` where Pillow and libpng differ (palette indices past the
PLTE's entries: libpng reads zeros).  Used by tests/golden/png_ext/make_png_ext_golden.py and the png_ext tests."""
import io
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
# Adam7 pass p: x = X0 + k * XS, y = Y0 + j * YS
A7 = [(0, 8, 0, 8), (4, 8, 0, 8), (0, 4, 4, 8), (2, 4, 0, 4), (0, 2, 2, 4), (1, 2, 0, 2), (0, 1, 1, 2)]
SPP = {0: 1, 2: 3, 3: 1, 6: 4}


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def passes(w, h, interlace):
    """[(pass, x0, xs, y0, ys, pass width, pass height)] of the non-empty passes (the whole image when not interlaced)"""
    if not interlace:
        return [(0, 0, 1, 0, 1, w, h)]
    out = []
    for p, (x0, xs, y0, ys) in enumerate(A7):
        pw = (w - x0 + xs - 1) // xs if w > x0 else 0
        ph = (h - y0 + ys - 1) // ys if h > y0 else 0
        if pw and ph:
            out.append((p, x0, xs, y0, ys, pw, ph))
    return out


def pack_row(samples, depth):
    """one row of samples (< 2 ** depth) -> bytes, the leftmost sample in the high bits"""
    s = np.asarray(samples, dtype=np.uint8).ravel()
    if depth == 8:
        return s.tobytes()
    per = 8 // depth
    pad = (-len(s)) % per
    s = np.concatenate([s, np.zeros(pad, np.uint8)]).reshape(-1, per).astype(np.int32)
    shifts = np.array([8 - depth * (i + 1) for i in range(per)], np.int32)
    return (s << shifts).sum(axis=1).astype(np.uint8).tobytes()


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_bytes(rows, fu, kinds):
    """rows: list of equal-length byte rows; fu: the filter unit in bytes; kinds[y] in 0..4 -> the filtered scanlines"""
    out = bytearray()
    prev = np.zeros(len(rows[0]), np.int32)
    for y, r in enumerate(rows):
        cur = np.frombuffer(r, np.uint8).astype(np.int32)
        left = np.concatenate([np.zeros(fu, np.int32), cur[:-fu]])[: len(cur)]
        upleft = np.concatenate([np.zeros(fu, np.int32), prev[:-fu]])[: len(cur)]
        k = int(kinds[y])
        pred = [0, left, prev, (left + prev) >> 1, None][k] if k < 4 else _paeth(left, prev, upleft)
        out.append(k)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def scanlines(samples, colour, depth, interlace, kinds):
    """samples: H x W x spp (values < 2 ** depth) in file order -> the filtered stream of every non-empty pass.
    kinds: a callable (pass, row) -> filter type, or an int."""
    h, w = samples.shape[:2]
    fu = max(1, SPP[colour] * depth // 8)
    out = b""
    for p, x0, xs, y0, ys, pw, ph in passes(w, h, interlace):
        sub = samples[y0::ys, x0::xs]
        rows = [pack_row(sub[j], depth) for j in range(ph)]
        out += filter_bytes(rows, fu, [kinds(p, j) if callable(kinds) else kinds for j in range(ph)])
    return out


def write(samples, colour, depth=8, interlace=0, kinds=0, palette=None, trns=None, extra=(), raw=None, pieces=1):
    """a PNG file.  palette: N x 3 (R,G,B) or raw PLTE bytes; trns: tRNS payload bytes; raw: the IDAT stream's bytes
    instead of the samples' scanlines (damaged files)"""
    samples = np.asarray(samples, np.uint8)
    if samples.ndim == 2:
        samples = samples[:, :, None]
    h, w = samples.shape[:2]
    ihdr = struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace)
    body = chunk(b"IHDR", ihdr) + b"".join(extra)
    if palette is not None:
        body += chunk(b"PLTE", palette if isinstance(palette, bytes) else np.asarray(palette, np.uint8).tobytes())
    if trns is not None:
        body += chunk(b"tRNS", trns)
    z = zlib.compress(raw if raw is not None else scanlines(samples, colour, depth, interlace, kinds), 9)
    cuts = [len(z) * i // pieces for i in range(pieces + 1)]
    body += b"".join(chunk(b"IDAT", z[cuts[i]:cuts[i + 1]]) for i in range(pieces))
    return SIG + body + chunk(b"IEND", b"")


def model(samples, colour, depth, palette=None):
    """what cvDecodeImage(blob, -1) gives (libpng 1.6 + OpenCV 2.4's flags), in OpenCV's channel order"""
    s = np.asarray(samples, np.uint8)
    if s.ndim == 2:
        s = s[:, :, None]
    if colour == 3:
        pal = np.zeros((256, 3), np.uint8)
        p = np.asarray(palette, np.uint8).reshape(-1, 3)
        pal[: len(p)] = p
        return np.ascontiguousarray(pal[s[:, :, 0]][:, :, ::-1])
    if colour == 0:
        return (s.astype(np.int32) * (255 // ((1 << depth) - 1))).astype(np.uint8)
    return np.ascontiguousarray(s[:, :, [2, 1, 0] + ([3] if colour == 6 else [])])


def pillow(blob):
    """Pillow's (libpng's) decode in OpenCV's order: palette -> B,G,R, gray -> 1 channel"""
    from PIL import Image

    im = Image.open(io.BytesIO(blob))
    if im.mode == "P":
        im = im.convert("RGB")
    a = np.asarray(im)
    if a.dtype == bool:
        a = a.astype(np.uint8) * 255
    if a.ndim == 2:
        return np.ascontiguousarray(a[:, :, None])
    return np.ascontiguousarray(a[:, :, [2, 1, 0] + ([3] if a.shape[2] == 4 else [])])


def random_file(rng, colour, depth, interlace, w, h, n_pal=None, out_of_range=False):
    """(file, expected pixels): random samples, a random filter per row, a random PLTE of n_pal entries"""
    spp = SPP[colour]
    top = 1 << depth
    palette = None
    if colour == 3:
        n_pal = n_pal or int(rng.integers(1, top + 1))
        palette = rng.integers(0, 256, size=(n_pal, 3), dtype=np.uint8)
        hi = top if out_of_range else n_pal
        samples = rng.integers(0, hi, size=(h, w, 1), dtype=np.uint8)
    else:
        samples = rng.integers(0, top, size=(h, w, spp), dtype=np.uint8)
    kinds_tab = rng.integers(0, 5, size=(7, h))
    blob = write(samples, colour, depth, interlace, kinds=lambda p, j: int(kinds_tab[p, j]), palette=palette)
    return blob, model(samples, colour, depth, palette)
