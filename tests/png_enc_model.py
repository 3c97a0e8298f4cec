"""A pure-Python oracle of the PNG answer (cvEncodeImage(".png", frame, {CV_IMWRITE_PNG_COMPRESSION, q}), bridge.c:704):
libpng 1.6's filter heuristic in numpy, Python's zlib at Z_RLE, libpng's CINFO rule for short streams and its 8192-byte
IDAT chunks.  tests/test_png_enc_host.py pins it to the libpng fixtures of tests/golden/png_enc, so that randomized GPU
tests can compare against it anywhere.  `libpng_encode` drives the system's libpng 1.6 itself (ctypes, no png.h needed)
where it can be loaded."""
import ctypes as C
import ctypes.util
import struct
import zlib

import numpy as np


def filter_rows(frame):
    """HxWxC BGR[A] / gray frame -> the filtered scanlines libpng writes (filter byte + R, G, B[, A] per row)."""
    a = frame if frame.ndim == 3 else frame[:, :, None]
    h, w, c = a.shape
    if c in (3, 4):
        a = a[:, :, [2, 1, 0] + ([3] if c == 4 else [])]
    raw = a.reshape(h, w * c).astype(np.int32)
    out = np.empty((h, 1 + w * c), dtype=np.uint8)
    prev = np.zeros(w * c, dtype=np.int32)
    allowed = [0, 1, 2, 3, 4]
    if h == 1:
        allowed = [k for k in allowed if k not in (2, 3, 4)]
    if w == 1:
        allowed = [k for k in allowed if k not in (1, 3, 4)]
    for y in range(h):
        x = raw[y]
        left = np.concatenate([np.zeros(c, np.int32), x[:-c]]) if w * c > c else np.zeros(w * c, np.int32)
        ul = np.concatenate([np.zeros(c, np.int32), prev[:-c]]) if w * c > c else np.zeros(w * c, np.int32)
        p = left + prev - ul
        pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - ul)
        pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
        cands = [x, x - left, x - prev, x - ((left + prev) >> 1), x - pred]
        best, mins = None, None
        for k in allowed:
            v = cands[k] & 255
            s = int(np.where(v < 128, v, 256 - v).sum())
            if mins is None or s < mins:
                best, mins = k, s
        out[y, 0] = best
        out[y, 1:] = cands[best] & 255
        prev = x
    return out.tobytes()


def zlib_stream(filtered, level=9):
    """zlib at Z_RLE over the whole filtered stream, with libpng's CMF/FLG rewrite when it holds at most 16 KB."""
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    z = bytearray(co.compress(filtered) + co.flush())
    n = len(filtered)
    if n <= 16384:
        cinfo, half = 7, 1 << 14
        if n <= half:
            while True:
                half >>= 1
                cinfo -= 1
                if not (cinfo > 0 and n <= half):
                    break
            cmf = (z[0] & 0x0F) | (cinfo << 4)
            tmp = z[1] & 0xE0
            tmp += 0x1F - ((cmf << 8) + tmp) % 0x1F
            z[0], z[1] = cmf, tmp
    return bytes(z)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode(frame, level=9):
    """The file libpng 1.6.37 + zlib 1.2.11 write at OpenCV 2.4.9's settings (levels 1..9 give the same file)."""
    a = frame if frame.ndim == 3 else frame[:, :, None]
    h, w, c = a.shape
    z = zlib_stream(filter_rows(a), level)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[c], 0, 0, 0)
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr)
    for k in range(0, len(z), 8192):
        out += _chunk(b"IDAT", z[k:k + 8192])
    return out + _chunk(b"IEND", b"")


def make_frame(kind, h, w, c, seed=0):
    """The fixtures' frames, rebuilt from their parameters."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "flat":
        return np.full((h, w, c), 37 + seed % 100, np.uint8)
    if kind.startswith("stripes"):
        run = int(kind[7:])
        x = (np.arange(w * c * h) // run) % 2 * 200 + 20
        return x.reshape(h, w, c).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    planes = [((xx * (3 + k) + yy * (5 - k)) // 4 + 40 * k + (seed % 17)) % 256 for k in range(c)]
    return np.stack(planes, axis=2).astype(np.uint8)                 # "smooth"


# ---------------------------------------------------------------- the system's libpng through ctypes
_WRITE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t)
_FLUSH_FN = C.CFUNCTYPE(None, C.c_void_p)


def load_libpng():
    for name in ("libpng16.so.16", ctypes.util.find_library("png16")):
        if not name:
            continue
        try:
            return C.CDLL(name)
        except OSError:
            pass
    return None


def libpng_versions(lib):
    lib.png_get_libpng_ver.restype = C.c_char_p
    lib.png_get_libpng_ver.argtypes = [C.c_void_p]
    z = C.CDLL(ctypes.util.find_library("z") or "libz.so.1")
    z.zlibVersion.restype = C.c_char_p
    return lib.png_get_libpng_ver(None).decode(), z.zlibVersion().decode()


def libpng_encode(lib, frame, level=9):
    """What OpenCV 2.4.9's PngEncoder::write asks libpng for: png_set_compression_level(level), strategy Z_RLE, no
    png_set_filter, png_set_bgr for 3 / 4 channels, 8-bit, no interlace, IHDR + IDAT + IEND."""
    a = np.ascontiguousarray(frame if frame.ndim == 3 else frame[:, :, None])
    h, w, c = a.shape
    ver = libpng_versions(lib)[0].encode()
    P = C.c_void_p
    lib.png_create_write_struct.restype = P
    lib.png_create_write_struct.argtypes = [C.c_char_p, P, P, P]
    lib.png_create_info_struct.restype = P
    lib.png_create_info_struct.argtypes = [P]
    lib.png_set_write_fn.argtypes = [P, P, _WRITE_FN, _FLUSH_FN]
    lib.png_set_IHDR.argtypes = [P, P, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.png_set_compression_level.argtypes = [P, C.c_int]
    lib.png_set_compression_strategy.argtypes = [P, C.c_int]
    lib.png_set_bgr.argtypes = [P]
    lib.png_write_info.argtypes = [P, P]
    lib.png_write_row.argtypes = [P, P]
    lib.png_write_end.argtypes = [P, P]
    lib.png_destroy_write_struct.argtypes = [C.POINTER(P), C.POINTER(P)]
    out = bytearray()

    def write(_png, data, n):
        out.extend(C.string_at(data, n))

    wfn, ffn = _WRITE_FN(write), _FLUSH_FN(lambda _png: None)
    png = P(lib.png_create_write_struct(ver, None, None, None))
    info = P(lib.png_create_info_struct(png))
    lib.png_set_write_fn(png, None, wfn, ffn)
    lib.png_set_IHDR(png, info, w, h, 8, {1: 0, 3: 2, 4: 6}[c], 0, 0, 0)
    lib.png_set_compression_level(png, int(level))
    lib.png_set_compression_strategy(png, 3)                   # Z_RLE
    if c > 1:
        lib.png_set_bgr(png)
    lib.png_write_info(png, info)
    for y in range(h):
        lib.png_write_row(png, a[y].ctypes.data)
    lib.png_write_end(png, info)
    lib.png_destroy_write_struct(C.byref(png), C.byref(info))
    return bytes(out)
