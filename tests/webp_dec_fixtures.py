"""The fixtures of tests/golden/webp_dec for the lossless WebP decoder's tests: every file with the B,G,R,A frame Pillow's
decoder gives for it, the three files the decoder refuses, and the DAMAGED files -- a fixture with one byte changed by a
rule that tests/c/webp_dec_test.cpp repeats, so the sanitizer driver has run each of them."""
import functools
import os

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "webp_dec")
IMP_OK, IMP_ERROR_UNSUPPORTED, IMP_ERROR_MALLOC_FAILED, IMP_ERROR_DECODE_FAILED = 0, 1, 2, 3
# (fixture, offset as a fraction of the file in 1/256, xor): the host model says IMP_ERROR_DECODE_FAILED for each; the first
# is refused by a prefix code of the main image (the table launch's verdict), the second inside the pixel stream
DAMAGED = (("p_photo_53x37_m3", 8, 0x5A), ("p_photo_53x37_m0", 124, 0x5A))


def read(name):
    with open(os.path.join(HERE, name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def load():
    """[(name, file bytes, expected HxWx4 array)] in name order"""
    exp = np.load(os.path.join(HERE, "expected.npz"))
    out = []
    for f in sorted(os.listdir(HERE)):
        if not f.endswith(".webp") or f[:2] not in ("p_", "h_"):
            continue
        name = f[:-5]
        out.append((name, read(f), exp[name[:-3] if name.startswith("p_") else name]))
    return out


def damaged():
    """[(name, file bytes)]"""
    out = []
    for name, frac, xor in DAMAGED:
        blob = bytearray(read(name + ".webp"))
        blob[len(blob) * frac // 256] ^= xor
        out.append(("%s@%d^%02x" % (name, frac, xor), bytes(blob)))
    return out
