"""Writes the fixtures of the lossless WebP decoder's tests into this directory: small .webp files and, in expected.npz, the
B,G,R,A frame Pillow's libwebp DECODER gives for each (alpha 255 where the file's alpha_is_used bit is clear: Pillow opens
such a file as RGB).  Two kinds of file:
  * Pillow's libwebp ENCODER (lossless=True, methods 0 / 3 / 6) on seeded numpy frames: p_<name>_m<method>.webp;
  * the hand-written streams of tests/webp_dec_cases.py: h_<name>.webp from cases() (the format) and h_b_<family><what>.webp
    from boundary_cases() (the implementation's seams);
and three files the decoder must refuse (lossy.webp, anim.webp, not_webp.png), which have no expectation.
expected.npz holds a Pillow-encoded frame once for its three methods (key p_<name>) and every hand-written file (h_<name>).
Made with Pillow 12.2.0 / libwebp 1.6.0:   python tests/golden/webp_dec/make_webp_dec_golden.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import webp_dec_cases  # noqa: E402


def photo(h, w, rng):
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 3 + y * 2) % 256, (x * 2 + y * 5) % 256, (x + y * 3) % 256], -1)
    return np.clip(base + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)


def pillow_frames():
    rng = np.random.default_rng(20240607)
    out = []
    for h, w in ((1, 1), (7, 1), (1, 7), (13, 17), (37, 53)):
        out.append(("photo_%dx%d" % (w, h), photo(h, w, rng), {}))
    base = photo(37, 53, rng)
    out.append(("rgba_53x37", np.dstack([base, rng.integers(0, 256, (37, 53, 1), dtype=np.uint8)]), {"exact": True}))
    for colours in (2, 4, 5, 16, 17, 200, 256):
        pal = rng.integers(0, 256, (colours, 3), dtype=np.uint8)
        for h, w in ((40, 64), (37, 61)):
            out.append(("pal%d_%dx%d" % (colours, w, h), pal[rng.integers(0, colours, (h, w))], {}))
    out.append(("tiling_318x222", np.tile(base // 16 * 16, (6, 6, 1)), {}))                 # coarser levels: the files stay small
    flat = np.full((300, 300, 3), 200, np.uint8)
    flat[50:120, 80:200] = (10, 20, 30)
    out.append(("flat_300x300", flat, {}))
    out.append(("noise_160x120", np.repeat(rng.integers(0, 256, (120, 160, 1), dtype=np.uint8), 3, axis=2), {}))      # gray noise: under 20 KB
    return out


def expect(blob):
    im = Image.open(io.BytesIO(blob))
    im.load()
    assert im.mode in ("RGB", "RGBA"), im.mode
    return np.ascontiguousarray(np.asarray(im.convert("RGBA"))[..., [2, 1, 0, 3]])


def main():
    files = []
    for name, frame, kw in pillow_frames():
        for method in (0, 3, 6):
            bio = io.BytesIO()
            Image.fromarray(frame).save(bio, "WEBP", lossless=True, method=method, **kw)
            files.append(("p_%s_m%d" % (name, method), bio.getvalue()))
    files += [("h_" + name, blob) for name, blob in webp_dec_cases.cases() + webp_dec_cases.boundary_cases()]
    for f in os.listdir(HERE):
        if f.endswith(".webp") or f.endswith(".png") or f.endswith(".npz"):
            os.remove(os.path.join(HERE, f))
    frames = {}                                   # a Pillow-encoded frame's three methods share one expectation (asserted)
    for name, blob in files:
        with open(os.path.join(HERE, name + ".webp"), "wb") as f:
            f.write(blob)
        key = name[:-3] if name.startswith("p_") else name
        frame = expect(blob)
        assert key not in frames or (frames[key].shape == frame.shape and (frames[key] == frame).all()), name
        frames[key] = frame
    np.savez_compressed(os.path.join(HERE, "expected.npz"), **frames)
    rng = np.random.default_rng(3)
    im = Image.fromarray(photo(24, 32, rng))
    im.save(os.path.join(HERE, "lossy.webp"), "WEBP", quality=80)
    im.save(os.path.join(HERE, "anim.webp"), "WEBP", save_all=True, append_images=[Image.fromarray(photo(24, 32, rng))], lossless=True, duration=50)
    im.save(os.path.join(HERE, "not_webp.png"), "PNG")
    total = sum(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE))
    print(len(files), "files,", total, "bytes in the directory, largest", max(len(b) for _, b in files))


if __name__ == "__main__":
    main()
