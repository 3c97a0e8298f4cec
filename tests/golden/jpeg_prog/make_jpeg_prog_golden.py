"""Writes the progressive JPEG fixtures: files as Pillow (libjpeg-turbo) writes them with progressive=True, each with its
progressive=False twin, Pillow's decoded pixels of the progressive file (B,G,R / gray) in expected_pixels.npz and a
manifest.  Run from the repository root:  python tests/golden/jpeg_prog/make_jpeg_prog_golden.py
"""
import io
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from conftest import noise_image, smooth_image  # noqa: E402

# name, kind, (h, w), gray?, save options
CASES = [
    ("gray_q90_57x43", "smooth", (43, 57), True, dict(quality=90)),
    ("gray_q25_dri3_200x120", "smooth", (120, 200), True, dict(quality=25, restart_marker_blocks=3)),
    ("gray_q90_1x1", "smooth", (1, 1), True, dict(quality=90)),
    ("c444_q90_48x40", "smooth", (40, 48), False, dict(quality=90, subsampling="4:4:4")),
    ("c444_q95_drirow_41x29", "smooth", (29, 41), False, dict(quality=95, subsampling="4:4:4", restart_marker_rows=1)),
    ("c422_q85_49x37", "smooth", (37, 49), False, dict(quality=85, subsampling="4:2:2")),
    ("c422_q90_4x9", "noise", (9, 4), False, dict(quality=90, subsampling="4:2:2")),
    ("c420_q90_1x1", "smooth", (1, 1), False, dict(quality=90, subsampling="4:2:0")),
    ("c420_q90_3x2", "noise", (2, 3), False, dict(quality=90, subsampling="4:2:0")),
    ("c420_q90_67x45", "smooth", (45, 67), False, dict(quality=90, subsampling="4:2:0")),
    ("c420_q90_dri4_95x51", "smooth", (51, 95), False, dict(quality=90, subsampling="4:2:0", restart_marker_blocks=4)),
    ("c420_q100_noise_33x31", "noise", (31, 33), False, dict(quality=100, subsampling="4:2:0")),
    ("c444_q100_noise_64x48", "noise", (48, 64), False, dict(quality=100, subsampling="4:4:4")),
    ("c420_q10_smooth_320x240", "smooth", (240, 320), False, dict(quality=10, subsampling="4:2:0")),
    ("c420_q92_opt_120x90", "smooth", (90, 120), False, dict(quality=92, subsampling="4:2:0", optimize=True)),
    ("c420_q50_400x300", "photo", (300, 400), False, dict(quality=50, subsampling="4:2:0")),
    ("gray_q75_640x480", "photo", (480, 640), True, dict(quality=75)),
]


def frame(kind, h, w, gray):
    if kind == "noise":
        a = noise_image(h, w, 3, 5)
    elif kind == "smooth":
        a = smooth_image(h, w, 3, 1)
    else:       # picture-like: smooth structure with noise of modest amplitude on top
        a = np.clip(smooth_image(h, w, 3, 2).astype(np.int32) + (noise_image(h, w, 3, 9).astype(np.int32) - 128) // 24, 0, 255).astype(np.uint8)
    return a[:, :, 0] if gray else a


def main():
    manifest, pixels = [], {}
    for name, kind, (h, w), gray, kw in CASES:
        a = frame(kind, h, w, gray)
        for prog in (True, False):
            b = io.BytesIO()
            Image.fromarray(a).save(b, "JPEG", progressive=prog, **kw)
            with open(os.path.join(HERE, name + (".prog.jpg" if prog else ".seq.jpg")), "wb") as f:
                f.write(b.getvalue())
            if prog:
                dec = np.asarray(Image.open(io.BytesIO(b.getvalue())))
                pixels[name] = dec[:, :, None] if gray else dec[:, :, ::-1].copy()
        manifest.append(dict(name=name, shape=[h, w, 1 if gray else 3]))
    np.savez_compressed(os.path.join(HERE, "expected_pixels.npz"), **pixels)
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(dict(pillow=Image.__version__ if hasattr(Image, "__version__") else "", cases=manifest), f, indent=1)


if __name__ == "__main__":
    main()
