"""Regenerate tests/golden/png_enc/{cases.npz, manifest.json}: PNG files written by the system's libpng 1.6 (ctypes, hand-
declared prototypes: no png.h needed) at OpenCV 2.4.9's PngEncoder settings -- compression level q, strategy Z_RLE, no
png_set_filter, png_set_bgr, 8-bit, no interlace.  The frames are rebuilt from their parameters by
tests/png_enc_model.make_frame, so only the files are stored.

    python tests/golden/png_enc/make_png_enc_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import png_enc_model as model  # noqa: E402


def cases():
    out = []
    for c in (1, 3, 4):
        for kind in ("smooth", "noise", "flat"):
            for (h, w) in ((1, 1), (1, 37), (29, 1), (224, 224), (168, 224)):
                out.append((kind, h, w, c, 1))
    for run in (3, 4, 258, 259, 516, 517):
        out.append(("stripes%d" % run, 40, 50, 3, 0))
    # filtered sizes around each CINFO step (h rows of 1 + w bytes, gray)
    for n in (256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385):
        for h in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            if n % h == 0 and n // h >= 2:
                out.append(("smooth", h, n // h - 1, 1, 2))
                out.append(("noise", h, n // h - 1, 1, 2))
                break
    out.append(("noise", 64, 2047, 1, 5))            # 131 072 filtered bytes of noise: a stream of 16 IDAT chunks + a tail
    out.append(("noise", 1, 8180, 1, 3))             # a zlib stream of exactly 8192 bytes: one full IDAT chunk, no empty one after it
    out.append(("smooth", 480, 640, 3, 7))
    out.append(("noise", 120, 160, 4, 7))
    out.append(("smooth", 1080, 1920, 3, 8))
    return out


def main():
    lib = model.load_libpng()
    if lib is None:
        sys.exit("libpng16 is not loadable here")
    png_ver, z_ver = model.libpng_versions(lib)
    files, manifest = {}, {"libpng": png_ver, "zlib": z_ver, "cases": []}
    for k, (kind, h, w, c, seed) in enumerate(cases()):
        frame = model.make_frame(kind, h, w, c, seed)
        blobs = {lv: model.libpng_encode(lib, frame, lv) for lv in (1, 6, 9)}
        if (kind, h, w, c, seed) == ("noise", 1, 8180, 1, 3):
            assert len(model.zlib_stream(model.filter_rows(frame))) == 8192
        assert blobs[1] == blobs[6] == blobs[9], (kind, h, w, c)
        files["f%03d" % k] = np.frombuffer(blobs[9], dtype=np.uint8)
        manifest["cases"].append({"key": "f%03d" % k, "kind": kind, "h": h, "w": w, "c": c, "seed": seed, "bytes": len(blobs[9])})
    np.savez_compressed(os.path.join(HERE, "cases.npz"), **files)
    with open(os.path.join(HERE, "manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1)
    print(len(files), "cases, libpng", png_ver, "zlib", z_ver)


if __name__ == "__main__":
    main()
