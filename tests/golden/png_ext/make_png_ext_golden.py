"""Writes the palette / low-bit gray / Adam7 fixtures of tests/golden/png_ext (python tests/golden/png_ext/make_png_ext_golden.py)
with tests/png_ext_writer.py, and expected_pixels.npz: Pillow's decode of each file in OpenCV's channel order, except where a
palette index lies past the PLTE's entries (libpng reads zeros there, Pillow does not): those take png_ext_writer.model.
manifest.json: per file, its kind, what the _ex calls answer (0 = decoded) and where its pixels came from."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import png_ext_writer as W  # noqa: E402


def main():
    rng = np.random.default_rng(0x9E57)
    files, want, manifest = {}, {}, {}

    def add(name, blob, pixels, code=0, source="pillow", note=""):
        files[name] = blob
        if pixels is not None:
            want[name] = pixels
        manifest[name] = {"code": code, "pixels": source if pixels is not None else None, "note": note}

    # decoded: every palette depth, low gray, Adam7 of each kind; a filter per row drawn at random
    for colour, depth, il, w, h in [(3, 1, 0, 37, 21), (3, 2, 0, 29, 17), (3, 4, 0, 33, 19), (3, 8, 0, 61, 40),
                                    (3, 8, 1, 45, 38), (3, 1, 1, 23, 27), (3, 4, 1, 19, 9),
                                    (0, 1, 0, 41, 13), (0, 2, 0, 30, 11), (0, 4, 0, 27, 15), (0, 2, 1, 35, 22),
                                    (0, 8, 1, 53, 31), (2, 8, 1, 47, 35), (6, 8, 1, 39, 29), (2, 8, 1, 1, 1), (6, 8, 1, 5, 3)]:
        blob, model = W.random_file(rng, colour, depth, il, w, h)
        pil = W.pillow(blob)
        assert np.array_equal(pil, model), (colour, depth, il)
        kind = {3: "palette", 0: "gray", 2: "rgb", 6: "rgba"}[colour]
        add("%s%d%s_%dx%d.png" % (kind, depth, "_adam7" if il else "", w, h), blob, pil)
    # palette indices past the PLTE: the model (zeros), not Pillow
    blob, model = W.random_file(rng, 3, 4, 0, 24, 16, n_pal=5, out_of_range=True)
    add("palette4_past_plte_24x16.png", blob, model, source="model", note="indices >= 5 of a 5-entry PLTE read (0,0,0)")
    # refused: tRNS on a palette, PLTE rules, a short Adam7 stream
    s = rng.integers(0, 4, size=(8, 8, 1), dtype=np.uint8)
    pal = rng.integers(0, 256, size=(4, 3), dtype=np.uint8)
    add("r_palette_trns.png", W.write(s, 3, 2, palette=pal, trns=b"\x00\x80"), None, code=1, note="tRNS on a palette: unsupported")
    add("r_palette_big_plte.png", W.write(s, 3, 2, palette=rng.integers(0, 256, size=(5, 3), dtype=np.uint8)), None, code=1,
        note="5 PLTE entries at depth 2: unsupported")
    add("d_palette_no_plte.png", W.write(s, 3, 2), None, code=3, note="no PLTE")
    add("d_palette_plte_len.png", W.write(s, 3, 2, palette=b"\x01\x02\x03\x04"), None, code=3, note="PLTE of 4 bytes")
    g = rng.integers(0, 256, size=(9, 10, 3), dtype=np.uint8)
    raw = W.scanlines(g, 2, 8, 1, 0)
    add("d_adam7_short.png", W.write(g, 2, 8, 1, raw=raw[:-5]), None, code=3, note="Adam7 stream 5 bytes short")
    bad = bytearray(raw)
    bad[W.passes(10, 9, 1)[0][6] * (1 + 3 * 2) + 0] = 7          # the filter byte of pass 2's first row
    add("d_adam7_filter7.png", W.write(g, 2, 8, 1, raw=bytes(bad)), None, code=3, note="filter type 7 in pass 2")

    for name, blob in files.items():
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(blob)
    np.savez_compressed(os.path.join(HERE, "expected_pixels.npz"), **want)
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
