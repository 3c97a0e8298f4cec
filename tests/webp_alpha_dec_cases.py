"""Writes tests/golden/webp_alpha_dec: the fixtures of the lossy-WebP-with-alpha decoder (VP8X + ALPH + `VP8 `).  Run it as a
script; Pillow's libwebp judges every file: expected.npz holds its convert("RGBA") frames, verdicts.json its verdicts for
the files whose ALPH payload was cut (webp_alpha_dec_fixtures.py loads both).

p_*  Pillow-written: quality 75, methods 0 / 4 / 6, alpha_quality 100 and 50, over a flat, a ramp, a vertical ramp, an 8x8
     checkerboard and a noise plane.  They reach the raw plane, the unfiltered and the horizontally filtered VP8L plane and
     pre-processing 1 (header bytes 00, 01, 05, 11) -- never the vertical or the gradient filter.
h_*  hand-assembled around a Pillow `VP8 ` chunk of the right size: ALPH chunks made here from include/impgpu.h's rule, all
     four filters x both methods, at the seams of a 64-lane scan and a 64-row band; the format's longest row and column;
     gradient residuals that clip at 0 and at 255 on one row; container details; VP8L streams through the lossless
     decoder's corners (2 / 4 / 16 / more levels, backward references, a colour cache); and the project's own answer,
     impgpu_webp_lossy_encode_host of a 53x37 B,G,R,A frame with a noise alpha (the one file here the library writes).
r_*  layouts the route refuses, d_* damaged files (Pillow fails each of these)."""
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webp_lz_writer  # noqa: E402
import webp_writer  # noqa: E402
from webp_vp8_dec_cases import chunk, pillow_frames, riff, vp8_payload  # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "webp_alpha_dec")
NONE, HORIZONTAL, VERTICAL, GRADIENT = range(4)
FILTERS = ("none", "horizontal", "vertical", "gradient")
SEAMS = ((1, 1), (2, 2), (1, 129), (129, 1), (2, 63), (63, 65), (64, 64), (65, 63), (65, 129), (129, 3))
# (fixture, bytes cut off the end of the ALPH payload)
CUTS = [("h_noise_raw_gradient_63x65", n) for n in (1, 2, 64, 2000)] + [("h_noise_vp8l_gradient_63x65", n) for n in (1, 2, 3, 5, 9, 40, 400)] + \
       [("h_lz_vp8l_horizontal", n) for n in (1, 4, 30)] + [("p_noise_q100_m4", n) for n in (1, 3, 100)] + [("h_long_alph_raw", n) for n in (1, 3, 4)]


# ---------------------------------------------------------------- the ALPH chunk
def residuals(a, f):
    """the filter of include/impgpu.h, forwards: a (HxW uint8) -> r"""
    a = a.astype(np.int32)
    pred = np.zeros_like(a)
    if f != NONE:
        pred[0, 1:] = a[0, :-1]
        pred[1:, 0] = a[:-1, 0]
        left, top, tl = a[1:, :-1], a[:-1, 1:], a[:-1, :-1]
        pred[1:, 1:] = left if f == HORIZONTAL else top if f == VERTICAL else np.clip(left + top - tl, 0, 255)
    return ((a - pred) & 255).astype(np.uint8)


def find_chunk(blob, name):
    at = 12
    while at + 8 <= len(blob):
        n = int.from_bytes(blob[at + 4:at + 8], "little")
        if blob[at:at + 4] == name:
            return blob[at + 8:at + 8 + n]
        at += 8 + n + (n & 1)
    return None


def green_frame(r):
    """the B,G,R frame whose green is r"""
    f = np.zeros(r.shape + (3,), np.uint8)
    f[:, :, 1] = r
    return f


def vp8l_stream(r, how="pillow"):
    """a VP8L image stream (no five header bytes) whose green channel is r"""
    if how == "pillow":
        from PIL import Image
        bio = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(green_frame(r)[:, :, ::-1])).save(bio, "WEBP", lossless=True, quality=60, method=4)
        blob = bio.getvalue()
    else:
        blob = (webp_lz_writer if how == "lz" else webp_writer).write(green_frame(r))
    return find_chunk(blob, b"VP8L")[5:]


def alph(a, f, method=0, pre=0, how="pillow"):
    r = residuals(a, f)
    return bytes([method | f << 2 | pre << 4]) + (r.tobytes() if method == 0 else vp8l_stream(r, how))


def vp8x(w, h, flags=0x10):
    return chunk(b"VP8X", bytes([flags, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little"))


def alpha_file(vp8, w, h, alph_payload):
    return riff(vp8x(w, h), chunk(b"ALPH", alph_payload), chunk(b"VP8 ", vp8))


def cut_alph(blob, n):
    """the file with n bytes cut off the end of its ALPH payload, sizes rewritten"""
    w = 1 + int.from_bytes(blob[24:27], "little")
    h = 1 + int.from_bytes(blob[27:30], "little")
    p = find_chunk(blob, b"ALPH")
    return alpha_file(find_chunk(blob, b"VP8 "), w, h, p[:len(p) - n])


# ---------------------------------------------------------------- seeded content
def plane(kind, w, h, seed=0):
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "flat":
        a = np.full((h, w), 200)
    elif kind == "ramp":
        a = xx * 255 // max(1, w - 1)
    elif kind == "vramp":
        a = yy * 255 // max(1, h - 1)
    elif kind == "checker":
        a = ((xx // 8 + yy // 8) & 1) * 255
    elif kind == "noise":
        a = rng.integers(0, 256, (h, w))
    elif kind == "saturate":                     # mostly 0 / 255 a pixel apart: left + top - topleft leaves 0..255 both ways
        a = np.where(rng.random((h, w)) < 0.8, rng.integers(0, 2, (h, w)) * 255, rng.integers(0, 256, (h, w)))
    elif kind == "edges":                        # row 0 and column 0 noise, the rest flat: the first row's and column's own rules
        a = np.full((h, w), 77)
        a[0, :] = rng.integers(0, 256, w)
        a[:, 0] = rng.integers(0, 256, h)
    elif kind == "mask":                         # a soft-edged cut-out
        d = np.hypot((xx - w / 2) / max(1.0, w / 2.5), (yy - h / 2) / max(1.0, h / 2.5))
        a = np.clip((1.15 - d) * 600, 0, 255)
    elif kind.startswith("levels"):              # that many alpha levels, in blobs
        k = int(kind[6:])
        a = (((xx // 3) * 5 + (yy // 2) * 3 + rng.integers(0, 2, (h, w))) % k) * 255 // (k - 1)
    else:
        raise ValueError(kind)
    return np.asarray(a).astype(np.uint8)


def colour(w, h, seed=3, kind="photo"):
    return pillow_frames()(kind, w, h, seed)


_vp8 = {}


def vp8_chunk(w, h):
    """a Pillow-written `VP8 ` chunk of that size (screenshot-like: its frame packs well into expected.npz)"""
    from PIL import Image
    if (w, h) not in _vp8:
        bio = io.BytesIO()
        Image.fromarray(colour(w, h, kind="screen")).save(bio, "WEBP", quality=75, method=2)
        _vp8[(w, h)] = vp8_payload(bio.getvalue())
    return _vp8[(w, h)]


def hand(kind, w, h, f, method, how="pillow", pre=0, seed=0):
    return alpha_file(vp8_chunk(w, h), w, h, alph(plane(kind, w, h, seed), f, method, pre, how))


def own_frame():
    """the 53x37 B,G,R,A frame of the project's own answer: smooth colour, noise alpha"""
    yy, xx = np.mgrid[0:37, 0:53]
    frame = np.clip(np.stack([xx * 4, yy * 6, (xx + yy) * 2, xx * 0], 2), 0, 255).astype(np.uint8)
    frame[:, :, 3] = plane("noise", 53, 37, 11)
    return frame


def own_answer():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from ngx_http_imgproc_amd import ops
    rc, blob, n, intact = ops.encode_webp_lossy_host(own_frame(), 75)
    assert rc == 0 and intact and find_chunk(blob, b"ALPH")[0] == 0
    return bytes(blob[:n])


def gradient_saturates(a):
    """does a row of the gradient-filtered plane clip at 0 AND at 255, and does a sum wrap past 255?"""
    a = a.astype(np.int32)
    g = a[1:, :-1] + a[:-1, 1:] - a[:-1, :-1]
    both = ((g < 0).any(axis=1) & (g > 255).any(axis=1)).any()
    r = residuals(a.astype(np.uint8), GRADIENT).astype(np.int32)[1:, 1:]
    return bool(both) and bool((r + np.clip(g, 0, 255) > 255).any())


def files():
    from PIL import Image
    out = {}
    k = 0
    for kind in ("flat", "ramp", "vramp", "checker", "noise"):
        for m in (0, 4, 6):
            for aq in (100, 50):
                w, h = ((53, 37), (64, 48), (17, 33))[k % 3]
                k += 1
                rgba = np.dstack([colour(w, h, k), plane(kind, w, h, k)])
                bio = io.BytesIO()
                Image.fromarray(rgba).save(bio, "WEBP", quality=75, method=m, alpha_quality=aq)
                out["p_%s_q%d_m%d" % (kind, aq, m)] = bio.getvalue()
    for w, h in SEAMS:                           # the seams of a 64-lane scan and a 64-row band: every filter, both methods
        for f in range(4):
            for method in (0, 1):
                out["h_noise_%s_%s_%dx%d" % ("vp8l" if method else "raw", FILTERS[f], w, h)] = hand("noise", w, h, f, method, seed=w * 131 + h)
    for f in range(4):                           # the format's longest row and column
        out["h_long_raw_%s_16383x1" % FILTERS[f]] = hand("noise", 16383, 1, f, 0, seed=f)
        out["h_long_raw_%s_1x16383" % FILTERS[f]] = hand("noise", 1, 16383, f, 0, seed=f + 4)
    a = plane("saturate", 70, 66, 1)
    assert gradient_saturates(a)
    for method in (0, 1):
        out["h_saturate_%s_gradient" % ("vp8l" if method else "raw")] = hand("saturate", 70, 66, GRADIENT, method, seed=1)
        for f in (HORIZONTAL, VERTICAL, GRADIENT):
            out["h_edges_%s_%s" % ("vp8l" if method else "raw", FILTERS[f])] = hand("edges", 67, 66, f, method, seed=2)
    for f in range(4):                           # a soft mask: what such files hold, with the pre-processing bit as Pillow sets it
        out["h_mask_vp8l_%s_pre1" % FILTERS[f]] = hand("mask", 96, 80, f, 1, pre=1)
    # container details
    out["h_pad_raw_63x65"] = hand("ramp", 63, 65, HORIZONTAL, 0)                           # w * h + 1 is even: no pad ...
    out["h_pad_raw_64x65"] = hand("ramp", 64, 65, HORIZONTAL, 0)                           # ... odd: the pad byte is there
    assert len(find_chunk(out["h_pad_raw_64x65"], b"ALPH")) & 1
    out["h_long_alph_raw"] = alpha_file(vp8_chunk(64, 64), 64, 64, alph(plane("noise", 64, 64, 9), VERTICAL) + b"\x01\x02\x03")
    out["h_flag_no_alph"] = riff(vp8x(64, 64), chunk(b"VP8 ", vp8_chunk(64, 64)))
    out["h_chunks_around"] = riff(vp8x(64, 64, 0x10 | 0x20 | 0x08 | 0x04), chunk(b"ICCP", b"icc"), chunk(b"ZZZZ", b"?"), chunk(b"ALPH", alph(plane("mask", 64, 64), GRADIENT)),
                                  chunk(b"VP8 ", vp8_chunk(64, 64)), chunk(b"EXIF", b"exif!"), chunk(b"XMP ", b"<x/>"))   # (Pillow's demuxer wants ALPH right in front of `VP8 `)
    # VP8L planes through the lossless decoder's corners
    for levels in (2, 4, 16, 40):
        out["h_levels%d_vp8l_none" % levels] = hand("levels%d" % levels, 70, 50, NONE, 1)
    out["h_writer_vp8l_gradient"] = hand("mask", 65, 70, GRADIENT, 1, how="writer")         # the project's own lossless writer: predictor + subtract-green
    out["h_lz_vp8l_horizontal"] = hand("checker", 80, 70, HORIZONTAL, 1, how="lz")          # ... with backward references
    out["h_dither_vp8l_vertical"] = hand("levels40", 128, 96, VERTICAL, 1, seed=5)          # Pillow on a dithered plane: a colour cache
    out["h_own_answer_53x37"] = own_answer()
    return out


def refused():
    from PIL import Image
    w, h = 48, 48
    v, a = vp8_chunk(w, h), alph(plane("noise", w, h), HORIZONTAL)
    bio = io.BytesIO()
    Image.fromarray(colour(w, h)).save(bio, "WEBP", lossless=True)
    return {
        "r_alph_before_vp8l": riff(vp8x(w, h), chunk(b"ALPH", a), chunk(b"VP8L", find_chunk(bio.getvalue(), b"VP8L"))),
        "r_alph_behind_image": riff(vp8x(w, h), chunk(b"VP8 ", v), chunk(b"ALPH", a)),
        "r_alph_twice": riff(vp8x(w, h), chunk(b"ALPH", a), chunk(b"ALPH", a), chunk(b"VP8 ", v)),
        "r_alph_no_vp8x": riff(chunk(b"ALPH", a), chunk(b"VP8 ", v)),
        "r_alph_flag_clear": riff(vp8x(w, h, 0), chunk(b"ALPH", a), chunk(b"VP8 ", v)),
        "r_canvas_differs": riff(vp8x(w + 1, h), chunk(b"ALPH", a), chunk(b"VP8 ", v)),
        "r_anim": riff(vp8x(w, h, 0x12), chunk(b"ANIM", bytes(6)), chunk(b"ALPH", a), chunk(b"VP8 ", v)),
        "r_anmf": riff(vp8x(w, h), chunk(b"ALPH", a), chunk(b"ANMF", bytes(16)), chunk(b"VP8 ", v)),
    }


def damaged():
    w, h = 48, 48
    v = vp8_chunk(w, h)
    raw, lossless = alph(plane("noise", w, h), GRADIENT), alph(plane("noise", w, h), GRADIENT, 1)
    twice = bytes([lossless[0], lossless[1] | 0x1f]) + lossless[2:]                         # transform bits: the predictor twice
    bad_vp8 = v[:3] + b"\x9d\x01\x2b" + v[6:]
    return {
        "d_alph_empty": alpha_file(v, w, h, b""),
        "d_alph_header_only": alpha_file(v, w, h, raw[:1]),
        "d_method2": alpha_file(v, w, h, bytes([raw[0] | 2]) + raw[1:]),
        "d_method3": alpha_file(v, w, h, bytes([raw[0] | 3]) + raw[1:]),
        "d_pre2": alpha_file(v, w, h, bytes([raw[0] | 0x20]) + raw[1:]),
        "d_pre3": alpha_file(v, w, h, bytes([raw[0] | 0x30]) + raw[1:]),
        "d_reserved40": alpha_file(v, w, h, bytes([raw[0] | 0x40]) + raw[1:]),
        "d_reserved80": alpha_file(v, w, h, bytes([lossless[0] | 0x80]) + lossless[1:]),
        "d_raw_one_short": alpha_file(v, w, h, raw[:-1]),
        "d_vp8l_transform_twice": alpha_file(v, w, h, twice),
        "d_vp8l_half": alpha_file(v, w, h, lossless[:len(lossless) // 2]),
        "d_vp8_badstart": alpha_file(bad_vp8, w, h, raw),
    }


def pillow_rgba(blob):
    """Pillow's frame, or None where it fails the file"""
    from PIL import Image
    try:
        return np.asarray(Image.open(io.BytesIO(blob)).convert("RGBA")).copy()
    except (OSError, ValueError, SyntaxError):
        return None


def main():
    os.makedirs(HERE, exist_ok=True)
    for f in os.listdir(HERE):
        os.remove(os.path.join(HERE, f))
    good = files()
    expected = {}
    for name, blob in sorted(good.items()):
        expected[name] = pillow_rgba(blob)
        assert expected[name] is not None, name
        with open(os.path.join(HERE, name + ".webp"), "wb") as f:
            f.write(blob)
    np.savez_compressed(os.path.join(HERE, "expected.npz"), **expected)
    for name, blob in list(refused().items()) + list(damaged().items()):
        with open(os.path.join(HERE, name + ".webp"), "wb") as f:
            f.write(blob)
        assert name[0] != "d" or pillow_rgba(blob) is None, "Pillow reads " + name
    verdicts = []
    for name, n in CUTS:
        got = pillow_rgba(cut_alph(good[name], n))
        verdicts.append([name, n, got is not None, got is not None and bool(np.array_equal(got, expected[name]))])
    with open(os.path.join(HERE, "verdicts.json"), "w") as f:
        json.dump(verdicts, f, indent=0)
    sizes = [os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE)]
    print(len(good), "fixtures,", len(sizes), "files,", sum(sizes), "bytes, largest", max(sizes))
    print(sorted({"%02x" % find_chunk(b, b"ALPH")[0] for n, b in good.items() if n[0] == "p" and find_chunk(b, b"ALPH")}))
    for v in verdicts:
        print(v)


if __name__ == "__main__":
    main()
