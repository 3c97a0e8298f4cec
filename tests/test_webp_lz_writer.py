"""tests/webp_lz_writer.py IS the definition of the lossless WebP file with backward references (include/impgpu.h, "WEBP
ANSWERS", IMPGPU_WEBP_ENC_BACKREFS); this file checks the definition against an independent implementation: every file
must decode, with Pillow's libwebp, to exactly the frame -- which also proves the 24 distance-map entries.  The CASES are
shared with the host twin's and the device's tests.

Shapes: 1x1, 1x7, 7x1; widths 2 and 3 (candidates with a distance below 1, candidates sharing a distance); 32x32 (one item
exactly); 41x25 (1025 positions: the second item is one position); 64x33 flat (a run cut at two item ends); 300x9 (4 w
> 1024: every vertical candidate reads an earlier item); 529x497 (past 256 workgroups).  Contents: under forced mode 0 the
residuals are the pixels, so stripes, repeating rows, diagonals and short runs plant the matches; with the chooser flat
colour, two colours, a Bayer-dithered frame, a synthetic screenshot, gray, BGRA with holes, and noise (no match: the
flag-less file).  The size conditions are asserted on 320x240 BGR frames."""
import numpy as np
import pytest

import webp_lz_writer as LZ
import webp_writer as W
from test_webp_writer import check_structure, content, decodes_to

SMALL = [(1, 1), (1, 7), (7, 1), (2, 9), (3, 9), (32, 32), (41, 25), (300, 9)]
PLANTED = ["stripes1", "stripes2", "stripes3", "stripes4", "rows1", "rows2", "rows3", "rows4", "diag_1_1", "diag_-1_1", "diag_-3_2", "diag_2_3", "runs"]
CHOSEN = ["flat_bgr", "flat_black", "two_colours", "dither", "screenshot", "gradient_gray", "bgra_holes", "noise_bgr"]


def _rng(name, w, h):
    return np.random.default_rng(sum(name.encode()) * 1000003 + w * 131 + h + 7)


def planted(name, w, h):
    """a BGR frame whose PIXELS repeat the way the name says (forced mode 0 keeps them as residuals)"""
    rng = _rng(name, w, h)
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if name.startswith("stripes"):
        p = int(name[7:])
        return np.broadcast_to(rng.integers(0, 256, (p, 3), dtype=np.uint8)[np.arange(w) % p][None], (h, w, 3)).copy()
    if name.startswith("rows"):
        p = int(name[4:])
        return noise[np.arange(h) % min(p, h)].copy()
    if name.startswith("diag"):
        xi, yi = (int(v) for v in name.split("_")[1:])
        f = noise.copy()
        for y in range(yi, h):
            lo, hi = max(0, xi), min(w, w + xi)
            if lo < hi:
                f[y, lo:hi] = f[y - yi, lo - xi:hi - xi]
        return f
    assert name == "runs", name
    flat = noise.reshape(-1, 3).copy()                              # pixels repeated 3 and 4 times: matches of 2 and of 3
    reps = np.where(np.arange(flat.shape[0]) % 2 == 0, 3, 4)
    return np.repeat(flat, reps, axis=0)[: w * h].reshape(h, w, 3)


def fixture(name, w, h):
    """the frames of the size conditions (B, G, R)"""
    rng = _rng(name, w, h)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    smooth = np.stack([127 + 90 * np.sin(x / (37.0 + k * 11)) * np.cos(y / (29.0 + k * 7)) + 30 * (x / max(w, 2) - 0.5) for k in range(3)], axis=2)
    if name == "photo":
        return np.clip(smooth + rng.normal(0, 2.5, smooth.shape), 0, 255).astype(np.uint8)
    if name == "dither":                                             # 4x4 Bayer to a 6-level cube
        bayer = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]]) / 16.0 - 0.5
        t = bayer[(np.arange(h) % 4)[:, None], (np.arange(w) % 4)[None, :]][..., None]
        q = np.clip(np.floor(smooth / 255.0 * 5 + 0.5 + t), 0, 5)
        return np.rint(q * 51.0).astype(np.uint8)
    assert name == "screenshot", name
    f = np.empty((h, w, 3), np.uint8)
    f[...] = [240, 240, 236]                                         # the ground
    f[: max(1, h // 12)] = [120, 60, 30]                             # a title bar
    f[:, : max(1, w // 6)] = [60, 56, 52]                            # a side bar
    for k in range(4):                                               # bars of a chart
        x0, top = w // 4 + k * (w // 8), h - 1 - (k + 1) * (h // 8)
        f[max(0, top): h - h // 10, x0: x0 + max(1, w // 12)] = [40 + 50 * k, 160, 220 - 40 * k]
    f[h // 6:: max(2, h // 10), w // 6:] = [200, 200, 200]           # grid lines
    f[h // 6:, w // 6:: max(2, w // 10)] = [200, 200, 200]
    return f


def lz_content(name, w, h):
    if name in ("dither", "screenshot", "photo"):
        return fixture(name, w, h)
    return planted(name, w, h) if name in PLANTED else content(name, w, h)


def zero_modes(w, h):
    tx, ty = W.tiles_of(w, h)
    return np.zeros(tx * ty, np.uint8)


def _cases():
    out = {}
    for (w, h) in SMALL:
        for name in PLANTED:
            out["%s_%dx%d" % (name, w, h)] = (planted(name, w, h), zero_modes(w, h))
        for name in CHOSEN:
            out["%s_%dx%d" % (name, w, h)] = (lz_content(name, w, h), None)
    out["flat_bgr_64x33"] = (content("flat_bgr", 64, 33), None)
    out["flat_black_64x33"] = (content("flat_black", 64, 33), None)
    return out


CASES = _cases()
BIG = {"screenshot_529x497": (fixture("screenshot", 529, 497), None), "dither_529x497": (fixture("dither", 529, 497), None),
       "rows3_529x497": (planted("rows3", 529, 497), zero_modes(529, 497))}
_want = {}


def want(name):
    """the model's flagged file of a case, written once"""
    if name not in _want:
        frame, modes = CASES[name] if name in CASES else BIG[name]
        _want[name] = LZ.write(frame, forced_modes=modes)
    return _want[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_file_decodes_to_its_pixels(name):
    frame, modes = CASES[name]
    blob = want(name)
    check_structure(blob, frame)
    assert decodes_to(blob, frame)
    assert LZ.file_size(frame, forced_modes=modes) == len(blob)


@pytest.mark.parametrize("name", sorted(BIG))
def test_the_large_frames_decode(name):
    assert decodes_to(want(name), BIG[name][0])


def test_prefix_values_round_trip():
    seen = set()
    for v in range(1, LZ.ITEM + 1):
        sym, extra, bits = LZ.prefix_value(v)
        assert 0 <= extra < (1 << bits) and LZ.unprefix_value(sym, extra) == v
        if v >= LZ.MIN_MATCH:
            seen.add(sym)
    assert seen == set(range(2, 20))                                 # lengths 3..1024 use symbols 2..19
    assert {LZ.prefix_value(k)[0] for k in range(1, 25)} == set(range(9))
    assert max(LZ.prefix_value(v)[2] for v in range(1, LZ.ITEM + 1)) == 8 and LZ.prefix_value(24)[2] == 3


def test_position_0_is_a_literal_and_tokens_tile_the_plane():
    for name in ["flat_bgr_64x33", "rows2_41x25", "stripes3_300x9", "runs_32x32", "flat_black_1x1"]:
        frame, modes = CASES[name]
        toks = LZ.tokens(frame, forced_modes=modes)
        assert toks[0] == (0, 1, 0)
        at = 0
        for p, n, k in toks:
            assert p == at and (k == 0 and n == 1 or 1 <= k <= 24 and LZ.MIN_MATCH <= n <= LZ.ITEM)
            assert p // LZ.ITEM == (p + n - 1) // LZ.ITEM           # no token crosses an item's end
            at += n
        assert at == frame.shape[0] * frame.shape[1]


def test_a_flat_run_is_cut_at_the_item_ends():
    """64x33 = 2112 positions of one residual: a literal and 1023 from the left; then an item is ONE reference from its first
    position, where the pixel above is usable and ties with the left one: the lowest k.  Flat colour: (0,0)'s residual differs"""
    assert LZ.tokens(CASES["flat_black_64x33"][0]) == [(0, 1, 0), (1, 1023, 2), (1024, 1024, 1), (2048, 64, 1)]
    assert LZ.tokens(CASES["flat_bgr_64x33"][0]) == [(0, 1, 0), (1, 1, 0), (2, 1022, 2), (1024, 1024, 1), (2048, 64, 1)]


def test_the_second_item_of_41x25_is_one_position():
    frame, modes = CASES["stripes1_41x25"]
    toks = LZ.tokens(frame, forced_modes=modes)
    assert toks[-1][0] == 1024 and toks[-1][1] == 1                  # a match of one position stays a literal


def test_runs_of_two_stay_literal_and_three_become_references():
    frame, modes = CASES["runs_32x32"]
    lengths = [n for _, n, k in LZ.tokens(frame, forced_modes=modes) if k]
    assert lengths and min(lengths) == LZ.MIN_MATCH
    literals = sum(1 for _, n, k in LZ.tokens(frame, forced_modes=modes) if not k)
    assert literals > 32 * 32 // 7                                   # the runs of 3 pixels: all three stay literals


@pytest.mark.parametrize("name,k", [("rows1", 1), ("rows2", 5), ("rows3", 13), ("rows4", 23), ("stripes1", 2), ("stripes2", 6), ("stripes3", 14), ("stripes4", 24),
                                    ("diag_1_1", 3), ("diag_-1_1", 4), ("diag_-3_2", 22), ("diag_2_3", 19)])
def test_the_planted_structure_is_found_by_its_candidate(name, k):
    frame, modes = CASES[name + "_32x32"]
    ks = [kk for _, n, kk in LZ.tokens(frame, forced_modes=modes) if kk]
    assert ks and max(set(ks), key=ks.count) == k


@pytest.mark.parametrize("shape", [(33, 20), (70, 45)])
def test_no_match_is_the_flagless_file(shape):
    for name in ("noise_bgr", "bgra_opaque"):
        frame = content(name, *shape)
        assert all(k == 0 for _, _, k in LZ.tokens(frame))
        assert LZ.write(frame) == W.write(frame)


# ---------------------------------------------------------------- the size conditions: 320x240 BGR, on the model's files
def sized(name):
    frame = content("flat_bgr", 320, 240) if name == "flat" else fixture(name, 320, 240)
    return LZ.file_size(frame), W.file_size(frame)


def test_size_flat_colour():
    lz, plain = sized("flat")
    print("flat: flagged %d, flag-less %d" % (lz, plain))
    assert lz * 50 <= plain


def test_size_screenshot():
    lz, plain = sized("screenshot")
    print("screenshot: flagged %d, flag-less %d" % (lz, plain))
    assert lz * 20 <= plain


def test_size_bayer_dither():
    lz, plain = sized("dither")
    print("dither: flagged %d, flag-less %d" % (lz, plain))
    assert lz <= 0.85 * plain


def test_size_photo_like():
    lz, plain = sized("photo")
    print("photo: flagged %d, flag-less %d" % (lz, plain))
    assert lz <= 1.01 * plain
