"""Hand-written lossless WebP (VP8L) streams for the decoder's tests: what an encoder does not emit at small sizes.  A
file is written from TOKENS -- ("lit", argb), ("copy", length, distance code) and ("cache", argb) -- by a writer that
knows the format from include/impgpu.h and webp_writer / webp_lz_writer (container, prefix codes, the prefix coding of
lengths and distances, _pack) and nothing of the library.  Pillow's libwebp is the judge of every file: the expected
frames of tests/golden/webp_dec come from its decoder, never from this module's idea of the pixels.

    cases()            [(name, file bytes)] in a fixed order: everything is seeded.  The FORMAT: every predictor mode, every
                       distance code, caches, groups, odd transform orders
    boundary_cases()   [(name, file bytes)], names b_<family><...>: files placed at the IMPLEMENTATION's seams -- the
                       512-token and 512-word round edges, the wave's width in a match, the predictor's 256-row bands,
                       codes longer than the 10-bit table, group indices past 255, the largest sides, sub-images with
                       matches and a cache (the families A..G below)
    boundary_facts()   {name: what the writer knows of the file}: "family", "tokens", "maxlen" (the longest code of the
                       main image), "rounds" / "window_rounds" (RoundModel) and what a family adds -- what
                       tests/test_webp_decode_boundaries_host.py holds against the host model's info words
"""
import functools

import numpy as np

import webp_lz_writer as LZ
import webp_writer as W

# VP8L's distance map, codes 1..120, as (xi, yi): the distance is xi + yi * width (below 1: 1).  The specification's list;
# the per-code files below put every entry before Pillow's decoder.
DISTANCE_MAP = (
    (0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3), (-1, 3), (3, 1), (-3, 1),
    (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3), (2, 4), (-2, 4), (4, 2), (-4, 2), (0, 5), (3, 4),
    (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5), (-2, 5), (5, 2), (-5, 2), (4, 4), (-4, 4), (3, 5), (-3, 5), (5, 3), (-5, 3),
    (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1), (2, 6), (-2, 6), (6, 2), (-6, 2), (4, 5), (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6), (6, 3), (-6, 3),
    (0, 7), (7, 0), (1, 7), (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1), (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7),
    (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5), (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6), (-6, 6), (8, 3), (5, 7), (-5, 7),
    (7, 5), (-7, 5), (8, 4), (6, 7), (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7))
assert len(DISTANCE_MAP) == 120 and len(set(DISTANCE_MAP)) == 120


def code_distance(code, width):
    """a distance code -> pixels"""
    if code > 120:
        return code - 120
    xi, yi = DISTANCE_MAP[code - 1]
    return max(1, xi + yi * width)


def cache_hash(argb, bits):
    return ((argb * 0x1E35A7BD) & 0xFFFFFFFF) >> (32 - bits)


class Bits:
    def __init__(self):
        self.vals, self.lens = [], []

    def put(self, v, n):
        if n:
            self.vals.append(int(v))
            self.lens.append(int(n))

    def pairs(self, pairs):
        for v, n in pairs:
            self.put(v, n)

    def payload(self):
        return W._pack(self.vals, self.lens)[0]


def simple_code(symbols, alphabet):
    """the simple form for one or two symbols (< 256) -> (header bits, lengths, codes)"""
    symbols = sorted(symbols)
    lengths, codes = [0] * alphabet, [0] * alphabet
    first8 = int(symbols[0] > 1)
    bits = [(1, 1), (len(symbols) - 1, 1), (first8, 1), (symbols[0], 8 if first8 else 1)]
    if len(symbols) == 2:
        bits.append((symbols[1], 8))
        lengths[symbols[0]] = lengths[symbols[1]] = 1
        codes[symbols[1]] = 1                     # canonical: the lower symbol is 0
    return bits, lengths, codes


def make_code(hist, alphabet, simple=False):
    used = [n for n, v in enumerate(hist) if v]
    if not used:
        return simple_code([0], alphabet)
    if simple and len(used) <= 2 and max(used) < 256:
        return simple_code(used, alphabet)
    return W.prefix_code(list(hist) + [0] * (alphabet - len(hist)), alphabet)


def token_symbols(tok, cache_bits):
    """a token -> [(which code 0..4, symbol, extra value, extra bits)]"""
    if tok[0] == "lit":
        v = tok[1]
        return [(0, (v >> 8) & 255, 0, 0), (1, (v >> 16) & 255, 0, 0), (2, v & 255, 0, 0), (3, v >> 24, 0, 0)]
    if tok[0] == "cache":
        return [(0, 280 + cache_hash(tok[1], cache_bits), 0, 0)]
    ls, lv, ln = LZ.prefix_value(tok[1])
    ds, dv, dn = LZ.prefix_value(tok[2])
    return [(0, 256 + ls, lv, ln), (4, ds, dv, dn)]


def token_step(tok):
    return tok[1] if tok[0] == "copy" else 1


def code_of_lengths(want, alphabet):
    """a code whose lengths are GIVEN ({symbol: length}; must be complete) -> (header bits, lengths, codes), the normal form"""
    lengths = [0] * alphabet
    for sym, n in want.items():
        lengths[sym] = n
    assert sum(1 << (15 - n) for n in lengths if n) == 1 << 15, "not a complete code"
    codes = W.canonical_codes(lengths)
    tokens = W.length_tokens(lengths)
    bfreq = [0] * 19
    for sym, _, _ in tokens:
        bfreq[sym] += 1
    blen = W.build_lengths(bfreq, 7)
    bcode = W.canonical_codes(blen)
    count = 19
    while count > 4 and blen[W.CL_ORDER[count - 1]] == 0:
        count -= 1
    bits = [(0, 1), (count - 4, 4)] + [(blen[W.CL_ORDER[i]], 3) for i in range(count)] + [(0, 1)]
    for sym, xv, xb in tokens:
        bits.append((bcode[sym], blen[sym]))
        if xb:
            bits.append((xv, xb))
    return bits, lengths, codes


def image_stream(out, tokens, width, cache_bits=0, meta=None, simple=False, is_main=True, forced=None, record=None):
    """an entropy-coded image: cache size, [meta prefix image], the groups' codes, the tokens.  meta: (bits, HxW groups[,
    {"tokens", "cache_bits"} for the meta image itself]).  forced: {code 0..4: {symbol: length}} instead of the lengths the
    histogram gives (one group).  record: a dict that receives "first_bit" (of the first token), "reads" (per token the
    bit counts the decoder reads one after the other) and "maxlen"."""
    out.put(1 if cache_bits else 0, 1)
    if cache_bits:
        out.put(cache_bits, 4)
    ngroups = 1
    if is_main:
        out.put(1 if meta else 0, 1)
        if meta:
            mbits, groups = meta[0], meta[1]
            sub = dict(meta[2]) if len(meta) > 2 else {}
            out.put(mbits - 2, 3)
            image_stream(out, sub.pop("tokens", None) or [("lit", 0xFF000000 | int(g) << 8) for g in groups.reshape(-1)], groups.shape[1], is_main=False, **sub)
            ngroups = int(groups.max()) + 1
    alphabets = (280 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)
    group_of, pos = [], 0
    for tok in tokens:
        group_of.append(int(meta[1][(pos // width) >> meta[0], (pos % width) >> meta[0]]) if meta and is_main else 0)
        pos += token_step(tok)
    hists = [[np.zeros(a, np.int64) for a in alphabets] for _ in range(ngroups)]
    for tok, g in zip(tokens, group_of):
        for k, s, _, _ in token_symbols(tok, cache_bits):
            hists[g][k][s] += 1
    codes = []
    for g in range(ngroups):
        codes.append([])
        for k, a in enumerate(alphabets):
            if forced and k in forced:
                assert ngroups == 1 and all(forced[k].get(s) for s in np.nonzero(hists[g][k])[0]), k
                bits, lengths, cds = code_of_lengths(forced[k], a)
            else:
                bits, lengths, cds = make_code(hists[g][k], a, simple)
            out.pairs(bits)
            codes[g].append((lengths, cds))
    if record is not None:
        record["first_bit"] = sum(out.lens)
        record["maxlen"] = max(max(lengths) for group in codes for lengths, _ in group)
        record["reads"] = reads = []
    for tok, g in zip(tokens, group_of):
        syms = token_symbols(tok, cache_bits)
        for k, s, xv, xn in syms:
            out.put(codes[g][k][1][s], codes[g][k][0][s])
            out.put(xv, xn)
        if record is not None:
            reads.append([n for k, s, _, xn in syms for n in ([codes[g][k][0][s]] + ([xn] if tok[0] == "copy" and s - (256 if k == 0 else 0) >= 4 else []))])


def vp8l(width, height, tokens, transforms=(), alpha=0, **kw):
    """the file.  transforms: ("green",), ("predictor", bits, modes HxW), ("color", bits, elements HxW uint32),
    ("index", [argb ...]) in the order they are written; a predictor or colour entry may end with {"tokens", "cache_bits"}:
    how its sub-image is coded instead of literals alone"""
    out = Bits()
    out.pairs([(0x2F, 8), (width - 1, 14), (height - 1, 14), (alpha, 1), (0, 3)])
    for t in transforms:
        out.put(1, 1)
        if t[0] == "green":
            out.put(2, 2)
        elif t[0] in ("predictor", "color"):
            out.put(0 if t[0] == "predictor" else 1, 2)
            out.put(t[1] - 2, 3)
            data = np.asarray(t[2])
            sub = dict(t[3]) if len(t) > 3 else {}
            image_stream(out, sub.pop("tokens", None) or [("lit", v) for v in sub_values(t[0], data)], data.shape[1], is_main=False, **sub)
        else:
            pal = [int(v) for v in t[1]]
            out.put(3, 2)
            out.put(len(pal) - 1, 8)
            deltas = [pal[0]] + [sum((((pal[i] >> s) - (pal[i - 1] >> s)) & 255) << s for s in (0, 8, 16, 24)) for i in range(1, len(pal))]
            image_stream(out, [("lit", v) for v in deltas], len(pal), is_main=False)
    out.put(0, 1)
    image_stream(out, tokens, width, **kw)
    return W.container(out.payload())


def sub_values(kind, data):
    """a transform's sub-image as ARGB values: a mode in green, a colour-transform element in its low 24 bits"""
    data = np.asarray(data)
    return [0xFF000000 | int(v) << 8 for v in data.reshape(-1)] if kind == "predictor" else [0xFF000000 | int(v) for v in data.reshape(-1)]


def distinct_pixels(n, seed):
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.choice(1 << 24, n, replace=False) + 0xFF000000]


def reference_file(code, width, height, col, row, seed=5):
    """distinct literal pixels and ONE length-1 reference with distance code `code` at (col, row)"""
    px = [0xFF000000 | (i >> 8) << 16 | (i & 255) << 8 | ((i * 5 + seed) & 255) for i in range(width * height)]      # distinct, and small to store
    at = row * width + col
    tokens = [("lit", v) for v in px[:at]] + [("copy", 1, code)] + [("lit", v) for v in px[at + 1:]]
    return vp8l(width, height, tokens)


def cache_file(cache_bits, seed):
    """literals, a copy of earlier pixels, then cache hits on the COPIED colours, a literal, and hits again"""
    width, height = 24, 8
    rng = np.random.default_rng(seed)
    colours = distinct_pixels(40, seed)
    tokens, px, cache = [], [], {}

    def lit(v):
        tokens.append(("lit", v)); px.append(v); cache[cache_hash(v, cache_bits)] = v

    def copy(length, dist):
        tokens.append(("copy", length, dist + 120))
        for _ in range(length):
            v = px[len(px) - dist]
            px.append(v); cache[cache_hash(v, cache_bits)] = v

    def hit(v):
        if cache.get(cache_hash(v, cache_bits)) == v:
            tokens.append(("cache", v)); px.append(v)
        else:
            lit(v)

    for v in colours[:20]:
        lit(v)
    while len(px) < width * height:
        left = width * height - len(px)
        kind = int(rng.integers(0, 4))
        if kind == 0 and left > 12:
            copy(int(rng.integers(2, 12)), int(rng.integers(1, min(len(px), 30))))
            for _ in range(min(3, width * height - len(px))):
                hit(px[len(px) - int(rng.integers(1, 6))])           # a colour the copy (or what lies just before) produced
        elif kind == 1:
            lit(colours[int(rng.integers(0, 40))])
        else:
            hit(px[int(rng.integers(0, len(px)))])
    assert len(px) == width * height and any(t[0] == "cache" for t in tokens)
    return vp8l(width, height, tokens, cache_bits=cache_bits)


def cases():
    out = []
    rng = np.random.default_rng(11)
    # every predictor mode, forced on every tile of a 37 x 21 frame
    y, x = np.mgrid[0:21, 0:37]
    frame = np.clip(np.stack([(x * 5 + y * 3) % 256, (x * 2 + y * 7) % 256, (x + y * 4) % 256], -1) + rng.integers(-9, 10, (21, 37, 3)), 0, 255).astype(np.uint8)
    tx, ty = W.tiles_of(37, 21)
    for mode in range(14):
        out.append(("mode%02d" % mode, W.write(frame, forced_modes=np.full((ty, tx), mode, np.uint8))))
    # every distance code: one length-1 reference at column 16 of row 9 of a 32 x 24 frame of distinct pixels
    for code in list(range(1, 121)) + [121, 300]:
        out.append(("dist%03d" % code, reference_file(code, 32, 24, 16, 9)))
    # mapped distances below 1: a frame 3 wide (no narrower-than-8 entry of the map falls below 1 at 32 wide), the
    # reference at column 0 of row 9
    for code in (18, 28, 44, 60, 64, 80, 88):
        xi, yi = DISTANCE_MAP[code - 1]
        assert xi + yi * 3 < 1
        out.append(("clamp%03d" % code, reference_file(code, 3, 24, 0, 9, seed=6)))
    for bits, seed in ((1, 21), (4, 22), (11, 23)):
        out.append(("cache%02d" % bits, cache_file(bits, seed)))
    # four groups at tile bits 2, each with its own five codes
    w, h = 19, 13
    groups = rng.integers(0, 4, ((h + 3) // 4, (w + 3) // 4))
    groups.reshape(-1)[:4] = (0, 1, 2, 3)
    px = [int(v) | 0xFF000000 for v in rng.integers(0, 1 << 24, w * h)]
    tokens = [("lit", v) for v in px[:60]] + [("copy", 7, 2)] + [("lit", v) for v in px[67:]]
    out.append(("groups4", vp8l(w, h, tokens, meta=(2, groups))))
    # a colour transform with elements of both signs
    w, h = 21, 11
    elems = rng.integers(0, 1 << 24, ((h + 3) // 4, (w + 3) // 4)).astype(np.uint32)
    elems.reshape(-1)[0] = 0x13E020                                   # green->red +0x20, green->blue -0x20, red->blue +0x13
    elems.reshape(-1)[1] = 0xF07F81
    out.append(("colour", vp8l(w, h, [("lit", int(v) | 0xFF000000) for v in rng.integers(0, 1 << 24, w * h)], transforms=(("color", 2, elems),))))
    # palette files whose pixels hold an index past the palette: 5 colours two to a value, 20 colours one to a value
    pal5, pal20 = distinct_pixels(5, 31), distinct_pixels(20, 32)
    w, h = 9, 6
    idx = rng.integers(0, 16, (h, w))
    packed = idx[:, 0::2].copy()
    packed[:, : w // 2] |= idx[:, 1::2] << 4
    out.append(("index_past5", vp8l(w, h, [("lit", 0xFF000000 | int(v) << 8) for v in packed.reshape(-1)], transforms=(("index", pal5),))))
    idx = rng.integers(0, 256, (h, w))
    out.append(("index_past20", vp8l(w, h, [("lit", 0xFF000000 | int(v) << 8) for v in idx.reshape(-1)], transforms=(("index", pal20),))))
    # simple codes of one and of two symbols
    two = [0xFF000000 | (200 if b else 3) << 8 | (1 if c else 0) << 16 | 77 for b, c in rng.integers(0, 2, (15 * 10, 2))]
    out.append(("simple2", vp8l(15, 10, [("lit", v) for v in two], simple=True)))
    out.append(("simple1", vp8l(6, 5, [("lit", 0xFF102030)] * 30, simple=True)))
    # the transforms in an order libwebp's encoder does not use: colour transform, predictor, subtract-green; and colour
    # indexing LAST, behind subtract-green and the predictor
    w, h = 18, 9
    modes = rng.integers(0, 14, ((h + 3) // 4, (w + 3) // 4))
    elems = rng.integers(0, 1 << 24, ((h + 3) // 4, (w + 3) // 4)).astype(np.uint32)
    lits = [("lit", int(v) | 0xFF000000) for v in rng.integers(0, 1 << 24, w * h)]
    out.append(("order_cpg", vp8l(w, h, lits, transforms=(("color", 2, elems), ("predictor", 2, modes), ("green",)))))
    idx = rng.integers(0, 4, (h, (w + 3) // 4 * 4))
    packed = idx[:, 0::4] | idx[:, 1::4] << 2 | idx[:, 2::4] << 4 | idx[:, 3::4] << 6
    out.append(("order_gpi", vp8l(w, h, [("lit", 0xFF000000 | int(v) << 8) for v in packed.reshape(-1)],
                                  transforms=(("green",), ("predictor", 2, modes), ("index", distinct_pixels(4, 33))))))
    return out


# ---------------------------------------------------------------- the implementation's seams: boundary_cases()
TOKENS, IN_WORDS, LOW_WORDS = 512, 512, 4          # WD_TOKENS, WD_IN_WORDS, and how many words from its end the window "runs low"


class RoundModel:
    """The decoder's round rule, restated from imp_webp_dec.h's description and fed with the bit counts the WRITER put
    out: a round stages IN_WORDS words from the word the next bit lies in; the reader moves a word into its 64-bit buffer
    whenever 32 bits or fewer are left in it, before every read; a round ends in front of a token when TOKENS tokens are
    listed or more than IN_WORDS - LOW_WORDS words have been moved."""

    def __init__(self, first_bit):
        self.bitpos, self.rounds, self.window_rounds, self.last_of_window = first_bit, 1, 0, []
        self.count = 0
        self._stage()

    def _stage(self):
        self.ntok, self.widx, self.bn = 0, 0, 0
        self._refill()
        self.bn -= self.bitpos & 31

    def _refill(self):
        if self.bn <= 32:
            self.bn += 32
            self.widx += 1

    def full(self):
        return self.ntok >= TOKENS or self.widx > IN_WORDS - LOW_WORDS

    def ends_on_window_after(self, reads):
        """would the round end on the WINDOW (not the token count) right behind a token of these reads?"""
        widx, bn = self.widx, self.bn
        for n in reads:
            if bn <= 32:
                bn, widx = bn + 32, widx + 1
            bn -= n
        return not self.full() and self.ntok + 1 < TOKENS and widx > IN_WORDS - LOW_WORDS

    def token(self, reads):
        if self.full():
            if self.ntok < TOKENS:
                self.window_rounds += 1
                self.last_of_window.append(self.count - 1)
            self.rounds += 1
            self._stage()
        for n in reads:
            self._refill()
            self.bn -= n
            self.bitpos += n
        self.ntok += 1
        self.count += 1


class Tokens:
    """a token list with the pixels and the colour cache it leaves behind (the writer's idea: Pillow's is what counts)"""

    def __init__(self, cache_bits=0):
        self.tokens, self.px, self.cache, self.bits = [], [], {}, cache_bits

    def _ins(self, v):
        self.px.append(v)
        if self.bits:
            self.cache[cache_hash(v, self.bits)] = v

    def lit(self, v):
        self.tokens.append(("lit", v))
        self._ins(v)

    def copy(self, length, dist):
        assert 1 <= dist <= len(self.px) and 1 <= length <= 4096, (length, dist, len(self.px))
        self.tokens.append(("copy", length, dist + 120))
        for _ in range(length):
            self._ins(self.px[len(self.px) - dist])

    def hit(self, v):
        """a cache token where the slot holds v, else a literal -> which"""
        if self.bits and self.cache.get(cache_hash(v, self.bits)) == v:
            self.tokens.append(("cache", v))
            self.px.append(v)
            return True
        self.lit(v)
        return False


def ramp(i, seed=5):
    """distinct for i < 65536, and small to store"""
    return 0xFF000000 | (i >> 8) << 16 | (i & 255) << 8 | ((i * 5 + seed) & 255)


def tokenise(px, cache_bits=0, dists=(1,), min_len=3):
    """pixels -> tokens, greedily: the longest match of at least min_len among `dists`, else a cache token where the slot
    holds the colour, else a literal"""
    t = Tokens(cache_bits)
    n = len(px)
    while len(t.px) < n:
        pos = len(t.px)
        best, bestd = 0, 0
        for d in dists:
            if d > pos:
                continue
            k = 0
            while pos + k < n and k < 4096 and px[pos + k] == px[pos + k - d]:
                k += 1
            if k > best:
                best, bestd = k, d
        if best >= min_len:
            t.copy(best, bestd)
        else:
            t.hit(px[pos])
    assert t.px == list(px)
    return t.tokens


def chain_lengths(symbols, longest, pair=None):
    """{symbol: length}: a complete code of lengths 1, 2, ... over `symbols` in that order, ending with two codes of
    `longest` bits; pair=(a, b): a code of a bits and two of b = a + 1 end it instead (10 and 11 side by side)"""
    if pair:
        a, b = pair
        assert b == a + 1 and len(symbols) >= a + 2
        lens = list(range(1, a)) + [a, b, b]
    else:
        assert len(symbols) >= longest + 1
        lens = list(range(1, longest)) + [longest, longest]
    return dict(zip(symbols, lens))


# lengths 1..6 once, then 9, 9, 10, 10, 4 x 11, 8 x 12, 16 x 13, 32 x 14, 64 x 15: complete, and 124 of the 134 symbols take more
# than the 10-bit table.  What a Fibonacci-like histogram gives its rare symbols, here FORCED, so that the symbols a file
# uses are the long ones whatever their counts: a literal of four such symbols costs 44..60 bits.
LONG_LENGTHS = [1, 2, 3, 4, 5, 6, 9, 9, 10, 10] + [11] * 4 + [12] * 8 + [13] * 16 + [14] * 32 + [15] * 64


def long_code(symbols):
    assert len(symbols) == len(LONG_LENGTHS)
    return dict(zip(symbols, LONG_LENGTHS))


def _finish(out, name, family, width, height, tokens, extra=None, **kw):
    """write the file, run the round model over what was written, keep the facts"""
    assert sum(token_step(t) for t in tokens) == (kw.pop("coded_width", width)) * height, name
    rec = {}
    blob = vp8l(width, height, tokens, record=rec, **kw)
    model = RoundModel(rec["first_bit"])
    for reads in rec["reads"]:
        model.token(reads)
    facts = {"family": family, "width": width, "height": height, "tokens": len(tokens), "maxlen": rec["maxlen"], "rounds": model.rounds,
             "window_rounds": model.window_rounds, "last_of_window": model.last_of_window}
    facts.update(extra or {})
    assert len(blob) < 65536, (name, len(blob))
    out.append(("b_" + name, blob, facts))


def _few(rng, n, values=5):
    """n literals with a handful of distinct values a channel: short codes"""
    ch = rng.integers(0, values, (n, 3))
    return [0xFF000000 | int(r) * 40 << 16 | int(g) * 50 << 8 | int(b) * 60 for r, g, b in ch]


def _family_a(out):
    rng = np.random.default_rng(101)
    # A1: the token count ends the round
    for w in (511, 512, 513, 1024, 1025):
        _finish(out, "a1_w%04d" % w, "A1", w, 1, [("lit", v) for v in _few(rng, w)])
    # A2: a match as token 512, as token 513, and one whose source is the literal in front of it, in the middle of a round
    w, h = 520, 2
    for bits in (0, 4):
        for what, before in (("tok512", 511), ("tok513", 512), ("mid", 300)):
            t = Tokens(bits)
            lits = _few(rng, w * h)
            for v in lits[:before - 1]:
                t.hit(v) if bits else t.lit(v)
            t.lit(0xFF010203 + before)                       # the source: a colour nothing else has, as a literal
            at = len(t.tokens)
            t.copy(70 if what == "mid" else 5, 1)
            if bits:
                t.hit(t.px[-1])                              # the colour the copy put into the cache last
            for v in lits[len(t.px):]:
                t.hit(v) if bits else t.lit(v)
            assert bits or at == before
            _finish(out, "a2_%s_c%d" % (what, bits), "A2", w, h, t.tokens, {"match_token": at}, cache_bits=bits)
    # A3: the window ends the round.  Every code is forced long; 64 x 48 of literals alone, then 260 x 130 where the last
    # token of a window-ended round is a match of 4096 (a green code of 15 bits, 10 extra bits, a distance code of 15 bits
    # with its extra bits: the longest token there is) and the first token of the next round reaches back to pixel 0
    green = list(range(0, 134))
    forced = {0: long_code(green), 1: long_code(green), 2: long_code(green), 3: long_code(green)}
    longs = [s for s, n in forced[0].items() if n >= 11]

    def long_literal():
        g, r, b, a = (int(longs[i]) for i in rng.integers(0, len(longs), 4))
        return a << 24 | r << 16 | g << 8 | b
    _finish(out, "a3_64x48", "A3", 64, 48, [("lit", long_literal()) for _ in range(64 * 48)], alpha=1, forced={**forced, 4: {0: 1, 1: 1}})
    w, h = 260, 130
    # green: the 134 literal symbols and, sharing the 15-bit end, the length symbols of 5 (4), 4096 (23) and 64 (11)
    gl = dict(zip(green[:131] + [256 + 4, 256 + 23, 256 + 11], LONG_LENGTHS))
    # distance: symbols 0..8 take 1..9 bits, 9 and 10 take 13, 20 (the distance 1030) and 39 take 15, every other one 14
    dl = {s: s + 1 if s < 9 else 13 if s < 11 else 15 if s in (20, 39) else 14 for s in range(40)}
    forced = {0: gl, 1: forced[1], 2: forced[2], 3: forced[3], 4: dl}
    longs = [s for s in longs if s < 131]
    rec = {}
    vp8l(w, h, [], alpha=1, forced=forced, record=rec)       # the header does not depend on the tokens: where the first one lies
    model, t, placed = RoundModel(rec["first_bit"]), Tokens(), []

    def reads_of(tok):
        return [n for k, s, _, xn in token_symbols(tok, 0) for n in ([forced[k][s]] + ([xn] if tok[0] == "copy" and s - (256 if k == 0 else 0) >= 4 else []))]

    def put(tok):
        model.token(reads_of(tok))
        t.copy(tok[1], tok[2] - 120) if tok[0] == "copy" else t.lit(tok[1])
    after_window = False
    while len(t.px) < w * h:
        left, pos = w * h - len(t.px), len(t.px)
        if after_window and left > 5:                        # first token of a round: from pixel 0 on, the largest distance here
            tok = ("copy", 5, pos + 120)
            placed.append(("far", len(t.tokens), pos))
            after_window = False
        elif model.rounds > 3 and left > 80:
            # (distance 1030: its symbol has a 15-bit code and 9 extra bits.)  4096 while the frame has room, then 64; in front
            # of pixel 32768 a 64 after every literal as well, so that the file stays small
            tok = ("copy", 4096 if left > 4096 + 600 else 64, 1030 + 120)
            if model.ends_on_window_after(reads_of(tok)):
                placed.append(("long", len(t.tokens), pos))
                after_window = True
            elif not (tok[1] == 64 and pos < 32768 + 100 and t.tokens[-1][0] == "lit"):
                tok = ("lit", long_literal())
        else:
            tok = ("lit", long_literal())
        put(tok)
    assert max(p for k, _, p in placed if k == "far") > 32768
    _finish(out, "a3_260x130", "A3", w, h, t.tokens, {"placed": placed}, alpha=1, forced=forced)


def _family_b(out):
    # a file a length: matches of that length at each distance that is legal there, distinct literals between them; the
    # first match's source starts at pixel 0, the last two lie back to back and the last ends on the last pixel
    w = 64
    for length in (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096):
        for bits in ((0, 1, 6, 11) if length in (2, 64, 65, 4096) else (0,)):
            t, n, after = Tokens(bits), 0, 0

            def lits(k):
                nonlocal n
                for _ in range(k):
                    t.lit(ramp(n, seed=length & 255))
                    n += 1
            lits(67)
            t.copy(length, 67)                               # dist == pos
            dists = sorted({1, 2, 3, 63, 64, 65, length - 1, length, length + 1} - {0})
            for d in dists + [None]:
                lits(3)
                if d is None:                                # the tail: a whole row's worth left, filled by two matches
                    lits((-(len(t.px) + 2 * length)) % w)
                    t.copy(length, 2)
                    t.copy(length, min(len(t.px), 4097))
                    break
                before = dict(t.cache)
                t.copy(length, d)
                if bits:
                    after += t.hit(t.px[-1])                 # what the copy put there last: always a cache token
                    for v in [v for k, v in sorted(before.items()) if t.cache.get(k) != v][:2]:
                        assert not t.hit(v)                  # what the copy overwrote: comes as a literal
                    after += t.hit(t.px[-2 - int(d > 1)])    # an earlier pixel of the copy: a token only if nothing displaced it
            assert len(t.px) % w == 0 and t.tokens[-1][0] == t.tokens[-2][0] == "copy" and (not bits or after >= len(dists))
            _finish(out, "b_len%04d_c%02d" % (length, bits), "B", w, len(t.px) // w, t.tokens, {"length": length, "cache_bits": bits}, cache_bits=bits)


def _residual_tokens(rng, n, values=None):
    if values is None:
        return [("lit", int(v)) for v in rng.integers(0, 1 << 32, n, dtype=np.uint64)]
    pick = rng.integers(0, len(values), (n, 4))
    return [("lit", int(values[a]) << 24 | int(values[r]) << 16 | int(values[g]) << 8 | int(values[b])) for a, r, g, b in pick]


def _argb_words(gs):
    """(H, W, 4) A,R,G,B -> ARGB words in raster order"""
    gs = np.asarray(gs, np.int64)
    return [int(v) for v in (gs[..., 0] << 24 | gs[..., 1] << 16 | gs[..., 2] << 8 | gs[..., 3]).reshape(-1)]


def _family_c(out):
    rng = np.random.default_rng(103)
    for h in (255, 256, 257, 513):
        for w in (1, 2, 3, 5):
            modes = rng.integers(0, 16, ((h + 3) // 4, (w + 3) // 4))
            modes.reshape(-1)[:2] = (14, 15)
            _finish(out, "c_%dx%d" % (w, h), "C", w, h, _residual_tokens(rng, w * h, values=(0, 1, 2, 3, 128, 250, 254, 255)), alpha=1,
                    transforms=(("predictor", 2, modes),))
    # pixels chosen, residuals from webp_writer's predictors: L + T - TL far outside 0..255 on both sides (modes 12, 13),
    # and L, T at equal distances from TL (mode 11's two sums tie; on a tie the choice is T)
    w, h = 5, 257
    y, x = np.mgrid[0:h, 0:w]
    sat = np.where(((x + y) % 2 == 0)[..., None], 255, 0) ^ np.where(((y // 3) % 2 == 0)[..., None], 0, 255)
    sat = np.clip(sat + rng.integers(-3, 4, (h, w, 4)) * np.array([1, 1, 1, 1]), 0, 255).astype(np.int32)
    modes = np.where(rng.integers(0, 2, ((h + 3) // 4, (w + 3) // 4)) == 0, 12, 13)
    _finish(out, "c_saturate_5x257", "C", w, h, [("lit", v) for v in _argb_words(W.residuals(sat, modes, 2))], alpha=1, transforms=(("predictor", 2, modes),))
    tie = np.zeros((h, w, 4), np.int32)
    tie[..., :] = (((x * 7 + y * 7) % 256)[..., None] + np.array([0, 40, 80, 120])) % 256      # L == T everywhere: both sums equal
    odd = rng.integers(0, 4, (h, w)) == 0
    tie[odd] = (tie[odd] + rng.integers(-2, 3, (int(odd.sum()), 4))) % 256                     # and near-ties of either sign
    modes = np.full(((h + 3) // 4, (w + 3) // 4), 11)
    _finish(out, "c_select_5x257", "C", w, h, [("lit", v) for v in _argb_words(W.residuals(tie, modes, 2))], alpha=1, transforms=(("predictor", 2, modes),))
    # one tile over the whole frame (transform bits 9); and the three transforms together
    _finish(out, "c_bits9_5x513", "C", 5, 513, _residual_tokens(rng, 5 * 513, values=(0, 1, 3, 255, 253)), alpha=1,
            transforms=(("predictor", 9, np.array([[13]])),))
    w, h = 3, 257
    modes = rng.integers(0, 14, ((h + 3) // 4, 1))
    elems = rng.integers(0, 1 << 24, ((h + 3) // 4, 1)).astype(np.uint32)
    _finish(out, "c_pcg_3x257", "C", w, h, _residual_tokens(rng, w * h, values=(0, 1, 2, 128, 254, 255)), alpha=1,
            transforms=(("predictor", 2, modes), ("color", 2, elems), ("green",)))


def _family_d(out):
    rng = np.random.default_rng(104)
    w, h = 16, 8
    for k, what in enumerate(("green", "red", "blue", "alpha", "dist")):
        for tag, kw in (("10_11", {"pair": (10, 11)}), ("15", {})):
            n = 12 if kw else 16
            if k < 4:
                syms = [int(v) for v in rng.choice(256, n, replace=False)]
                forced = {k: chain_lengths(syms, 15, **kw)}
                shift = (8, 16, 0, 24)[k]
                toks = [("lit", (0xFF000000 if k != 3 else 0) | int(syms[i]) << shift | (int(j) * 3 << (0 if k == 0 else 8)))
                        for i, j in zip(rng.integers(n - 3, n, w * h), rng.integers(0, 4, w * h))]
                for i in range(n):                           # every symbol of the code once
                    toks[i * 5] = ("lit", (toks[i * 5][1] & ~(255 << shift)) | int(syms[i]) << shift)
            else:
                # distance symbols 0..n-1 are codes 1..n of the map, or plain distances: the long codes go to symbols
                # whose distances are legal in the second row
                syms = [int(v) for v in rng.permutation(n)]
                forced = {4: chain_lengths(syms, 15, **kw)}
                t = Tokens()
                for i in range(130):                         # (the farthest of these distances is 120)
                    t.lit(ramp(i, seed=k))
                for s in syms[::-1] + syms[-3:]:
                    code = LZ.unprefix_value(s, 1)           # (extra bits 1: some code of that symbol)
                    d = code_distance(code, w)
                    t.tokens.append(("copy", 2, code))
                    for _ in range(2):
                        t.px.append(t.px[len(t.px) - d])
                    t.lit(ramp(100 + len(t.px), seed=k))
                while len(t.px) < w * 14:
                    t.lit(ramp(len(t.px), seed=k))
                toks = t.tokens
            _finish(out, "d_%s_%s" % (what, tag), "D", w, h if k < 4 else 14, toks, {"code": k}, alpha=1, forced=forced)
    # the highest key of an 11-bit cache: green symbol 280 + 2047
    top = next(v for v in range(0xFF000000, 0xFF100000) if cache_hash(v, 11) == 2047)
    t = Tokens(11)
    for i in range(20):
        t.lit(ramp(i))
    t.lit(top)
    t.lit(ramp(21))
    assert t.hit(top) and t.hit(top)
    for i in range(w * h - len(t.px)):
        t.hit(ramp(i % 24))
    _finish(out, "d_cache_top", "D", w, h, t.tokens, {"top_key": sum(1 for tok in t.tokens if tok == ("cache", top))}, cache_bits=11)
    # distance symbol 39 (distance codes from 786 433 on): a frame of 16383 x 49 that is nearly all matches of 4096
    w, h = 16383, 49
    t = Tokens()
    for i in range(24):
        t.lit(ramp(i * 37))
    while w * h - len(t.px) > 16000:
        t.copy(4096, 24 if len(t.tokens) % 3 else 23)
    far = len(t.px) - 5
    assert LZ.prefix_value(far + 120)[0] == 39
    t.lit(0xFF123456)
    t.copy(4096, far)
    t.copy(7, len(t.px))
    while w * h - len(t.px) > 0:
        t.copy(min(4096, w * h - len(t.px)), 4097)
    _finish(out, "d_dist39", "D", w, h, t.tokens, {"far": far})


def _family_e(out):
    # 72 x 72 at meta bits 2: each of the 324 tiles its own group, with its own five codes; matches that are the last token of
    # a tile's piece of a row and run across the tile's edge
    w = h = 72
    groups = np.arange(324).reshape(18, 18)
    for bits in (0, 3):
        rng = np.random.default_rng(105)
        t, crossing = Tokens(bits), 0
        while len(t.px) < w * h:
            pos = len(t.px)
            y, x = divmod(pos, w)
            if y and x % 4 == 3 and x < w - 8 and rng.integers(0, 3) == 0:
                t.copy(int(rng.integers(2, 9)), int(rng.choice((1, w, w - 1, 4))))
                crossing += 1
            else:
                g = int(groups[y >> 2, x >> 2])
                v = 0xFF000000 | ((g * 7 + int(rng.integers(0, 3))) & 255) << 16 | ((g + int(rng.integers(0, 3)) * 9) & 255) << 8 | int(rng.integers(0, 2)) * 200
                t.hit(v)
        _finish(out, "e_groups324_c%d" % bits, "E", w, h, t.tokens, {"groups": 324, "crossing": crossing}, cache_bits=bits, meta=(2, groups))


def _sparse_residuals(rng, n, every):
    px = [0xFF000000 if i == 0 else 0 for i in range(n)]
    for i in range(every, n, every):
        px[i] = int(rng.integers(0, 4)) << 16 | int(rng.integers(0, 4)) << 8 | int(rng.integers(0, 4))
    return px


def _family_f(out):
    rng = np.random.default_rng(106)
    for w, h in ((16383, 1), (1, 16383)):
        sh = ((h + 511) // 512, (w + 511) // 512)
        modes = rng.integers(1, 14, sh)
        elems = rng.integers(0, 1 << 24, sh).astype(np.uint32)
        toks = tokenise(_sparse_residuals(rng, w * h, 97), dists=(1, 97))
        _finish(out, "f_pcg_%dx%d" % (w, h), "F", w, h, toks, alpha=1, transforms=(("predictor", 9, modes), ("color", 9, elems), ("green",)))
    # palettes: eight pixels a value over the widest row (2047 whole values and one of seven pixels); width 1 at four and at
    # two pixels a value (one pixel in a value's low bits, a row)
    pal = distinct_pixels(2, 41)
    cw = (16383 + 7) // 8
    vals = [0xFF000000 | ((i * 37 + (i >> 5)) & 255) << 8 for i in range(cw)]
    _finish(out, "f_pal2_16383x1", "F", 16383, 1, tokenise(vals, dists=(1, 32)), transforms=(("index", pal),), coded_width=cw)
    for colours, h in ((4, 300), (16, 300)):
        pal = distinct_pixels(colours, 42 + colours)
        vals = [0xFF000000 | int(v) << 8 for v in rng.integers(0, colours, h)]
        _finish(out, "f_pal%d_1x%d" % (colours, h), "F", 1, h, [("lit", v) for v in vals], transforms=(("index", pal),), coded_width=1)


def _family_g(out):
    # sub-images coded with matches and a colour cache of their own: the predictor's modes, the colour transform's elements,
    # the entropy image's groups -- one file each, and one with all three
    rng = np.random.default_rng(107)
    w = h = 64
    sw = 16

    def repeating(values):
        base = [int(v) for v in rng.choice(values, 24)]
        tiles = [base[(i * 5 + (i // 16) * 3) % 24] if (i // 7) % 3 else base[i % 5] for i in range(sw * sw)]
        return np.array(tiles).reshape(sw, sw)

    modes, groups = repeating(np.arange(14)), repeating(np.arange(6))
    groups.reshape(-1)[:6] = np.arange(6)
    elems = repeating(rng.integers(0, 1 << 24, 9)).astype(np.uint32)

    def sub(kind, data, bits):
        toks = tokenise(sub_values(kind, data) if kind != "meta" else [0xFF000000 | int(g) << 8 for g in data.reshape(-1)], cache_bits=bits, dists=(1, 2, 5, sw))
        assert any(tk[0] == "copy" for tk in toks) and any(tk[0] == "cache" for tk in toks), kind
        return {"tokens": toks, "cache_bits": bits}

    main = _residual_tokens(rng, w * h, values=(0, 1, 2, 254, 255))
    p = ("predictor", 2, modes, sub("predictor", modes, 2))
    c = ("color", 2, elems, sub("color", elems, 3))
    m = (2, groups, sub("meta", groups, 1))
    _finish(out, "g_predictor", "G", w, h, main, alpha=1, transforms=(p,))
    _finish(out, "g_colour", "G", w, h, main, alpha=1, transforms=(c,))
    _finish(out, "g_meta", "G", w, h, main, {"groups": 6}, alpha=1, meta=m)
    _finish(out, "g_all", "G", w, h, main, {"groups": 6}, alpha=1, transforms=(p, c, ("green",)), meta=m)


@functools.lru_cache(maxsize=None)
def _boundary():
    out = []
    for family in (_family_a, _family_b, _family_c, _family_d, _family_e, _family_f, _family_g):
        family(out)
    assert len({name for name, _, _ in out}) == len(out)
    return out


def boundary_cases():
    return [(name, blob) for name, blob, _ in _boundary()]


def boundary_facts():
    return {name: facts for name, _, facts in _boundary()}
