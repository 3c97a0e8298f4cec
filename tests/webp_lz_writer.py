"""The lossless WebP file of include/impgpu.h ("WEBP ANSWERS") WITH backward references (IMPGPU_WEBP_ENC_BACKREFS), written
with numpy alone from that paragraph: this module, never the library, says what the flagged bytes are.  Container, payload
header, transforms, predictions, mode choice, mode image and the prefix-code rules are webp_writer's and are reused; what
differs is the main image's pixel stream: the residual plane is cut into items of ITEM positions, every item is parsed
greedily on its own against the first 24 entries of VP8L's distance map, and a token is a literal pixel or (length, k).

    write(frame)                      as webp_writer.write, the flagged file
    write(frame, forced_modes=m)      under forced mode 0 the residuals ARE the green-subtracted pixels (but for the edges)
    tokens(frame, forced_modes=m)     [(position, length, k)] with k = 0 and length = 1 for a literal
"""
import numpy as np

import webp_writer as W

ITEM = 1024                                    # WEBP_ITEM
MIN_MATCH = 3                                  # IMPGPU_WEBP_MIN_MATCH
# candidates k = 1 .. 24 as (xi, yi): the distance is xi + yi * w
CANDIDATES = ((0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3), (-1, 3),
              (3, 1), (-3, 1), (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0))


def prefix_value(v):
    """VP8L's prefix coding of a value v >= 1 -> (symbol, extra value, extra bits)"""
    assert v >= 1
    if v <= 4:
        return v - 1, 0, 0
    u = v - 1
    hb = u.bit_length() - 1
    sb = (u >> (hb - 1)) & 1
    return 2 * hb + sb, u & ((1 << (hb - 1)) - 1), hb - 1


def unprefix_value(sym, bits):
    """the decoder's side of prefix_value"""
    if sym < 4:
        return sym + 1
    eb = (sym - 2) >> 1
    return ((2 + (sym & 1)) << eb) + bits + 1


def match_lengths(res, w):
    """(24, n): L_k(p) for every position of the residual plane `res` (uint32, raster order) of a frame `w` wide"""
    n = res.size
    idx = np.arange(n, dtype=np.int64)
    item_end = np.minimum((idx // ITEM + 1) * ITEM, n)
    out = np.zeros((len(CANDIDATES), n), np.int64)
    for k, (xi, yi) in enumerate(CANDIDATES):
        d = xi + yi * w
        if d < 1 or d > n - 1:
            continue                                             # usable nowhere
        eq = np.zeros(n, bool)
        eq[d:] = res[d:] == res[:-d]
        stop = np.where(eq, n, idx)                              # the next position at or after p that does not match ...
        stop = np.minimum.accumulate(stop[::-1])[::-1]
        out[k] = np.minimum(stop, item_end) - idx                # ... or the item's end
    return out


def parse(res, w):
    """the greedy parse -> (positions, lengths, ks) of the tokens; k = 0 and length 1: a literal"""
    lengths = match_lengths(res, w)
    best_k = np.argmax(lengths, axis=0)                          # the first maximum: a tie goes to the lowest k
    best = lengths[best_k, np.arange(res.size)]
    step = np.where(best >= MIN_MATCH, best, 1).tolist()
    pos, p, n = [], 0, res.size
    while p < n:
        pos.append(p)
        p += step[p]
    assert p == n
    pos = np.array(pos, np.int64)
    ln = best[pos]
    is_ref = ln >= MIN_MATCH
    return pos, np.where(is_ref, ln, 1), np.where(is_ref, best_k[pos] + 1, 0)


def _planes(frame, forced_modes, tile_bits):
    argb = W.argb_of(frame)
    h, w, _ = argb.shape
    assert 1 <= w <= 16384 and 1 <= h <= 16384
    channels = 1 if np.asarray(frame).ndim == 2 else np.asarray(frame).shape[2]
    alpha_used = int(channels == 4 and bool((argb[..., 0] != 255).any()))
    gs = W.subtract_green(argb)
    tx, ty = W.tiles_of(w, h, tile_bits)
    if forced_modes is None:
        modes = W.choose_modes(gs, tile_bits)
    else:
        modes = np.asarray(forced_modes, np.uint8).reshape(ty, tx)
        assert int(modes.max()) < W.MODES
    res = W.residuals(gs, modes, tile_bits).reshape(-1, 4).astype(np.uint32)     # channels A, R, G, B
    return w, h, alpha_used, modes, res


def tokens(frame, forced_modes=None, tile_bits=W.TILE_BITS):
    w, h, _, _, res = _planes(frame, forced_modes, tile_bits)
    pos, ln, k = parse(res[:, 0] << 24 | res[:, 1] << 16 | res[:, 2] << 8 | res[:, 3], w)
    return list(zip(pos.tolist(), ln.tolist(), k.tolist()))


def _stream(frame, forced_modes, tile_bits):
    w, h, alpha_used, modes, res = _planes(frame, forced_modes, tile_bits)
    vals, lens = [], []

    def put(pairs):
        for v, n in pairs:
            vals.append(v)
            lens.append(n)

    # everything up to the main image is webp_writer's, bit for bit
    put([(0x2F, 8), (w - 1, 14), (h - 1, 14), (alpha_used, 1), (0, 3)])
    put([(1, 1), (2, 2)])
    put([(1, 1), (0, 2), (tile_bits - 2, 3)])
    put([(0, 1)])
    mbits, mlen, mcode = W.prefix_code(np.bincount(modes.reshape(-1), minlength=W.MODES), 280)
    put(mbits)
    put(W.prefix_code([1], 256)[0])
    put(W.prefix_code([1], 256)[0])
    put(W.prefix_code([0] * 255 + [1], 256)[0])
    put(W.SIMPLE_ZERO)                                                          # the mode image has no backward references
    flat = modes.reshape(-1)
    put(zip(np.array(mcode, np.uint64)[flat].tolist(), np.array(mlen, np.int64)[flat].tolist()))
    put([(0, 1)])
    put([(0, 1), (0, 1)])
    # the tokens and what they count
    pos, ln, k = parse(res[:, 0] << 24 | res[:, 1] << 16 | res[:, 2] << 8 | res[:, 3], w)
    lit = k == 0
    lsym = np.array([prefix_value(v) for v in range(1, ITEM + 1)] + [(0, 0, 0)], np.int64)             # row v - 1; the last: a literal
    dsym = np.array([prefix_value(v) for v in range(1, len(CANDIDATES) + 1)] + [(0, 0, 0)], np.int64)
    tl, td = lsym[np.where(lit, ITEM, ln - 1)], dsym[np.where(lit, len(CANDIDATES), k - 1)]
    green = np.where(lit, res[pos, 2], 256 + tl[:, 0])
    ghist = np.bincount(green, minlength=280)
    dhist = np.bincount(td[~lit, 0], minlength=40)
    codes = []
    for hist, alphabet in ((ghist, 280), (np.bincount(res[pos[lit], 1], minlength=256), 256), (np.bincount(res[pos[lit], 3], minlength=256), 256),
                           (np.bincount(res[pos[lit], 0], minlength=256), 256)):
        bits, cl, cd = W.prefix_code(hist, alphabet)
        put(bits)
        codes.append((np.array(cd, np.uint64), np.array(cl, np.int64)))
    if not dhist.any():
        put(W.SIMPLE_ZERO)
        dcode, dlen = np.zeros(40, np.uint64), np.zeros(40, np.int64)
    else:
        bits, cl, cd = W.prefix_code(dhist, 40)
        put(bits)
        dcode, dlen = np.array(cd, np.uint64), np.array(cl, np.int64)
    # a token is four parts: green, red, blue, alpha -- or length symbol, its extra bits, distance symbol, its extra bits
    tv, tn = np.zeros((pos.size, 4), np.uint64), np.zeros((pos.size, 4), np.int64)
    tv[:, 0], tn[:, 0] = codes[0][0][green], codes[0][1][green]
    r, b, a = res[pos, 1], res[pos, 3], res[pos, 0]
    tv[:, 1], tn[:, 1] = np.where(lit, codes[1][0][r], tl[:, 1].astype(np.uint64)), np.where(lit, codes[1][1][r], tl[:, 2])
    tv[:, 2], tn[:, 2] = np.where(lit, codes[2][0][b], dcode[td[:, 0]]), np.where(lit, codes[2][1][b], dlen[td[:, 0]])
    tv[:, 3], tn[:, 3] = np.where(lit, codes[3][0][a], td[:, 1].astype(np.uint64)), np.where(lit, codes[3][1][a], td[:, 2])
    return np.concatenate([np.array(vals, np.uint64), tv.reshape(-1)]), np.concatenate([np.array(lens, np.int64), tn.reshape(-1)])


def write(frame, forced_modes=None, tile_bits=W.TILE_BITS):
    vals, lens = _stream(frame, forced_modes, tile_bits)
    payload, _ = W._pack(vals, lens)
    return W.container(payload)


def file_size(frame, forced_modes=None, tile_bits=W.TILE_BITS):
    _, lens = _stream(frame, forced_modes, tile_bits)
    n = (int(lens.sum()) + 7) // 8
    return 20 + n + (n & 1)
