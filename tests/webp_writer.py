"""The lossless WebP file of include/impgpu.h ("WEBP ANSWERS"), written with numpy alone: this module, never the library,
says what the bytes are.  A VP8L stream with two transforms (subtract-green, then the spatial predictor with a mode per
tile of 2^TILE_BITS pixels), no colour cache, no meta prefix image and no backward references; five prefix codes per
entropy-coded image whose lengths come from zlib's build_tree (heap order and 15-bit / 7-bit repair replayed exactly) and
whose length lists are coded by zlib's send_tree run rule.  Not libwebp's bytes: only its decoder must agree on the pixels.

    write(frame)                      HxW, HxWx1, HxWx3 (B,G,R) or HxWx4 (B,G,R,A) uint8 -> the file's bytes
    write(frame, forced_modes=m)      m: one mode 0..13 per tile, raster order; the chooser is skipped
    file_size(frame, tile_bits=b)     the file's length alone (how TILE_BITS was chosen)
"""
import numpy as np

TILE_BITS = 4                                 # IMPGPU_WEBP_TILE_BITS
MODES = 14
CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
BLACK = np.array([255, 0, 0, 0], np.int32)    # 0xff000000, channels in the order A, R, G, B


# ---------------------------------------------------------------- pixels
def argb_of(frame):
    """-> (H, W, 4) int32, channels A, R, G, B"""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = f[..., None]
    assert f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] in (1, 3, 4), (f.dtype, f.shape)
    h, w, c = f.shape
    out = np.empty((h, w, 4), np.int32)
    if c == 1:
        out[..., 0] = 255
        out[..., 1] = out[..., 2] = out[..., 3] = f[..., 0]
    else:
        out[..., 0] = f[..., 3] if c == 4 else 255
        out[..., 1], out[..., 2], out[..., 3] = f[..., 2], f[..., 1], f[..., 0]
    return out


def subtract_green(argb):
    gs = argb.copy()
    gs[..., 1] = (gs[..., 1] - gs[..., 2]) & 255
    gs[..., 3] = (gs[..., 3] - gs[..., 2]) & 255
    return gs


def _neighbours(gs):
    left, top, tl, tr = (np.zeros_like(gs) for _ in range(4))
    left[:, 1:] = gs[:, :-1]
    top[1:] = gs[:-1]
    tl[1:, 1:] = gs[:-1, :-1]
    tr[1:, :-1] = gs[:-1, 1:]
    tr[1:, -1] = gs[1:, 0]                     # TR of the last column: column 0 of the current row
    return left, top, tl, tr


def _avg2(a, b):
    return (a + b) >> 1


def _clamp(v):
    return np.clip(v, 0, 255)


def _half(a, b):
    d = a - b
    return _clamp(a + np.sign(d) * (np.abs(d) // 2))          # C division, toward zero


def _mode(m, left, top, tl, tr):
    if m == 0:
        return np.broadcast_to(BLACK, left.shape)
    if m == 1:
        return left
    if m == 2:
        return top
    if m == 3:
        return tr
    if m == 4:
        return tl
    if m == 5:
        return _avg2(_avg2(left, tr), top)
    if m == 6:
        return _avg2(left, tl)
    if m == 7:
        return _avg2(left, top)
    if m == 8:
        return _avg2(tl, top)
    if m == 9:
        return _avg2(top, tr)
    if m == 10:
        return _avg2(_avg2(left, tl), _avg2(top, tr))
    if m == 11:                                                # Select: p = L + T - TL; L when sum|p - L| < sum|p - T|
        to_l = np.abs(top - tl).sum(axis=2)
        to_t = np.abs(left - tl).sum(axis=2)
        return np.where((to_l < to_t)[..., None], left, top)
    if m == 12:
        return _clamp(left + top - tl)
    assert m == 13, m
    return _half(_avg2(left, top), tl)


def _edged(pred, left, top):
    """the predictions the edge rules fix, whatever the tile's mode"""
    p = np.array(pred, np.int32)
    p[0, 1:] = left[0, 1:]
    p[1:, 0] = top[1:, 0]
    p[0, 0] = BLACK
    return p


def tiles_of(w, h, tile_bits=TILE_BITS):
    t = 1 << tile_bits
    return (w + t - 1) // t, (h + t - 1) // t


def mode_costs(gs, tile_bits=TILE_BITS):
    """(14, tiles_y, tiles_x): the sum over a tile's pixels and four channels of min(r, 256 - r)"""
    h, w, _ = gs.shape
    tx, ty = tiles_of(w, h, tile_bits)
    t = 1 << tile_bits
    nb = _neighbours(gs)
    out = np.zeros((MODES, ty, tx), np.int64)
    for m in range(MODES):
        r = (gs - _edged(_mode(m, *nb), nb[0], nb[1])) & 255
        cost = np.minimum(r, 256 - r).sum(axis=2)
        pad = np.zeros((ty * t, tx * t), np.int64)
        pad[:h, :w] = cost
        out[m] = pad.reshape(ty, t, tx, t).sum(axis=(1, 3))
    return out


def choose_modes(gs, tile_bits=TILE_BITS):
    return np.argmin(mode_costs(gs, tile_bits), axis=0).astype(np.uint8)     # a tie goes to the lowest mode


def residuals(gs, modes, tile_bits=TILE_BITS):
    h, w, _ = gs.shape
    t = 1 << tile_bits
    per_pixel = np.repeat(np.repeat(modes, t, axis=0), t, axis=1)[:h, :w]
    nb = _neighbours(gs)
    out = np.zeros_like(gs)
    for m in np.unique(modes):
        r = (gs - _edged(_mode(int(m), *nb), nb[0], nb[1])) & 255
        sel = per_pixel == m
        out[sel] = r[sel]
    return out


# ---------------------------------------------------------------- prefix codes (zlib's trees.c)
def build_lengths(freq, max_length):
    """zlib's build_tree + gen_bitlen over `freq`: the heap is ordered by (frequency, depth) and replayed exactly"""
    elems = len(freq)
    heap_size = 2 * elems + 1
    f = [int(v) for v in freq] + [0] * (elems + 1)
    heap, depth, dl = [0] * heap_size, [0] * heap_size, [0] * heap_size
    heap_len, heap_max, max_code = 0, heap_size, -1
    for n in range(elems):
        if f[n]:
            heap_len += 1
            heap[heap_len] = max_code = n
    while heap_len < 2:                                        # at least two codes of non-zero frequency
        if max_code < 2:
            max_code += 1
            node = max_code
        else:
            node = 0
        heap_len += 1
        heap[heap_len] = node
        f[node] = 1

    def smaller(n, m):
        return f[n] < f[m] or (f[n] == f[m] and depth[n] <= depth[m])

    def down(k):
        v = heap[k]
        j = k << 1
        while j <= heap_len:
            if j < heap_len and smaller(heap[j + 1], heap[j]):
                j += 1
            if smaller(v, heap[j]):
                break
            heap[k] = heap[j]
            k = j
            j <<= 1
        heap[k] = v

    for n in range(heap_len // 2, 0, -1):
        down(n)
    node = elems
    while True:
        n = heap[1]
        heap[1] = heap[heap_len]
        heap_len -= 1
        down(1)
        m = heap[1]
        heap_max -= 1
        heap[heap_max] = n
        heap_max -= 1
        heap[heap_max] = m
        f[node] = f[n] + f[m]
        depth[node] = max(depth[n], depth[m]) + 1
        dl[n] = dl[m] = node
        heap[1] = node
        node += 1
        down(1)
        if heap_len < 2:
            break
    heap_max -= 1
    heap[heap_max] = heap[1]
    bl_count = [0] * (max_length + 1)
    dl[heap[heap_max]] = 0
    overflow = 0
    hh = heap_max + 1
    while hh < heap_size:
        n = heap[hh]
        bits = dl[dl[n]] + 1
        if bits > max_length:
            bits = max_length
            overflow += 1
        dl[n] = bits
        if n <= max_code:
            bl_count[bits] += 1
        hh += 1
    if overflow:
        while overflow > 0:
            bits = max_length - 1
            while bl_count[bits] == 0:
                bits -= 1
            bl_count[bits] -= 1
            bl_count[bits + 1] += 2
            bl_count[max_length] -= 1
            overflow -= 2
        for bits in range(max_length, 0, -1):
            n = bl_count[bits]
            while n:
                hh -= 1
                m = heap[hh]
                if m > max_code:
                    continue
                dl[m] = bits
                n -= 1
    return [dl[n] if n <= max_code else 0 for n in range(elems)]


def canonical_codes(lengths):
    """canonical codes, bit-reversed (written LSB first), as deflate's gen_codes"""
    top = max(max(lengths), 1)
    count = [0] * (top + 2)
    for v in lengths:
        count[v] += 1
    count[0] = 0
    nxt, c = [0] * (top + 2), 0
    for bits in range(1, top + 1):
        c = (c + count[bits - 1]) << 1
        nxt[bits] = c
    out = []
    for v in lengths:
        if not v:
            out.append(0)
            continue
        code = nxt[v]
        nxt[v] += 1
        out.append(int(format(code, "0%db" % v)[::-1], 2))
    return out


def length_tokens(lengths):
    """zlib's send_tree over all of `lengths`: [(symbol 0..18, extra value, extra bits)]"""
    out = []
    prev, nextlen, count = -1, lengths[0], 0
    max_count, min_count = (138, 3) if nextlen == 0 else (7, 4)
    for n in range(len(lengths)):
        cur = nextlen
        nextlen = lengths[n + 1] if n + 1 < len(lengths) else -1
        count += 1
        if count < max_count and cur == nextlen:
            continue
        if count < min_count:
            out += [(cur, 0, 0)] * count
        elif cur != 0:
            if cur != prev:
                out.append((cur, 0, 0))
                count -= 1
            out.append((16, count - 3, 2))
        elif count <= 10:
            out.append((17, count - 3, 3))
        else:
            out.append((18, count - 11, 7))
        count = 0
        prev = cur
        if nextlen == 0:
            max_count, min_count = 138, 3
        elif cur == nextlen:
            max_count, min_count = 6, 3
        else:
            max_count, min_count = 7, 4
    return out


def prefix_code(hist, alphabet):
    """-> (header bits [(value, count)], lengths, codes) of the code of an alphabet whose first len(hist) symbols have
    those frequencies.  One used symbol: the simple form, zero bits a symbol.  Otherwise the normal form."""
    used = [n for n, v in enumerate(hist) if v]
    assert used, "a code nobody uses is not written this way"
    lengths = [0] * alphabet
    if len(used) == 1:
        return [(1, 1), (0, 1), (1, 1), (used[0], 8)], lengths, [0] * alphabet
    freq = [int(v) for v in hist] + [0] * (alphabet - len(hist))
    lengths = build_lengths(freq, 15)
    codes = canonical_codes(lengths)
    tokens = length_tokens(lengths)
    bfreq = [0] * 19
    for s, _, _ in tokens:
        bfreq[s] += 1
    blen = build_lengths(bfreq, 7)
    bcode = canonical_codes(blen)
    count = 19
    while count > 4 and blen[CL_ORDER[count - 1]] == 0:
        count -= 1
    bits = [(0, 1), (count - 4, 4)] + [(blen[CL_ORDER[i]], 3) for i in range(count)] + [(0, 1)]
    for s, xv, xb in tokens:
        bits.append((bcode[s], blen[s]))
        if xb:
            bits.append((xv, xb))
    return bits, lengths, codes


SIMPLE_ZERO = [(1, 1), (0, 1), (0, 1), (0, 1)]                 # the distance code: one symbol, 0, written in one bit


# ---------------------------------------------------------------- bits
def _pack(vals, lens):
    """LSB-first concatenation of vals[i]'s low lens[i] bits (lens <= 32) -> (bytes, bit count)"""
    vals = np.asarray(vals, np.uint64)
    lens = np.asarray(lens, np.int64)
    pos = np.concatenate([[0], np.cumsum(lens)])
    total = int(pos[-1])
    bits = np.zeros(((total + 7) // 8) * 8, np.uint8)
    for k in range(int(lens.max()) if lens.size else 0):
        sel = lens > k
        bits[pos[:-1][sel] + k] = ((vals[sel] >> np.uint64(k)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits, bitorder="little").tobytes(), total


def _stream(frame, forced_modes, tile_bits):
    argb = argb_of(frame)
    h, w, _ = argb.shape
    assert 1 <= w <= 16384 and 1 <= h <= 16384
    channels = 1 if np.asarray(frame).ndim == 2 else np.asarray(frame).shape[2]
    alpha_used = int(channels == 4 and bool((argb[..., 0] != 255).any()))
    gs = subtract_green(argb)
    tx, ty = tiles_of(w, h, tile_bits)
    if forced_modes is None:
        modes = choose_modes(gs, tile_bits)
    else:
        modes = np.asarray(forced_modes, np.uint8).reshape(ty, tx)
        assert int(modes.max()) < MODES
    res = residuals(gs, modes, tile_bits)
    vals, lens = [], []

    def put(pairs):
        for v, n in pairs:
            vals.append(v)
            lens.append(n)

    put([(0x2F, 8), (w - 1, 14), (h - 1, 14), (alpha_used, 1), (0, 3)])
    put([(1, 1), (2, 2)])                                                       # subtract-green
    put([(1, 1), (0, 2), (tile_bits - 2, 3)])                                   # predictor, then its mode image
    put([(0, 1)])                                                               # no colour cache
    mbits, mlen, mcode = prefix_code(np.bincount(modes.reshape(-1), minlength=MODES), 280)
    put(mbits)
    put(prefix_code([1], 256)[0])                                               # red 0
    put(prefix_code([1], 256)[0])                                               # blue 0
    put(prefix_code([0] * 255 + [1], 256)[0])                                   # alpha 255
    put(SIMPLE_ZERO)
    flat = modes.reshape(-1)
    head_vals, head_lens = vals, lens
    mode_vals, mode_lens = np.array(mcode, np.uint64)[flat], np.array(mlen, np.int64)[flat]
    vals, lens = [], []
    put([(0, 1)])                                                               # no further transform
    put([(0, 1), (0, 1)])                                                       # no colour cache, no meta prefix image
    tabs = []
    for ch, alphabet in ((2, 280), (1, 256), (3, 256), (0, 256)):               # green, red, blue, alpha
        bits, ln, cd = prefix_code(np.bincount(res[..., ch].reshape(-1), minlength=256), alphabet)
        put(bits)
        tabs.append((np.array(cd, np.uint64), np.array(ln, np.int64), res[..., ch].reshape(-1)))
    put(SIMPLE_ZERO)
    px_vals = np.stack([cd[s] for cd, ln, s in tabs], axis=1).reshape(-1)
    px_lens = np.stack([ln[s] for cd, ln, s in tabs], axis=1).reshape(-1)
    all_vals = np.concatenate([np.array(head_vals, np.uint64), mode_vals, np.array(vals, np.uint64), px_vals])
    all_lens = np.concatenate([np.array(head_lens, np.int64), mode_lens, np.array(lens, np.int64), px_lens])
    return all_vals, all_lens, modes


def container(payload):
    pad = b"\0" if len(payload) & 1 else b""
    body = b"WEBP" + b"VP8L" + len(payload).to_bytes(4, "little") + payload + pad
    return b"RIFF" + len(body).to_bytes(4, "little") + body


def write(frame, forced_modes=None, tile_bits=TILE_BITS):
    vals, lens, _ = _stream(frame, forced_modes, tile_bits)
    payload, _ = _pack(vals, lens)
    return container(payload)


def file_size(frame, forced_modes=None, tile_bits=TILE_BITS):
    _, lens, _ = _stream(frame, forced_modes, tile_bits)
    n = (int(lens.sum()) + 7) // 8
    return 20 + n + (n & 1)


def chosen_modes(frame, tile_bits=TILE_BITS):
    """(tiles_y, tiles_x): what the chooser picks"""
    return choose_modes(subtract_green(argb_of(frame)), tile_bits)


def decode(blob):
    """Pillow's libwebp on the file -> (mode, HxWxC array in Pillow's channel order)"""
    import io

    from PIL import Image

    im = Image.open(io.BytesIO(blob))
    im.load()
    return im.mode, np.asarray(im)
