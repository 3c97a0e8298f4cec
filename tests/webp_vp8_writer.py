"""A model of the lossy WebP answer (include/impgpu.h, "LOSSY WEBP ANSWERS"), written from that paragraph alone: plain
Python and numpy, one macroblock after the other, no shared code with the library.  encode() returns the file and what the
encoder reconstructed, which is what a decoder must show; decoded_rgb() is libwebp's output conversion of those planes."""
from collections import namedtuple

import numpy as np

from webp_vp8_tables import AC_STEPS, COEF_PROBS, DC_STEPS, UPDATE_PROBS

ZIGZAG = (0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15)
BANDS = (0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7, 0)
CAT3, CAT4, CAT5 = (173, 148, 140), (176, 155, 140, 135), (180, 157, 141, 134, 130)
CAT6 = (254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129)
DC, V, H, TM = 0, 1, 2, 3
MAX_SIDE = 16383

Encoded = namedtuple("Encoded", "file y u v ymodes uvmodes levels nz skipped partitions")


def coef_prob(t, band, ctx, node):
    return COEF_PROBS[((t * 8 + band) * 3 + ctx) * 11 + node]


class BoolCoder:
    """RFC 6386 section 7.3, with its flush."""

    def __init__(self):
        self.out = bytearray()
        self.range, self.bottom, self.count = 255, 0, 24

    def _carry(self):
        i = len(self.out) - 1
        while i >= 0 and self.out[i] == 255:
            self.out[i] = 0
            i -= 1
        self.out[i] += 1

    def put(self, prob, bit):
        split = 1 + (((self.range - 1) * prob) >> 8)
        if bit:
            self.bottom += split
            self.range -= split
        else:
            self.range = split
        while self.range < 128:
            self.range <<= 1
            if self.bottom & (1 << 31):
                self._carry()
            self.bottom = (self.bottom << 1) & 0xFFFFFFFF
            self.count -= 1
            if not self.count:
                self.out.append(self.bottom >> 24)
                self.bottom &= (1 << 24) - 1
                self.count = 8

    def literal(self, value, bits):
        for i in range(bits - 1, -1, -1):
            self.put(128, (value >> i) & 1)

    def finish(self):
        c, v = self.count, self.bottom
        if v & (1 << (32 - c)):
            self._carry()
        v = (v << (c & 7)) & 0xFFFFFFFF
        for _ in range(c >> 3):
            v = (v << 8) & 0xFFFFFFFF
        for _ in range(4):
            self.out.append(v >> 24)
            v = (v << 8) & 0xFFFFFFFF
        return bytes(self.out)


def quant_index(quality):
    return 127 - (127 * quality + 50) // 100


def steps(qi):
    """(y dc, y ac, y2 dc, y2 ac, uv dc, uv ac)"""
    return (DC_STEPS[qi], AC_STEPS[qi], DC_STEPS[qi] * 2, max(8, AC_STEPS[qi] * 155 // 100), min(132, DC_STEPS[qi]), AC_STEPS[qi])


def planes(frame):
    """B,G,R(,A) or gray -> padded Y, U, V and the alpha plane (None without a fourth channel)"""
    a = np.asarray(frame)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, c = a.shape
    px = a.astype(np.int64)
    if c == 1:
        r = g = b = px[:, :, 0]
    else:
        b, g, r = px[:, :, 0], px[:, :, 1], px[:, :, 2]
    y = (16839 * r + 33059 * g + 6420 * b + (16 << 16) + (1 << 15)) >> 16
    he, we = h + (h & 1), w + (w & 1)

    def cells(p):
        q = np.pad(p, ((0, he - h), (0, we - w)), mode="edge")
        return q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2]

    rs, gs, bs = cells(r), cells(g), cells(b)
    u = np.clip((-9719 * rs - 19081 * gs + 28800 * bs + (128 << 18) + (1 << 17)) >> 18, 0, 255)
    v = np.clip((28800 * rs - 24116 * gs - 4684 * bs + (128 << 18) + (1 << 17)) >> 18, 0, 255)
    mw, mh = (w + 15) // 16, (h + 15) // 16
    y = np.pad(y, ((0, mh * 16 - h), (0, mw * 16 - w)), mode="edge")
    u = np.pad(u, ((0, mh * 8 - u.shape[0]), (0, mw * 8 - u.shape[1])), mode="edge")
    v = np.pad(v, ((0, mh * 8 - v.shape[0]), (0, mw * 8 - v.shape[1])), mode="edge")
    alpha = a[:, :, 3].astype(np.uint8) if c == 4 else None
    return y, u, v, alpha


def fdct(d):
    """d: 4x4 differences -> 16 coefficients in raster order"""
    tmp = [0] * 16
    for i in range(4):
        d0, d1, d2, d3 = (int(x) for x in d[i])
        a0, a1, a2, a3 = d0 + d3, d1 + d2, d1 - d2, d0 - d3
        tmp[i * 4] = (a0 + a1) * 8
        tmp[i * 4 + 1] = (a2 * 2217 + a3 * 5352 + 1812) >> 9
        tmp[i * 4 + 2] = (a0 - a1) * 8
        tmp[i * 4 + 3] = (a3 * 2217 - a2 * 5352 + 937) >> 9
    out = [0] * 16
    for i in range(4):
        a0, a1 = tmp[i] + tmp[12 + i], tmp[4 + i] + tmp[8 + i]
        a2, a3 = tmp[4 + i] - tmp[8 + i], tmp[i] - tmp[12 + i]
        out[i] = (a0 + a1 + 7) >> 4
        out[4 + i] = ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (1 if a3 != 0 else 0)
        out[8 + i] = (a0 - a1 + 7) >> 4
        out[12 + i] = (a3 * 2217 - a2 * 5352 + 51000) >> 16
    return out


def fwht(dc):
    tmp = [0] * 16
    for i in range(4):
        i0, i1, i2, i3 = dc[i * 4:i * 4 + 4]
        a0, a1, a2, a3 = i0 + i2, i1 + i3, i1 - i3, i0 - i2
        tmp[i * 4:i * 4 + 4] = [a0 + a1, a3 + a2, a3 - a2, a0 - a1]
    out = [0] * 16
    for i in range(4):
        a0, a1 = tmp[i] + tmp[8 + i], tmp[4 + i] + tmp[12 + i]
        a2, a3 = tmp[4 + i] - tmp[12 + i], tmp[i] - tmp[8 + i]
        out[i], out[4 + i], out[8 + i], out[12 + i] = (a0 + a1) >> 1, (a3 + a2) >> 1, (a3 - a2) >> 1, (a0 - a1) >> 1
    return out


def _m1(a):
    return ((a * 20091) >> 16) + a


def _m2(a):
    return (a * 35468) >> 16


def idct(c):
    """16 coefficients -> 4x4 residual (rows)"""
    tmp = [0] * 16
    for i in range(4):
        a, b = c[i] + c[8 + i], c[i] - c[8 + i]
        cc, d = _m2(c[4 + i]) - _m1(c[12 + i]), _m1(c[4 + i]) + _m2(c[12 + i])
        tmp[4 * i:4 * i + 4] = [a + d, b + cc, b - cc, a - d]
    out = [[0] * 4 for _ in range(4)]
    for i in range(4):
        dc = tmp[i] + 4
        a, b = dc + tmp[8 + i], dc - tmp[8 + i]
        cc, d = _m2(tmp[4 + i]) - _m1(tmp[12 + i]), _m1(tmp[4 + i]) + _m2(tmp[12 + i])
        out[i] = [(a + d) >> 3, (b + cc) >> 3, (b - cc) >> 3, (a - d) >> 3]
    return out


def iwht(c):
    tmp = [0] * 16
    for i in range(4):
        a0, a1 = c[i] + c[12 + i], c[4 + i] + c[8 + i]
        a2, a3 = c[4 + i] - c[8 + i], c[i] - c[12 + i]
        tmp[i], tmp[8 + i], tmp[4 + i], tmp[12 + i] = a0 + a1, a0 - a1, a3 + a2, a3 - a2
    out = [0] * 16
    for i in range(4):
        dc = tmp[i * 4] + 3
        a0, a1 = dc + tmp[i * 4 + 3], tmp[i * 4 + 1] + tmp[i * 4 + 2]
        a2, a3 = tmp[i * 4 + 1] - tmp[i * 4 + 2], dc - tmp[i * 4 + 3]
        out[i * 4:i * 4 + 4] = [(a0 + a1) >> 3, (a3 + a2) >> 3, (a0 - a1) >> 3, (a3 - a2) >> 3]
    return out


def quantise(c, q):
    m = min(2047, (abs(c) + q // 2) // q)
    return -m if c < 0 else m


def predictions(top, left, tl, n, have_top, have_left):
    """the four n x n predictions from the n samples above, the n to the left and the corner"""
    if have_top and have_left:
        dc = (int(top.sum()) + int(left.sum()) + n) >> (5 if n == 16 else 4)
    elif have_top:
        dc = (int(top.sum()) + n // 2) >> (4 if n == 16 else 3)
    elif have_left:
        dc = (int(left.sum()) + n // 2) >> (4 if n == 16 else 3)
    else:
        dc = 128
    return (np.full((n, n), dc, np.int64), np.tile(top, (n, 1)), np.tile(left[:, None], (1, n)),
            np.clip(top[None, :] + left[:, None] - tl, 0, 255))


def neighbours(rec, mx, my, n):
    top = rec[my * n - 1, mx * n:mx * n + n] if my else np.full(n, 127, np.int64)
    left = rec[my * n:my * n + n, mx * n - 1] if mx else np.full(n, 129, np.int64)
    if my == 0:
        tl = 127
    elif mx == 0:
        tl = 129
    else:
        tl = int(rec[my * n - 1, mx * n - 1])
    return top, left, tl


def block_tokens(put, coefs, t, ctx, first):
    """one block's tokens; coefs in zigzag order; -> whether a coefficient was coded"""
    last = -1
    for i in range(15, first - 1, -1):
        if coefs[i]:
            last = i
            break
    n = first
    ctx_now = ctx
    put(coef_prob(t, BANDS[n], ctx_now, 0), 1 if last >= n else 0)
    if last < n:
        return 0
    while n < 16:
        c = coefs[n]
        b = BANDS[n]
        n += 1
        v = abs(c)
        if not v:
            put(coef_prob(t, b, ctx_now, 1), 0)
            ctx_now = 0
            continue
        put(coef_prob(t, b, ctx_now, 1), 1)
        if v == 1:
            put(coef_prob(t, b, ctx_now, 2), 0)
            nxt = 1
        else:
            put(coef_prob(t, b, ctx_now, 2), 1)
            pr = lambda node: coef_prob(t, b, ctx_now, node)
            if v <= 4:
                put(pr(3), 0)
                if v == 2:
                    put(pr(4), 0)
                else:
                    put(pr(4), 1)
                    put(pr(5), 1 if v == 4 else 0)
            elif v <= 10:
                put(pr(3), 1)
                put(pr(6), 0)
                if v <= 6:
                    put(pr(7), 0)
                    put(159, 1 if v == 6 else 0)
                else:
                    put(pr(7), 1)
                    put(165, 1 if v >= 9 else 0)
                    put(145, 0 if v & 1 else 1)
            else:
                put(pr(3), 1)
                put(pr(6), 1)
                if v < 19:
                    put(pr(8), 0), put(pr(9), 0)
                    extra, tab = v - 11, CAT3
                elif v < 35:
                    put(pr(8), 0), put(pr(9), 1)
                    extra, tab = v - 19, CAT4
                elif v < 67:
                    put(pr(8), 1), put(pr(10), 0)
                    extra, tab = v - 35, CAT5
                else:
                    put(pr(8), 1), put(pr(10), 1)
                    extra, tab = v - 67, CAT6
                for k, prob in enumerate(tab):
                    put(prob, (extra >> (len(tab) - 1 - k)) & 1)
            nxt = 2
        put(128, 1 if c < 0 else 0)
        ctx_now = nxt
        if n == 16:
            return 1
        put(coef_prob(t, BANDS[n], ctx_now, 0), 1 if n <= last else 0)
        if n > last:
            return 1
    return 1


def encode(frame, quality):
    a = np.asarray(frame)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, c = a.shape
    assert c in (1, 3, 4) and 1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE and 0 <= quality <= 100
    ysrc, usrc, vsrc, alpha = planes(a)
    mw, mh = (w + 15) // 16, (h + 15) // 16
    qy_dc, qy_ac, q2_dc, q2_ac, quv_dc, quv_ac = steps(quant_index(quality))
    yrec, urec, vrec = np.zeros_like(ysrc), np.zeros_like(usrc), np.zeros_like(vsrc)
    nmb = mw * mh
    ymodes, uvmodes = np.zeros(nmb, np.uint8), np.zeros(nmb, np.uint8)
    levels = np.zeros((nmb, 25, 16), np.int16)
    nz = np.zeros((nmb, 25), np.uint8)
    for my in range(mh):
        for mx in range(mw):
            mb = my * mw + mx
            # luma
            src = ysrc[my * 16:my * 16 + 16, mx * 16:mx * 16 + 16]
            top, left, tl = neighbours(yrec, mx, my, 16)
            preds = predictions(top, left, tl, 16, my > 0, mx > 0)
            costs = [int(((p - src) ** 2).sum()) for p in preds]
            ym = costs.index(min(costs))
            pred = preds[ym]
            coefs = [fdct(src[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] - pred[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4]) for by in range(4) for bx in range(4)]
            y2 = fwht([cf[0] for cf in coefs])
            l2 = [quantise(y2[i], q2_dc if i == 0 else q2_ac) for i in range(16)]
            levels[mb, 24] = l2
            dcs = iwht([l2[i] * (q2_dc if i == 0 else q2_ac) for i in range(16)])
            for b in range(16):
                lv = [0] + [quantise(coefs[b][i], qy_ac) for i in range(1, 16)]
                levels[mb, b] = lv
                res = idct([dcs[b]] + [lv[i] * qy_ac for i in range(1, 16)])
                by, bx = b // 4, b % 4
                yrec[my * 16 + by * 4:my * 16 + by * 4 + 4, mx * 16 + bx * 4:mx * 16 + bx * 4 + 4] = np.clip(
                    pred[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] + np.array(res), 0, 255)
            # chroma: one mode for both planes
            both = []
            for srcp, recp in ((usrc, urec), (vsrc, vrec)):
                s = srcp[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8]
                t, l, c0 = neighbours(recp, mx, my, 8)
                both.append((s, predictions(t, l, c0, 8, my > 0, mx > 0)))
            costs = [sum(int(((pp[m] - s) ** 2).sum()) for s, pp in both) for m in range(4)]
            um = costs.index(min(costs))
            for k, (recp, (s, pp)) in enumerate(zip((urec, vrec), both)):
                pred = pp[um]
                for b in range(4):
                    by, bx = b // 2, b % 2
                    cf = fdct(s[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] - pred[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4])
                    lv = [quantise(cf[i], quv_dc if i == 0 else quv_ac) for i in range(16)]
                    levels[mb, 16 + 4 * k + b] = lv
                    res = idct([lv[i] * (quv_dc if i == 0 else quv_ac) for i in range(16)])
                    recp[my * 8 + by * 4:my * 8 + by * 4 + 4, mx * 8 + bx * 4:mx * 8 + bx * 4 + 4] = np.clip(
                        pred[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] + np.array(res), 0, 255)
            ymodes[mb], uvmodes[mb] = ym, um
            for b in range(25):
                nz[mb, b] = 1 if np.any(levels[mb, b]) else 0
    skipped = np.array([0 if nz[mb].any() else 1 for mb in range(nmb)], np.uint8)
    # token partitions
    nparts = max(p for p in (1, 2, 4, 8) if p <= mh)
    coders = [BoolCoder() for _ in range(nparts)]
    for my in range(mh):
        put = coders[my % nparts].put
        for mx in range(mw):
            mb = my * mw + mx
            if skipped[mb]:
                continue
            lf = nz[mb - 1] if mx else np.zeros(25, np.uint8)
            up = nz[mb - mw] if my else np.zeros(25, np.uint8)
            zz = lambda b: [int(levels[mb, b, ZIGZAG[i]]) for i in range(16)]
            got = block_tokens(put, zz(24), 1, int(lf[24]) + int(up[24]), 0)
            assert got == nz[mb, 24]
            for b in range(16):
                bx, by = b % 4, b // 4
                l = nz[mb, b - 1] if bx else lf[b + 3]
                t = nz[mb, b - 4] if by else up[b + 12]
                assert block_tokens(put, zz(b), 0, int(l) + int(t), 1) == nz[mb, b]
            for base in (16, 20):
                for b in range(4):
                    bx, by = b % 2, b // 2
                    l = nz[mb, base + b - 1] if bx else lf[base + b + 1]
                    t = nz[mb, base + b - 2] if by else up[base + b + 2]
                    assert block_tokens(put, zz(base + b), 2, int(l) + int(t), 0) == nz[mb, base + b]
    parts = [cd.finish() for cd in coders]
    # the first partition
    hd = BoolCoder()
    hd.literal(0, 1)                                        # colour space
    hd.literal(0, 1)                                        # clamping type
    hd.literal(0, 1)                                        # no segmentation
    hd.literal(0, 1)                                        # filter type
    hd.literal(0, 6)                                        # filter level
    hd.literal(0, 3)                                        # sharpness
    hd.literal(0, 1)                                        # no filter deltas
    hd.literal({1: 0, 2: 1, 4: 2, 8: 3}[nparts], 2)
    hd.literal(quant_index(quality), 7)
    for _ in range(5):
        hd.literal(0, 1)                                    # no quantiser delta
    hd.literal(0, 1)                                        # refresh_entropy_probs
    for p in UPDATE_PROBS:
        hd.put(p, 0)
    hd.literal(1, 1)                                        # mb_no_coeff_skip
    nskip = int(skipped.sum())
    pskip = min(255, max(1, (256 * (nmb - nskip) + nmb // 2) // nmb))
    hd.literal(pskip, 8)
    for mb in range(nmb):
        hd.put(pskip, int(skipped[mb]))
        hd.put(145, 1)                                      # not B_PRED
        m = ymodes[mb]
        hd.put(156, 1 if m in (H, TM) else 0)
        if m in (H, TM):
            hd.put(128, 1 if m == TM else 0)
        else:
            hd.put(163, 1 if m == V else 0)
        m = uvmodes[mb]
        hd.put(142, 0 if m == DC else 1)
        if m != DC:
            hd.put(114, 0 if m == V else 1)
            if m != V:
                hd.put(183, 1 if m == TM else 0)
    first = hd.finish()
    tag = 0 | (0 << 1) | (1 << 4) | (len(first) << 5)
    vp8 = bytes([tag & 255, (tag >> 8) & 255, (tag >> 16) & 255, 0x9D, 0x01, 0x2A, w & 255, w >> 8, h & 255, h >> 8]) + first
    for p in parts[:-1]:
        vp8 += bytes([len(p) & 255, (len(p) >> 8) & 255, (len(p) >> 16) & 255])
    vp8 += b"".join(parts)

    def chunk(name, body):
        return name + len(body).to_bytes(4, "little") + body + (b"\0" if len(body) & 1 else b"")

    body = b""
    if alpha is not None and not np.all(alpha == 255):
        body += chunk(b"VP8X", bytes([0x10, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little"))
        body += chunk(b"ALPH", b"\0" + alpha.tobytes())
    body += chunk(b"VP8 ", vp8)
    data = b"RIFF" + (4 + len(body)).to_bytes(4, "little") + b"WEBP" + body
    return Encoded(data, yrec.astype(np.uint8), urec.astype(np.uint8), vrec.astype(np.uint8), ymodes, uvmodes, levels, nz, skipped, parts)


def _mh(a, c):
    return (a * c) >> 8


def decoded_rgb(y, u, v, w, h):
    """libwebp's output conversion of decoded planes: fancy upsampling, then its fixed-point YUV -> RGB"""
    y = y[:h, :w].astype(np.int64)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    out = []
    for p in (u, v):
        p = p[:ch, :cw].astype(np.int64)
        q = np.pad(p, 1, mode="edge")                       # q[i + 1, j + 1] = p[i, j]
        full = np.zeros((2 * ch, 2 * cw), np.int64)
        for dy in (0, 1):
            for dx in (0, 1):
                near = q[1:-1, 1:-1]
                vert = q[0:-2, 1:-1] if dy == 0 else q[2:, 1:-1]
                horz = q[1:-1, 0:-2] if dx == 0 else q[1:-1, 2:]
                diag = q[0 if dy == 0 else 2:(-2 if dy == 0 else None), 0 if dx == 0 else 2:(-2 if dx == 0 else None)]
                full[dy::2, dx::2] = (9 * near + 3 * vert + 3 * horz + diag + 8) >> 4
        out.append(full[:h, :w])
    uu, vv = out
    r = np.clip((_mh(y, 19077) + _mh(vv, 26149) - 14234) >> 6, 0, 255)
    g = np.clip((_mh(y, 19077) - _mh(uu, 6419) - _mh(vv, 13320) + 8708) >> 6, 0, 255)
    b = np.clip((_mh(y, 19077) + _mh(uu, 33050) - 17685) >> 6, 0, 255)
    return np.stack([r, g, b], axis=2).astype(np.uint8)
