"""Writes tests/golden/webp_lossy_dec: the lossy WebP decoder's fixtures.  Run it as a script; Pillow's libwebp judges every
file (the expected frames in expected.npz are its mode-RGB decodes, and the verdicts of the truncated files are recorded in
verdicts.json, which webp_lossy_dec_fixtures.py loads).

Pillow-encoded files (p_*) only ever have one partition, the normal filter, sharpness 0, no lf deltas and segments with a
map update and absolute values; the hand-written files (h_*, s_* for the kernels' seams) exist because of that.  Stream is
a writer for any VP8 key frame: it imports webp_vp8_writer's boolean coder and tables and adds what that writer lacks --
segments, filter header, lf deltas, quantiser deltas, probability updates, B_PRED, any partition count, any token."""
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from webp_vp8_tables import COEF_PROBS, UPDATE_PROBS  # noqa: E402
from webp_vp8_writer import BANDS, CAT3, CAT4, CAT5, CAT6, BoolCoder  # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "webp_lossy_dec")
DC, TM, VE, HE, RD, VR, LD, VL, HD, HU = range(10)                 # libwebp's order: the first four are the 16x16 / chroma modes too
BPRED = "B"
# RFC 6386 section 11.5: kf_bmode_probs [above][left][node]
BMODE_PROBS = (
    231,120,48,89,115,113,120,152,112,152,179,64,126,170,118,46,70,95,175,69,143,80,85,82,72,155,103,56,58,10,
    171,218,189,17,13,152,114,26,17,163,44,195,21,10,173,121,24,80,195,26,62,44,64,85,144,71,10,38,171,213,
    144,34,26,170,46,55,19,136,160,33,206,71,63,20,8,114,114,208,12,9,226,81,40,11,96,182,84,29,16,36,
    134,183,89,137,98,101,106,165,148,72,187,100,130,157,111,32,75,80,66,102,167,99,74,62,40,234,128,41,53,9,
    178,241,141,26,8,107,74,43,26,146,73,166,49,23,157,65,38,105,160,51,52,31,115,128,104,79,12,27,217,255,
    87,17,7,87,68,71,44,114,51,15,186,23,47,41,14,110,182,183,21,17,194,66,45,25,102,197,189,23,18,22,
    88,88,147,150,42,46,45,196,205,43,97,183,117,85,38,35,179,61,39,53,200,87,26,21,43,232,171,56,34,51,
    104,114,102,29,93,77,39,28,85,171,58,165,90,98,64,34,22,116,206,23,34,43,166,73,107,54,32,26,51,1,
    81,43,31,68,25,106,22,64,171,36,225,114,34,19,21,102,132,188,16,76,124,62,18,78,95,85,57,50,48,51,
    193,101,35,159,215,111,89,46,111,60,148,31,172,219,228,21,18,111,112,113,77,85,179,255,38,120,114,40,42,1,
    196,245,209,10,25,109,88,43,29,140,166,213,37,43,154,61,63,30,155,67,45,68,1,209,100,80,8,43,154,1,
    51,26,71,142,78,78,16,255,128,34,197,171,41,40,5,102,211,183,4,1,221,51,50,17,168,209,192,23,25,82,
    138,31,36,171,27,166,38,44,229,67,87,58,169,82,115,26,59,179,63,59,90,180,59,166,93,73,154,40,40,21,
    116,143,209,34,39,175,47,15,16,183,34,223,49,45,183,46,17,33,183,6,98,15,32,183,57,46,22,24,128,1,
    54,17,37,65,32,73,115,28,128,23,128,205,40,3,9,115,51,192,18,6,223,87,37,9,115,59,77,64,21,47,
    104,55,44,218,9,54,53,130,226,64,90,70,205,40,41,23,26,57,54,57,112,184,5,41,38,166,213,30,34,26,
    133,152,116,10,32,134,39,19,53,221,26,114,32,73,255,31,9,65,234,2,15,1,118,73,75,32,12,51,192,255,
    160,43,51,88,31,35,67,102,85,55,186,85,56,21,23,111,59,205,45,37,192,55,38,70,124,73,102,1,34,98,
    125,98,42,88,104,85,117,175,82,95,84,53,89,128,100,113,101,45,75,79,123,47,51,128,81,171,1,57,17,5,
    71,102,57,53,41,49,38,33,13,121,57,73,26,1,85,41,10,67,138,77,110,90,47,114,115,21,2,10,102,255,
    166,23,6,101,29,16,10,85,128,101,196,26,57,18,10,102,102,213,34,20,43,117,20,15,36,163,128,68,1,26,
    102,61,71,37,34,53,31,243,192,69,60,71,38,73,119,28,222,37,68,45,128,34,1,47,11,245,171,62,17,19,
    70,146,85,55,62,70,37,43,37,154,100,163,85,160,1,63,9,92,136,28,64,32,201,85,75,15,9,9,64,255,
    184,119,16,86,6,28,5,64,255,25,248,1,56,8,17,132,137,255,55,116,128,58,15,20,82,135,57,26,121,40,
    164,50,31,137,154,133,25,35,218,51,103,44,131,131,123,31,6,158,86,40,64,135,148,224,45,183,128,22,26,17,
    131,240,154,14,1,209,45,16,21,91,64,222,7,1,197,56,21,39,155,60,138,23,102,213,83,12,13,54,192,255,
    68,47,28,85,26,85,85,128,128,32,146,171,18,11,7,63,144,171,4,4,246,35,27,10,146,174,171,12,26,128,
    190,80,35,99,180,80,126,54,45,85,126,47,87,176,51,41,20,32,101,75,128,139,118,146,116,128,85,56,41,15,
    176,236,85,37,9,62,71,30,17,119,118,255,17,18,138,101,38,60,138,55,70,43,26,142,146,36,19,30,171,255,
    97,27,20,138,45,61,62,219,1,81,188,64,32,41,20,117,151,142,20,21,163,112,19,12,61,195,128,48,4,24
)


def put_signed(bc, v, bits):
    bc.literal(abs(v), bits)
    bc.literal(1 if v < 0 else 0, 1)


def put_opt_signed(bc, v, bits):
    bc.literal(1 if v else 0, 1)
    if v:
        put_signed(bc, v, bits)


def block_tokens(put, prob, coefs, t, ctx, first):
    """one block (coefs in zigzag order) with the probabilities prob[t][band][ctx][node] -> whether a token was coded"""
    last = -1
    for i in range(15, first - 1, -1):
        if coefs[i]:
            last = i
            break
    n = first
    p = lambda node: prob[((t * 8 + BANDS[n]) * 3 + ctx) * 11 + node]
    put(p(0), 1 if last >= n else 0)
    if last < n:
        return 0
    while n < 16:
        c = coefs[n]
        v = abs(c)
        if not v:
            put(p(1), 0)
            n += 1
            ctx = 0
            continue
        put(p(1), 1)
        if v == 1:
            put(p(2), 0)
            nxt = 1
        else:
            put(p(2), 1)
            if v <= 4:
                put(p(3), 0)
                if v == 2:
                    put(p(4), 0)
                else:
                    put(p(4), 1)
                    put(p(5), 1 if v == 4 else 0)
            elif v <= 10:
                put(p(3), 1)
                put(p(6), 0)
                if v <= 6:
                    put(p(7), 0)
                    put(159, 1 if v == 6 else 0)
                else:
                    put(p(7), 1)
                    put(165, 1 if v >= 9 else 0)
                    put(145, 0 if v & 1 else 1)
            else:
                put(p(3), 1)
                put(p(6), 1)
                if v < 19:
                    put(p(8), 0), put(p(9), 0)
                    extra, tab = v - 11, CAT3
                elif v < 35:
                    put(p(8), 0), put(p(9), 1)
                    extra, tab = v - 19, CAT4
                elif v < 67:
                    put(p(8), 1), put(p(10), 0)
                    extra, tab = v - 35, CAT5
                else:
                    put(p(8), 1), put(p(10), 1)
                    extra, tab = v - 67, CAT6
                    assert extra < 2048
                for k, pr in enumerate(tab):
                    put(pr, (extra >> (len(tab) - 1 - k)) & 1)
            nxt = 2
        put(128, 1 if c < 0 else 0)
        n += 1
        ctx = nxt
        if n == 16:
            return 1
        put(p(0), 1 if n <= last else 0)
        if n > last:
            return 1
    return 1


class Stream:
    """A VP8 key frame.  mbs: one dict a macroblock in raster order: ymode (DC, TM, VE, HE or BPRED), bmodes (16, with BPRED),
    uvmode, segment, skip (coded only with skip_prob), coefs: 25 blocks x 16 levels in zigzag order (16 Y, 4 U, 4 V, Y2; with
    a 16x16 mode the Y blocks' first level is not coded)."""

    def __init__(self, w, h, mbs, **kw):
        self.w, self.h, self.mbs = w, h, mbs
        self.version = kw.get("version", 0)
        self.colorspace, self.clamp = kw.get("colorspace", 0), kw.get("clamp", 0)
        self.xscale, self.yscale = kw.get("xscale", 0), kw.get("yscale", 0)
        self.segments = kw.get("segments")         # None or dict(update_map, update_data, absolute, quant[4], lf[4], probs[3])
        self.simple, self.level, self.sharpness = kw.get("simple", 0), kw.get("level", 0), kw.get("sharpness", 0)
        self.lf_delta = kw.get("lf_delta")         # None or dict(update, ref[4], mode[4])
        self.nparts = kw.get("nparts", 1)
        self.base_q, self.dq = kw.get("base_q", 40), kw.get("dq", (0, 0, 0, 0, 0))
        self.prob_updates = kw.get("prob_updates", {})      # index into the 1056 -> value
        self.skip_prob = kw.get("skip_prob", 128)  # None: mb_no_coeff_skip 0
        self.show, self.key = kw.get("show", 1), kw.get("key", 1)
        self.start = kw.get("start", b"\x9d\x01\x2a")

    def payload(self):
        mw, mh = (self.w + 15) // 16, (self.h + 15) // 16
        assert len(self.mbs) == mw * mh
        prob = list(COEF_PROBS)
        for i, v in self.prob_updates.items():
            prob[i] = v
        hd = BoolCoder()
        hd.literal(self.colorspace, 1)
        hd.literal(self.clamp, 1)
        sg = self.segments
        hd.literal(1 if sg else 0, 1)
        update_map = 0
        if sg:
            update_map = sg.get("update_map", 1)
            hd.literal(update_map, 1)
            hd.literal(sg.get("update_data", 1), 1)
            if sg.get("update_data", 1):
                hd.literal(sg.get("absolute", 1), 1)
                for v in sg["quant"]:
                    put_opt_signed(hd, v, 7)
                for v in sg["lf"]:
                    put_opt_signed(hd, v, 6)
            if update_map:
                for v in sg["probs"]:
                    hd.literal(0 if v == 255 else 1, 1)
                    if v != 255:
                        hd.literal(v, 8)
        hd.literal(self.simple, 1)
        hd.literal(self.level, 6)
        hd.literal(self.sharpness, 3)
        ld = self.lf_delta
        hd.literal(1 if ld else 0, 1)
        if ld:
            hd.literal(ld.get("update", 1), 1)
            if ld.get("update", 1):
                for v in ld["ref"]:
                    put_opt_signed(hd, v, 6)
                for v in ld["mode"]:
                    put_opt_signed(hd, v, 6)
        hd.literal({1: 0, 2: 1, 4: 2, 8: 3}[self.nparts], 2)
        hd.literal(self.base_q, 7)
        for v in self.dq:
            put_opt_signed(hd, v, 4)
        hd.literal(0, 1)                                   # refresh_entropy_probs
        for i, p in enumerate(UPDATE_PROBS):
            if i in self.prob_updates:
                hd.put(p, 1)
                hd.literal(self.prob_updates[i], 8)
            else:
                hd.put(p, 0)
        hd.literal(0 if self.skip_prob is None else 1, 1)
        if self.skip_prob is not None:
            hd.literal(self.skip_prob, 8)
        coders = [BoolCoder() for _ in range(self.nparts)]
        top_modes = [[DC] * 4 for _ in range(mw)]
        top_nz = [[0] * 9 for _ in range(mw)]              # 4 Y, 2 U, 2 V, Y2
        for my in range(mh):
            left_modes, left_nz = [DC] * 4, [0] * 9
            put = coders[my % self.nparts].put
            for mx in range(mw):
                mb = self.mbs[my * mw + mx]
                # the first partition
                if update_map:
                    s, pr = mb.get("segment", 0), sg["probs"]
                    hd.put(pr[0], s >> 1)
                    hd.put(pr[1 + (s >> 1)], s & 1)
                skip = bool(mb.get("skip", 0)) and self.skip_prob is not None
                if self.skip_prob is not None:
                    hd.put(self.skip_prob, 1 if skip else 0)
                ym = mb["ymode"]
                hd.put(145, 0 if ym == BPRED else 1)
                if ym != BPRED:
                    hd.put(156, 1 if ym in (TM, HE) else 0)
                    if ym in (TM, HE):
                        hd.put(128, 1 if ym == TM else 0)
                    else:
                        hd.put(163, 1 if ym == VE else 0)
                    top_modes[mx] = [ym] * 4
                    left_modes = [ym] * 4
                else:
                    for y in range(4):
                        for x in range(4):
                            m = mb["bmodes"][4 * y + x]
                            pb = BMODE_PROBS[(top_modes[mx][x] * 10 + left_modes[y]) * 9:][:9]
                            path = {DC: [(0, 0)], TM: [(0, 1), (1, 0)], VE: [(0, 1), (1, 1), (2, 0)],
                                    HE: [(0, 1), (1, 1), (2, 1), (3, 0), (4, 0)], RD: [(0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 0)],
                                    VR: [(0, 1), (1, 1), (2, 1), (3, 0), (4, 1), (5, 1)], LD: [(0, 1), (1, 1), (2, 1), (3, 1), (6, 0)],
                                    VL: [(0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 0)], HD: [(0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 1), (8, 0)],
                                    HU: [(0, 1), (1, 1), (2, 1), (3, 1), (6, 1), (7, 1), (8, 1)]}[m]
                            for node, bit in path:
                                hd.put(pb[node], bit)
                            top_modes[mx][x] = m
                            left_modes[y] = m
                um = mb.get("uvmode", DC)
                hd.put(142, 0 if um == DC else 1)
                if um != DC:
                    hd.put(114, 0 if um == VE else 1)
                    if um != VE:
                        hd.put(183, 1 if um == TM else 0)
                # the tokens
                tn = top_nz[mx]
                if skip:
                    for k in range(8):
                        tn[k] = left_nz[k] = 0
                    if ym != BPRED:
                        tn[8] = left_nz[8] = 0
                    continue
                cf = mb["coefs"]
                if ym != BPRED:
                    tn[8] = left_nz[8] = block_tokens(put, prob, cf[24], 1, tn[8] + left_nz[8], 0)
                    t, first = 0, 1
                else:
                    t, first = 3, 0
                for y in range(4):
                    for x in range(4):
                        tn[x] = left_nz[y] = block_tokens(put, prob, cf[4 * y + x], t, tn[x] + left_nz[y], first)
                for base, o in ((16, 4), (20, 6)):
                    for y in range(2):
                        for x in range(2):
                            tn[o + x] = left_nz[o + y] = block_tokens(put, prob, cf[base + 2 * y + x], 2, tn[o + x] + left_nz[o + y], 0)
        first = hd.finish()
        self.parts = [c.finish() for c in coders]
        tag = (0 if self.key else 1) | (self.version << 1) | (self.show << 4) | (len(first) << 5)
        out = bytes([tag & 255, (tag >> 8) & 255, (tag >> 16) & 255]) + self.start
        wv, hv = self.w | (self.xscale << 14), self.h | (self.yscale << 14)
        out += bytes([wv & 255, wv >> 8, hv & 255, hv >> 8]) + first
        for p in self.parts[:-1]:
            out += len(p).to_bytes(3, "little")
        return out + b"".join(self.parts)


def chunk(name, body):
    return name + len(body).to_bytes(4, "little") + body + (b"\0" if len(body) & 1 else b"")


def riff(*chunks):
    body = b"".join(chunks)
    return b"RIFF" + (4 + len(body)).to_bytes(4, "little") + b"WEBP" + body


def container(payload):
    return riff(chunk(b"VP8 ", payload))


def vp8_payload(blob):
    """the VP8 chunk's payload of a file written by container() or by Pillow (the chunk may sit behind VP8X)"""
    at = 12
    while at + 8 <= len(blob):
        n = int.from_bytes(blob[at + 4:at + 8], "little")
        if blob[at:at + 4] == b"VP8 ":
            return blob[at + 8:at + 8 + n]
        at += 8 + n + (n & 1)
    raise ValueError("no VP8 chunk")


def cut(blob, nbytes, where="last"):
    """the file with nbytes cut off the end of its last partition (the chunk's end) or of its first, sizes rewritten"""
    p = vp8_payload(blob)
    if where == "last":
        return container(p[:len(p) - nbytes])
    tag = p[0] | p[1] << 8 | p[2] << 16
    first = tag >> 5
    tag = (tag & 31) | ((first - nbytes) << 5)
    return container(bytes([tag & 255, (tag >> 8) & 255, (tag >> 16) & 255]) + p[3:10 + first - nbytes] + p[10 + first:])


# ---------------------------------------------------------------- seeded content
def rand_block(rng, first, density, big):
    c = [0] * 16
    for i in range(first, 16):
        if rng.random() < density / (1 + i * 0.35):
            v = int(rng.integers(1, big + 1))
            c[i] = -v if rng.random() < 0.5 else v
    return c


def rand_mb(rng, ymodes=(DC, TM, VE, HE, BPRED), uvmodes=(DC, TM, VE, HE), bmodes=tuple(range(10)), density=0.5, big=6, skip=0.0, segments=1):
    ym = ymodes[int(rng.integers(len(ymodes)))]
    mb = {"ymode": ym, "uvmode": uvmodes[int(rng.integers(len(uvmodes)))], "segment": int(rng.integers(segments)),
          "skip": 1 if rng.random() < skip else 0}
    if ym == BPRED:
        mb["bmodes"] = [bmodes[int(rng.integers(len(bmodes)))] for _ in range(16)]
    first = 0 if ym == BPRED else 1
    mb["coefs"] = [rand_block(rng, first, density, big) for _ in range(16)] + [rand_block(rng, 0, density, big) for _ in range(8)] + [rand_block(rng, 0, density, big)]
    return mb


def rand_frame(seed, w, h, **kw):
    rng = np.random.default_rng(seed)
    mbkw = {k: kw.pop(k) for k in ("ymodes", "uvmodes", "bmodes", "density", "big", "skip") if k in kw}
    if kw.get("segments") and kw["segments"].get("update_map", 1):
        mbkw["segments"] = 4
    n = ((w + 15) // 16) * ((h + 15) // 16)
    return Stream(w, h, [rand_mb(rng, **mbkw) for _ in range(n)], **kw)


def pillow_frames():
    """seeded source frames: photo-like, flat, dithered, screenshot-like"""
    def make(kind, w, h, seed):
        rng = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:h, 0:w]
        if kind == "photo":
            a = np.stack([128 + 90 * np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0), 128 + 80 * np.sin((xx + yy) / 11.0), 100 + 0.8 * xx + 0.5 * yy], 2)
            a = a + rng.normal(0, 6, (h, w, 3))
        elif kind == "flat":
            a = np.broadcast_to(np.array([200, 30, 90]), (h, w, 3))
        elif kind == "dither":
            a = np.stack([(xx * 3 + yy * 2) % 256, (xx ^ yy) * 8 % 256, (xx + 2 * yy) % 256], 2) + rng.integers(-24, 24, (h, w, 3))
        else:
            a = np.full((h, w, 3), 245.0)
            a[(yy // 6) % 3 == 0] = (30, 30, 40)
            a[:, (xx[0] // 10) % 4 == 0] = (250, 250, 250)
            a[h // 3:h // 2, w // 4:w // 2] = (0, 120, 215)
        return np.clip(a, 0, 255).astype(np.uint8)
    return make


def hand_cases():
    """{name: Stream}"""
    C = {}
    # 16x16 and chroma modes at the corner, the top row, the left column and inside (TM among them)
    for m, nm in ((DC, "dc"), (TM, "tm"), (VE, "v"), (HE, "h")):
        C["h_mode16_%s" % nm] = rand_frame(100 + m, 48, 48, ymodes=(m,), uvmodes=(m,), big=12)
    # each sub-block mode at all 16 positions, in three columns and two rows of macroblocks (the rightmost ones read above-right)
    for m in range(10):
        C["h_bmode_%d" % m] = rand_frame(200 + m, 48, 32, ymodes=(BPRED,), bmodes=(m,), big=10)
    C["h_bmode_mix"] = rand_frame(211, 64, 48, ymodes=(BPRED,), density=0.7, big=20)
    C["h_bmode_ld_vl"] = rand_frame(212, 40, 40, ymodes=(BPRED,), bmodes=(LD, VL), density=0.8, big=30)
    # the filters
    C["h_simple_l20"] = rand_frame(300, 40, 40, simple=1, level=20, sharpness=0, big=20)
    C["h_simple_l63_s5"] = rand_frame(301, 40, 40, simple=1, level=63, sharpness=5, big=20)
    for lv in (1, 14, 15, 39, 40, 63):
        for sh in (0, 1, 4, 5, 7):
            C["h_normal_l%02d_s%d" % (lv, sh)] = rand_frame(310 + lv * 8 + sh, 40, 36, level=lv, sharpness=sh, big=16, skip=0.2, base_q=60)
    seg = dict(update_map=1, update_data=1, absolute=1, quant=(20, 50, 80, 110), lf=(10, 30, 50, 63), probs=(120, 80, 200))
    C["h_level0_segments"] = rand_frame(400, 48, 32, level=0, segments=seg, big=10)
    C["h_lfdelta_neg"] = rand_frame(401, 48, 32, level=6, lf_delta=dict(ref=(-20, 0, 0, 0), mode=(10, 0, 0, 0)), big=10)
    C["h_lfdelta_pos"] = rand_frame(402, 48, 32, level=50, lf_delta=dict(ref=(30, 5, -5, 1), mode=(-9, 2, 3, -4)), big=10)
    C["h_lfdelta_noupdate"] = rand_frame(403, 48, 32, level=30, sharpness=3, lf_delta=dict(update=0), big=10)
    C["h_lfdelta_bpred_only"] = rand_frame(404, 48, 32, level=8, lf_delta=dict(ref=(0, 0, 0, 0), mode=(40, 0, 0, 0)), big=10, skip=0.3)
    # the inner-edge rule: skipped 16x16 macroblocks beside B_PRED ones
    C["h_inner_edges"] = rand_frame(410, 64, 48, level=40, sharpness=0, skip=0.5, big=25, base_q=80)
    C["h_inner_edges_simple"] = rand_frame(411, 64, 48, simple=1, level=33, skip=0.5, big=25, base_q=80)
    # partitions on 1, 3, 8 and 9 rows
    for np_ in (2, 4, 8):
        for rows in (1, 3, 8, 9):
            C["h_parts%d_rows%d" % (np_, rows)] = rand_frame(500 + np_ * 16 + rows, 24, rows * 16 - 5, nparts=np_, level=12, skip=0.2)
    # segments
    C["h_seg_nomap"] = rand_frame(600, 40, 40, segments=dict(update_map=0, update_data=1, absolute=1, quant=(90, 5, 5, 5), lf=(25, 0, 0, 0)), level=9)
    C["h_seg_nodata"] = rand_frame(601, 40, 40, segments=dict(update_map=1, update_data=0, probs=(100, 100, 100)), level=9)
    C["h_seg_delta"] = rand_frame(602, 40, 40, segments=dict(update_map=1, absolute=0, quant=(-40, 30, 100, -100), lf=(-10, 20, 60, -60), probs=(128, 128, 128)), level=20)
    for i, pr in enumerate(((0, 128, 128), (255, 128, 128), (128, 0, 128), (128, 255, 128), (128, 128, 0), (128, 128, 255))):
        C["h_seg_tree%d" % i] = _tree_case(610 + i, pr)
    # quantiser deltas at +-15 on base index 0 and 127
    for k, nm in enumerate(("y1dc", "y2dc", "y2ac", "uvdc", "uvac")):
        for sign in (-15, 15):
            for base in (0, 127):
                dq = [0] * 5
                dq[k] = sign
                C["h_dq_%s_%s_q%d" % (nm, "m" if sign < 0 else "p", base)] = rand_frame(700 + k * 4 + (sign > 0) * 2 + (base > 0), 32, 32, base_q=base, dq=tuple(dq), big=8)
    # probability updates: every band of one type
    for t in range(4):
        rng = np.random.default_rng(800 + t)
        upd = {((t * 8 + b) * 3 + c) * 11 + k: int(rng.integers(1, 256)) for b in range(8) for c in range(3) for k in range(11)}
        C["h_probs_type%d" % t] = rand_frame(810 + t, 32, 32, prob_updates=upd, big=40, density=0.8)
    C["h_skip_off"] = rand_frame(900, 40, 24, skip_prob=None, level=10)
    # the largest DCT_CAT6 coefficient of either sign at the largest step
    for pos, nm in ((0, "dc"), (5, "ac"), (None, "y2")):
        for sign in (1, -1):
            C["h_cat6_%s_%s" % (nm, "p" if sign > 0 else "m")] = _cat6_case(pos, sign)
    C["h_last15"] = _shape_case(15)
    C["h_eob_only"] = _shape_case(None)
    for v in (1, 2, 3):
        C["h_version%d" % v] = rand_frame(950 + v, 40, 24, version=v, level=20, simple=v & 1)
    C["h_scale_bits"] = rand_frame(960, 40, 24, xscale=2, yscale=3, level=5)
    C["h_colour_clamp_bits"] = rand_frame(961, 40, 24, colorspace=1, clamp=1, level=5)
    # the implementation's seams: one and two macroblock columns against the filter's and the predictors' reach across
    # columns; many macroblock rows for the one-macroblock-at-a-time walks; the longest row and the longest column
    C["s_cols1"] = rand_frame(1000, 9, 70, level=30, big=12)
    C["s_cols2"] = rand_frame(1001, 25, 70, level=30, big=12)
    C["s_rows40"] = rand_frame(1002, 20, 16 * 40 - 3, level=22, nparts=8, big=8, skip=0.3)
    C["s_16383x1"] = rand_frame(1003, 16383, 1, level=18, big=8, skip=0.6, density=0.3)
    C["s_1x16383"] = rand_frame(1004, 1, 16383, level=18, nparts=4, big=8, skip=0.6, density=0.3)
    return C


def _tree_case(seed, probs):
    seg = dict(update_map=1, absolute=1, quant=(10, 60, 100, 127), lf=(5, 20, 40, 60), probs=probs)
    s = rand_frame(seed, 40, 40, segments=seg, level=15)
    for mb in s.mbs:                                       # a probability of 0 codes only the 1 branch, 255 is the default (not sent)
        sid = mb["segment"]
        if probs[0] == 0:
            sid |= 2
        if probs[1] == 0 and sid < 2:
            sid = 1
        if probs[2] == 0 and sid >= 2:
            sid = 3
        mb["segment"] = sid
    return s


def _cat6_case(pos, sign):
    s = rand_frame(970 + (pos or 20) + (sign > 0), 32, 32, base_q=127, dq=(15, 15, 15, 15, 15), big=3, density=0.2,
                   ymodes=(DC, BPRED) if pos is not None else (DC, TM))
    for i, mb in enumerate(s.mbs):
        if pos is None:
            mb["coefs"][24][i % 16] = sign * 2114
        elif mb["ymode"] == BPRED or pos > 0:
            mb["coefs"][i % 16][pos] = sign * 2114
        mb["coefs"][16 + i % 8][pos or 0] = -sign * 2114
    return s


def _shape_case(last):
    s = rand_frame(990 + (last or 0), 32, 32, level=10)
    for mb in s.mbs:
        for b in range(25):
            first = 1 if (b < 16 and mb["ymode"] != BPRED) else 0
            mb["coefs"][b] = [0] * 16
            if last is not None:
                mb["coefs"][b][last] = 1 + b % 3
                if b % 2:
                    mb["coefs"][b][first] = -2
    return s


# (fixture, bytes cut, from the last partition or the first)
CUTS = [(n, c, wh) for n in ("h_parts2_rows3", "p_photo_53x37_q50_m3", "h_bmode_mix") for wh in ("last", "first") for c in (1, 3, 4, "half")]


def main():
    from PIL import Image

    os.makedirs(HERE, exist_ok=True)
    for f in os.listdir(HERE):
        os.remove(os.path.join(HERE, f))
    files = {}
    make = pillow_frames()
    pairs = [(q, m) for q in (0, 10, 50, 75, 90, 100) for m in (0, 3, 6)]
    k = 0
    for size in ((1, 1), (15, 17), (16, 16), (17, 33), (53, 37), (160, 120)):
        for kind in ("photo", "flat", "dither", "screen"):
            for _ in range(1 if size == (160, 120) else 3):
                q, m = pairs[(k * 7) % 18]
                k += 1
                bio = io.BytesIO()
                Image.fromarray(make(kind, size[0], size[1], k)).save(bio, "WEBP", quality=q, method=m)
                files["p_%s_%dx%d_q%d_m%d" % (kind, size[0], size[1], q, m)] = bio.getvalue()
    bio = io.BytesIO()
    Image.fromarray(make("photo", 53, 37, 999)).save(bio, "WEBP", quality=50, method=3)
    files["p_photo_53x37_q50_m3"] = bio.getvalue()
    # the same image inside VP8X with skipped chunks around it
    p = vp8_payload(files["p_photo_53x37_q50_m3"])
    files["h_vp8x_chunks"] = riff(chunk(b"VP8X", bytes([0x2c, 0, 0, 0]) + (52).to_bytes(3, "little") + (36).to_bytes(3, "little")),
                                   chunk(b"ICCP", b"icc"), chunk(b"VP8 ", p), chunk(b"EXIF", b"exif!"), chunk(b"XMP ", b"<x/>"), chunk(b"ZZZZ", b"?"))
    for name, s in hand_cases().items():
        files[name] = container(s.payload())
    expected = {}
    for name, blob in sorted(files.items()):
        im = Image.open(io.BytesIO(blob))
        assert im.mode == "RGB", (name, im.mode)
        expected[name] = np.asarray(im.convert("RGB")).copy()
        with open(os.path.join(HERE, name + ".webp"), "wb") as f:
            f.write(blob)
    np.savez_compressed(os.path.join(HERE, "expected.npz"), **expected)
    # refused and damaged
    base = hand_cases()["h_mode16_dc"]
    refused = {
        "r_alph": riff(chunk(b"VP8X", bytes([0x10, 0, 0, 0]) + (47).to_bytes(3, "little") * 2), chunk(b"ALPH", b"\0" + bytes(48 * 48)),
                       chunk(b"VP8 ", base.payload())),
    }
    base.key = 0
    refused["r_inter"] = container(base.payload())
    base.key, base.show = 1, 0
    refused["r_hidden"] = container(base.payload())
    base.show, base.start = 1, b"\x9d\x01\x2b"
    damaged = {"d_badstart": container(base.payload())}
    base.start, base.version = b"\x9d\x01\x2a", 5
    damaged["d_version5"] = container(base.payload())
    base.version = 0
    p = base.payload()
    tag = (p[0] | p[1] << 8 | p[2] << 16) & 31 | (len(p) << 5)
    damaged["d_first_past_chunk"] = container(bytes([tag & 255, (tag >> 8) & 255, (tag >> 16) & 255]) + p[3:])
    s8 = hand_cases()["h_parts8_rows1"]
    p = s8.payload()
    first = (p[0] | p[1] << 8 | p[2] << 16) >> 5
    damaged["d_table_past_chunk"] = container(p[:10 + first + 9])
    for name, blob in list(refused.items()) + list(damaged.items()):
        with open(os.path.join(HERE, name + ".webp"), "wb") as f:
            f.write(blob)
        if name != "r_alph":
            try:
                Image.open(io.BytesIO(blob)).load()
                raise AssertionError("Pillow reads " + name)
            except (OSError, ValueError, SyntaxError):
                pass
    verdicts = []
    for name, c, where in CUTS:
        p = vp8_payload(files[name])
        first = (p[0] | p[1] << 8 | p[2] << 16) >> 5
        n = c if c != "half" else (len(p) - 10 - first) // 2 if where == "last" else first // 2
        blob = cut(files[name], n, where)
        try:
            got = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))
            ok = True
            same = bool(np.array_equal(got, expected[name]))
        except (OSError, ValueError, SyntaxError):
            ok, same = False, False
        verdicts.append([name, n, where, ok, same])
    with open(os.path.join(HERE, "verdicts.json"), "w") as f:
        json.dump(verdicts, f, indent=0)
    print(len(files), "fixtures,", sum(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE)), "bytes")
    for v in verdicts:
        print(v)


if __name__ == "__main__":
    main()
