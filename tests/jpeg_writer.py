"""A baseline JPEG writer for the tests, from quantised coefficients (the way jpeg_prog_writer.py serves the progressive
tests): geometry, components, quantisation tables and coefficient planes -> a SOF0 / SOF1 file of one interleaved scan,
written from ITU T.81 annexes B, C and F.  It exists to reach what Pillow's encoder never writes -- untransformed RGB
files (Adobe transform 0, component ids 'R','G','B'), three quantisation tables, 16-bit tables, table selectors in any
mix, DC differences of category 11, AC category 10, Huffman codes of 15 and 16 bits, ZRL runs in front of coefficient
63, blocks without an end-of-block symbol, restart intervals of one MCU, fill bytes in front of markers.  The writer
writes what it is told: an illegal request gives an illegal file.

idct_domain() states on which blocks "bit-identical to libjpeg-turbo" holds at all: its int64
restatement of jidctint's two passes shares no code with oracle/ or csrc/.
"""
import struct

import numpy as np

from jpeg_prog_writer import ZIGZAG, Bits, code_lengths, magnitude, make_table

DOMAIN_LIMIT = 16383        # max |coef * q| and max |pass-1 output| of a block the SIMD and the 32-bit IDCT agree on

SAMPLINGS = {"gray": None, "4:4:4": (1, 1), "4:2:2": (2, 1), "4:4:0": (1, 2), "4:2:0": (2, 2)}


def components(sampling, ids=(1, 2, 3), tq=(0, 1, 1)):
    """-> [(id, h, v, tq)] of a sampling's name"""
    if sampling == "gray":
        return [(ids[0], 1, 1, tq[0])]
    h, v = SAMPLINGS[sampling]
    return [(ids[0], h, v, tq[0]), (ids[1], 1, 1, tq[1]), (ids[2], 1, 1, tq[2])]


def geometry(width, height, comps):
    """-> (mcux, mcuy, [(bh, bw)] of every component's MCU-padded block plane)"""
    if len(comps) == 1:                                  # a one-component scan is not interleaved: an MCU is a block
        mcux, mcuy = (width + 7) // 8, (height + 7) // 8
        return mcux, mcuy, [(mcuy, mcux)]
    hs, vs = max(c[1] for c in comps), max(c[2] for c in comps)
    mcux, mcuy = (width + 8 * hs - 1) // (8 * hs), (height + 8 * vs - 1) // (8 * vs)
    return mcux, mcuy, [(mcuy * c[2], mcux * c[1]) for c in comps]


def skewed_table(freq, extra=()):
    """A table whose rarest used symbol takes a 16-bit code: the symbols of `freq` by falling frequency, the never-used
    symbols of `extra` in front of the last two, and frequencies that fall by halves along the tail -- the longest tail
    make_table() codes without flattening it.  -> make_table()'s triple"""
    used = sorted(freq, key=lambda s: (-freq[s], s))
    order = used[:-2] + [s for s in extra if s not in freq] + used[-2:]
    for tail in range(min(15, len(order)), 0, -1):
        head = len(order) - tail
        # the tail and the reserved all-ones symbol weigh together what one head symbol weighs: head + 1 equal leaves above a
        # chain of `tail` levels (code_lengths() would flatten anything deeper than 16, and the skew with it)
        if tail + (head if head < 2 else (head).bit_length()) > 16:
            continue
        f = {s: float(2 ** (tail + 1)) for s in order[:head]}
        f.update({s: float(2 ** (tail - i)) for i, s in enumerate(order[head:])})
        depth = code_lengths(f)
        if max(depth.values()) == 16 and depth[order[-1]] == 16:
            return make_table(f)
    raise AssertionError("no skew of %d symbols reaches a 16-bit code: list more of them in `extra`" % len(order))


def block_tokens(zz, pred, td, ta, toks):
    """one block (zig-zag order) as tokens: ('h', table key, symbol) = a Huffman code, ('b', value, length) = plain bits"""
    s, extra = magnitude(int(zz[0]) - pred)
    toks += [("h", ("dc", td), s), ("b", extra, s)]
    if not zz[1:].any():
        toks.append(("h", ("ac", ta), 0x00))
        return int(zz[0])
    r = 0
    for k in range(1, 64):
        c = int(zz[k])
        if c == 0:
            r += 1
            continue
        while r > 15:
            toks.append(("h", ("ac", ta), 0xF0))
            r -= 16
        s, extra = magnitude(c)
        toks += [("h", ("ac", ta), (r << 4) | s), ("b", extra, s)]
        r = 0
    if r:
        toks.append(("h", ("ac", ta), 0x00))
    return int(zz[0])


def write(width, height, comps, qtabs, planes, sof=0xC0, pq=0, dri=0, tables=None, jfif=True, adobe=None, fill=0,
          one_dht=False, one_dqt=False, skew=(), extra=None, report=None):
    """-> (the file's bytes, the longest Huffman code the scan uses)

    comps     [(id, h, v, tq)]
    qtabs     {slot: 64 values in natural order}
    planes    per component (bh, bw, 64) quantised coefficients in natural order, over the MCU-padded plane (geometry())
    sof       0xC0 or 0xC1
    pq        0 or 1 (8- or 16-bit quantisation tables), or {slot: 0 or 1}
    dri       restart interval in MCUs, 0 = none
    tables    [(td, ta)] per component; default (0, 0), (1, 1), (1, 1)
    jfif      a JFIF APP0
    adobe     None, or the transform byte of an Adobe APP14
    fill      FF fill bytes in front of every RSTn and of EOI
    one_dht / one_dqt   all tables in one segment
    skew      table keys ('dc' | 'ac', id) whose rarest used symbol is to take a 16-bit code (skewed_table)
    extra     {table key: never-used symbols to list as well}
    report    a dict to fill with {table key: the longest code of that table the scan uses}
    """
    ncomp = len(comps)
    if tables is None:
        tables = [(0, 0), (1, 1), (1, 1)][:ncomp]
    mcux, mcuy, shapes = geometry(width, height, comps)
    zz = []
    for ci in range(ncomp):
        p = np.asarray(planes[ci])
        assert p.shape == shapes[ci] + (64,), (ci, p.shape, shapes[ci])
        zz.append(p[:, :, ZIGZAG])
    hv = [(1, 1)] if ncomp == 1 else [(c[1], c[2]) for c in comps]

    # ---- the scan as tokens, an interval at a time
    nmcu = mcux * mcuy
    per = dri if dri else nmcu
    intervals = []
    for m0 in range(0, nmcu, per):
        toks, pred = [], [0] * ncomp
        for m in range(m0, min(m0 + per, nmcu)):
            my, mx = divmod(m, mcux)
            for ci in range(ncomp):
                h, v = hv[ci]
                for by in range(v):
                    for bx in range(h):
                        pred[ci] = block_tokens(zz[ci][my * v + by, mx * h + bx], pred[ci], tables[ci][0], tables[ci][1], toks)
        intervals.append(toks)

    # ---- a Huffman table per key the scan names
    freq = {}
    for ci in range(ncomp):
        freq.setdefault(("dc", tables[ci][0]), {})
        freq.setdefault(("ac", tables[ci][1]), {})
    for toks in intervals:
        for tk in toks:
            if tk[0] == "h":
                freq[tk[1]][tk[2]] = freq[tk[1]].get(tk[2], 0) + 1
    extra = extra or {}
    built = {}
    for key in sorted(freq):
        f = dict(freq[key]) or {0: 1}
        if key in skew:
            built[key] = skewed_table(f, extra.get(key, ()))
        else:
            for s in extra.get(key, ()):
                f.setdefault(s, 0.25)
            built[key] = make_table(f)
        if key[0] == "dc":
            assert max(built[key][1]) <= 15, "a DC table lists symbols 0..15 at most"

    # ---- the file
    out = bytearray(b"\xff\xd8")

    def seg(marker, payload):
        out.extend(bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload))

    if jfif:
        seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if adobe is not None:
        seg(0xEE, b"Adobe\0\x64\x00\x00\x00\x00" + bytes([adobe]))
    body = []
    for slot in sorted(qtabs):
        wide = pq[slot] if isinstance(pq, dict) else pq
        q = np.asarray(qtabs[slot]).reshape(64)[ZIGZAG]
        vals = b"".join(struct.pack(">H", int(x)) for x in q) if wide else bytes(int(x) for x in q)
        body.append(bytes([(wide << 4) | slot]) + vals)
    for b in ([b"".join(body)] if one_dqt else body):
        seg(0xDB, b)
    sof_body = struct.pack(">BHHB", 8, height, width, ncomp)
    for cid, h, v, tq in comps:
        sof_body += bytes([cid, (h << 4) | v, tq])
    seg(sof, sof_body)
    body = [bytes([(0 if key[0] == "dc" else 0x10) | key[1]]) + bytes(built[key][0]) + bytes(built[key][1]) for key in sorted(built, key=lambda k: (k[0] != "dc", k[1]))]
    for b in ([b"".join(body)] if one_dht else body):
        seg(0xC4, b)
    if dri:
        seg(0xDD, struct.pack(">H", dri))
    sos = bytes([ncomp])
    for ci in range(ncomp):
        sos += bytes([comps[ci][0], (tables[ci][0] << 4) | tables[ci][1]])
    seg(0xDA, sos + bytes([0, 63, 0]))
    longest = 0
    for n, toks in enumerate(intervals):
        b = Bits()
        for tk in toks:
            if tk[0] == "h":
                code, length = built[tk[1]][2][tk[2]]
                longest = max(longest, length)
                if report is not None:
                    report[tk[1]] = max(report.get(tk[1], 0), length)
                b.put(code, length)
            else:
                b.put(tk[1], tk[2])
        b.flush()
        out.extend(b.out)
        if n + 1 < len(intervals):
            out.extend(b"\xff" * fill + bytes([0xFF, 0xD0 + (n & 7)]))
    out.extend(b"\xff" * fill + b"\xff\xd9")
    return bytes(out), longest


# ---- the domain on which the SIMD IDCT of libjpeg-turbo and a 32-bit IDCT with saturation agree
_C = dict(c0_298=2446, c0_390=3196, c0_541=4433, c0_765=6270, c0_899=7373, c1_175=9633, c1_501=12299, c1_847=15137,
          c1_961=16069, c2_053=16819, c2_562=20995, c3_072=25172)


def _pass(x, shift):
    """jidctint's one-dimensional pass over axis -2 of x (..., 8, n) in int64, descaled by `shift`"""
    c = _C
    x = x.astype(np.int64)
    e0, e1, e2, e3 = x[..., 0, :], x[..., 2, :], x[..., 4, :], x[..., 6, :]
    o0, o1, o2, o3 = x[..., 7, :], x[..., 5, :], x[..., 3, :], x[..., 1, :]
    w = (e1 + e3) * c["c0_541"]
    a2 = w - e3 * c["c1_847"]
    a3 = w + e1 * c["c0_765"]
    a0 = (e0 + e2) << 13
    a1 = (e0 - e2) << 13
    s = [a0 + a3, a1 + a2, a1 - a2, a0 - a3]
    w5 = (o0 + o2 + o1 + o3) * c["c1_175"]
    p1 = -(o0 + o3) * c["c0_899"]
    p2 = -(o1 + o2) * c["c2_562"]
    p3 = -(o0 + o2) * c["c1_961"] + w5
    p4 = -(o1 + o3) * c["c0_390"] + w5
    d = [o3 * c["c1_501"] + p1 + p4, o2 * c["c3_072"] + p2 + p3, o1 * c["c2_053"] + p2 + p4, o0 * c["c0_298"] + p1 + p3]
    half = 1 << (shift - 1)
    rows = [s[k] + d[k] for k in range(4)] + [s[3 - k] - d[3 - k] for k in range(4)]
    return np.stack([(r + half) >> shift for r in rows], axis=-2)


def idct_domain(coef, q):
    """coef (..., 64) quantised coefficients and q (64) in natural order -> per block (max |coef * q|, max |pass-1
    output|, max |final output|): the column pass descaled by CONST_BITS - PASS1_BITS = 11, the row pass by 18, before
    the +128 and the range limit.  A block is in-domain when the first two are <= DOMAIN_LIMIT."""
    coef = np.asarray(coef, dtype=np.int64)
    deq = (coef * np.asarray(q, dtype=np.int64).reshape(64)).reshape(coef.shape[:-1] + (8, 8))
    ws = _pass(deq, 11)                                              # columns: along the row index
    fin = np.swapaxes(_pass(np.swapaxes(ws, -1, -2), 18), -1, -2)    # rows
    flat = lambda a: np.abs(a).reshape(a.shape[:-2] + (64,)).max(axis=-1)
    return flat(deq), flat(ws), flat(fin)


def in_domain(coef, q):
    a, b, _ = idct_domain(coef, q)
    return bool(np.all(a <= DOMAIN_LIMIT) and np.all(b <= DOMAIN_LIMIT))
