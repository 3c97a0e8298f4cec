"""A small progressive JPEG writer for the tests (the way png_ext_writer.py serves the PNG tests): the quantised
coefficients of a baseline file (oracle_lib.jpeg_coefficients) + a scan script -> a SOF2 file, written from ITU T.81
annex G.  It exists to reach what Pillow never writes -- DC scans that are not interleaved, spectral selection without
successive approximation, Al chains 3 -> 2 -> 1 -> 0, a band per scan, tables and restart intervals that change
between scans -- and the scripts a decoder has to refuse.  The writer writes what it is told: an illegal script gives an
illegal file.

A script is a list of scans: dict(comps=[component indices], ss=, se=, ah=, al=, dri=None or the restart interval to
announce in front of the scan).  Every scan is preceded by the optimal Huffman tables of its own symbols under the table
ids it uses, so the tables are redefined between scans as a matter of course.
"""
import heapq
import struct

import numpy as np

import oracle_lib as orc

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def segments(blob):
    """marker segments of a baseline file up to its SOS: [(marker, payload)]"""
    at, out = 2, []
    while True:
        assert blob[at] == 0xFF
        m = blob[at + 1]
        n = struct.unpack(">H", blob[at + 2:at + 4])[0]
        out.append((m, blob[at + 4:at + 2 + n]))
        if m == 0xDA:
            return out
        at += 2 + n


class Source:
    """a baseline file taken apart: geometry, the segments a progressive twin keeps, the coefficients in zig-zag order"""

    def __init__(self, blob):
        rc, info = orc.jpeg_info(blob)
        assert rc == 0
        self.info = info
        self.ncomp = info["components"]
        segs = segments(blob)
        self.keep = [(m, p) for m, p in segs if m in (0xE0, 0xDB, 0xEE)]
        self.sof = [p for m, p in segs if m in (0xC0, 0xC1)][0]
        self.ids = [self.sof[6 + 3 * i] for i in range(self.ncomp)]
        self.h = [info["hs"] if i == 0 and self.ncomp > 1 else 1 for i in range(self.ncomp)]
        self.v = [info["vs"] if i == 0 and self.ncomp > 1 else 1 for i in range(self.ncomp)]
        self.planes = []
        for ci in range(self.ncomp):
            rc, c = orc.jpeg_coefficients(blob, ci)
            assert rc == 0
            bh, bw = c.shape[:2]
            self.planes.append(c.reshape(bh, bw, 64)[:, :, ZIGZAG].astype(np.int32))
        hs, vs = (info["hs"], info["vs"]) if self.ncomp > 1 else (1, 1)
        w, h = info["width"], info["height"]
        self.grid = []                                   # the component's own block grid (a one-component scan walks it)
        for ci in range(self.ncomp):
            dsw = (w * self.h[ci] + hs - 1) // hs
            dsh = (h * self.v[ci] + vs - 1) // vs
            self.grid.append(((dsh + 7) // 8, (dsw + 7) // 8))
        self.mcux, self.mcuy = info["mcux"], info["mcuy"]

    def units(self, comps):
        """the scan's units in order: each a list of (position in the scan, block's 64 coefficients)"""
        if len(comps) == 1:
            ci = comps[0]
            rows, cols = self.grid[ci]
            return [[(0, self.planes[ci][r, c])] for r in range(rows) for c in range(cols)]
        out = []
        for my in range(self.mcuy):
            for mx in range(self.mcux):
                u = []
                for i, ci in enumerate(comps):
                    for by in range(self.v[ci]):
                        for bx in range(self.h[ci]):
                            u.append((i, self.planes[ci][my * self.v[ci] + by, mx * self.h[ci] + bx]))
                out.append(u)
        return out


def code_lengths(freq):
    """Huffman code lengths (<= 16) for the symbols of `freq`; the all-ones code stays unused (a reserved extra symbol)"""
    f = {s: float(n) for s, n in freq.items() if n > 0}
    f[256] = 0.5
    while True:
        heap = [(n, i, (s,)) for i, (s, n) in enumerate(sorted(f.items()))]
        heapq.heapify(heap)
        depth = dict.fromkeys(f, 0)
        tick = len(heap)
        if len(heap) == 1:
            depth[heap[0][2][0]] = 1
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
            tick += 1
        if max(depth.values()) <= 16:
            break
        top = max(f.values())
        f = {s: max(n, top / 4096.0) if s != 256 else n for s, n in f.items()}     # flatten and try again
        f[256] = min(f.values()) / 2
    if len(depth) == 1:
        depth[256] = 1
    return depth


def make_table(freq):
    """-> (bits[1..16], vals, {symbol: (code, length)}) with canonical codes; the reserved symbol takes the longest code"""
    depth = code_lengths(freq)
    order = sorted(depth, key=lambda s: (depth[s], s == 256, s))
    codes, code, prev = {}, 0, 0
    for s in order:
        code <<= depth[s] - prev
        prev = depth[s]
        codes[s] = (code, depth[s])
        code += 1
    real = [s for s in order if s != 256]
    bits = [0] * 17
    for s in real:
        bits[depth[s]] += 1
    return bits[1:], real, codes


class Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, length):
        if length == 0:
            return
        self.acc = (self.acc << length) | (value & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def magnitude(v):
    """-> (category, the bits that follow the code)"""
    a = abs(int(v))
    s = a.bit_length()
    return s, (int(v) if v >= 0 else int(v) - 1) & ((1 << s) - 1)


def scan_symbols(src, scan, interval):
    """The scan as a list of intervals, each a list of tokens: ('h', table index in the scan, symbol) = a Huffman code,
    ('b', value, length) = plain bits."""
    comps, ss, se, ah, al = scan["comps"], scan["ss"], scan["se"], scan["ah"], scan["al"]
    units = src.units(comps)
    per = interval if interval else len(units)
    out = []
    for u0 in range(0, len(units), per):
        toks = []
        pred = [0] * len(comps)
        eobrun, pending = 0, []                          # an end-of-band run and the correction bits that wait for it

        def flush_eobrun():
            nonlocal eobrun, pending
            if eobrun:
                n = eobrun.bit_length() - 1
                toks.append(("h", 0, n << 4))
                toks.append(("b", eobrun - (1 << n), n))
                eobrun = 0
            toks.extend(pending)
            pending = []

        for unit in units[u0:u0 + per]:
            for i, blk in unit:
                if ss == 0 and ah == 0:                  # DC, first pass: the point transform is an arithmetic shift
                    v = int(blk[0]) >> al
                    s, extra = magnitude(v - pred[i])
                    pred[i] = v
                    toks += [("h", i, s), ("b", extra, s)]
                elif ss == 0:                            # DC refinement
                    toks.append(("b", (int(blk[0]) >> al) & 1, 1))
                elif ah == 0:                            # AC, first pass: magnitudes divided, towards zero
                    r = 0
                    for k in range(ss, se + 1):
                        c = int(blk[k])
                        a = abs(c) >> al
                        if a == 0:
                            r += 1
                            continue
                        flush_eobrun()
                        while r > 15:
                            toks.append(("h", 0, 0xF0))
                            r -= 16
                        s, extra = magnitude(a if c > 0 else -a)
                        toks += [("h", 0, (r << 4) | s), ("b", extra, s)]
                        r = 0
                    if r:
                        eobrun += 1
                        if eobrun == 0x7FFF:
                            flush_eobrun()
                else:                                    # AC refinement
                    mags = [abs(int(blk[k])) >> al for k in range(64)]
                    last_new = max([k for k in range(ss, se + 1) if mags[k] == 1], default=-1)
                    r, local = 0, []                     # local: correction bits met since the last symbol of this block
                    for k in range(ss, se + 1):
                        a = mags[k]
                        if a == 0:
                            r += 1
                            continue
                        while r > 15 and k <= last_new:
                            flush_eobrun()
                            toks.append(("h", 0, 0xF0))
                            r -= 16
                            toks.extend(local)
                            local = []
                        if a > 1:
                            local.append(("b", a & 1, 1))
                            continue
                        flush_eobrun()
                        toks += [("h", 0, (r << 4) | 1), ("b", 1 if blk[k] > 0 else 0, 1)]
                        toks.extend(local)
                        local = []
                        r = 0
                    if r or local:
                        eobrun += 1
                        pending.extend(local)
                        if eobrun == 0x7FFF or len(pending) > 900:
                            flush_eobrun()
        flush_eobrun()
        out.append(toks)
    return out


def write(src, script, tables_once=False):
    """-> the file's bytes"""
    out = bytearray(b"\xff\xd8")

    def seg(marker, payload):
        out.extend(bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload))

    for m, p in src.keep:
        seg(m, p)
    seg(0xC2, src.sof)
    interval = 0
    for scan in script:
        if scan.get("dri") is not None:
            interval = scan["dri"]
            seg(0xDD, struct.pack(">H", interval))
        intervals = scan_symbols(src, scan, interval)
        is_dc = scan["ss"] == 0
        ntab = len(scan["comps"]) if is_dc else 1
        tabs = []
        for t in range(ntab):
            freq = {}
            for toks in intervals:
                for tk in toks:
                    if tk[0] == "h" and tk[1] == t:
                        freq[tk[2]] = freq.get(tk[2], 0) + 1
            tabs.append(make_table(freq) if freq else None)
        for t, tb in enumerate(tabs):
            if tb:
                seg(0xC4, bytes([(0 if is_dc else 0x10) | t]) + bytes(tb[0]) + bytes(tb[1]))
        hdr = bytes([len(scan["comps"])])
        for i, ci in enumerate(scan["comps"]):
            hdr += bytes([src.ids[ci], (i << 4) if is_dc else 0])
        hdr += bytes([scan["ss"], scan["se"], (scan["ah"] << 4) | scan["al"]])
        seg(0xDA, hdr)
        for n, toks in enumerate(intervals):
            b = Bits()
            for tk in toks:
                if tk[0] == "h":
                    code, length = tabs[tk[1]][2][tk[2]]
                    b.put(code, length)
                else:
                    b.put(tk[1], tk[2])
            b.flush()
            out.extend(b.out)
            if n + 1 < len(intervals):
                out.extend(bytes([0xFF, 0xD0 + (n & 7)]))
    out.extend(b"\xff\xd9")
    return bytes(out)


# ---- scan scripts
def dc_then_full_ac(ncomp):
    """spectral selection only: one interleaved DC scan, then every component's whole AC band"""
    return [dict(comps=list(range(ncomp)), ss=0, se=0, ah=0, al=0)] + [dict(comps=[c], ss=1, se=63, ah=0, al=0) for c in range(ncomp)]


def dc_not_interleaved(ncomp):
    return [dict(comps=[c], ss=0, se=0, ah=0, al=0) for c in range(ncomp)] + [dict(comps=[c], ss=1, se=63, ah=0, al=0) for c in range(ncomp)]


def al_chain(ncomp, top=3):
    """successive approximation all the way: DC and the whole AC band at Al = top, then refined a bit at a time"""
    s = [dict(comps=list(range(ncomp)), ss=0, se=0, ah=0, al=top)]
    s += [dict(comps=[c], ss=1, se=63, ah=0, al=top) for c in range(ncomp)]
    for al in range(top - 1, -1, -1):
        s.append(dict(comps=list(range(ncomp)), ss=0, se=0, ah=al + 1, al=al))
        s += [dict(comps=[c], ss=1, se=63, ah=al + 1, al=al) for c in range(ncomp)]
    return s


def band_per_scan(ncomp):
    """many narrow bands (gray: 1 + 9 scans; colour: luma in bands, chroma whole)"""
    s = [dict(comps=list(range(ncomp)), ss=0, se=0, ah=0, al=0)]
    edges = [1, 2, 3, 6, 10, 15, 21, 28, 40, 64]
    s += [dict(comps=[0], ss=a, se=b - 1, ah=0, al=0) for a, b in zip(edges, edges[1:])]
    s += [dict(comps=[c], ss=1, se=63, ah=0, al=0) for c in range(1, ncomp)]
    return s


def mozjpeg_like(ncomp):
    """the shape of mozjpeg's default colour script: DC apart for luma and chroma pair, luma 1-8 and 9-63 with one
    refinement, chroma bands with successive approximation"""
    if ncomp == 1:
        return [dict(comps=[0], ss=0, se=0, ah=0, al=1), dict(comps=[0], ss=1, se=8, ah=0, al=2), dict(comps=[0], ss=9, se=63, ah=0, al=2),
                dict(comps=[0], ss=1, se=63, ah=2, al=1), dict(comps=[0], ss=0, se=0, ah=1, al=0), dict(comps=[0], ss=1, se=63, ah=1, al=0)]
    return [dict(comps=[0], ss=0, se=0, ah=0, al=0), dict(comps=[1, 2], ss=0, se=0, ah=0, al=0),
            dict(comps=[0], ss=1, se=8, ah=0, al=2), dict(comps=[1], ss=1, se=8, ah=0, al=0), dict(comps=[2], ss=1, se=8, ah=0, al=0),
            dict(comps=[0], ss=9, se=63, ah=0, al=2), dict(comps=[0], ss=1, se=63, ah=2, al=1), dict(comps=[0], ss=1, se=63, ah=1, al=0),
            dict(comps=[1], ss=9, se=63, ah=0, al=1), dict(comps=[2], ss=9, se=63, ah=0, al=1),
            dict(comps=[1], ss=9, se=63, ah=1, al=0), dict(comps=[2], ss=9, se=63, ah=1, al=0)]


def dri_changes(ncomp):
    """restart intervals that change between scans (and go away again)"""
    s = al_chain(ncomp, 1)
    for i, scan in enumerate(s):
        scan["dri"] = [3, 0, 7, 1, 5, 0, 2, 4][i % 8]
    return s


LEGAL = {"dc_then_full_ac": dc_then_full_ac, "dc_not_interleaved": dc_not_interleaved, "al_chain_3": al_chain, "band_per_scan": band_per_scan,
         "mozjpeg_like": mozjpeg_like, "dri_changes": dri_changes}


def illegal_scripts(ncomp):
    """name -> script that include/impgpu.h says is refused at the header (IMP_ERROR_UNSUPPORTED)"""
    full = dc_then_full_ac(ncomp)
    out = {
        "incomplete_no_ac_tail": [full[0]] + [dict(comps=[c], ss=1, se=40, ah=0, al=0) for c in range(ncomp)],
        "incomplete_al_left_at_1": al_chain(ncomp, 2)[:-(1 + ncomp)],
        "ac_before_dc": [full[1], full[0]] + full[2:],
        "refinement_skips_a_bit": [dict(comps=list(range(ncomp)), ss=0, se=0, ah=0, al=2), dict(comps=list(range(ncomp)), ss=0, se=0, ah=1, al=0)] + full[1:],
        "band_sent_twice": full + [full[1]],
        "dc_scan_with_ac_band": [dict(comps=list(range(ncomp)), ss=0, se=5, ah=0, al=0)] + full[1:],
        "too_many_scans": [full[0]] + [dict(comps=[0], ss=k, se=k, ah=0, al=0) for k in range(1, 64)] + full[2:],
    }
    if ncomp > 1:
        out["ac_scan_of_two_components"] = [full[0], dict(comps=[1, 2], ss=1, se=63, ah=0, al=0), full[1]]
    return out
