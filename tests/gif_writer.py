"""A GIF writer and a page model in numpy / Python for the GIF decode tests: an LZW encoder with a choice of
min_code_size, clear codes at chosen pixels, `never_clear` (the table fills at 4096 and 12-bit codes go on: the deferred
clear), interlace, local and global colour tables of 2..256 entries, graphic control extensions, page offsets and chosen
sub-block sizes -- and a parser and a plain decoder that give the `page(...)` dicts of test_gif.py (what FreeImage would
hand LoadGIF: 8-bit indices bottom-up, pitch (w + 3) & ~3, pad bytes 0, a 256 x B,G,R,0 palette)."""
import struct

import numpy as np


def width_of(next_code):
    w = 1
    while (1 << w) <= next_code and w < 12:
        w += 1
    return w


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, width):
        self.acc |= code << self.n
        self.n += width
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def lzw_encode(pixels, mcs, clear_at=(), never_clear=False, eoi=True, first_clear=True):
    """pixels (values < 1 << mcs) -> the LZW byte stream.  A clear code is written in front of every pixel position in
    `clear_at`, and when the table is full unless never_clear.  The decoder's next free code is tracked as the decoder
    sees it: the first code after a clear adds no entry there."""
    clear, end = 1 << mcs, (1 << mcs) + 1
    bw = BitWriter()
    clear_at = set(clear_at)
    state = {}

    def reset():
        state["table"] = {}
        state["next"] = clear + 2            # the encoder's next entry
        state["dec"] = clear + 2             # the decoder's next free code when it reads the next code
        state["first"] = True

    def emit(code):
        bw.put(code, width_of(state["dec"]))
        if state["first"]:
            state["first"] = False
        else:
            state["dec"] = min(4096, state["dec"] + 1)

    def emit_clear():
        bw.put(clear, width_of(state["dec"]))
        reset()

    reset()
    if first_clear:
        emit_clear()
    cur = None
    for pos, b in enumerate(int(v) for v in pixels):
        if pos in clear_at and pos > 0:
            if cur is not None:
                emit(cur)
                cur = None
            emit_clear()
        if cur is None:
            cur = b
            continue
        hit = state["table"].get((cur, b))
        if hit is not None:
            cur = hit
            continue
        emit(cur)
        if state["next"] < 4096:
            state["table"][(cur, b)] = state["next"]
            state["next"] += 1
        elif not never_clear:
            emit_clear()
        cur = b
    if cur is not None:
        emit(cur)
    if eoi:
        bw.put(end, width_of(state["dec"]))
    return bw.done()


def sub_blocks(data, size=255):
    out = bytearray()
    for at in range(0, len(data), size):
        piece = data[at:at + size]
        out.append(len(piece))
        out += piece
    out.append(0)
    return bytes(out)


def interlace_order(h):
    return list(range(0, h, 8)) + list(range(4, h, 8)) + list(range(2, h, 4)) + list(range(1, h, 2))


def table_bytes(pal):
    """an (n, 3) R,G,B table, n a power of two in 2..256 -> (size field, bytes)"""
    pal = np.asarray(pal, np.uint8)
    n = pal.shape[0]
    assert n in (2, 4, 8, 16, 32, 64, 128, 256)
    return n.bit_length() - 2, pal.tobytes()


def make_page(indices, left=0, top=0, interlaced=False, palette=None, gce=None, mcs=8, clear_at=(), never_clear=False,
              block=255, lzw=None, eoi=True):
    """A page for write(): `indices` top-down (h, w) uint8; palette (n, 3) R,G,B = a local table; gce = dict(dispose, key,
    delay) or None; lzw = ready-made stream bytes instead of the encoder's (damage cases)."""
    return dict(indices=np.asarray(indices, np.uint8), left=left, top=top, interlaced=bool(interlaced), palette=palette, gce=gce,
                mcs=mcs, clear_at=tuple(clear_at), never_clear=never_clear, block=block, lzw=lzw, eoi=eoi)


def page_stream(p):
    if p["lzw"] is not None:
        return p["lzw"]
    a = p["indices"]
    rows = a[interlace_order(a.shape[0])] if p["interlaced"] else a
    return lzw_encode(rows.reshape(-1), p["mcs"], p["clear_at"], p["never_clear"], p["eoi"])


def write(pages, screen=None, global_palette=None, version=b"GIF89a", trailer=True, loop=False):
    first = pages[0]["indices"]
    sw, sh = screen or (first.shape[1], first.shape[0])
    out = bytearray(version)
    if global_palette is not None:
        bits, tb = table_bytes(global_palette)
        out += struct.pack("<HHBBB", sw, sh, 0x80 | 0x70 | bits, 0, 0) + tb
    else:
        out += struct.pack("<HHBBB", sw, sh, 0x70, 0, 0)
    if loop:
        out += b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"
    for p in pages:
        g = p["gce"]
        if g is not None:
            key = g.get("key", -1)
            flags = (g.get("dispose", 0) << 2) | (1 if key >= 0 else 0)
            out += b"\x21\xf9\x04" + struct.pack("<BHB", flags, g.get("delay", 0), key if key >= 0 else 0) + b"\x00"
        h, w = p["indices"].shape
        flags = 0x40 if p["interlaced"] else 0
        tb = b""
        if p["palette"] is not None:
            bits, tb = table_bytes(p["palette"])
            flags |= 0x80 | bits
        out += b"\x2c" + struct.pack("<HHHHB", p["left"], p["top"], w, h, flags) + tb
        out.append(p["mcs"])
        out += sub_blocks(page_stream(p), p["block"])
    if trailer:
        out.append(0x3B)
    return bytes(out)


# ---------------------------------------------------------------- the model: what FreeImage would hand LoadGIF
def fi_palette(rgb):
    pal = np.zeros((256, 4), np.uint8)
    rgb = np.asarray(rgb, np.uint8)
    pal[: rgb.shape[0], :3] = rgb[:, ::-1]
    return pal


def model_page(idx_top_down, left=0, top=0, dispose=0, key=-1, pal=None, time_ms=0):
    a = np.asarray(idx_top_down, np.uint8)
    h, w = a.shape
    buf = np.zeros((h, (w + 3) & ~3), np.uint8)
    buf[:, :w] = a[::-1]
    return {"indices": buf, "width": w, "left": left, "top": top, "dispose": dispose, "key": key, "palette": pal, "time_ms": time_ms}


def model(pages, global_palette=None):
    """the page dicts of the pages given to write()"""
    out = []
    for p in pages:
        g = p["gce"] or {}
        rgb = p["palette"] if p["palette"] is not None else global_palette
        out.append(model_page(p["indices"], p["left"], p["top"], g.get("dispose", 0), g.get("key", -1), fi_palette(rgb), g.get("delay", 0) * 10))
    return out


def planes(model_pages):
    """impgpu_gif_pages' bytes for these pages"""
    return b"".join(p["indices"].tobytes() for p in model_pages)


def lzw_decode(data, mcs, count):
    """the plain decoder: up to `count` indices of the stream (the sub-block payloads)"""
    clear, end = 1 << mcs, (1 << mcs) + 1
    table = [[i] for i in range(clear)] + [None, None]
    out = []
    bit, prev = 0, None
    nbits = len(data) * 8
    acc = int.from_bytes(data, "little")
    while len(out) < count:
        w = width_of(len(table))
        if bit + w > nbits:
            break
        c = (acc >> bit) & ((1 << w) - 1)
        bit += w
        if c == clear:
            table = table[: clear + 2]
            prev = None
            continue
        if c == end:
            break
        if prev is None:
            assert c < clear
            s = table[c]
        else:
            assert c <= len(table)
            s = table[c] if c < len(table) else prev + prev[:1]
            if len(table) < 4096:
                table.append(prev + s[:1])
        out += s
        prev = s
    return out[:count]


def parse(blob):
    """A GIF file -> (page dicts as model() gives them, (canvas w, canvas h)); an independent walk of the container."""
    assert blob[:6] in (b"GIF87a", b"GIF89a")
    flags = blob[10]
    at = 13
    gpal = None
    if flags & 0x80:
        n = 2 << (flags & 7)
        gpal = np.frombuffer(blob[at:at + 3 * n], np.uint8).reshape(n, 3)
        at += 3 * n
    pages, gce = [], {}
    while blob[at] != 0x3B:
        if blob[at] == 0x21:
            label = blob[at + 1]
            at += 2
            if label == 0xF9:
                f, delay, key = struct.unpack("<BHB", blob[at + 1:at + 5])
                gce = {"dispose": (f >> 2) & 7, "key": key if f & 1 else -1, "delay": delay}
            while blob[at]:
                at += blob[at] + 1
            at += 1
            continue
        assert blob[at] == 0x2C
        left, top, w, h, f = struct.unpack("<HHHHB", blob[at + 1:at + 10])
        at += 10
        pal = gpal
        if f & 0x80:
            n = 2 << (f & 7)
            pal = np.frombuffer(blob[at:at + 3 * n], np.uint8).reshape(n, 3)
            at += 3 * n
        mcs = blob[at]
        at += 1
        data = bytearray()
        while blob[at]:
            data += blob[at + 1:at + 1 + blob[at]]
            at += blob[at] + 1
        at += 1
        idx = np.array(lzw_decode(bytes(data), mcs, w * h), np.uint8).reshape(h, w)
        if f & 0x40:
            plain = np.zeros_like(idx)
            plain[interlace_order(h)] = idx
            idx = plain
        pages.append(model_page(idx, left, top, gce.get("dispose", 0), gce.get("key", -1), fi_palette(pal), gce.get("delay", 0) * 10))
        gce = {}
    return pages, (pages[0]["width"], pages[0]["indices"].shape[0])
