"""A MODEL of the GIF file with delta frames (IMPGPU_GIF_ENC_DELTA; include/impgpu.h has the definition): candidates, held
pixels, the window, the written keys, sets A and B and the choice, in numpy and Python ints, written from that text and not
from the C.  model_file_d() gives the whole file through gif_writer; the quantiser is gif_quant_model's, run on the window
with the held pixels made transparent.  The model, never the library, says what the bytes are.  Shared by the host,
sanitizer and GPU tests, which also share CASES: the smallest albums at which each part can go wrong."""
import struct

import numpy as np

import gif_writer as G
import gif_quant_model as Q
from test_gif_encode_host import frame_keys, frame_of, model_table, palette

import ngx_http_imgproc_amd as imp

TRANSPARENT = 1 << 25                                                      # a key no colour has


def keys_of(frame):
    """a frame's keys: R << 16 | G << 8 | B, or TRANSPARENT"""
    rgb, t = frame_keys(frame)
    return np.where(t, TRANSPARENT, rgb.astype(np.int64))


def candidates(count, dispose):
    d = list(dispose) if dispose else [0] * count
    return [i >= 1 and d[i - 1] in (0, 1) and d[i] in (0, 1) for i in range(count)]


def held_mask(frame, before):
    k, kb = keys_of(frame), keys_of(before)
    return (k != TRANSPARENT) & (k == kb)


def window_of(held):
    """x0, y0, ww, wh: the smallest rectangle round the pixels that are not held; 1 x 1 at 0,0 when all are"""
    ys, xs = np.nonzero(~held)
    if len(ys) == 0:
        return 0, 0, 1, 1
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def plan(frames, dispose=None, quantize=False):
    """per frame a dict: kind ('plain' | 'delta'), quant, window, written keys (wh, ww); or None when the album is refused"""
    cand = candidates(len(frames), dispose)
    out = []
    for i, f in enumerate(frames):
        k = keys_of(f)
        h, w = k.shape
        own = dict(kind="plain", window=(0, 0, w, h), written=k)
        nb = len(np.unique(k))
        if cand[i]:
            held = held_mask(f, frames[i - 1])
            x0, y0, ww, wh = window_of(held)
            written = np.where(held, TRANSPARENT, k)[y0:y0 + wh, x0:x0 + ww]
            mine = dict(kind="delta", window=(x0, y0, ww, wh), written=written)
            if len(np.unique(written)) <= 256:
                out.append(dict(mine, quant=False))
            elif nb <= 256:
                out.append(dict(own, quant=False))
            elif quantize:
                out.append(dict(mine, quant=True))
            else:
                return None
        elif nb <= 256:
            out.append(dict(own, quant=False))
        elif quantize:
            out.append(dict(own, quant=True))
        else:
            return None
    return out


def as_bgra(written):
    """written keys -> a B,G,R,A frame whose transparent keys have alpha 0 (what gif_quant_model.quantise takes)"""
    t = written == TRANSPARENT
    v = np.where(t, 0, written)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16, np.where(t, 0, 255)], 2).astype(np.uint8)


def model_pages_d(frames, time_ms=None, dispose=None, segment=0, quantize=False):
    """-> (gif_writer pages, global palette or None, the plan), or None when refused"""
    p = plan(frames, dispose, quantize)
    if p is None:
        return None
    segment = segment or imp.GIF_ENC_SEGMENT
    sets = [np.unique(e["written"][e["written"] != TRANSPARENT]) for e in p]
    ts = [bool((e["written"] == TRANSPARENT).any()) for e in p]
    union = np.unique(np.concatenate(sets))
    use_global = not any(e["quant"] for e in p) and len(union) + any(ts) <= 256
    pages = []
    for i, e in enumerate(p):
        wr = e["written"]
        t = wr == TRANSPARENT
        if e["quant"]:
            colours, T, idx = Q.quantise(as_bgra(wr))
            assert T == int(ts[i])
            pal, tkey, mcs = model_table(colours, T)
        else:
            colours, has_t = (union, any(ts)) if use_global else (sets[i], ts[i])
            pal, tkey, mcs = model_table(colours, has_t)
            idx = np.searchsorted(colours, np.where(t, 0, wr)).astype(np.int64)
            idx[t] = tkey
        x0, y0, ww, wh = e["window"]
        gce = dict(dispose=dispose[i] if dispose else 0, key=tkey if ts[i] else -1, delay=min(65535, (time_ms[i] if time_ms else 0) // 10))
        pages.append(G.make_page(idx.astype(np.uint8), left=x0, top=y0, palette=None if use_global else pal, gce=gce, mcs=mcs,
                                 clear_at=range(segment, ww * wh, segment)))
    return pages, (model_table(union, any(ts))[0] if use_global else None), p


def model_file_d(frames, time_ms=None, dispose=None, loop_count=-1, segment=0, quantize=False):
    """the file under IMPGPU_GIF_ENC_DELTA (| IMPGPU_GIF_ENC_QUANTIZE), or None when the album is refused"""
    m = model_pages_d(frames, time_ms, dispose, segment, quantize)
    if m is None:
        return None
    h, w = frames[0].shape[:2]
    blob = bytearray(G.write(m[0], screen=(w, h), global_palette=m[1], loop=loop_count >= 0))
    if loop_count > 0:
        at = blob.index(b"NETSCAPE2.0") + 13
        blob[at:at + 2] = struct.pack("<H", loop_count)
    return bytes(blob)


def kinds(frames, dispose=None, quantize=False):
    p = plan(frames, dispose, quantize)
    return None if p is None else [("q" if e["quant"] else "") + e["kind"] for e in p]


# ---------------------------------------------------------------- the cases
def opaque(bgr):
    return np.ascontiguousarray(np.concatenate([bgr, np.full(bgr.shape[:2] + (1,), 255, np.uint8)], 2))


def make_cases():
    """name -> (frames, keyword arguments of the encode call, quantize)"""
    rng = np.random.default_rng(20261022)
    c = {}
    base = frame_of(rng, 16, 16, palette(rng, 40))
    c["identical_16x16"] = ([base, base.copy()], dict(), False)
    for name, (y, x) in dict(top_left=(0, 0), top_right=(0, 15), bottom_left=(15, 0), bottom_right=(15, 15)).items():
        g = base.copy()
        g[y, x, :3] ^= 0x55
        c["corner_" + name] = ([base, g], dict(), False)
    # 130 x 67: three 4096-pixel items, rows that end mid-wave; the changes lie in different items
    still = frame_of(rng, 130, 67, palette(rng, 90))
    a, b = still.copy(), still.copy()
    a[3, 100, :3] ^= 0x11; a[40, 7, :3] ^= 0x22; a[66, 120, :3] ^= 0x33          # items 0, 1 and 2: rows 3 .. 66
    b[35:39, 60:64, :3] ^= 0x44                                                      # against a: every change of a and this patch
    c["bgra_130x67_seg256"] = ([still, a, b], dict(segment=256, time_ms=[40, 50, 60], loop_count=0), False)
    s3 = frame_of(rng, 23, 9, palette(rng, 30), alpha=False)
    t3 = s3.copy()
    t3[2:5, 4:11] = palette(rng, 21)[:21].reshape(3, 7, 3)
    c["bgr_3_channels"] = ([s3, t3, t3.copy()], dict(), False)
    four = [frame_of(rng, 20, 12, palette(rng, 25)) for _ in range(2)]
    four = [four[0], four[0].copy(), four[1], four[1].copy()]
    four[1][5, 5, :3] ^= 9; four[3][6, 6, :3] ^= 9
    c["dispose_1200"] = (four, dict(dispose=[1, 2, 0, 0]), False)
    c["dispose_0311"] = (four, dict(dispose=[0, 3, 1, 1]), False)
    c["dispose_null"] = (four, dict(), False)
    holes = frame_of(rng, 16, 16, palette(rng, 12))
    g = holes.copy()
    g[2, 3, 3] = 0                                                                   # transparent over opaque
    g2 = g.copy()
    g2[2, 3, 3] = 255                                                                # opaque over transparent, the colour of frame 0
    g2[9, 9, 3] = 0
    c["transparent_over_opaque_and_back"] = ([holes, g, g2, g2.copy()], dict(), False)
    # 256 colours, all of them in the window, one held pixel inside it: |A| = 257, |B| = 256 -> plain
    p257 = palette(rng, 257)
    p256 = p257[:256]
    f0 = opaque(np.zeros((16, 17, 3), np.uint8) + p256[0])
    f0[5, 5, :3] = p257[256]
    f1 = opaque(np.zeros((16, 17, 3), np.uint8) + p256[0])
    f1[:, :16, :3] = p256.reshape(16, 16, 3)                                         # (0,0) keeps p256[0]: held, inside the window
    f1[5, 5, :3] = p256[0]                                                           # ... and p256[0] is written too, where frame 0 differs
    f1[15, 16, :3] = p256[5 * 16 + 5]                                                # the colour that made room for it
    c["exactly_256_plain"] = ([f0, f1], dict(), False)
    f2 = f1.copy()
    f2[15, 16, :3] = p256[0]                                                         # 255 colours, and held again
    c["exactly_255_delta"] = ([f0, f2], dict(), False)
    # a noise frame over a held border, past 256 colours either way
    e0 = frame_of(rng, 40, 30, palette(rng, 8))
    e1 = e0.copy()
    e1[5:25, 6:34, :3] = rng.integers(0, 256, (20, 28, 3))
    e1[10, 10] = e0[10, 10]                                                          # held inside the window
    e2 = e1.copy()
    e2[0, 0, :3] ^= 1
    c["noise_over_held_border"] = ([e0, e1, e2], dict(time_ms=[30, 30, 30], segment=256), True)
    return c


CASES = make_cases()
