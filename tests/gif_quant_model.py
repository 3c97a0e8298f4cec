"""A MODEL of the GIF file past 256 colours (IMPGPU_GIF_ENC_QUANTIZE; include/impgpu.h has the definition): steps 1-5 --
keys, the 5:5:5 histogram, the median-cut boxes, their colours, the table and the indices -- in numpy and Python ints,
written from that text and not from the C.  model_file_q() gives the whole file through gif_writer, the way
test_gif_encode_host.model_file() gives the exact-palette one; an album whose frames all fit IS that file.  The model,
never the library, says what the bytes are.  Shared by the host, sanitizer and GPU tests, which also share CASES."""
import struct

import numpy as np

import gif_writer as G
from test_gif_encode_host import frame_keys, frame_of, model_pages, model_table, palette

import ngx_http_imgproc_amd as imp


def tight(n, box):
    """the box (r0, r1, g0, g1, b0, b1; inclusive cells) shrunk to the bounds of its non-empty cells"""
    r0, r1, g0, g1, b0, b1 = box
    sub = n[r0:r1 + 1, g0:g1 + 1, b0:b1 + 1]
    out = []
    for axis, base in ((0, r0), (1, g0), (2, b0)):
        planes = np.nonzero(sub.sum(axis=tuple(a for a in range(3) if a != axis)))[0]
        out += [base + int(planes[0]), base + int(planes[-1])]
    return tuple(out)


def box_count(n, box):
    r0, r1, g0, g1, b0, b1 = box
    return int(n[r0:r1 + 1, g0:g1 + 1, b0:b1 + 1].sum())


def quantise(frame):
    """steps 1-5 on a B,G,R[,A] frame -> (box colours ascending as R << 16 | G << 8 | B, T, (h, w) indices)"""
    key, t = frame_keys(frame)
    T = int(t.any())
    K = 256 - T
    opaque = key[~t].astype(np.int64)
    R, Gc, B = opaque >> 16, (opaque >> 8) & 255, opaque & 255
    cells = (R >> 3, Gc >> 3, B >> 3)
    n = np.zeros((32, 32, 32), np.int64)
    sums = [np.zeros((32, 32, 32), np.int64) for _ in range(3)]
    np.add.at(n, cells, 1)
    for s, v in zip(sums, (R, Gc, B)):
        np.add.at(s, cells, v)
    boxes = [tight(n, (0, 31, 0, 31, 0, 31))] if len(opaque) else []
    while boxes and len(boxes) < K:
        best, pick = 0, -1
        for i, b in enumerate(boxes):
            s = max(b[1] - b[0], b[3] - b[2], b[5] - b[4])
            score = box_count(n, b) * s
            if s > 0 and score > best:
                best, pick = score, i
        if pick < 0:
            break
        b = boxes[pick]
        sides = [b[1] - b[0], b[3] - b[2], b[5] - b[4]]
        s = max(sides)
        axis = sides.index(s)                                           # ties: R, then G, then B
        sub = n[b[0]:b[1] + 1, b[2]:b[3] + 1, b[4]:b[5] + 1]
        m = [int(v) for v in sub.sum(axis=tuple(a for a in range(3) if a != axis))]
        total = sum(m)
        half = (total + 1) // 2
        run, cut = 0, s
        for j in range(s + 1):
            run += m[j]
            if run >= half:
                cut = j
                break
        cut = min(cut, s - 1)
        low, high = list(b), list(b)
        low[2 * axis + 1] = b[2 * axis] + cut
        high[2 * axis] = b[2 * axis] + cut + 1
        boxes[pick] = tight(n, tuple(low))
        boxes.append(tight(n, tuple(high)))
    colours, owner = [], np.zeros((32, 32, 32), np.int64)
    for i, b in enumerate(boxes):
        cnt = box_count(n, b)
        c = [(2 * int(s[b[0]:b[1] + 1, b[2]:b[3] + 1, b[4]:b[5] + 1].sum()) + cnt) // (2 * cnt) for s in sums]
        colours.append(c[0] << 16 | c[1] << 8 | c[2])
        owner[b[0]:b[1] + 1, b[2]:b[3] + 1, b[4]:b[5] + 1] = i
    assert len(set(colours)) == len(colours)
    order = np.argsort(np.array(colours, np.int64), kind="stable")
    rank = np.zeros(max(1, len(boxes)), np.int64)
    rank[order] = np.arange(len(boxes))
    k = key.astype(np.int64)
    idx = rank[owner[k >> 19, (k >> 11) & 31, (k >> 3) & 31]] if boxes else np.zeros(key.shape, np.int64)
    idx = np.where(t, len(boxes) + T - 1, idx)
    return np.array(sorted(colours), np.uint32), T, idx.astype(np.uint8)


def overflows(frame):
    key, t = frame_keys(frame)
    return len(np.unique(key[~t])) + int(t.any()) > 256


def quantised_pixels(frame):
    """what a decoder must show for a quantised frame: (h, w, 3) R,G,B and the transparency mask"""
    colours, T, idx = quantise(frame)
    pal = model_table(colours, T)[0]
    return pal[idx], frame_keys(frame)[1]


def model_pages_q(frames, time_ms=None, dispose=None, segment=0):
    """-> (gif_writer pages, global palette or None) under the flag"""
    over = [overflows(f) for f in frames]
    if not any(over):
        return model_pages(frames, time_ms, dispose, segment)
    segment = segment or imp.GIF_ENC_SEGMENT
    h, w = frames[0].shape[:2]
    pages = []
    for i, f in enumerate(frames):
        key, t = frame_keys(f)
        if over[i]:
            colours, T, idx = quantise(f)
        else:
            colours, T = np.unique(key[~t]), int(t.any())
            idx = np.searchsorted(colours, key).astype(np.int64)
        pal, tkey, mcs = model_table(colours, T)
        idx = np.where(t, tkey, idx).astype(np.uint8)
        gce = dict(dispose=dispose[i] if dispose else 0, key=tkey if T else -1, delay=min(65535, (time_ms[i] if time_ms else 0) // 10))
        pages.append(G.make_page(idx, palette=pal, gce=gce, mcs=mcs, clear_at=range(segment, w * h, segment)))
    return pages, None


def model_file_q(frames, time_ms=None, dispose=None, loop_count=-1, segment=0):
    pages, gpal = model_pages_q(frames, time_ms, dispose, segment)
    blob = bytearray(G.write(pages, global_palette=gpal, loop=loop_count >= 0))
    if loop_count > 0:
        at = blob.index(b"NETSCAPE2.0") + 13
        blob[at:at + 2] = struct.pack("<H", loop_count)
    return bytes(blob)


# ---------------------------------------------------------------- frames
def spread(rng, n):
    """n distinct colours spread over the cube, (n, 3) B,G,R"""
    return palette(rng, n)


def in_cells(rng, n, cells):
    """n distinct colours, dealt round the given (r, g, b) cells: (n, 3) B,G,R"""
    seen, out = set(), []
    while len(out) < n:
        r, g, b = cells[len(out) % len(cells)]
        c = (8 * r + int(rng.integers(0, 8)), 8 * g + int(rng.integers(0, 8)), 8 * b + int(rng.integers(0, 8)))
        if c not in seen:
            seen.add(c)
            out.append((c[2], c[1], c[0]))
    return np.array(out, np.uint8)


def ramp(w=128, h=96):
    """R = 2x, G = 2y + 30, B = x + y, clipped: (h, w, 3) B,G,R"""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([np.clip(x + y, 0, 255), np.clip(2 * y + 30, 0, 255), np.clip(2 * x, 0, 255)], 2).astype(np.uint8)


def with_holes(rng, bgr, share):
    """the frame as B,G,R,A with `share` of its pixels transparent (alpha 0, a colour of their own)"""
    h, w = bgr.shape[:2]
    f = np.concatenate([bgr, rng.integers(1, 256, (h, w, 1)).astype(np.uint8)], 2)
    hole = rng.random((h, w)) < share
    f[hole] = np.concatenate([rng.integers(0, 256, (int(hole.sum()), 3)), np.zeros((int(hole.sum()), 1))], 1).astype(np.uint8)
    return np.ascontiguousarray(f)


def make_cases():
    """name -> (frames, keyword arguments): the issue's cases 1-9 (the views, offsets, batches and capacities are the tests')"""
    rng = np.random.default_rng(20261021)
    c = {}
    c["bgr_272"] = ([frame_of(rng, 17, 16, spread(rng, 272), alpha=False)], dict())
    c["bgra_256_and_holes"] = ([frame_of(rng, 17, 16, spread(rng, 256), transparent=0.05)], dict(dispose=[2]))
    c["one_cell_400"] = ([frame_of(rng, 20, 20, in_cells(rng, 400, [(9, 20, 3)]), alpha=False)], dict())
    c["two_cells_300"] = ([frame_of(rng, 20, 20, in_cells(rng, 300, [(9, 20, 3), (9, 20, 4)]), alpha=False)], dict())
    p300 = spread(rng, 300)
    c["row_300"] = ([frame_of(rng, 300, 1, p300, alpha=False)], dict())
    c["column_300"] = ([frame_of(rng, 1, 300, p300, alpha=False)], dict())
    noise = rng.integers(0, 256, (67, 130, 3)).astype(np.uint8)
    c["noise_130x67"] = ([noise], dict(segment=0))
    c["noise_130x67_seg256"] = ([noise], dict(segment=256))
    c["ramp_holes"] = ([with_holes(rng, ramp(), 0.3)], dict(loop_count=0))
    rare = frame_of(rng, 64, 64, spread(rng, 297), alpha=False).reshape(-1, 3)
    first = {}
    for i, px in enumerate(map(bytes, rare)):
        first.setdefault(px, i)
    keep = np.zeros(len(rare), bool)
    keep[list(first.values())] = True
    common = rare[0].copy()
    rare[~keep] = common                                              # 296 rare colours once each, the rest one colour
    c["one_colour_and_296_rare"] = ([np.ascontiguousarray(rare.reshape(64, 64, 3))], dict())
    c["album_exact_noise_holes"] = ([frame_of(rng, 40, 30, spread(rng, 8)), with_holes(rng, rng.integers(0, 256, (30, 40, 3)).astype(np.uint8), 0.0),
                                     frame_of(rng, 40, 30, spread(rng, 300), transparent=0.1)],
                                    dict(time_ms=[100, 250, 40], dispose=[1, 2, 1], loop_count=3, segment=512))
    return c


CASES = make_cases()
