"""GIF files in: impgpu_batch_decode_gif (container walk on the host, k_gif_lzw + k_gif_compose_mix on the device) against
the route it replaces -- every page LZW-decoded on ONE host thread, then impgpu_batch_gif_compose over the index planes.
FreeImage is not installed here, so impgpu_gif_pages(how = 0), the library's plain sequential decoder, stands in for
FreeImage's LZW: the host figure is that decoder's, not FreeImage's.

Albums of 1 / 8 / 64 pages at 64 x 64, 320 x 240 and 640 x 480, a lone file and 64 files to a call.  Every page is a full
canvas of a drifting gradient with a noisy patch (Pillow's encoder writes each page's LZW stream; tests/gif_writer.py puts
the container around them).  Times are wall time from the call to the end of the device's work (impgpu_sync inside the timed
region), medians over --iters calls after warm-up, microseconds, the two routes interleaved in halves.  A row whose planes
and albums would pass --max-gb of device memory is written with "skipped".

    timeout -k 10 900 python tools/gif_decode_probe.py [--iters 7] [--out profiles/gif_decode_probe.json]"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import torch  # noqa: F401  (first: the HIP runtime torch bundles, as in bench.py)

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [(64, 64), (320, 240), (640, 480)]
PAGES = [1, 8, 64]
FILES = [1, 64]


def pillow_stream(idx):
    """(min_code_size, the LZW bytes) Pillow's encoder writes for this index picture"""
    im = Image.fromarray(idx, "P")
    im.putpalette([v for k in range(256) for v in (k, k, k)])
    buf = io.BytesIO()
    im.save(buf, format="GIF")
    b = buf.getvalue()
    at = 13 + (3 * (2 << (b[10] & 7)) if b[10] & 0x80 else 0)
    while b[at] != 0x2C:                                    # extensions in front of the image
        at += 2
        while b[at]:
            at += b[at] + 1
        at += 1
    flags = b[at + 9]
    at += 10 + (3 * (2 << (flags & 7)) if flags & 0x80 else 0)
    mcs = b[at]
    at += 1
    data = bytearray()
    while b[at]:
        data += b[at + 1: at + 1 + b[at]]
        at += b[at] + 1
    return mcs, bytes(data)


def make_file(w, h, pages, seed):
    import gif_writer as G

    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    distinct = []
    for f in range(min(pages, 8)):                          # eight distinct pages, in turn
        idx = ((xx * 3 + yy * 2) // 8 + 11 * f).astype(np.uint8)
        ph, pw = max(1, h // 3), max(1, w // 3)
        y0, x0 = (f * 7) % (h - ph + 1), (f * 13) % (w - pw + 1)
        idx[y0: y0 + ph, x0: x0 + pw] = rng.integers(0, 256, (ph, pw), dtype=np.uint8)
        mcs, stream = pillow_stream(idx)
        distinct.append(G.make_page(idx, palette=pal, gce=dict(dispose=1 + f % 2, key=-1, delay=4), mcs=mcs, lzw=stream))
    return G.write([distinct[f % len(distinct)] for f in range(pages)])


def median_us(fn, iters):
    fn()
    ts = []
    for _ in range(max(1, iters)):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--max-gb", type=float, default=3.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gif_decode_probe.json"))
    a = ap.parse_args()
    import ngx_http_imgproc_amd as imp
    from ngx_http_imgproc_amd._lib import CGifPage, CGifSet

    imp.env_start(0)
    rows = []
    for w, h in SIZES:
        for pages in PAGES:
            blob = make_file(w, h, pages, 100 + pages)
            pitch = (w + 3) & ~3
            plane = pitch * h * pages
            for files in FILES:
                row = {"probe": "gif_decode", "canvas": [w, h], "pages": pages, "files": files, "file_bytes": len(blob), "plane_bytes": plane, "iters": a.iters}
                if files * plane * 5 > a.max_gb * (1 << 30):
                    row["skipped"] = "planes and albums of %d files pass %.1f GB" % (files, a.max_gb)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    continue
                blobs = (C.c_char_p * files)(*[blob] * files)
                sizes = (C.c_size_t * files)(*[len(blob)] * files)
                destr, which = (C.c_int * files)(*[1] * files), (C.c_int * files)(*[-1] * files)
                outs, codes, launches = (C.c_void_p * files)(), (C.c_int * files)(), C.c_int()
                # the parent's route: the planes of every file into its own buffer, page records pointing into them
                planes = [np.zeros(plane, np.uint8) for _ in range(files)]
                pal = np.zeros((256, 4), np.uint8)
                arrs = []
                for k in range(files):
                    arr = (CGifPage * pages)()
                    for f in range(pages):
                        arr[f].indices = planes[k].ctypes.data + f * pitch * h
                        arr[f].width, arr[f].height, arr[f].pitch = w, h, pitch
                        arr[f].dispose, arr[f].transparency_key, arr[f].palette = 1 + (f % 8) % 2, -1, pal.ctypes.data
                    arrs.append(arr)
                sets = (CGifSet * files)()
                for k in range(files):
                    sets[k].pages, sets[k].count, sets[k].destructive, sets[k].page = arrs[k], pages, 1, -1
                n = C.c_size_t()
                lzw_s = [0.0]

                def release():
                    for i in range(files):
                        imp.lib.impgpu_image_release(C.byref(C.c_void_p(outs[i])))

                def new():
                    rc = imp.lib.impgpu_batch_decode_gif(blobs, sizes, destr, which, files, outs, codes, C.byref(launches))
                    assert rc == 0 and not any(codes), (rc, list(codes))
                    imp.sync()
                    release()

                def parent():
                    t0 = time.perf_counter()
                    for k in range(files):
                        rc = imp.lib.impgpu_gif_pages(blob, len(blob), 0, planes[k].ctypes.data, plane, C.byref(n))
                        assert rc == 0, rc
                    lzw_s[0] = time.perf_counter() - t0
                    rc = imp.lib.impgpu_batch_gif_compose(sets, files, outs, codes, C.byref(launches))
                    assert rc == 0 and not any(codes), (rc, list(codes))
                    imp.sync()
                    release()

                h1, h2 = a.iters // 2, a.iters - a.iters // 2
                n1, p1 = median_us(new, h1), median_us(parent, h1)
                p2, n2 = median_us(parent, h2), median_us(new, h2)
                row.update({"decode_gif_us": round((n1 + n2) / 2, 1), "host_lzw_plus_compose_us": round((p1 + p2) / 2, 1),
                            "host_lzw_us_last": round(lzw_s[0] * 1e6, 1), "decode_gif_halves_us": [round(n1, 1), round(n2, 1)],
                            "host_halves_us": [round(p1, 1), round(p2, 1)], "speedup": round((p1 + p2) / (n1 + n2), 3),
                            "host_decoder": "impgpu_gif_pages(how=0), one thread (FreeImage is not installed)"})
                rows.append(row)
                print(json.dumps(row), flush=True)
    imp.env_destroy()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
