"""The device inflate against the host inflate on one device -> profiles/png_inflate_probe.json: ONE
impgpu_batch_decode_png_ex call with IMPGPU_PNG_DEVICE_INFLATE (k_png_inflate: one wavefront per zlib stream) against the
same call without the bit (the host route, which this change leaves as it was), for 1 / 8 / 64 / 256 files of 640x480 RGB and
64 files of 1080p RGB, photograph-like content, zlib level 6.  Every figure is the median of repeated calls after a warm-up
call, milliseconds, the device's work included (impgpu_sync behind the call; the device route waits by itself).

    timeout -k 10 900 python tools/png_inflate_probe.py [--iters N] [--out profiles/png_inflate_probe.json]
Kernel time: run `--trace` (64 files of 640x480 RGB, 10 calls) under
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/png_inflate_probe.py --trace
then `python tools/png_inflate_probe.py --stats <...kernel_stats.csv> --out <the json>` adds k_png_inflate's time per launch."""
import argparse
import csv
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
import ngx_http_imgproc_amd as imp  # noqa: E402
from ngx_http_imgproc_amd.workloads import photo_like  # noqa: E402

CASES = [("640x480", 480, 640, 1), ("640x480", 480, 640, 8), ("640x480", 480, 640, 64), ("640x480", 480, 640, 256), ("1080p", 1080, 1920, 64)]
TRACE_REPS = 10


def files(h, w, n, distinct=8):
    out = []
    for k in range(min(n, distinct)):
        b = io.BytesIO()
        Image.fromarray(photo_like(h, w, 500 + k)).save(b, "PNG", compress_level=6)
        out.append(b.getvalue())
    return [out[k % len(out)] for k in range(n)]


class Calls:
    """the C call on prebuilt ctypes arrays: the probe times the library, not the Python wrapper"""

    def __init__(self, blobs):
        self.n = len(blobs)
        self.keep = blobs
        self.arr = (C.c_char_p * self.n)(*blobs)
        self.sizes = (C.c_size_t * self.n)(*[len(b) for b in blobs])
        self.imgs = (C.c_void_p * self.n)()
        self.codes = (C.c_int * self.n)()
        self.launches = C.c_int()

    def release(self):
        for i in range(self.n):
            if self.imgs[i]:
                h = C.c_void_p(self.imgs[i])
                imp.lib.impgpu_image_release(C.byref(h))
                self.imgs[i] = None

    def decode(self, accept):
        rc = imp.lib.impgpu_batch_decode_png_ex(self.arr, self.sizes, self.n, accept, self.imgs, self.codes, C.byref(self.launches))
        assert rc == 0 and all(c == 0 for c in self.codes), (rc, list(self.codes))
        imp.sync()


def median_ms(fn, iters, after):
    ts = []
    for _ in range(iters + 1):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        after()
    ts = sorted(ts[1:])                                          # (the first is warm-up)
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3, ts[-1] * 1e3


def case(name, h, w, n, iters):
    blobs = files(h, w, n)
    calls = Calls(blobs)
    host = median_ms(lambda: calls.decode(0), iters, calls.release)
    dev = median_ms(lambda: calls.decode(imp.PNG_DEVICE_INFLATE), iters, calls.release)
    calls.decode(imp.PNG_DEVICE_INFLATE)
    launches = calls.launches.value
    calls.release()
    raw_mb = n * (w * 3 + 1) * h / 1e6
    return {"case": "%s_rgb" % name, "files": n, "host_ms": round(host[0], 3), "host_min_max_ms": [round(host[1], 3), round(host[2], 3)],
            "device_ms": round(dev[0], 3), "device_min_max_ms": [round(dev[1], 3), round(dev[2], 3)],
            "device_over_host": round(dev[0] / host[0], 3), "launches_device": launches,
            "file_kb": round(sum(len(b) for b in blobs) / n / 1024, 1), "scanline_mb": round(raw_mb, 2),
            "device_mb_per_s": round(raw_mb / (dev[0] / 1e3), 1), "host_mb_per_s": round(raw_mb / (host[0] / 1e3), 1)}


def trace():
    calls = Calls(files(480, 640, 64))
    for _ in range(TRACE_REPS):
        calls.decode(imp.PNG_DEVICE_INFLATE)
        calls.release()


def stats(path, out):
    found = None
    with open(path) as fh:
        for row in csv.DictReader(fh):
            if "k_png_inflate" in row.get("Name", ""):
                found = {"launches": int(row["Calls"]), "us_per_launch": round(float(row["TotalDurationNs"]) / int(row["Calls"]) / 1e3, 1),
                         "files_per_launch": 64, "case": "640x480_rgb"}
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["k_png_inflate_trace"] = found
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps(found))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_inflate_probe.json"))
    ap.add_argument("--trace", action="store_true", help="the kernel-trace workload (run under rocprofv3)")
    ap.add_argument("--stats", default=None, help="a rocprofv3 kernel_stats.csv of a --trace run")
    args = ap.parse_args()
    if args.stats:
        stats(args.stats, args.out)
        return
    imp.env_start(0)
    try:
        if args.trace:
            trace()
            return
        rows = []
        for name, h, w, n in CASES:
            rows.append(case(name, h, w, n, args.iters))
            print(json.dumps(rows[-1]), flush=True)
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc["cases"] = rows
        doc["note"] = "medians of %d calls after one warm-up call, ms, device work included; host = the same call without the bit" % args.iters
        json.dump(doc, open(args.out, "w"), indent=1)
    finally:
        imp.env_destroy()


if __name__ == "__main__":
    main()
