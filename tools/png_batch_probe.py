"""PNG input in batches on one device -> one JSON line per case: a batch of 1 / 8 / 64 files at 640x480 and 1080p (RGB,
RGBA, gray) through ONE impgpu_batch_decode_png call, the same files through N impgpu_image_decode_png calls, and Pillow on
this core.  Times are medians, milliseconds, the device's work included (impgpu_sync after the calls); host_ms is the batch
call's own return (it does not wait), i.e. the host's share: headers, inflates on the helper threads, enqueue.

    timeout -k 10 900 python tools/png_batch_probe.py [--iters N] [--only 640x480]
Kernel times: run `--trace` (a 64-file batch and the same 64 files one at a time, 640x480 RGB) under
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/png_batch_probe.py --trace
then `python tools/png_batch_probe.py --stats <...kernel_stats.csv>` prints k_png_unfilter_batch per launch against one
file's k_png_unfilter launches (a single-file decode slices its rows: several launches per file)."""
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

SIZES = {"640x480": (480, 640), "1080p": (1080, 1920)}
KINDS = {"rgb": 3, "rgba": 4, "gray": 1}
TRACE_REPS = 20


def files(h, w, c, n, distinct=8):
    out = []
    for k in range(min(n, distinct)):
        rgb = photo_like(h, w, 500 + k)
        a = rgb[:, :, 1] if c == 1 else rgb if c == 3 else np.dstack([rgb, (rgb[:, :, 0] // 2 + 100).astype(np.uint8)])
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(a)).save(b, "PNG")          # Pillow's default level (6), its own filter choice
        out.append(b.getvalue())
    return [out[k % len(out)] for k in range(n)]


class Calls:
    """the C calls on prebuilt ctypes arrays: the probe times the library, not the Python wrapper"""

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

    def batch(self):
        rc = imp.lib.impgpu_batch_decode_png(self.arr, self.sizes, self.n, self.imgs, self.codes, C.byref(self.launches))
        assert rc == 0 and all(c == 0 for c in self.codes), (rc, list(self.codes))

    def singles(self):
        for i in range(self.n):
            h = C.c_void_p()
            rc = imp.lib.impgpu_image_decode_png(self.keep[i], len(self.keep[i]), C.byref(h))
            assert rc == 0, rc
            self.imgs[i] = h.value


def median_ms(fn, iters, after=None):
    ts = []
    for k in range(iters + 1):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        if after:
            after()
    ts = sorted(ts[1:])                                          # (the first is warm-up)
    return ts[len(ts) // 2] * 1e3


def case(size, kind, n, iters):
    h, w = SIZES[size]
    blobs = files(h, w, KINDS[kind], n)
    calls = Calls(blobs)

    def batch_total():
        calls.batch()
        imp.sync()

    def singles_total():
        calls.singles()
        imp.sync()

    host = median_ms(calls.batch, iters, after=lambda: (imp.sync(), calls.release()))
    batch = median_ms(batch_total, iters, after=calls.release)
    single = median_ms(singles_total, iters, after=calls.release)
    pil = median_ms(lambda: [np.asarray(Image.open(io.BytesIO(b))) for b in blobs], max(3, iters // 2))
    calls.batch()
    launches = calls.launches.value
    imp.sync()
    calls.release()
    return {"case": "%s_%s" % (size, kind), "files": n, "batch_ms": round(batch, 3), "host_ms": round(host, 3),
            "singles_ms": round(single, 3), "pillow_ms": round(pil, 3), "batch_over_singles": round(batch / single, 3),
            "launches": launches, "file_kb": round(sum(len(b) for b in blobs) / n / 1024, 1)}


def trace():
    calls = Calls(files(480, 640, 3, 64))
    for _ in range(TRACE_REPS):
        calls.batch()
        imp.sync()
        calls.release()
    for _ in range(TRACE_REPS):
        calls.singles()
        imp.sync()
        calls.release()


def stats(path):
    rows = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            for k in ("k_png_unfilter_batch", "k_png_unfilter"):
                if k + "<" in name or name.startswith(k + "("):
                    rows.setdefault(k, [0, 0.0])
                    rows[k][0] += int(row["Calls"])
                    rows[k][1] += float(row["TotalDurationNs"])
                    break
    b, s = rows.get("k_png_unfilter_batch"), rows.get("k_png_unfilter")
    out = {"batch_launches": b and b[0], "batch_us_per_launch": b and round(b[1] / b[0] / 1e3, 1),
           "single_launches": s and s[0], "single_files": 64 * TRACE_REPS,
           "single_us_per_launch": s and round(s[1] / s[0] / 1e3, 1),
           "single_us_per_file": s and round(s[1] / (64 * TRACE_REPS) / 1e3, 1)}
    if b and s:
        out["batch_launch_over_lone_file"] = round((b[1] / b[0]) / (s[1] / (64 * TRACE_REPS)), 2)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--only", default=None, help="one size: 640x480 or 1080p")
    ap.add_argument("--trace", action="store_true", help="the kernel-trace workload (run under rocprofv3)")
    ap.add_argument("--stats", default=None, help="a rocprofv3 kernel_stats.csv of a --trace run")
    args = ap.parse_args()
    if args.stats:
        stats(args.stats)
        return
    imp.env_start(0)
    try:
        if args.trace:
            trace()
            return
        for size in SIZES:
            if args.only and size != args.only:
                continue
            for kind in KINDS:
                for n in (1, 8, 64):
                    print(json.dumps(case(size, kind, n, args.iters)), flush=True)
    finally:
        imp.env_destroy()


if __name__ == "__main__":
    main()
