"""The json and text exits in batches on one device -> one JSON line per row: ONE impgpu_batch_calc_perceived_brightness /
impgpu_batch_ascii call over `count` frames against the loop of impgpu_calc_perceived_brightness / impgpu_ascii calls over
clones of the same frames (the only path before the batch calls existed, so it is the baseline, taken in the same process).
Times are wall time to the answer, medians over --iters calls after warm-up, microseconds; both forms return with their
answers, so the device's work and every wait is inside.
  pools: thumbs -- the mixed pool's frames (ngx_http_imgproc_amd/workloads.py) as 224-wide BGR thumbnails (60-wide for the
         text exit: what a text request realistically asks for), count 1 / 2 / 8 / 64;
         1080p  -- 1920 x 1080 BGR frames, count 1 / 2 / 8 / 16 (brightness only).

    timeout -k 10 600 python tools/info_batch_probe.py [--iters 30] [--out rows.jsonl]
Kernel times (the probe itself takes wall time only): `--trace thumbs` runs the count = 64 thumbnail case of both exits,
`--trace 1080p` sixteen 1080p frames' brightness, batch then loop, TRACE_REPS times each, for
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/info_batch_probe.py --trace thumbs
and `--stats <...kernel_stats.csv> --trace thumbs|1080p` turns that file into one JSON line: device time per kernel and
per call of either form."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import torch  # noqa: F401  (first: the HIP runtime torch bundles, as in bench.py)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ngx_http_imgproc_amd as imp  # noqa: E402
from ngx_http_imgproc_amd.workloads import mixed_sizes, photo_like  # noqa: E402

TRACE_REPS = 20


def thumbs(n, width):
    out = []
    for k, (w, h) in enumerate(mixed_sizes(n)):
        th = max(1, int(round(width * h / w)))
        out.append(photo_like(th, width, 900 + k)[:, :, ::-1].copy())           # B, G, R
    return out


def full_hd(n):
    base = [photo_like(1080, 1920, 950 + k)[:, :, ::-1].copy() for k in range(min(n, 4))]
    return [base[k % len(base)] for k in range(n)]


class Frames:
    """the C calls on prebuilt ctypes arrays: the probe times the library, not the Python wrapper"""

    def __init__(self, arrs):
        self.n = n = len(arrs)
        self.ims = [imp.Image(a) for a in arrs]                 # the batch call's frames
        self.clones = [im.clone() for im in self.ims]           # the loop's
        self.handles = (C.c_void_p * n)(*[im.h.value for im in self.ims])
        self.vals = (C.c_float * n)()
        self.codes = (C.c_int * n)()
        self.launches = C.c_int()
        need = [(a.shape[1] + 1) * a.shape[0] for a in arrs]
        self.bufs = [(C.c_ubyte * k)() for k in need]
        self.outs = (C.c_void_p * n)(*[C.addressof(b) for b in self.bufs])
        self.caps = (C.c_long * n)(*need)
        self.lens = (C.c_long * n)()
        self.one = C.c_float()
        self.len1 = C.c_long()
        imp.sync()

    def release(self):
        for im in self.ims + self.clones:
            im.release()

    def brightness_batch(self):
        rc = imp.lib.impgpu_batch_calc_perceived_brightness(self.handles, self.n, self.vals, self.codes, C.byref(self.launches))
        assert rc == 0 and not any(self.codes), (rc, list(self.codes))

    def brightness_loop(self):
        for cl in self.clones:
            rc = imp.lib.impgpu_calc_perceived_brightness(cl.h, C.byref(self.one))
            assert rc == 0, rc

    def ascii_batch(self):
        rc = imp.lib.impgpu_batch_ascii(self.handles, None, self.n, self.outs, self.caps, self.lens, self.codes, C.byref(self.launches))
        assert rc == 0 and not any(self.codes), (rc, list(self.codes))

    def ascii_loop(self):
        for cl, buf, cap in zip(self.clones, self.bufs, self.caps):
            rc = imp.lib.impgpu_ascii(cl.h, b"", buf, cap, C.byref(self.len1))
            assert rc == 0, rc


def median_us(fn, iters):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e6


def row(exit_, pool, arrs, iters):
    f = Frames(arrs)
    batch_fn, loop_fn = (f.brightness_batch, f.brightness_loop) if exit_ == "brightness" else (f.ascii_batch, f.ascii_loop)
    # interleaved halves, so that a drift of the machine lands on both forms
    b1, l1 = median_us(batch_fn, iters // 2), median_us(loop_fn, iters // 2)
    l2, b2 = median_us(loop_fn, iters - iters // 2), median_us(batch_fn, iters - iters // 2)
    batch, loop = (b1 + b2) / 2, (l1 + l2) / 2
    launches = f.launches.value
    f.release()
    return {"exit": exit_, "pool": pool, "count": len(arrs), "batch_us": round(batch, 1), "loop_us": round(loop, 1),
            "batch_over_loop": round(batch / loop, 3), "launches": launches, "iters": iters,
            "pixels": int(sum(a.shape[0] * a.shape[1] for a in arrs))}


def trace(which):
    """thumbs: 64 thumbnails (brightness, 224 wide; text, 60 wide); 1080p: 16 frames of 1920 x 1080 (brightness)"""
    if which == "1080p":
        f, g = Frames(full_hd(16)), None
    else:
        f, g = Frames(thumbs(64, 224)), Frames(thumbs(64, 60))
    for _ in range(TRACE_REPS):
        f.brightness_batch()
    for _ in range(TRACE_REPS):
        f.brightness_loop()
    f.release()
    if g:
        for _ in range(TRACE_REPS):
            g.ascii_batch()
        for _ in range(TRACE_REPS):
            g.ascii_loop()
        g.release()


def stats(path, which):
    """device time per call of either form (64 thumbnails, or 16 frames of 1080p), from the kernel_stats.csv of a --trace run"""
    tot = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name", "")
            for k in ("k_brightness_fold_mix", "k_brightness_walk_mix", "k_brightness_fold", "k_brightness_walk", "k_ascii_mix", "k_ascii"):
                if k + "<" in name:
                    t = tot.setdefault(k, [0, 0.0])
                    t[0] += int(r["Calls"])
                    t[1] += float(r["TotalDurationNs"])
                    break
    count = 16 if which == "1080p" else 64
    out = {"trace": "count=%d %s, %d calls of each form" % (count, which, TRACE_REPS)}
    for k, (calls, ns) in sorted(tot.items()):
        out[k] = {"launches": calls, "us_per_launch": round(ns / calls / 1e3, 2), "us_per_call": round(ns / TRACE_REPS / 1e3, 1)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    ap.add_argument("--trace", default=None, choices=("thumbs", "1080p"), help="a kernel-trace workload (run under rocprofv3)")
    ap.add_argument("--stats", default=None, help="a rocprofv3 kernel_stats.csv of a --trace run")
    args = ap.parse_args()
    if args.stats:
        stats(args.stats, args.trace or "thumbs")
        return
    imp.env_start(0)
    try:
        if args.trace:
            trace(args.trace)
            return
        rows = []
        for n in (1, 2, 8, 64):
            rows.append(("brightness", "thumbs224", thumbs(n, 224)))
        for n in (1, 2, 8, 16):
            rows.append(("brightness", "1080p", full_hd(n)))
        for n in (1, 2, 8, 64):
            rows.append(("ascii", "thumbs60", thumbs(n, 60)))
        for exit_, pool, arrs in rows:
            line = json.dumps(row(exit_, pool, arrs, max(30, args.iters)))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")
    finally:
        imp.env_destroy()


if __name__ == "__main__":
    main()
