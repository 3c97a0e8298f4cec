#!/usr/bin/env python3
"""Wide Gaussian blurs (the two-pass matrix-unit form: blur=8) of a request queue, through impgpu_batch_run_ops alone, and
the lone kernel pair as a guard.  --root names the checkout whose package and library are timed (default: this one), so
the same script times the commit before and after; alternate them in one session.  Requests are whole thumbnails with one
blur filter, so a call launches nothing but the blurs; each call blurs the frames the call before left (same geometry).
  a  64 thumbnails of 64 different sizes around 224 wide, blur=8
  b  1024 of them (the 64 sizes, sixteen times)
  c  the 64 of a with sigmas 6, 7 .. 16 in turn
  d  the lone pair k_blur_mfma_rows + k_blur_mfma_cols: one 1920x1080 BGRA frame, impgpu_filter blur=8
  e  the same at blur=16
Host clock around a window of calls that ends in impgpu_sync: 3 warm-up calls, then REPEATS windows of CALLS calls;
ms per call = a window / CALLS.  launches is what one call enqueued.
    tools/blur_mix_probe.py --label parent-1 [--root DIR] [--out FILE.jsonl] [--mixes abcde] [--repeats 5] [--calls 10]"""
import argparse, ctypes as C, json, os, statistics, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--label", required=True)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out")
ap.add_argument("--mixes", default="abcde")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=10)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import numpy as np
import torch  # noqa: F401  (first: one HIP runtime per process)
import ngx_http_imgproc_amd as imp
from ngx_http_imgproc_amd._lib import CConfig, CJob
from ngx_http_imgproc_amd.ops import _job

imp.env_start(0)
lib = imp.lib
rng = np.random.Generator(np.random.PCG64(0x0B17))


def sizes(n):
    return [(192 + k % 64, (192 + k % 64) * (3 if k % 2 else 9) // (4 if k % 2 else 16)) for k in range(n)]


def windows(call, calls):
    for _ in range(3):
        call()
    imp.sync()
    out = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        imp.sync()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def batch(mix, c):
    n = 1024 if mix == "b" else 64
    ims = [imp.Image(rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)) for w, h in sizes(n)]
    handles = (C.c_void_p * n)(*[im.h.value for im in ims])
    cfg = imp.Config(allow_experiments=True)
    cfgs = (C.POINTER(CConfig) * n)(*[C.pointer(cfg.c)] * n)
    jobs = (CJob * n)()
    keep = [_job(jobs[i], filters=["blur=%d" % (6 + i % 11 if mix == "c" else 8)]) for i in range(n)]  # noqa: F841
    codes, steps, launches = (C.c_int * n)(), (C.c_int * n)(), C.c_int()

    def call():
        rc = lib.impgpu_batch_run_ops(handles, jobs, cfgs, n, codes, steps, C.byref(launches))
        assert rc == 0 and not any(codes), (rc, list(codes)[:8])

    ms = windows(call, max(1, args.calls // 4) if mix == "b" else args.calls)
    for i, im in enumerate(ims):                           # the handles the last call left
        im.h = C.c_void_p(handles[i])
        im.release()
    return ms, launches.value, n


def lone(mix):
    im = imp.Image(rng.integers(0, 256, size=(1080, 1920, 4), dtype=np.uint8))
    request = b"blur=8" if mix == "d" else b"blur=16"

    def call():
        rc = lib.impgpu_filter(C.byref(im.h), request, 1)
        assert rc == 0, rc

    ms = windows(call, 4 * args.calls)
    im.release()
    return ms, 2, 1


lines = []
for mix in args.mixes:
    for c in ((3, 4) if mix in "abc" else (4,)):
        ms, launches, n = batch(mix, c) if mix in "abc" else lone(mix)
        med = statistics.median(ms)
        lines.append(json.dumps({"label": args.label, "mix": mix, "channels": c, "frames": n, "launches_per_call": launches,
                                 "ms_per_call_median": round(med, 4), "ms_per_call_min": round(min(ms), 4),
                                 "ms_per_call_max": round(max(ms), 4), "frames_per_s": round(n / med * 1e3),
                                 "repeats": args.repeats}))
        print(lines[-1], flush=True)
if args.out:
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
imp.env_destroy()
