#!/usr/bin/env python3
"""AREA shrinks past 18x (cells of 21..66 source columns) of resident phone-photo frames, through impgpu_batch_cv_resize and
impgpu_batch_resize_mixed alone (so the same script times any build: IMPGPU_LIB names the library).  Kinds of frame:
  bgr, bgra  4-byte aligned rows and starts (what cvCreateImage makes)
  bgr-off    BGR off the 4-byte grid: the window starts 1..3 pixels into a wider frame (a crop folded into the resize)
  gray       one channel; the photo sizes are replaced by a 600 dpi A4 scan, 4960x3508 (33x at 150 wide), at 100..160 wide
Cases:
  lone150   one 4032x3024 -> 150x113 frame, one launch                                  (26.9x)
  lone224   one 6000x4000 -> 224x149 frame, one launch                                  (26.8x)
  mix64     64 frames, 4032x3024 and 3024x4032 in turn, at 120..200 wide, one impgpu_batch_resize_mixed call
  fresh64   the same 64 frames with geometries no earlier call had (dw moves with the call, dh grows by one a call), so a
            build that needs per-geometry tables builds them every call: HOST clock around the calls and one synchronise
Event timing on one stream for the first three: 3 warm-up calls, then REPEATS windows of CALLS calls each; ms per call = a
window / CALLS.
    tools/wide_area_probe.py --label parent-1 [--out FILE.jsonl] [--cases lone150,lone224,mix64,fresh64] [--kinds bgr,bgra,gray,bgr-off]
                             [--repeats 7]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import ngx_http_imgproc_amd as imp

ap = argparse.ArgumentParser()
ap.add_argument("--label", required=True)
ap.add_argument("--out")
ap.add_argument("--cases", default="lone150,lone224,mix64,fresh64")
ap.add_argument("--kinds", default="bgr,bgra,gray,bgr-off")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--calls", type=int, default=10)
args = ap.parse_args()
INTER_AREA = 3

torch.cuda.set_device(0)
imp.env_start(0)
stream = torch.cuda.Stream()


def timed(call, calls, host_clock=False):
    """ms per call: the median, the least and the most of REPEATS windows.  call(k) is the k-th call since the start."""
    k = 0
    for _ in range(3):
        call(k)
        k += 1
    torch.cuda.synchronize()
    windows = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        for _ in range(calls):
            call(k)
            k += 1
        e1.record(stream)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        windows.append((t1 - t0) * 1e3 / calls if host_clock else e0.elapsed_time(e1) / calls)
    return round(statistics.median(windows), 4), round(min(windows), 4), round(max(windows), 4)


CHANNELS = {"bgr": 3, "bgra": 4, "gray": 1, "bgr-off": 3}
SCAN = (4960, 3508)


def lone(sw, sh, dw, dh, kind, pool):
    c = CHANNELS[kind]
    ox = 1 if kind == "bgr-off" else 0                 # the window starts one pixel into a frame four pixels wider: pointer % 4 = 3
    pitch = (sw + 4 * ox) * c
    dst = torch.zeros((dh, dw, c), dtype=torch.uint8, device="cuda")

    def call(_):
        rc = imp.lib.impgpu_batch_cv_resize(pool.data_ptr() + ox * c, 0, sw, sh, pitch, dst.data_ptr(), 0, dw, dh, dw * c, c, 1, INTER_AREA,
                                            stream.cuda_stream)
        assert rc == 0, rc

    return call, (sw * sh + dw * dh) * c / 1e9, 1


def mixed(kind, pool, fresh):
    c = CHANNELS[kind]
    long_side, short_side = SCAN if kind == "gray" else (4032, 3024)
    lo, span = (100, 61) if kind == "gray" else (120, 81)
    src, off = [], 0
    for i in range(64):                                # every frame its own bytes of the pool
        sw, sh = (long_side, short_side) if i % 2 == 0 else (short_side, long_side)
        ox = 1 + i % 3 if kind == "bgr-off" else 0     # pointer % 4 = 3, 2, 1 in turn; the pitch stays a multiple of 4
        pitch = (sw + 4 * (ox > 0)) * c
        src.append((pool.data_ptr() + off + ox * c, sw, sh, pitch))
        off += (pitch * sh + 255) & ~255
    assert off <= pool.numel()
    dst = torch.zeros((64, 400 * 200 * c), dtype=torch.uint8, device="cuda")      # (room for the tallest thumbnail, 266 rows, plus the shift)

    def items(k):
        out = []
        for i, (p, sw, sh, pitch) in enumerate(src):
            dw = lo + ((i * 5 + k) % span if fresh else (i * 5) % span)
            dh = max(1, dw * sh // sw) + (k if fresh else 0)          # (dw, dh + k): no call repeats a geometry of an earlier one
            out.append(imp.ResizeItem(p, sw, sh, pitch, dst[i].data_ptr(), dw, dh, dw * c))
        return (imp.ResizeItem * 64)(*out)

    fixed = items(0)

    def call(k):
        arr = items(k) if fresh else fixed
        rc = imp.lib.impgpu_batch_resize_mixed(arr, 64, c, 0, stream.cuda_stream)
        assert rc == 0, rc

    return call, sum(sw * sh for _, sw, sh, _ in src) * c / 1e9, 64


need = 64 * ((4036 * 3024 * 4 + 255) & ~255)
pool = torch.randint(0, 256, (need,), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
lines = []
for case in args.cases.split(","):
    for kind in args.kinds.split(","):
        c = CHANNELS[kind]
        if case == "lone150":
            call, gb, frames = lone(*(SCAN + (150, 106) if kind == "gray" else (4032, 3024, 150, 113)), kind, pool)
        elif case == "lone224":
            call, gb, frames = lone(6000, 4000, 224, 149, kind, pool)
        else:
            call, gb, frames = mixed(kind, pool, case == "fresh64")
        calls = args.calls * (10 if frames == 1 else 1)
        med, lo, hi = timed(call, calls, host_clock=(case == "fresh64"))
        lines.append(json.dumps({"label": args.label, "case": case, "kind": kind, "channels": c, "frames": frames, "clock": "host" if case == "fresh64" else "events",
                                 "ms_per_call_median": med, "ms_per_call_min": lo, "ms_per_call_max": hi, "gb_per_s": round(gb / med * 1e3, 1),
                                 "repeats": args.repeats, "calls": calls}))
        print(lines[-1], flush=True)
if args.out:
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
imp.env_destroy()
