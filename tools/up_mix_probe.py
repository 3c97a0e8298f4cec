#!/usr/bin/env python3
"""Mixed-size batches of CUBIC enlargements on resident frames, through impgpu_batch_resize_mixed alone (so the same script
times any build: IMPGPU_LIB names the library).  Three mixes, BGR and BGRA:
  a  64 frames, sources drawn from 160..480 wide at 4:3 and 16:9, each to 640 wide
  b  1024 of the same
  c  64 frames, all 480x270 -> 1920x1080: alone each runs the PS = 4 kernel, in the mix the generic footprint advance
and, as a control of the lone kernels (they share their body with the mix kernel):
  d  the 64 frames of c as ONE uniform batch through impgpu_batch_cv_resize (k_resize_up_cubic3/4<4>, in any build)
Event timing on one stream: 3 warm-up calls, then REPEATS windows of CALLS calls each; ms per batch = a window / CALLS.
host_ms_per_call is the host clock around the same calls: what a call costs the calling thread before it returns.
    tools/up_mix_probe.py --label parent-1 [--out FILE.jsonl] [--mixes abcd] [--repeats 7] [--calls 10]"""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ngx_http_imgproc_amd as imp

ap = argparse.ArgumentParser()
ap.add_argument("--label", required=True)
ap.add_argument("--out")
ap.add_argument("--mixes", default="abcd")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--calls", type=int, default=10)
args = ap.parse_args()

torch.cuda.set_device(0)
imp.env_start(0)
stream = torch.cuda.Stream()
INTER_CUBIC = 2


def geometry(mix):
    if mix in "cd":
        return [(480, 270, 1920, 1080)] * 64
    rng = np.random.Generator(np.random.PCG64(0x0B1C))
    out = []
    for k in range(64 if mix == "a" else 1024):
        sw = int(rng.integers(160, 481))
        sh = sw * 3 // 4 if k % 2 else sw * 9 // 16
        out.append((sw, sh, 640, max(1, round(sh * 640 / sw))))
    return out


def measure(mix, c, pool):
    geo = geometry(mix)
    items, off, dsts = [], 0, []
    if mix == "d":
        sw, sh, dw, dh = geo[0]
        dst = torch.zeros((len(geo), dh, dw, c), dtype=torch.uint8, device="cuda")
    for sw, sh, dw, dh in geo:                         # every frame its own bytes of the pool
        if mix != "d":
            dsts.append(torch.zeros((dh, dw, c), dtype=torch.uint8, device="cuda"))
            items.append((pool.data_ptr() + off, sw, sh, sw * c, dsts[-1].data_ptr(), dw, dh, dw * c))
        off += (sw * sh * c + 255) & ~255
    assert off <= pool.numel()
    arr = (imp.ResizeItem * len(items))(*[imp.ResizeItem(*it) for it in items])

    def call():
        if mix == "d":
            stride = (sw * sh * c + 255) & ~255
            rc = imp.lib.impgpu_batch_cv_resize(C.c_void_p(pool.data_ptr()), stride, sw, sh, sw * c, C.c_void_p(dst.data_ptr()),
                                                dw * dh * c, dw, dh, dw * c, c, len(geo), INTER_CUBIC, C.c_void_p(stream.cuda_stream))
        else:
            rc = imp.lib.impgpu_batch_resize_mixed(arr, len(items), c, 0, stream.cuda_stream)
        assert rc == 0, rc

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    windows, host = [], []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        host.append((time.perf_counter() - t0) * 1e3 / args.calls)     # the host's time inside a call (planning, tables, enqueue)
        e1.record(stream)
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / args.calls)
    gb = sum((sw * sh + dw * dh) * c for sw, sh, dw, dh in geo) / 1e9
    med = statistics.median(windows)
    return {"label": args.label, "mix": mix, "channels": c, "frames": len(geo), "ms_per_batch_median": round(med, 4),
            "ms_per_batch_min": round(min(windows), 4), "ms_per_batch_max": round(max(windows), 4),
            "host_ms_per_call_median": round(statistics.median(host), 4),
            "frames_per_s": round(len(geo) / med * 1e3), "gb_per_s": round(gb / med * 1e3, 1),
            "repeats": args.repeats, "calls": args.calls}


need = max(sum((w * h * 4 + 255) & ~255 for w, h, _, _ in geometry(m)) for m in args.mixes)
pool = torch.randint(0, 256, (need,), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
lines = []
for mix in args.mixes:
    for c in (3, 4):
        lines.append(json.dumps(measure(mix, c, pool)))
        print(lines[-1], flush=True)
if args.out:
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
imp.env_destroy()
