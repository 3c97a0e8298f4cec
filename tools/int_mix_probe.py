#!/usr/bin/env python3
"""Mixed-size batches of whole-factor AREA shrinks on resident frames, through impgpu_batch_resize_mixed alone (so the same
script times any build: IMPGPU_LIB names the library).  Three mixes, BGR and BGRA:
  a  64 frames of the usual source sizes (640x480 ... 3840x2160) at 320 wide: factors 2, 3, 4, 5, 6, 8, 12
  b  1024 of the same
  c  64 frames, all 3840x2160 -> 480x270 (8x)
Event timing on one stream: 3 warm-up calls, then REPEATS windows of CALLS calls each; ms per batch = a window / CALLS.
    tools/int_mix_probe.py --label parent-1 [--out FILE.jsonl] [--mixes abc] [--repeats 7] [--calls 20]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import ngx_http_imgproc_amd as imp

SIZES = [(640, 480), (960, 540), (1280, 720), (1600, 900), (1920, 1080), (2560, 1440), (3840, 2160)]
ap = argparse.ArgumentParser()
ap.add_argument("--label", required=True)
ap.add_argument("--out")
ap.add_argument("--mixes", default="abc")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
args = ap.parse_args()

torch.cuda.set_device(0)
imp.env_start(0)
stream = torch.cuda.Stream()


def geometry(mix):
    if mix == "c":
        return [(3840, 2160, 480, 270)] * 64
    n = 64 if mix == "a" else 1024
    return [(w, h, 320, 320 * h // w) for w, h in (SIZES[k % len(SIZES)] for k in range(n))]


def measure(mix, c, pool):
    geo = geometry(mix)
    items, off, dsts = [], 0, []
    for sw, sh, dw, dh in geo:                         # every frame its own bytes of the pool: nothing is served from a cache twice
        dsts.append(torch.zeros((dh, dw, c), dtype=torch.uint8, device="cuda"))
        items.append((pool.data_ptr() + off, sw, sh, sw * c, dsts[-1].data_ptr(), dw, dh, dw * c))
        off += (sw * sh * c + 255) & ~255
    assert off <= pool.numel()
    arr = (imp.ResizeItem * len(items))(*[imp.ResizeItem(*it) for it in items])

    def call():
        rc = imp.lib.impgpu_batch_resize_mixed(arr, len(items), c, 0, stream.cuda_stream)
        assert rc == 0, rc

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    windows = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.calls):
            call()
        e1.record(stream)
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / args.calls)
    gb = sum((sw * sh + dw * dh) * c for sw, sh, dw, dh in geo) / 1e9
    med = statistics.median(windows)
    return {"label": args.label, "mix": mix, "channels": c, "frames": len(geo), "ms_per_batch_median": round(med, 4),
            "ms_per_batch_min": round(min(windows), 4), "ms_per_batch_max": round(max(windows), 4),
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
