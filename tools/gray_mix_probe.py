#!/usr/bin/env python3
"""Gray frames of all-different sizes (bench.py --mixed's size distribution, workloads.mixed_sizes) -> 224-wide thumbnails,
resident in HBM, on any build (IMPGPU_LIB names the library):
  resize   one impgpu_batch_resize_mixed_ex call, channels = 1
  ops      the same queue through impgpu_batch_run_ops, bare resize=224,0
  ops+f    ... with filter gamma=1.4 and a BGRA overlay
Per mode: wall ms per call (host issue + one wait, median of REPEATS), host issue ms (the call's own return, before the
wait), kernels enqueued, microseconds per frame.
    tools/gray_mix_probe.py --label parent [--out FILE.jsonl] [--frames 64,256] [--repeats 9] [--modes resize,ops,ops+f]
(under `rocprofv3 --kernel-trace --stats`, `--modes resize --frames 64` gives the kernels of the resize call alone)"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ngx_http_imgproc_amd as imp
from ngx_http_imgproc_amd.workloads import mixed_sizes

ap = argparse.ArgumentParser()
ap.add_argument("--label", required=True)
ap.add_argument("--out")
ap.add_argument("--frames", default="64,256")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--modes", default="resize,ops,ops+f")
args = ap.parse_args()

torch.cuda.set_device(0)
imp.env_start(0)
rng = np.random.Generator(np.random.PCG64(0x1A4D9000))


def stats(walls, issues, launches, n, mode):
    w, i = statistics.median(walls), statistics.median(issues)
    return {"label": args.label, "mode": mode, "frames": n, "wall_ms_median": round(w, 4), "wall_ms_min": round(min(walls), 4),
            "wall_ms_max": round(max(walls), 4), "issue_ms_median": round(i, 4), "launches": launches,
            "us_per_frame": round(w * 1e3 / n, 2), "repeats": args.repeats}


def resize_mode(n):
    sizes = mixed_sizes(n)
    srcs, dsts, items = [], [], []
    for w, h in sizes:
        dw, dh = 224, max(1, int(round(224 * h / w)))
        step = (w + 3) & ~3
        srcs.append(torch.randint(0, 256, (h, step), dtype=torch.uint8, device="cuda"))
        dsts.append(torch.zeros((dh, (dw + 3) & ~3), dtype=torch.uint8, device="cuda"))
        items.append((srcs[-1].data_ptr(), w, h, step, dsts[-1].data_ptr(), dw, dh, (dw + 3) & ~3))
    walls, issues, launches = [], [], 0
    for r in range(args.repeats + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc, launches = imp.batch_resize_mixed(items, 1, count_launches=True)
        t1 = time.perf_counter()
        imp.sync()
        t2 = time.perf_counter()
        assert rc == 0, rc
        if r >= 2:
            walls.append((t2 - t0) * 1e3)
            issues.append((t1 - t0) * 1e3)
    return stats(walls, issues, launches, n, "resize")


def ops_mode(n, filtered):
    sizes = mixed_sizes(n)
    frames = [rng.integers(0, 256, size=(h, w, 1), dtype=np.uint8) for w, h in sizes]
    cfg = imp.Config()
    job = dict(resize="224,0")
    if filtered:
        assert cfg.prepare_watermark(rng.integers(0, 256, size=(30, 76, 4), dtype=np.uint8), "r", "b", 6, 4, 70) == 0
        job["filters"] = ["gamma=1.4"]
    walls, issues, launches = [], [], 0
    for r in range(args.repeats + 2):
        ims = [imp.Image(a) for a in frames]                       # (the call consumes its frames: uploaded anew, untimed)
        imp.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res, launches = imp.batch_run_ops(ims, [cfg] * n, [job] * n)
        t1 = time.perf_counter()
        imp.sync()
        t2 = time.perf_counter()
        assert all(rc == 0 for rc, _ in res), res[:4]
        for im in ims:
            im.release()
        if r >= 2:
            walls.append((t2 - t0) * 1e3)
            issues.append((t1 - t0) * 1e3)
    cfg.release()
    return stats(walls, issues, launches, n, "ops+f" if filtered else "ops")


lines = []
for n in (int(v) for v in args.frames.split(",")):
    for mode in args.modes.split(","):
        line = resize_mode(n) if mode == "resize" else ops_mode(n, mode == "ops+f")
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
if args.out:
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
imp.env_destroy()
