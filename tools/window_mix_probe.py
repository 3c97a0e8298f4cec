#!/usr/bin/env python3
"""Requests without a resize through impgpu_batch_run_ops, on resident 1920x1080 frames, for two builds of the library in ONE
call: the driver starts a fresh process per side -- parent, branch, parent, branch (IMPGPU_LIB names the library) -- and each
process times every line with events on the env stream.  On a build from before the window launch the batch call IS the
per-request loop, so the same script measures both.
  a  64 and 1024 BGR frames, bare crop to 320x240 at x offsets 0..3
  b  the same, BGRA
  c  64 BGR frames, crop + gamma + a BGRA watermark
  d  64 gray frames, bare crop (promoted to BGR)
  e  a lone impgpu_crop of an unaligned BGR window, 1920x1080 -> 960x540 (k_copy<1> against the 16-byte runs)
The frames are wrapped windows of one device buffer (impgpu_image_wrap), so a call consumes handles, not memory.
3 warm-up calls, then REPEATS windows of CALLS calls; ms per batch = a window / CALLS.
    tools/window_mix_probe.py --parent-lib PATH [--out FILE.jsonl] [--lines abcde] [--repeats 5] [--calls 10]
    tools/window_mix_probe.py --label NAME [...]          # one side, in this process"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib")
ap.add_argument("--label")
ap.add_argument("--out")
ap.add_argument("--lines", default="abcde")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--child-timeout", type=int, default=420)
args = ap.parse_args()

if args.label is None:                                     # the driver: never touches the GPU itself
    if not args.parent_lib:
        ap.error("--parent-lib or --label")
    for rnd in (1, 2):
        for side, lib in (("parent", os.path.abspath(args.parent_lib)), ("branch", None)):
            env = dict(os.environ)
            env.pop("IMPGPU_LIB", None)
            if lib:
                env["IMPGPU_LIB"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--label", "%s-%d" % (side, rnd), "--lines", args.lines,
                   "--repeats", str(args.repeats), "--calls", str(args.calls)] + (["--out", args.out] if args.out else [])
            r = subprocess.run(cmd, env=env, timeout=args.child_timeout)
            if r.returncode != 0:                              # nothing more is started on the device after a failure
                sys.exit("side %s-%d ended with status %d" % (side, rnd, r.returncode))
    sys.exit(0)

import torch
import ngx_http_imgproc_amd as imp
from ngx_http_imgproc_amd._lib import CConfig, CJob

W, H = 1920, 1080
torch.cuda.set_device(0)
imp.env_start(0)
lib = imp.lib
stream = torch.cuda.ExternalStream(lib.impgpu_env_stream())
rng_overlay = torch.randint(0, 256, (30, 76, 4), dtype=torch.uint8).numpy()


def windows_timed(call, after):
    """ms per call: the median, least and largest of REPEATS windows of CALLS calls (`after` runs untimed behind each window)."""
    for k in range(3):
        call(k)
    after()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(args.calls):
            call(k)
        e1.record(stream)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / args.calls)
        after()
    return statistics.median(out), min(out), max(out)


def batch_line(name, n, c, cw, ch, filters=(), watermark=False):
    pool = torch.randint(0, 256, (n, H, W * c), dtype=torch.uint8, device="cuda")     # every frame its own bytes
    torch.cuda.synchronize()
    cfg = imp.Config()
    if watermark:
        assert cfg.prepare_watermark(rng_overlay, "r", "b", 6, 4, 70) == 0
    slots = max(3, args.calls)
    handles = [(C.c_void_p * n)() for _ in range(slots)]
    jobs = (CJob * n)()
    keep = [imp.ops._job(jobs[i], crop="%dpx,%dpx,%dpx,100px" % (cw, ch, 200 + i % 4), filters=list(filters)) for i in range(n)]
    cfgs = (C.POINTER(CConfig) * n)(*[C.pointer(cfg.c) for _ in range(n)])
    codes, steps, launches = (C.c_int * n)(), (C.c_int * n)(), C.c_int()

    def fill():
        for hs in handles:
            for i in range(n):
                h = C.c_void_p()
                assert lib.impgpu_image_wrap(C.c_void_p(pool[i].data_ptr()), W, H, c, W * c, C.byref(h)) == 0
                hs[i] = h.value

    def drain():                                           # the frames the calls left, and fresh handles for the next window
        for hs in handles:
            for i in range(n):
                h = C.c_void_p(hs[i])
                lib.impgpu_image_release(C.byref(h))
        fill()

    def call(k):
        rc = lib.impgpu_batch_run_ops(handles[k % slots], jobs, cfgs, n, codes, steps, C.byref(launches))
        assert rc == 0 and not any(codes), (rc, list(codes)[:4])

    fill()
    med, lo, hi = windows_timed(call, drain)
    out_c = 3 if c == 1 else c
    gb = n * cw * ch * (c + out_c) / 1e9                   # window bytes read plus written
    line = {"label": args.label, "line": name, "requests": n, "channels": c, "launches": launches.value,
            "ms_per_batch_median": round(med, 4), "ms_per_batch_min": round(lo, 4), "ms_per_batch_max": round(hi, 4),
            "requests_per_s": round(n / med * 1e3), "repeats": args.repeats, "calls": args.calls}
    if not filters and not watermark and c != 1:
        line["gb_per_s"] = round(gb / med * 1e3, 1)
    for hs in handles:
        for i in range(n):
            h = C.c_void_p(hs[i])
            lib.impgpu_image_release(C.byref(h))
    cfg.release()
    del keep
    return line


def lone_line():
    frame = torch.randint(0, 256, (H, W * 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    made = []

    def call(k):
        h = C.c_void_p()
        assert lib.impgpu_image_wrap(C.c_void_p(frame.data_ptr()), W, H, 3, W * 3, C.byref(h)) == 0
        assert lib.impgpu_crop(C.byref(h), b"960px,540px,201px,100px", None) == 0
        made.append(h)

    def drain():
        while made:
            lib.impgpu_image_release(C.byref(made.pop()))

    med, lo, hi = windows_timed(call, drain)
    gb = 960 * 540 * 3 * 2 / 1e9
    return {"label": args.label, "line": "e", "requests": 1, "channels": 3, "ms_per_batch_median": round(med, 5),
            "ms_per_batch_min": round(lo, 5), "ms_per_batch_max": round(hi, 5), "gb_per_s": round(gb / med * 1e3, 1),
            "repeats": args.repeats, "calls": args.calls}


lines = []
for name in args.lines:
    todo = {"a": [lambda: batch_line("a", 64, 3, 320, 240), lambda: batch_line("a", 1024, 3, 320, 240)],
            "b": [lambda: batch_line("b", 64, 4, 320, 240), lambda: batch_line("b", 1024, 4, 320, 240)],
            "c": [lambda: batch_line("c", 64, 3, 320, 240, filters=["gamma=1.4"], watermark=True)],
            "d": [lambda: batch_line("d", 64, 1, 320, 240)],
            "e": [lone_line]}[name]
    for f in todo:
        lines.append(json.dumps(f()))
        print(lines[-1], flush=True)
if args.out:
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
imp.env_destroy()
