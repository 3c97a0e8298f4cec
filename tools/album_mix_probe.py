"""Albums through the batched operator and FreeImage exits on one device -> one JSON line per row and profiles/album_mix_probe.json.

16 and 64 BGRA albums of 8 frames, 200 x 150 to 400 x 300, each asked resize=100,0 with simple=1 (the GIF route, bridge.c:594) and
a 32-bit FreeImage answer for every frame:
  (a) loop  -- per request impgpu_run_ops + impgpu_album_download_fi: a launch per operator, a k_pack_fi launch per frame and a
               wait per request (the only route before albums' frames joined the shared launches)
  (b) batch -- ONE impgpu_batch_run_ops + ONE impgpu_batch_download_fi
Times are wall time around work that ends in the download's wait (the bitmaps are in host memory when the clock stops),
medians over --iters calls after warm-up, microseconds, the two forms alternating call by call so that a drift of the machine
lands on both; fresh clones of the albums are made, and waited for, outside the timed region.  Launches: (b) as the two calls
report them; (a) as a one-request impgpu_batch_run_ops reports impgpu_run_ops' launches for that album (a lone album is answered
by impgpu_run_ops there) plus one k_pack_fi launch per frame.

    timeout -k 10 600 python tools/album_mix_probe.py [--iters 30] [--out profiles/album_mix_probe.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch  # noqa: F401  (first: the HIP runtime torch bundles, as in bench.py)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, BPP = 8, 32
JOB = dict(resize="100,0", simple=1)


def sizes(count):
    """`count` canvases from 200 x 150 to 400 x 300, all different for count <= 64"""
    return [(200 + (200 * k) // max(1, count - 1), 150 + (150 * k) // max(1, count - 1)) for k in range(count)]


def rows_for(imp, count, iters):
    from ngx_http_imgproc_amd._lib import CConfig, CJob
    from ngx_http_imgproc_amd.ops import _job

    lib = imp.lib
    rng = np.random.default_rng(9100 + count)
    sources = [imp.Image.album([rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(FRAMES)]) for w, h in sizes(count)]
    cfg = imp.Config()
    jobs = (CJob * count)()
    keep = [_job(jobs[i], **JOB) for i in range(count)]  # noqa: F841
    cfgs = (C.POINTER(CConfig) * count)(*[C.pointer(cfg.c) for _ in range(count)])
    codes, steps, launches = (C.c_int * count)(), (C.c_int * count)(), C.c_int()
    # the answers' bitmaps: 100 pixels wide, the height resize_geometry gives each canvas
    dims = [imp.resize_geometry(w, h, JOB["resize"], cfg, 1)[1][:2] for w, h in sizes(count)]
    pitch = (100 * BPP // 8 + 3) & ~3
    maps = [[np.empty((dh, pitch), np.uint8) for _ in range(FRAMES)] for dw, dh in dims]
    assert all(dw == 100 for dw, dh in dims), dims
    bits = (C.c_void_p * (count * FRAMES))(*[m.ctypes.data for ms in maps for m in ms])
    pitches = (C.c_int * (count * FRAMES))(*[pitch] * (count * FRAMES))
    bits_of = [(C.c_void_p * FRAMES)(*[m.ctypes.data for m in ms]) for ms in maps]       # the same bitmaps, per album
    bpps = (C.c_int * count)(*[BPP] * count)
    seen = {}

    def clones():
        hs = (C.c_void_p * count)()
        for i, s in enumerate(sources):
            h = C.c_void_p()
            assert lib.impgpu_image_clone(s.h, C.byref(h)) == 0
            hs[i] = h.value
        imp.sync()
        return hs

    def release(hs):
        for i in range(count):
            lib.impgpu_image_release(C.byref(C.c_void_p(hs[i])))

    def loop(hs):
        step = C.c_int()
        for i in range(count):
            h = C.c_void_p(hs[i])
            assert lib.impgpu_run_ops(C.byref(h), C.byref(jobs[i]), cfgs[i], C.byref(step)) == 0
            hs[i] = h.value
            assert lib.impgpu_album_download_fi(h, BPP, bits_of[i], pitches) == 0

    def batch(hs):
        assert lib.impgpu_batch_run_ops(hs, jobs, cfgs, count, codes, steps, C.byref(launches)) == 0 and not any(codes), list(codes)
        seen["ops"] = launches.value
        assert lib.impgpu_batch_download_fi(hs, bpps, count, bits, pitches, codes, C.byref(launches)) == 0 and not any(codes), list(codes)
        seen["exit"] = launches.value

    def timed(fn):
        hs = clones()
        t0 = time.perf_counter()
        fn(hs)
        dt = time.perf_counter() - t0
        release(hs)
        return dt * 1e6, [m.copy() for ms in maps for m in ms] if not seen.get("checked") else None

    # the two routes give the same bitmaps
    _, a = timed(loop)
    _, b = timed(batch)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "the batched route's bitmaps differ from the loop's"
    seen["checked"] = True
    # impgpu_run_ops' launches for one album, as a one-request batch call reports them
    hs = clones()
    loop_launches = 0
    for i in range(count):
        one = (C.c_void_p * 1)(hs[i])
        assert lib.impgpu_batch_run_ops(one, C.byref(jobs[i]), (C.POINTER(CConfig) * 1)(cfgs[i]), 1, codes, steps, C.byref(launches)) == 0
        assert codes[0] == 0
        hs[i] = one[0]
        loop_launches += launches.value + FRAMES
    imp.sync()
    release(hs)
    for _ in range(3):
        timed(loop), timed(batch)
    ta, tb = [], []
    for k in range(iters):
        for fn, ts in ((loop, ta), (batch, tb)) if k % 2 == 0 else ((batch, tb), (loop, ta)):
            ts.append(timed(fn)[0])
    ta.sort(), tb.sort()
    for s in sources:
        s.release()
    cfg.release()
    out_bytes = sum(dh * pitch * FRAMES for dw, dh in dims)
    return {"probe": "album_mix", "albums": count, "frames_each": FRAMES, "canvases": [sizes(count)[0], sizes(count)[-1]], "job": JOB, "bpp": BPP,
            "iters": iters, "answer_bytes": out_bytes,
            "loop_us": round(ta[len(ta) // 2], 1), "batch_us": round(tb[len(tb) // 2], 1),
            "loop_min_max_us": [round(ta[0], 1), round(ta[-1], 1)], "batch_min_max_us": [round(tb[0], 1), round(tb[-1], 1)],
            "speedup": round(ta[len(ta) // 2] / tb[len(tb) // 2], 3),
            "loop_launches": loop_launches, "loop_waits": count,
            "batch_launches": seen["ops"] + seen["exit"], "batch_ops_launches": seen["ops"], "batch_exit_launches": seen["exit"], "batch_waits": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "album_mix_probe.json"))
    a = ap.parse_args()
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    rows = []
    for count in (16, 64):
        rows.append(rows_for(imp, count, a.iters))
        print(json.dumps(rows[-1]), flush=True)
    imp.env_destroy()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
