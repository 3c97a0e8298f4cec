"""The kernels of impgpu_batch_run_ops on a broker-sized batch, for `rocprofv3 --kernel-trace --stats`: the first 64 files
of the mixed-size pool, decoded once, then run REPS times as resize=224,0 + a watermark (k_resize_area_mix_tail) and REPS
times as the bare resize=224,0 (k_resize_area_mix), alternated.  Each call works on clones, so both see the same frames.
    rocprofv3 --kernel-trace --stats -d OUT -o trace -- python tools/batch_ops_trace.py [--reps 20] [--count 64]"""
import argparse
import json
import os
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--watermark", default="r,b,6,4,70")
    ap.add_argument("--pool", default=os.path.join(tempfile.gettempdir(), "impgpu_jpeg_pool_64.bin"),
                    help="the 64-file mixed-size pool (bench.jpeg_pool; written there when missing)")
    args = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see ngx_http_imgproc_amd/_lib.py)
    import ngx_http_imgproc_amd as imp
    import worker_scaling as ws

    ws.make_pool(args.pool)
    with open(args.pool, "rb") as f:
        data = f.read()
    n, at, blobs = struct.unpack_from("<I", data, 0)[0], 4, []
    for _ in range(n):
        sz = struct.unpack_from("<I", data, at)[0]
        blobs.append(data[at + 4:at + 4 + sz])
        at += 4 + sz
    blobs = (blobs * ((args.count + len(blobs) - 1) // len(blobs)))[:args.count]
    imp.env_start(0)
    try:
        frames = [imp.batch_decode_jpeg([b])[0][1] for b in blobs]
        plain, marked = imp.Config(), imp.Config()
        gx, gy, ox, oy, op = args.watermark.split(",")
        assert marked.prepare_watermark(ws.overlay_frame(), gx, gy, int(ox), int(oy), int(op)) == 0
        job = dict(resize="224,0")
        out = {}
        for rep in range(args.reps):
            for name, cfg in (("watermark", marked), ("bare", plain)):
                ims = [f.clone() for f in frames]
                imp.sync()
                t0 = time.perf_counter()
                res, launches = imp.batch_run_ops(ims, [cfg] * len(ims), [job] * len(ims))
                imp.sync()
                dt = time.perf_counter() - t0
                assert all(code == 0 for code, _ in res), res
                o = out.setdefault(name, {"launches": launches, "us": []})
                o["us"].append(round(dt * 1e6, 1))
                for im in ims:
                    im.release()
        for name, o in out.items():
            us = sorted(o["us"][1:] or o["us"])
            print(json.dumps({"batch": name, "requests": len(frames), "launches": o["launches"], "host_us_p50": us[len(us) // 2],
                              "host_us_min": us[0]}), flush=True)
        for f in frames:
            f.release()
        marked.release()
    finally:
        imp.env_destroy()


if __name__ == "__main__":
    main()
