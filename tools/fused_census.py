"""How many files of a pool take impgpu_batch_run_ops' shared launch under a given request, and how many go through
impgpu_run_ops one by one.  Each file is decoded and run TWICE in one call: two requests that ride the mixed launch share
its one kernel (launches == 1); two that do not take at least one launch each.  One JSON line per query.
    python tools/fused_census.py --query "crop=16,9&resize=224,0" --watermark r,b,6,4,70 [--pool FILE]"""
import argparse
import json
import os
import struct
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--query", action="append", required=True)
    ap.add_argument("--watermark", action="append", default=None, help="placement per --query ('-': none)")
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
    marks = args.watermark or ["-"] * len(args.query)
    imp.env_start(0)
    try:
        for query, mark in zip(args.query, marks):
            cfg = imp.Config()
            if mark != "-":
                gx, gy, ox, oy, op = mark.split(",")
                assert cfg.prepare_watermark(ws.overlay_frame(), gx, gy, int(ox), int(oy), int(op)) == 0
            req = imp.Request("/pool.jpg?" + query, "jpg", cfg)
            job = dict(crop=req.crop, gravity=req.gravity, resize=req.resize, simple=req.simple, filters=req.filters,
                       need_flatten=req.need_flatten)
            fused, errors = 0, 0
            for b in blobs:
                rc, a = imp.Image.decode_jpeg(b)
                assert rc == 0
                pair = [a, a.clone()]
                res, launches = imp.batch_run_ops(pair, [cfg, cfg], [job, job])
                errors += sum(1 for code, _ in res if code)
                fused += launches == 1
                for im in pair:
                    im.release()
            print(json.dumps({"query": query, "watermark": None if mark == "-" else mark, "files": len(blobs), "fused": fused,
                              "run_ops": len(blobs) - fused, "errors": errors}), flush=True)
            cfg.release()
    finally:
        imp.env_destroy()


if __name__ == "__main__":
    main()
