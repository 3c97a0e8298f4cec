"""impgpu_batch_run_ops on filtered requests, against the per-request loop, for a plain run and for
`rocprofv3 --kernel-trace --stats`: the first 64 files of the mixed-size pool, decoded once, then run REPS times as
resize=224,0 + a watermark + a flatten + one of {gamma, blur=2, gotham, flip=01 + blur=1.5} (request k takes chain k mod 4),
alternating the batch with the loop of impgpu_run_ops.  Each call works on clones, so both see the same frames; each records
its wall time to a sync (and the batch its kernel count).
    python tools/batch_chains_trace.py [--reps 20] [--count 64]
    rocprofv3 --kernel-trace --stats -d OUT -o trace -- python tools/batch_chains_trace.py
--lone: the lone kernels instead -- filter-blur (sigma 0.5, 2, 8) and a pointwise program (gamma; gotham) on one 1920x1080
BGRA frame per call -- to compare two builds (IMPGPU_LIB).
--lds A|B: k_blur_mix's LDS policy, one process per side under rocprofv3 --kernel-trace: A = the 64 files as resize=224,0 +
blur=1.5 (one radius); B = the same 64 plus one 48x64 frame with blur=LDS_SIGMA, so the launch is sized for that larger radius
while its work barely grows.  Grouping by radius would instead pay A's launch plus a launch for the small frame."""
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

CHAINS = [["gamma=1.4"], ["blur=2"], ["gotham=1"], ["flip=01", "blur=1.5"]]


def _pool(path, count):
    import worker_scaling as ws

    ws.make_pool(path)
    with open(path, "rb") as f:
        data = f.read()
    n, at, blobs = struct.unpack_from("<I", data, 0)[0], 4, []
    for _ in range(n):
        sz = struct.unpack_from("<I", data, at)[0]
        blobs.append(data[at + 4:at + 4 + sz])
        at += 4 + sz
    return (blobs * ((count + len(blobs) - 1) // len(blobs)))[:count]


def lone(imp, reps):
    import numpy as np

    rng = np.random.Generator(np.random.PCG64(7))
    base = imp.Image(rng.integers(0, 256, size=(1080, 1920, 4), dtype=np.uint8))
    for req in ["blur=0.5", "blur=2", "blur=8", "gamma=1.4", "gotham=1"]:
        imgs = [base.clone() for _ in range(reps)]
        w = base.clone()
        assert w.filter(req, 1) == 0
        w.release()
        imp.sync()
        t0 = time.perf_counter()
        for im in imgs:
            assert im.filter(req, 1) == 0
        imp.sync()
        dt = (time.perf_counter() - t0) / reps
        print(json.dumps({"lone": req, "frame": "1920x1080x4", "us_per_frame": round(dt * 1e6, 1)}), flush=True)
        for im in imgs:
            im.release()
    base.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--watermark", default="r,b,6,4,70")
    ap.add_argument("--lone", action="store_true")
    ap.add_argument("--lds", choices=["A", "B"])
    ap.add_argument("--lds-sigma", default="5")
    ap.add_argument("--pool", default=os.path.join(tempfile.gettempdir(), "impgpu_jpeg_pool_64.bin"),
                    help="the 64-file mixed-size pool (bench.jpeg_pool; written there when missing)")
    args = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see ngx_http_imgproc_amd/_lib.py)
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    try:
        if args.lone:
            lone(imp, max(args.reps, 48))
            return
        import worker_scaling as ws

        blobs = _pool(args.pool, args.count)
        frames = [imp.batch_decode_jpeg([b])[0][1] for b in blobs]
        cfg = imp.Config(allow_experiments=True)
        if not args.lds:
            gx, gy, ox, oy, op = args.watermark.split(",")
            assert cfg.prepare_watermark(ws.overlay_frame(), gx, gy, int(ox), int(oy), int(op)) == 0
        jobs = [dict(resize="224,0", filters=CHAINS[k % len(CHAINS)], need_flatten=1) for k in range(len(frames))]
        if args.lds:
            import numpy as np

            jobs = [dict(resize="224,0", filters=["blur=1.5"]) for _ in frames]
            if args.lds == "B":
                frames.append(imp.Image(np.random.Generator(np.random.PCG64(5)).integers(0, 256, size=(48, 64, 3), dtype=np.uint8)))
                jobs.append(dict(resize="40,0", filters=["blur=" + args.lds_sigma]))
        out = {}
        for rep in range(args.reps):
            for name in (("batch",) if args.lds else ("batch", "loop")):
                ims = [f.clone() for f in frames]
                imp.sync()
                t0 = time.perf_counter()
                if name == "batch":
                    res, launches = imp.batch_run_ops(ims, [cfg] * len(ims), jobs)
                else:
                    res, launches = [imp.run_ops(im, cfg, **j) for im, j in zip(ims, jobs)], None
                imp.sync()
                dt = time.perf_counter() - t0
                assert all(code == 0 for code, _ in res), res
                o = out.setdefault(name, {"launches": launches, "us": []})
                o["us"].append(round(dt * 1e6, 1))
                for im in ims:
                    im.release()
        for name, o in out.items():
            us = sorted(o["us"][1:] or o["us"])
            print(json.dumps({"path": name, "requests": len(frames), "lds": args.lds,
                              "chains": sorted(set(" + ".join(j.get("filters", ())) for j in jobs)),
                              "launches": o["launches"], "us_p50": us[len(us) // 2], "us_min": us[0], "us_max": us[-1]}), flush=True)
        for f in frames:
            f.release()
        cfg.release()
    finally:
        imp.env_destroy()


if __name__ == "__main__":
    main()
