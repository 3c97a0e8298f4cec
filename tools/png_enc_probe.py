"""PNG answer timings on one device -> one JSON line: lone encodes (224x224 BGR / BGRA, 1080p BGR), a batch of 64
thumbnails per image, and host libpng at the same settings on this box's core when libpng16 is loadable.

    timeout -k 10 300 python tools/png_enc_probe.py [--iters N]
Kernel times: run `--only 1080p` under rocprofv3 --kernel-trace --stats --output-format csv, then
    python tools/png_enc_probe.py --filter-rate <...kernel_stats.csv>
prints k_png_filter's bytes (the 1080p BGR frame read once, its filtered rows written once) over its mean time, against 8 TB/s."""
import argparse
import csv
import json
import os
import sys
import time

import torch  # noqa: F401  (first: the HIP runtime torch bundles, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ngx_http_imgproc_amd as imp  # noqa: E402
import png_enc_model as model  # noqa: E402


def best_ms(fn, iters):
    fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3


def filter_rate(path):
    h, w, c = 1080, 1920, 3
    moved = h * w * c + h * (1 + w * c)
    with open(path) as fh:
        for row in csv.DictReader(fh):
            if "k_png_filter" in row.get("Name", ""):
                ns = float(row["AverageNs"])
                return {"k_png_filter_1080p_us": round(ns / 1e3, 2), "bytes": moved,
                        "TBps": round(moved / ns / 1e3, 3), "of_8TBps": round(moved / ns / 1e3 / 8.0, 4)}
    raise SystemExit("no k_png_filter row in %s" % path)


def only_1080p(iters):
    imp.env_start(0)
    try:
        frame = model.make_frame("smooth", 1080, 1920, 3, 1)
        im = imp.Image(frame)
        for _ in range(iters):
            assert im.encode_png(9)[0] == 0
        im.release()
    finally:
        imp.env_destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--only", choices=["1080p"])
    ap.add_argument("--filter-rate", metavar="KERNEL_STATS_CSV")
    a = ap.parse_args()
    if a.filter_rate:
        print(json.dumps(filter_rate(a.filter_rate)))
        return
    if a.only:
        only_1080p(a.iters)
        return
    imp.env_start(0)
    out = {}
    try:
        for name, (h, w, c) in (("lone_224_bgr_ms", (224, 224, 3)), ("lone_224_bgra_ms", (224, 224, 4)), ("lone_1080p_bgr_ms", (1080, 1920, 3))):
            frame = model.make_frame("smooth", h, w, c, 1)
            im = imp.Image(frame)
            rc, blob = im.encode_png(9)
            assert rc == 0 and blob == model.encode(frame)
            out[name] = round(best_ms(lambda: im.encode_png(9), a.iters), 4)
            im.release()
        frames = [model.make_frame(["smooth", "noise"][i % 2], 224, 224, 3, i) for i in range(64)]
        ims = [imp.Image(f) for f in frames]
        out["batch64_224_bgr_ms"] = round(best_ms(lambda: imp.batch_encode_png(ims, 9), max(5, a.iters // 3)), 4)
        out["batch64_per_image_us"] = round(out["batch64_224_bgr_ms"] * 1e3 / 64, 2)
        for im in ims:
            im.release()
        lib = model.load_libpng()
        if lib is None:
            out["host_libpng"] = "libpng16 not loadable on this box"
        else:
            for name, (h, w, c) in (("host_libpng_224_bgr_ms", (224, 224, 3)), ("host_libpng_1080p_bgr_ms", (1080, 1920, 3))):
                frame = model.make_frame("smooth", h, w, c, 1)
                out[name] = round(best_ms(lambda: model.libpng_encode(lib, frame, 9), 5), 3)
    finally:
        imp.env_destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
