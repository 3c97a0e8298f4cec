"""Measurements of the device's lossless WebP encoder (impgpu_image_encode_webp / impgpu_batch_encode_webp) against the
routes it replaces -> profiles/webp_encode_probe.json.

    python tools/webp_encode_probe.py --sizes      CPU only: total file size of the probe's frames at tile bits 3, 4, 5
                                                   (tests/webp_writer.py), how IMPGPU_WEBP_TILE_BITS was chosen
    python tools/webp_encode_probe.py              needs the device: per case the time of the call, of impgpu_batch_download
                                                   of the same frames alone, of that plus Pillow's lossless save (method 0) on
                                                   one core, and the file sizes beside Pillow's (method 0 and 6) and the
                                                   device's PNG answer at level 9
    python tools/webp_encode_probe.py --trace CASE one call of one case and nothing else, to be run under
                                                   `rocprofv3 --kernel-trace --stats -- python tools/webp_encode_probe.py --trace CASE`

    python tools/webp_encode_probe.py --lz-sizes   CPU only: the 320x240 B,G,R frames of the size conditions of
                                                   tests/test_webp_lz_writer.py, written by tests/webp_writer.py and by
                                                   tests/webp_lz_writer.py (IMPGPU_WEBP_ENC_BACKREFS), beside Pillow's method 0
                                                   and 6 -> profiles/webp_lz_sizes.json
    python tools/webp_encode_probe.py --lz [--out FILE]
                                                   needs the device: the same cases with the flag off and on in ONE session,
                                                   the two calls alternating: times, launches, file sizes and the bytes that
                                                   cross the link -> profiles/webp_lz_probe.json (or FILE)
    python tools/webp_encode_probe.py --lz-trace   every case once with the flag off and once with it on after a warm-up of
                                                   each, to be run under `rocprofv3 --kernel-trace --output-format csv`
    python tools/webp_encode_probe.py --lz-fold CSV [--out FILE]
                                                   CPU only: the per-kernel times of such a run's kernel_trace.csv, k_webp_parse
                                                   among them, into the --lz file

Cases: a lone 640x480 frame, a lone 1920x1080 frame, 64 frames of 320x240; each as a photo-like frame (smooth structure
plus sensor-like noise), a dithered 256-colour frame and a flat-colour frame.  All BGRA.
"""
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GEOMETRIES = {"640x480": (640, 480, 1), "1920x1080": (1920, 1080, 1), "64x320x240": (320, 240, 64)}
KINDS = ("photo", "dither", "flat")


def frame_of(kind, w, h, seed):
    rng = np.random.default_rng(1000 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "flat":
        f = np.empty((h, w, 4), np.uint8)
        f[...] = [40 + seed % 100, 120, 200, 255]
        return f
    base = np.stack([127 + 90 * np.sin(x / (37.0 + k * 11) + seed) * np.cos(y / (29.0 + k * 7)) + 30 * (x / w - 0.5) for k in range(3)], axis=2)
    if kind == "photo":
        f = np.clip(base + rng.normal(0, 2.5, base.shape), 0, 255).astype(np.uint8)
    else:                                                    # 6 x 7 x 6 colour cube, ordered dither
        assert kind == "dither", kind
        bayer = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]]) / 16.0 - 0.5
        t = bayer[(np.arange(h) % 4)[:, None], (np.arange(w) % 4)[None, :]][..., None]
        levels = np.array([6, 7, 6])
        q = np.clip(np.floor(base / 255.0 * (levels - 1) + 0.5 + t), 0, levels - 1)
        f = np.rint(q * 255.0 / (levels - 1)).astype(np.uint8)
    return np.concatenate([f, np.full((h, w, 1), 255, np.uint8)], axis=2)


def frames_of(geometry, kind):
    w, h, n = GEOMETRIES[geometry]
    return [frame_of(kind, w, h, k) for k in range(n)]


def sizes():
    import webp_writer as W

    totals = {}
    for bits in (3, 4, 5):
        total = 0
        for g in GEOMETRIES:
            for kind in KINDS:
                fs = frames_of(g, kind)[:4]                  # four of the 64 small frames stand for them all
                total += sum(W.file_size(f, tile_bits=bits) for f in fs)
        totals[bits] = total
        print("tile bits %d: %d bytes" % (bits, total), flush=True)
    return totals


def median_ms(fn, reps=9):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out))


def pillow_webp(frame, method):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(frame[..., [2, 1, 0, 3]], "RGBA").save(buf, format="WEBP", lossless=True, method=method)
    return buf.getvalue()


def download(imp, images, frames):
    """impgpu_batch_download of the frames into host arrays of their size: one call, one wait"""
    import ctypes as C

    outs = [np.empty_like(f) for f in frames]
    hs = (C.c_void_p * len(images))(*[im.h.value for im in images])
    ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    steps = (C.c_int * len(outs))(*[o.shape[1] * o.shape[2] for o in outs])
    rc = imp.lib.impgpu_batch_download(hs, len(images), ptrs, steps)
    assert rc == 0, rc
    return outs


def measure():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    out = {"tile_bits": imp.WEBP_TILE_BITS, "cases": {}}
    for g in GEOMETRIES:
        for kind in KINDS:
            fs = frames_of(g, kind)
            images = [imp.Image(f) for f in fs]
            rc, results, launches = imp.batch_encode_webp(images)
            assert rc == 0 and all(r[0] == 0 for r in results), (g, kind)
            from PIL import Image

            back = np.asarray(Image.open(io.BytesIO(results[0][1])).convert("RGBA"))
            assert np.array_equal(back, fs[0][..., [2, 1, 0, 3]]), (g, kind)          # the first file decodes to its frame
            assert results[0][1] == imp.encode_webp_host(fs[0])[1], (g, kind)          # and is the host twin's
            case = {"frames": len(fs), "launches": launches, "bytes_device_webp": sum(r[2] for r in results),
                    "bytes_raw": sum(f.nbytes for f in fs)}
            case["ms_encode_webp"] = median_ms(lambda: imp.batch_encode_webp(images))
            case["ms_download"] = median_ms(lambda: download(imp, images, fs))
            t = time.perf_counter()
            m0 = [pillow_webp(f, 0) for f in fs]
            case["ms_pillow_method0_one_core"] = (time.perf_counter() - t) * 1e3
            case["ms_download_plus_pillow"] = case["ms_download"] + case["ms_pillow_method0_one_core"]
            case["bytes_pillow_method0"] = sum(len(b) for b in m0)
            case["bytes_pillow_method6"] = sum(len(pillow_webp(f, 6)) for f in fs[:4]) * len(fs) // min(4, len(fs))
            case["bytes_device_png9"] = sum(len(b) for _, b in imp.batch_encode_png(images, level=9))
            out["cases"]["%s_%s" % (g, kind)] = case
            print(g, kind, json.dumps(case), flush=True)
            for im in images:
                im.release()
    imp.env_destroy()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "webp_encode_probe.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)


def pillow_bgr(frame, method):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame[..., ::-1]), "RGB").save(buf, format="WEBP", lossless=True, method=method)
    return len(buf.getvalue())


def lz_sizes():
    import webp_lz_writer as LZ
    import webp_writer as W
    from test_webp_lz_writer import fixture
    from test_webp_writer import content

    out = {"geometry": "320x240 B,G,R", "frames": {}}
    for name in ("flat", "screenshot", "dither", "photo"):
        frame = content("flat_bgr", 320, 240) if name == "flat" else fixture(name, 320, 240)
        toks = LZ.tokens(frame)
        row = {"bytes_flagless": W.file_size(frame), "bytes_backrefs": LZ.file_size(frame), "tokens": len(toks),
               "references": sum(1 for t in toks if t[2]), "bytes_pillow_method0": pillow_bgr(frame, 0), "bytes_pillow_method6": pillow_bgr(frame, 6)}
        row["ratio_to_flagless"] = round(row["bytes_backrefs"] / row["bytes_flagless"], 4)
        out["frames"][name] = row
        print(name, json.dumps(row), flush=True)
    with open(os.path.join(ROOT, "profiles", "webp_lz_sizes.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)


def lz_out_path():
    return sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "webp_lz_probe.json")


def lz_measure(reps=9):
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    out = {"flag": "IMPGPU_WEBP_ENC_BACKREFS", "reps": reps, "cases": {}}
    for g in GEOMETRIES:
        for kind in KINDS:
            fs = frames_of(g, kind)
            images = [imp.Image(f) for f in fs]
            case = {"frames": len(fs), "bytes_raw": sum(f.nbytes for f in fs)}
            calls = {"off": lambda: imp.batch_encode_webp(images), "on": lambda: imp.batch_encode_webp(images, flags=imp.WEBP_ENC_BACKREFS)}
            for key, call in calls.items():
                rc, results, launches = call()                                             # (the warm-up as well)
                assert rc == 0 and all(r[0] == 0 for r in results), (g, kind, key)
                from PIL import Image

                back = np.asarray(Image.open(io.BytesIO(results[0][1])).convert("RGBA"))
                assert np.array_equal(back, fs[0][..., [2, 1, 0, 3]]), (g, kind, key)      # the first file decodes to its frame
                host = imp.encode_webp_host(fs[0], flags=None if key == "off" else imp.WEBP_ENC_BACKREFS)[1]
                assert results[0][1] == host, (g, kind, key)                               # and is the host twin's
                case["launches_" + key] = launches
                case["bytes_" + key] = sum(r[2] for r in results)
                case["bytes_link_down_" + key] = case["bytes_" + key] + 16 * len(fs)         # the files and a record a frame
            times = {"off": [], "on": []}
            for _ in range(reps):                                                          # the two calls alternate
                for key, call in calls.items():
                    t = time.perf_counter()
                    call()
                    times[key].append((time.perf_counter() - t) * 1e3)
            for key in times:
                case["ms_" + key] = float(np.median(times[key]))
                case["ms_%s_min_max" % key] = [float(min(times[key])), float(max(times[key]))]
            case["bytes_pillow_method0"] = sum(len(pillow_webp(f, 0)) for f in fs)
            out["cases"]["%s_%s" % (g, kind)] = case
            print(g, kind, json.dumps(case), flush=True)
            for im in images:
                im.release()
    imp.env_destroy()
    with open(lz_out_path(), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)


def lz_trace():
    import torch  # noqa: F401
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    for g in GEOMETRIES:
        for kind in KINDS:
            images = [imp.Image(f) for f in frames_of(g, kind)]
            for _ in range(2):                                                             # a warm-up of each, then the traced pair
                imp.batch_encode_webp(images)
                imp.batch_encode_webp(images, flags=imp.WEBP_ENC_BACKREFS)
            for im in images:
                im.release()
    imp.env_destroy()


def lz_fold(csv_path):
    """the k_webp_* rows of a --lz-trace run, in start order: per case 6 + 7 warm-up dispatches, then the 6 + 7 that count"""
    import csv
    import re

    with open(csv_path, newline="") as fh:
        rows = [r for r in csv.DictReader(fh) if "k_webp_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cases = ["%s_%s" % (g, kind) for g in GEOMETRIES for kind in KINDS]
    assert len(rows) == 26 * len(cases), len(rows)
    with open(lz_out_path()) as fh:
        out = json.load(fh)
    for k, case in enumerate(cases):
        mine = rows[26 * k + 13: 26 * k + 26]
        for key, part in (("off", mine[:6]), ("on", mine[6:])):
            names = [re.search(r"k_webp_\w+", r["Kernel_Name"]).group(0) for r in part]
            assert names == (["k_webp_modes", "k_webp_resid"] + (["k_webp_parse"] if key == "on" else []) +
                             ["k_webp_codes", "k_webp_measure", "k_webp_scan", "k_webp_emit"]), names
            out["cases"][case]["kernels_us_" + key] = {n: round((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, 1) for n, r in zip(names, part)}
        print(case, json.dumps({key: out["cases"][case]["kernels_us_" + key] for key in ("off", "on")}), flush=True)
    with open(lz_out_path(), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)


def trace(case):
    import torch  # noqa: F401
    import ngx_http_imgproc_amd as imp

    g, kind = case.rsplit("_", 1)
    imp.env_start(0)
    images = [imp.Image(f) for f in frames_of(g, kind)]
    imp.batch_encode_webp(images)
    imp.env_destroy()


if __name__ == "__main__":
    if "--sizes" in sys.argv:
        sizes()
    elif "--lz-sizes" in sys.argv:
        lz_sizes()
    elif "--lz-trace" in sys.argv:
        lz_trace()
    elif "--lz-fold" in sys.argv:
        lz_fold(sys.argv[sys.argv.index("--lz-fold") + 1])
    elif "--lz" in sys.argv:
        lz_measure()
    elif "--trace" in sys.argv:
        trace(sys.argv[sys.argv.index("--trace") + 1])
    else:
        measure()
