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
    elif "--trace" in sys.argv:
        trace(sys.argv[sys.argv.index("--trace") + 1])
    else:
        measure()
