"""Measurements of the device's lossy WebP encoder (impgpu_image_encode_webp_lossy / impgpu_batch_encode_webp_lossy) against
the routes it replaces.

    python tools/webp_lossy_probe.py --sizes       CPU only (the host twin): a 320x240 photo-like frame at qualities 50, 75
                                                   and 90: file size and PSNR against the source, beside Pillow's lossy file
                                                   (method 4) at the quality whose size is nearest -> profiles/webp_lossy_sizes.json
    python tools/webp_lossy_probe.py               needs the device: the three workloads of profiles/webp_encode_probe.json,
                                                   photo-like at quality 75: the time of the call, of impgpu_batch_download of
                                                   the same frames alone, and of Pillow's lossy save (methods 0 and 4) on one
                                                   core -> profiles/webp_lossy_probe.json
    python tools/webp_lossy_probe.py --trace       every workload twice (a warm-up, then the call that counts), to be run under
                                                   `rocprofv3 --kernel-trace --output-format csv`
    python tools/webp_lossy_probe.py --fold CSV    CPU only: the per-kernel times of such a run's kernel_trace.csv into the
                                                   probe file
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from webp_encode_probe import GEOMETRIES, download, frames_of, median_ms  # noqa: E402

QUALITY = 75
KERNELS = ["k_vp8_planes", "k_vp8_recon", "k_vp8_tokens", "k_vp8_bool", "k_vp8_pack"]
PROBE = os.path.join(ROOT, "profiles", "webp_lossy_probe.json")


def pillow_lossy(frame, quality, method):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame[..., [2, 1, 0]]), "RGB").save(buf, format="WEBP", quality=quality, method=method)
    return buf.getvalue()


def psnr_of(blob, frame):
    from PIL import Image

    rgb = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB")).astype(np.float64)
    return float(10 * np.log10(255.0 ** 2 / np.mean((rgb - frame[..., [2, 1, 0]]) ** 2)))


def sizes():
    import ngx_http_imgproc_amd as imp

    frame = np.ascontiguousarray(frames_of("64x320x240", "photo")[0][..., :3])
    pillow = {q: pillow_lossy(frame, q, 4) for q in range(1, 101)}
    out = {"geometry": "320x240 B,G,R photo-like", "pillow_method": 4, "qualities": {}}
    for q in (50, 75, 90):
        rc, blob, n, intact = imp.encode_webp_lossy_host(frame, q)
        assert rc == 0 and intact
        near = min(pillow, key=lambda k: abs(len(pillow[k]) - n))
        same = min(pillow, key=lambda k: abs(psnr_of(pillow[k], frame) - psnr_of(blob, frame)))
        row = {"bytes": n, "psnr_db": round(psnr_of(blob, frame), 2), "pillow_nearest_size_quality": near, "pillow_nearest_size_bytes": len(pillow[near]),
               "pillow_nearest_size_psnr_db": round(psnr_of(pillow[near], frame), 2), "pillow_same_quality_bytes": len(pillow[q]),
               "pillow_same_quality_psnr_db": round(psnr_of(pillow[q], frame), 2), "pillow_nearest_psnr_quality": same,
               "pillow_nearest_psnr_bytes": len(pillow[same]), "pillow_nearest_psnr_db": round(psnr_of(pillow[same], frame), 2)}
        row["bytes_over_pillow_at_equal_psnr"] = round(n / len(pillow[same]), 3)
        out["qualities"][str(q)] = row
        print(q, json.dumps(row), flush=True)
    with open(os.path.join(ROOT, "profiles", "webp_lossy_sizes.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)


def measure():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    out = {"quality": QUALITY, "content": "photo-like, BGRA with alpha 255", "cases": {}}
    for g in GEOMETRIES:
        fs = frames_of(g, "photo")
        images = [imp.Image(f) for f in fs]
        qs = [QUALITY] * len(fs)
        caps = [imp.webp_lossy_encode_bound(f.shape[1], f.shape[0], 4) // 8 for f in fs]      # buffers a caller would bring, not the worst case
        rc, results, launches = imp.batch_encode_webp_lossy(images, qs, capacities=caps)
        assert rc == 0 and all(r[0] == 0 for r in results), g
        assert results[0][1] == imp.encode_webp_lossy_host(fs[0], QUALITY)[1], g             # the first file is the host twin's
        caps = [r[2] + 1024 for r in results]
        case = {"frames": len(fs), "launches": launches, "bytes_device_webp": sum(r[2] for r in results), "bytes_raw": sum(f.nbytes for f in fs),
                "psnr_db_first": round(psnr_of(results[0][1], fs[0]), 2)}
        case["ms_encode_webp_lossy"] = median_ms(lambda: imp.batch_encode_webp_lossy(images, qs, capacities=caps))
        case["ms_download"] = median_ms(lambda: download(imp, images, fs))
        for method in (0, 4):
            t = time.perf_counter()
            files = [pillow_lossy(f, QUALITY, method) for f in fs]
            case["ms_pillow_method%d_one_core" % method] = (time.perf_counter() - t) * 1e3
            case["ms_download_plus_pillow_method%d" % method] = case["ms_download"] + case["ms_pillow_method%d_one_core" % method]
            case["bytes_pillow_method%d" % method] = sum(len(b) for b in files)
        out["cases"]["%s_photo" % g] = case
        print(g, json.dumps(case), flush=True)
        for im in images:
            im.release()
    imp.env_destroy()
    with open(PROBE, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)


def trace():
    import torch  # noqa: F401
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    for g in GEOMETRIES:
        fs = frames_of(g, "photo")
        images = [imp.Image(f) for f in fs]
        caps = [imp.webp_lossy_encode_bound(f.shape[1], f.shape[0], 4) // 8 for f in fs]
        for _ in range(2):
            rc, results, launches = imp.batch_encode_webp_lossy(images, [QUALITY] * len(fs), capacities=caps)
            assert rc == 0 and launches % len(KERNELS) == 0 and all(r[0] == 0 for r in results)
        for im in images:
            im.release()
    imp.env_destroy()


def fold(csv_path):
    """the k_vp8_* rows of a --trace run, in start order: per workload the warm-up call's dispatches, then those of the call
    that counts (five a group of the call; a kernel's time is summed over the groups)"""
    import csv
    import re

    with open(csv_path, newline="") as fh:
        rows = [r for r in csv.DictReader(fh) if "k_vp8_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    with open(PROBE) as fh:
        out = json.load(fh)
    at = 0
    for g in GEOMETRIES:
        case = out["cases"]["%s_photo" % g]
        n = case["launches"]
        part = rows[at + n: at + 2 * n]
        at += 2 * n
        names = [re.search(r"k_vp8_\w+", r["Kernel_Name"]).group(0) for r in part]
        assert names == KERNELS * (n // len(KERNELS)), names
        case["kernels_us"] = {k: 0.0 for k in KERNELS}
        for k, r in zip(names, part):
            case["kernels_us"][k] = round(case["kernels_us"][k] + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, 1)
        print(g, json.dumps(case["kernels_us"]), flush=True)
    assert at == len(rows), (at, len(rows))
    with open(PROBE, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    if "--sizes" in sys.argv:
        sizes()
    elif "--trace" in sys.argv:
        trace()
    elif "--fold" in sys.argv:
        fold(sys.argv[sys.argv.index("--fold") + 1])
    else:
        measure()
