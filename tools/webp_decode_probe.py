"""Measurements of the device's lossless WebP decoder (impgpu_batch_decode_webp) against the route it replaces -- Pillow's
libwebp decode of the same file on one core plus impgpu_image_upload of the pixels -> profiles/webp_decode_probe.json.

    python tools/webp_decode_probe.py [--out FILE]   needs the device: per case the time of the device call (host front,
                                                     upload, three launches, the one wait), of the host front alone
                                                     (impgpu_webp_decode_host is NOT it: the front is timed through a call
                                                     of refused capacity, which stops behind the parse), and of the host
                                                     route; the files' sizes; whether the frames are Pillow's
    python tools/webp_decode_probe.py --trace        every case once after a warm-up of each, to be run under
                                                     `rocprofv3 --kernel-trace --output-format csv -- python tools/webp_decode_probe.py --trace`
    python tools/webp_decode_probe.py --fold CSV [--out FILE]
                                                     CPU only: the per-kernel times of such a run's kernel_trace.csv into the file

Cases (tools/webp_encode_probe.py's frames): a lone 640x480 frame, a lone 1920x1080 frame, 64 files of 320x240; each
photo-like, dithered 256-colour and flat.  The files are Pillow's lossless encodings (method 4, its default).
"""
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from webp_encode_probe import GEOMETRIES, KINDS, frames_of  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "webp_decode_probe.json")
KERNELS = ("k_webp_dec_tables", "k_webp_dec_pixels", "k_webp_dec_inverse")


def files_of(geometry, kind):
    from PIL import Image

    out = []
    for f in frames_of(geometry, kind):
        buf = io.BytesIO()
        Image.fromarray(f[..., [2, 1, 0]]).save(buf, format="WEBP", lossless=True)
        out.append((buf.getvalue(), f))
    return out


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out))


def pillow_bgr(blob):
    from PIL import Image

    im = Image.open(io.BytesIO(blob))
    im.load()
    return np.asarray(im)[..., ::-1]


def cases():
    return [(g, k) for g in GEOMETRIES for k in KINDS]


def measure(out_path):
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    rows = []
    for g, kind in cases():
        files = files_of(g, kind)
        blobs = [b for b, _ in files]
        big = GEOMETRIES[g][0] >= 1920

        def device():
            res, launches = imp.batch_decode_webp(blobs)
            for rc, im in res:
                assert rc == 0, rc
                im.release()
            return launches

        def front():
            for b in blobs:
                imp.webp_decode_host(b, capacity=0, guard=0)

        def host():
            for b in blobs:
                imp.Image(np.ascontiguousarray(pillow_bgr(b))).release()
            imp.sync()

        res, launches = imp.batch_decode_webp(blobs)
        same = all(rc == 0 and np.array_equal(im.numpy()[..., :3], f[..., :3]) and bool((im.numpy()[..., 3] == 255).all()) for (rc, im), (_, f) in zip(res, files))
        for _, im in res:
            im.release()
        info = imp.webp_decode_host(blobs[0])[2]
        row = {"geometry": g, "kind": kind, "files": len(blobs), "file_bytes": sum(len(b) for b in blobs), "launches": launches, "frames_equal_pillow": bool(same),
               "feature_word": info[0], "groups": info[1], "cache_bits": info[2],
               "device_ms": median_ms(device, 3 if big else 5), "host_front_ms": median_ms(front, 3), "pillow_plus_upload_ms": median_ms(host, 3 if big else 5)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    imp.env_destroy()
    doc = {"what": "impgpu_batch_decode_webp against Pillow's decode on one core + impgpu_image_upload; medians, one session", "rows": rows}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def trace():
    import torch  # noqa: F401
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    for g, kind in cases():
        blobs = [b for b, _ in files_of(g, kind)]
        for _ in range(2):                                   # a warm-up, then the call the fold reads (the LAST of each case)
            res, _ = imp.batch_decode_webp(blobs)
            for _, im in res:
                im.release()
    imp.env_destroy()


def fold(csv_path, out_path):
    """the decoder's kernels appear in launch order, two calls a case: the second call's durations, in microseconds"""
    import csv

    with open(csv_path) as f:
        rows = [r for r in csv.DictReader(f) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_call = [rows[i:i + 3] for i in range(0, len(rows), 3)]
    assert len(per_call) == 2 * len(cases()), len(per_call)
    with open(out_path) as f:
        doc = json.load(f)
    for k, (g, kind) in enumerate(cases()):
        call = per_call[2 * k + 1]
        split = {[k for k in KERNELS if k in r["Kernel_Name"]][0]: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in call}
        row = [r for r in doc["rows"] if r["geometry"] == g and r["kind"] == kind][0]
        row["kernel_us"] = split
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    if "--trace" in sys.argv:
        trace()
    elif "--fold" in sys.argv:
        fold(sys.argv[sys.argv.index("--fold") + 1], out)
    else:
        measure(out)
